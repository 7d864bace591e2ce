"""ms per call of ``splice_batches`` (the causal parts of a batch spliced with the trivial parts of a permutation of it, the
read-back of the totals included) and of ``structure_intervention(partners=1)``, beside a torch composition of the same splice on
the same device in the same process.  Three shapes: the headline batch (SPMotif ``node_num`` 7, B 128), ``nodenum15_bs128`` and
ba5000 (B 32).  The composition and the operator are asserted equal before anything is timed.

    python scripts/bench_splice.py [--iters 50]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _feat(b):
    return b.x if b.x is not None else b.feat


def torch_splice(a, b, gb):
    """The splice of graph g of ``a`` with graph ``gb[g]`` of ``b`` by repeat_interleave / cumsum / index_select, for sources
    without a column that leaves its graph: -> (x, edge_index, batch, ptr, edge_ptr, max_nodes, max_edges).  One read-back (the
    four sizes the Batch needs), as the operator has."""
    dev = gb.device
    P = int(a.num_graphs)
    xa, xb = _feat(a), _feat(b)
    zero = torch.zeros(1, dtype=torch.long, device=dev)
    an, bn = a.ptr[1:] - a.ptr[:-1], (b.ptr[1:] - b.ptr[:-1])[gb]
    ae, be = a.edge_ptr[1:] - a.edge_ptr[:-1], (b.edge_ptr[1:] - b.edge_ptr[:-1])[gb]
    ptr, eptr = torch.cat([zero, (an + bn).cumsum(0)]), torch.cat([zero, (ae + be).cumsum(0)])
    n2, e2, mn, me = torch.stack([ptr[-1], eptr[-1], (an + bn).max(), (ae + be).max()]).tolist()
    pairs = torch.arange(P, device=dev)
    batch = torch.repeat_interleave(pairs, an + bn, output_size=n2)
    loc = torch.arange(n2, device=dev) - ptr[batch]
    from_a = loc < an[batch]
    sa = (a.ptr[batch] + loc).clamp(max=max(xa.size(0) - 1, 0))
    sb = (b.ptr[gb[batch]] + loc - an[batch]).clamp(0, max(xb.size(0) - 1, 0))
    x = torch.where(from_a.view(-1, 1), xa[sa], xb[sb])
    gid = torch.repeat_interleave(pairs, ae + be, output_size=e2)
    loc = torch.arange(e2, device=dev) - eptr[gid]
    from_a = loc < ae[gid]
    ca = (a.edge_ptr[gid] + loc).clamp(max=max(a.edge_index.size(1) - 1, 0))
    cb = (b.edge_ptr[gb[gid]] + loc - ae[gid]).clamp(0, max(b.edge_index.size(1) - 1, 0))
    ea = a.edge_index[:, ca] - a.ptr[gid] + ptr[gid]
    eb = b.edge_index[:, cb] - b.ptr[gb[gid]] + ptr[gid] + an[gid]
    return x, torch.where(from_a, ea, eb), batch, ptr, eptr, mn, me


def timed(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    from cal_amd import model as M, spmotif, synth
    from cal_amd.data import Batch
    from cal_amd.explain import explain, extract_subgraph
    from cal_amd.splice import splice_batches, structure_intervention
    dev = "cuda"
    shapes = (("headline_nodenum7_bs128", lambda: spmotif.train_mix(128, node_num=7, seed=1), 128, a.iters),
              ("nodenum15_bs128", lambda: spmotif.train_mix(128, node_num=15, seed=1), 128, a.iters),
              ("ba5000_bs32", lambda: synth.ba_graphs(32, n=5000, seed=1), 256, max(a.iters // 5, 5)))
    out = {}
    for name, graphs, hidden, iters in shapes:
        args = argparse.Namespace(layers=3, hidden=hidden, with_random=True, without_node_attention=False,
                                  without_edge_attention=False, fc_num="222", cat_or_add="add", c=0.5, o=1.0, co=0.5)
        torch.manual_seed(0)
        m = M.CausalGCN(10, 4, args).to(dev).eval()
        b = Batch.from_data_list(graphs()).to(dev)
        B = int(b.num_graphs)
        perm = torch.randperm(B, generator=torch.Generator().manual_seed(2)).to(dev)
        nm = explain(m, b, ratio=0.3).node_mask
        causal = extract_subgraph(b, node_mask=nm, relabel=True)
        trivial = extract_subgraph(b, node_mask=nm, complement=True, relabel=True)
        sp = splice_batches(causal, trivial, None, perm)
        ref = torch_splice(causal, trivial, perm)
        got = (_feat(sp), sp.edge_index, sp.batch, sp.ptr, sp.edge_ptr, sp.max_nodes, sp.max_edges)
        for u, v in zip(got, ref):
            assert torch.equal(u, v) if torch.is_tensor(u) else u == v, name
        gen = torch.Generator().manual_seed(3)
        out[name] = {"nodes": int(sp.batch.numel()), "columns": int(sp.edge_index.size(1)),
                     "splice_ms": timed(lambda: splice_batches(causal, trivial, None, perm), iters),
                     "torch_ms": timed(lambda: torch_splice(causal, trivial, perm), iters),
                     "structure_intervention_ms": timed(lambda: structure_intervention(m, b, ratio=0.3, partners=1, generator=gen),
                                                        iters)}
        r = out[name]
        print("%-26s N' %8d  E' %8d  splice %8.3f ms  torch %8.3f ms  structure_intervention %8.3f ms"
              % (name, r["nodes"], r["columns"], r["splice_ms"], r["torch_ms"], r["structure_intervention_ms"]), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""ms per call of the occlusion operators on one GPU, each beside its yardstick in the same process:

* ``occlude_batch`` (two launches, one read-back) against the composition it replaces -- ``splice_batches(a, a, rep_graph, -1)``,
  a mask from torch ops, ``extract_subgraph`` (four launches, two read-backs, the mask ops) -- at the same list of 512 replicas of
  the headline batch (SPMotif ``node_num`` 7, B 128), edges (both columns of an undirected edge) and nodes.  The two are asserted
  equal before anything is timed, and timed alternately.
* ``occlusion()`` at the headline batch, directed and undirected, against the sum of its forwards alone (the same replica batches
  built once, only the engine's eval forwards timed).
* ``rank_agreement`` against a torch restatement of the ten counts (padded [B, L, L] comparisons) on the headline batch's edge
  segments.

    python scripts/bench_occlude.py [--iters 50] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def composition(b, rg, re, use, twin):
    """The replica batch from the operators that existed before: replicate, mask, extract."""
    from cal_amd.explain import extract_subgraph
    from cal_amd.splice import splice_batches
    rep = splice_batches(b, b, rg, torch.full_like(rg, -1))
    if use == "edges":
        src = rep.edge_src
        gone = re[torch.repeat_interleave(torch.arange(rg.numel(), device=rg.device), rep.edge_ptr[1:] - rep.edge_ptr[:-1],
                                          output_size=src.numel())]
        tw = twin.long()[gone.clamp(min=0)]
        return extract_subgraph(rep, edge_mask=(src != gone) & ((gone < 0) | (src != tw)))
    return extract_subgraph(rep, node_mask=rep.node_src != re[rep.batch], relabel=True)


def torch_counts(a, b, seg, max_seg, k):
    """The ten counts by padding every segment to max_seg (no NaN, no sel, top k)."""
    dev = a.device
    B = seg.numel() - 1
    n = seg[1:] - seg[:-1]
    col = torch.arange(max_seg, device=dev)
    ok = col.view(1, -1) < n.view(-1, 1)                                   # [B, L]
    idx = (seg[:-1].view(-1, 1) + col.view(1, -1)).clamp(max=a.numel() - 1)
    pair = ok.unsqueeze(2) & ok.unsqueeze(1)                               # [B, i, j]
    out = []
    sgn, r2, top = [], [], []
    kg = n.clamp(max=k)
    for v in (a, b):
        p = v[idx]
        pj, pi = p.unsqueeze(1), p.unsqueeze(2)
        s = ((pj > pi).to(torch.int8) - (pj < pi).to(torch.int8)) * pair                # sign(v_j - v_i)
        eq = (s == 0) & pair
        r2.append(2 * (s < 0).sum(2) + eq.sum(2) + 1)
        before = col.view(1, 1, -1) < col.view(1, -1, 1)
        pos = (s > 0).sum(2) + (eq & before).sum(2)
        top.append((pos < kg.view(-1, 1)) & ok)
        sgn.append(s)
        out.append((eq.sum((1, 2)) - n) // 2)
    prod = sgn[0] * sgn[1]
    z = lambda t: torch.where(ok, t, torch.zeros_like(t)).sum(1)
    return torch.stack([n, (prod > 0).sum((1, 2)) // 2, (prod < 0).sum((1, 2)) // 2, out[0], out[1], z(r2[0] * r2[0]),
                        z(r2[1] * r2[1]), z(r2[0] * r2[1]), kg, (top[0] & top[1]).sum(1)], 1)


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def alternate(fns, iters, repeats):
    """Median ms per call of every function, the functions timed in turns (so drift hits all of them alike)."""
    for fn in fns:
        for _ in range(5):
            fn()
    runs = [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            runs[i].append(timed(fn, iters))
    return [statistics.median(r) for r in runs], [max(r) - min(r) for r in runs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    from cal_amd import model as M, spmotif
    from cal_amd.data import Batch
    from cal_amd.explain import _Layout, _log_probs, edge_twins, explain
    from cal_amd.occlude import occlude_batch, occlusion, rank_agreement
    from cal_amd.replica import _grouped
    dev = "cuda"
    args = argparse.Namespace(layers=3, hidden=128, with_random=True, without_node_attention=False,
                              without_edge_attention=False, fc_num="222", cat_or_add="add", c=0.5, o=1.0, co=0.5)
    torch.manual_seed(0)
    m = M.CausalGCN(10, 4, args).to(dev).eval()
    b = Batch.from_data_list(spmotif.train_mix(128, node_num=7, seed=1)).to(dev)
    twin = edge_twins(b)[0]
    out = {"batch": {"graphs": int(b.num_graphs), "nodes": int(b.batch.numel()), "columns": int(b.edge_index.size(1))}}

    # 1. the builder against the composition, 512 replicas
    for use in ("edges", "nodes"):
        off = b.edge_ptr if use == "edges" else b.ptr
        re = torch.arange(0, int(off[-1]), max(int(off[-1]) // 512, 1), device=dev)[:512]
        rg = torch.searchsorted(off, re, right=True) - 1
        tw = twin if use == "edges" else None
        one, two = occlude_batch(b, rg, re, use=use, twin=tw), composition(b, rg, re, use, twin)
        for key in ("edge_index", "ptr", "edge_ptr", "batch", "feat" if one.x is None else "x"):
            assert torch.equal(getattr(one, key), getattr(two, key)), (use, key)
        (t1, t2), (s1, s2) = alternate([lambda: occlude_batch(b, rg, re, use=use, twin=tw), lambda: composition(b, rg, re, use, twin)],
                                       a.iters, a.repeats)
        out["builder_" + use] = {"replicas": int(rg.numel()), "nodes": int(one.batch.numel()), "columns": int(one.edge_index.size(1)),
                                 "occlude_batch_ms": t1, "composition_ms": t2, "spread_ms": [s1, s2]}
        print("builder %-6s R %4d  N' %7d  E' %7d  occlude_batch %7.3f ms (spread %.3f)  composition %7.3f ms (spread %.3f)"
              % (use, rg.numel(), one.batch.numel(), one.edge_index.size(1), t1, s1, t2, s2), flush=True)

    # 2. occlusion() against the sum of its forwards alone
    lay = _Layout(b)
    src = _grouped(b, lay)
    for undirected in (None, "mean"):
        occ = occlusion(m, b, undirected=undirected)
        tw = occ.twin
        ids = (~occ.score.isnan()).nonzero().view(-1)
        if tw is not None:
            ids = ids[~((tw[ids] >= 0) & (tw[ids] < ids))]
        gid = torch.searchsorted(b.edge_ptr, ids, right=True) - 1
        reps = [occlude_batch(src, gid[i:i + 512], ids[i:i + 512], twin=tw) for i in range(0, ids.numel(), 512)]
        assert len(reps) + 1 == occ.forwards and ids.numel() == occ.replicas

        def forwards():
            with torch.no_grad():
                _log_probs(m, src)
                for r in reps:
                    _log_probs(m, r)
        (t1, t2), (s1, s2) = alternate([lambda: occlusion(m, b, undirected=undirected), forwards], max(a.iters // 10, 3), a.repeats)
        name = "occlusion_" + ("undirected" if undirected else "directed")
        out[name] = {"replicas": occ.replicas, "forwards": occ.forwards, "occlusion_ms": t1, "forwards_alone_ms": t2,
                     "spread_ms": [s1, s2]}
        print("%-22s replicas %6d  forwards %3d  occlusion %8.3f ms (spread %.3f)  its forwards alone %8.3f ms (spread %.3f)"
              % (name, occ.replicas, occ.forwards, t1, s1, t2, s2), flush=True)

    # 3. rank_agreement against the torch restatement
    ex = explain(m, b, ratio=0.3)
    sa, sb = ex.edge_score.contiguous(), occlusion(m, b).score
    got = rank_agreement(sa, sb, b.edge_ptr, b.max_edges, k=10)[0]
    assert torch.equal(got, torch_counts(sa, sb, b.edge_ptr, b.max_edges, 10))
    (t1, t2), (s1, s2) = alternate([lambda: rank_agreement(sa, sb, b.edge_ptr, b.max_edges, k=10),
                                    lambda: torch_counts(sa, sb, b.edge_ptr, b.max_edges, 10)], a.iters, a.repeats)
    out["rank_agreement"] = {"segments": int(b.num_graphs), "elements": int(sa.numel()), "max_seg": int(b.max_edges),
                             "rank_agreement_ms": t1, "torch_ms": t2, "spread_ms": [s1, s2]}
    print("rank_agreement  B %4d  M %6d  max_seg %4d  kernel + metrics %7.3f ms (spread %.3f)  torch %7.3f ms (spread %.3f)"
          % (b.num_graphs, sa.numel(), b.max_edges, t1, s1, t2, s2), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

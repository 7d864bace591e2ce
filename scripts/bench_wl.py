"""ms per call of the WL operators on one GPU, each beside its yardstick in the same process:

* ``wl_refine`` (``iters`` 3) on the headline batch (SPMotif ``node_num`` 7, B 128) -- the public call, which derives the layout
  every time -- against a torch composition of the same rounds on the same tensors: int64 ``index_add_``, wrapping multiplies,
  logical shifts as an arithmetic shift and a mask.  The composition's colours and hashes are asserted equal to the kernel's.
* ``eval_explanation_census`` per batch, split into its parts: ``explain``, ``extract_subgraph``, ``wl_refine`` of the subgraphs,
  ``wl_match`` against the four motif prototypes, and the whole ``explanation_census`` call.

The median of ``--repeats`` rounds and the spread (max - min) are reported for each.

    python scripts/bench_wl.py [--iters 50] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def sync():
    if torch.cuda.is_initialized():
        torch.cuda.synchronize()


def timed(fn, iters):
    sync()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    sync()
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


def _i64(c):
    return c - (1 << 64) if c >= (1 << 63) else c


def _lsr(x, s):
    return (x >> s) & ((1 << (64 - s)) - 1)


def sm(x):
    """splitmix64 on int64 tensors: adds and multiplies wrap, the shifts are made logical by a mask"""
    x = x + _i64(0x9E3779B97F4A7C15)
    x = (x ^ _lsr(x, 30)) * _i64(0xBF58476D1CE4E5B9)
    x = (x ^ _lsr(x, 27)) * _i64(0x94D049BB133111EB)
    return x ^ _lsr(x, 31)


def torch_refine(ei, batch, ptr, B, T):
    """The rounds of cal_wl_refine as torch ops (every column inside its graph, no initial labels) -> (colors, hash)."""
    from cal_amd import wl
    N = int(batch.numel())
    u, v = ei[0], ei[1]
    c = sm(torch.zeros(N, dtype=torch.long, device=ei.device) ^ _i64(wl.C_INIT))
    h = sm((ptr[1:] - ptr[:-1]) ^ _i64(wl.C_GRAPH))
    cols, hs = [], []
    for t in range(T + 1):
        if t:
            so = torch.zeros_like(c).index_add_(0, u, sm(c[v] ^ _i64(wl.C_OUT)))
            si = torch.zeros_like(c).index_add_(0, v, sm(c[u] ^ _i64(wl.C_IN)))
            c = sm(sm(sm(c + _i64(wl.C_SELF)) + so) + si)
        cols.append(c)
        h = sm(h + torch.zeros(B, dtype=torch.long, device=ei.device).index_add_(0, batch, sm(c ^ _i64(wl.C_NODE))))
        hs.append(h)
    return torch.stack(cols), torch.stack(hs, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--graphs", type=int, default=128, help="batch size (128: the headline batch)")
    ap.add_argument("--device", default="cuda", help="cpu rehearses the script through libcalhost; its times say nothing")
    a = ap.parse_args()
    from cal_amd import model as M, spmotif
    from cal_amd.data import Batch
    from cal_amd.explain import explain, extract_subgraph
    from cal_amd.wl import explanation_census, wl_match, wl_refine
    dev = a.device
    args = argparse.Namespace(layers=3, hidden=128, with_random=True, without_node_attention=False,
                              without_edge_attention=False, fc_num="222", cat_or_add="add", c=0.5, o=1.0, co=0.5)
    torch.manual_seed(0)
    m = M.CausalGCN(10, 4, args).to(dev).eval()
    b = Batch.from_data_list(spmotif.train_mix(a.graphs, node_num=7, seed=1)).to(dev)
    B, T = int(b.num_graphs), 3
    out = {"batch": {"graphs": B, "nodes": int(b.batch.numel()), "columns": int(b.edge_index.size(1))}, "iters": T}

    # 1. the refinement against the torch composition
    ptr = b.ptr.to(dev)
    kernel = lambda: wl_refine(b, iters=T)
    torch_ = lambda: torch_refine(b.edge_index, b.batch, ptr, B, T)
    res, (tc, th) = kernel(), torch_()
    assert torch.equal(res.colors, tc) and torch.equal(res.hash, th)
    (t0, t1), (s0, s1) = alternate([kernel, torch_], a.iters, a.repeats)
    out["refine"] = {"wl_refine_ms": t0, "torch_ms": t1, "ratio": t1 / t0, "spread_ms": [s0, s1]}
    print("wl_refine T %d  B %4d  N %6d  E %6d   kernel %7.3f ms (spread %.3f)   torch composition %7.3f ms (spread %.3f)   x%.2f"
          % (T, B, b.batch.numel(), b.edge_index.size(1), t0, s0, t1, s1, t1 / t0), flush=True)

    # 2. the census of one batch, part by part
    protos = wl_refine(spmotif.motif_batch(dev), iters=T)
    ex = explain(m, b, ratio=0.3, undirected="mean")
    sub = extract_subgraph(b, edge_mask=ex.edge_mask, relabel=True)
    col = wl_refine(sub, iters=T)
    parts = [lambda: explain(m, b, ratio=0.3, undirected="mean"), lambda: extract_subgraph(b, edge_mask=ex.edge_mask, relabel=True),
             lambda: wl_refine(sub, iters=T), lambda: wl_match(col, protos),
             lambda: explanation_census(m, b, ratio=0.3, prototypes=protos)]
    names = ["explain", "extract", "refine", "match", "explanation_census"]
    ts, ss = alternate(parts, max(a.iters // 5, 3), a.repeats)
    out["census"] = {"subgraph_nodes": int(sub.batch.numel()), "subgraph_columns": int(sub.edge_index.size(1)),
                     **{n + "_ms": t for n, t in zip(names, ts)}, "spread_ms": ss}
    print("census of one batch (ratio 0.3, N' %d, E' %d):  " % (sub.batch.numel(), sub.edge_index.size(1))
          + "   ".join("%s %.3f ms (spread %.3f)" % (n, t, s) for n, t, s in zip(names, ts, ss)), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

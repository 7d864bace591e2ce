"""ms per call of exact motif matching on one GPU, beside the host twin in the same process:

* ``motif_match`` of whole SPMotif graphs against the four motifs (not induced, the default budget), on the headline batch
  (``node_num`` 7, B 128) and at ``node_num`` 15 (graphs of up to ~250 nodes: the longest searches the operator is meant for) --
  the public call, which derives the layout every time -- against libcalhost on ``--threads`` OpenMP threads on a host copy of
  the same batch.  The two results are asserted equal bit for bit.
* ``eval_explanation_motifs`` (``k="gt"``) over the same graphs in one batch, and its parts: ``explain``, ``extract_subgraph``
  and ``motif_match`` of the extracted explanations.

The median of ``--repeats`` rounds and the spread (max - min) are reported for each.

    python scripts/bench_motif.py [--iters 20] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--graphs", type=int, default=128, help="batch size (128: the headline batch)")
    ap.add_argument("--threads", type=int, default=16, help="OpenMP threads of the host twin")
    ap.add_argument("--device", default="cuda", help="cpu rehearses the script through libcalhost; its times say nothing")
    a = ap.parse_args()
    os.environ["OMP_NUM_THREADS"] = str(a.threads)                           # (read when libcalhost's first parallel loop runs)
    import torch
    from cal_amd import model as M, spmotif
    from cal_amd.data import Batch, DataLoader
    from cal_amd.explain import explain, extract_subgraph
    from cal_amd.motif import MotifPatterns, eval_explanation_motifs, motif_match

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
            for _ in range(3):
                fn()
        runs = [[] for _ in fns]
        for _ in range(repeats):
            for i, fn in enumerate(fns):
                runs[i].append(timed(fn, iters))
        return [statistics.median(r) for r in runs], [max(r) - min(r) for r in runs]

    dev = a.device
    args = argparse.Namespace(layers=3, hidden=128, with_random=True, without_node_attention=False,
                              without_edge_attention=False, fc_num="222", cat_or_add="add", c=0.5, o=1.0, co=0.5)
    torch.manual_seed(0)
    m = M.CausalGCN(10, 4, args).to(dev).eval()
    protos = spmotif.motif_batch()
    pp = MotifPatterns(protos)
    out = {"threads": a.threads}
    for node_num in (7, 15):
        gs = spmotif.train_mix(a.graphs, node_num=node_num, seed=1)
        hb, b = Batch.from_data_list(gs), Batch.from_data_list(gs).to(dev)
        B = int(b.num_graphs)
        # 1. whole graphs against the four motifs, device and host twin
        kernel = lambda: motif_match(b, pp)
        host = lambda: motif_match(hb, pp)
        res, ref = kernel(), host()
        for x, y in zip(res, ref):
            assert torch.equal(x.cpu(), y)
        y = hb.y.view(-1)
        assert bool((ref.count[torch.arange(B), y] > 0).all())               # every graph contains its own label's motif
        (t0, t1), (s0, s1) = alternate([kernel, host], a.iters, a.repeats)
        row = {"graphs": B, "nodes": int(b.batch.numel()), "columns": int(b.edge_index.size(1)), "max_nodes": int(hb.max_nodes),
               "embeddings": int(ref.count.clamp(min=0).sum()), "truncated": int(ref.truncated.sum()),
               "motif_match_ms": t0, "host_ms": t1, "ratio": t1 / t0, "spread_ms": [s0, s1]}
        print("motif_match node_num %2d  B %4d  N %6d  E %6d  max nodes %3d  truncated %d   kernel %8.3f ms (spread %.3f)   "
              "host twin on %d threads %8.3f ms (spread %.3f)   x%.2f"
              % (node_num, B, row["nodes"], row["columns"], row["max_nodes"], row["truncated"], t0, s0, a.threads, t1, s1, t1 / t0),
              flush=True)
        # 2. the explanations of one batch, part by part
        ngt, egt = spmotif.ground_truth(b)
        ex = explain(m, b, k="gt", undirected="mean", edge_gt=egt, node_gt=ngt)
        sub = extract_subgraph(b, edge_mask=ex.edge_mask, relabel=True)
        loader = DataLoader(gs, batch_size=B, shuffle=False)
        parts = [lambda: explain(m, b, k="gt", undirected="mean", edge_gt=egt, node_gt=ngt),
                 lambda: extract_subgraph(b, edge_mask=ex.edge_mask, relabel=True), lambda: motif_match(sub, pp),
                 lambda: eval_explanation_motifs(m, loader, dev, k="gt", prototypes=protos)]
        names = ["explain", "extract", "match", "eval_explanation_motifs"]
        ts, ss = alternate(parts, max(a.iters // 5, 3), a.repeats)
        row["explanations"] = {"subgraph_nodes": int(sub.batch.numel()), "subgraph_columns": int(sub.edge_index.size(1)),
                               **{n + "_ms": t for n, t in zip(names, ts)}, "spread_ms": ss}
        print("explanations of one batch (k gt, N' %d, E' %d):  " % (sub.batch.numel(), sub.edge_index.size(1))
              + "   ".join("%s %.3f ms (spread %.3f)" % (n, t, s) for n, t, s in zip(names, ts, ss)), flush=True)
        out["node_num_%d" % node_num] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()

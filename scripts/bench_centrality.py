"""ms per call of the graph centralities on one GPU, beside the host twin in the same process and networkx where it imports:

* ``centrality`` (hop distances, node and edge betweenness, PageRank: ONE launch) of whole SPMotif batches, on the headline
  shape (``node_num`` 7: graphs of 54 to 63 nodes) and at ``node_num`` 15 (graphs of 230 to 247 nodes, the largest the device
  operator is meant for) -- the public call, which derives the layout every time -- against libcalhost on ``--threads`` OpenMP
  threads on a host copy of the same batch, and against networkx's ``betweenness_centrality`` + ``edge_betweenness_centrality`` +
  ``closeness_centrality`` + ``pagerank`` on a few of the graphs (scaled to the batch).  The integer outputs of the two libraries
  are asserted equal, the fp64 outputs compared.
* ``hop_distance`` alone (the launch with only ``hop`` wanted).
* ``eval_structural_baseline`` (the five kinds and the ascending orientation of two) next to ``eval_explanation`` for a briefly
  trained CausalGCN: how much of the attention's precision@k the graph's geometry gives for free.

The median of ``--repeats`` rounds and the spread (max - min) are reported for each time.  No time here is a pass criterion.

    python scripts/bench_centrality.py [--iters 20] [--repeats 5] [--train-steps 60]
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
    ap.add_argument("--train-steps", type=int, default=60, help="steps of the brief training before the baselines")
    ap.add_argument("--nx-graphs", type=int, default=4, help="graphs networkx is timed on (scaled to the batch)")
    ap.add_argument("--device", default="cuda", help="cpu rehearses the script through libcalhost; its times say nothing")
    a = ap.parse_args()
    os.environ["OMP_NUM_THREADS"] = str(a.threads)                           # (read when libcalhost's first parallel loop runs)
    import torch
    from cal_amd import model as M, spmotif
    from cal_amd.centrality import KINDS, centrality, eval_explanation_locality, eval_structural_baseline, hop_distance
    from cal_amd.data import Batch, DataLoader
    from cal_amd.explain import eval_explanation

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

    try:
        import networkx as nx
    except ImportError:
        nx = None

    dev = a.device
    out = {"threads": a.threads}
    for node_num in (7, 15):
        gs = spmotif.train_mix(a.graphs, node_num=node_num, seed=1)
        hb, b = Batch.from_data_list(gs), Batch.from_data_list(gs).to(dev)
        B = int(b.num_graphs)
        ngt = spmotif.ground_truth(b)[0]
        kernel, host = (lambda: centrality(b)), (lambda: centrality(hb))
        hop = lambda: hop_distance(b, ngt)
        res, ref = kernel(), host()
        for k in ("far", "reach", "ecc", "deg", "pr_iters", "skipped", "ignored"):
            assert torch.equal(getattr(res, k).cpu(), getattr(ref, k)), k
        diff = {k: float((getattr(res, k).cpu() - getattr(ref, k)).abs().max()) for k in ("bc", "ebc", "pr")}
        (t0, t1, t2), (s0, s1, s2) = alternate([kernel, host, hop], a.iters, a.repeats)
        row = {"graphs": B, "nodes": int(b.batch.numel()), "columns": int(b.edge_index.size(1)), "max_nodes": int(hb.max_nodes),
               "pr_iters_max": int(ref.pr_iters.max()), "centrality_ms": t0, "host_ms": t1, "ratio": t1 / t0, "hop_ms": t2,
               "spread_ms": [s0, s1, s2], "device_vs_host_max_abs": diff}
        print("centrality node_num %2d  B %4d  N %6d  E %6d  max nodes %3d  PageRank steps <= %d   kernel %8.3f ms (spread %.3f)   "
              "host twin on %d threads %8.3f ms (spread %.3f)   x%.2f   hop only %.3f ms"
              % (node_num, B, row["nodes"], row["columns"], row["max_nodes"], row["pr_iters_max"], t0, s0, a.threads, t1, s1, t1 / t0, t2),
              flush=True)
        if nx is not None:
            k = min(a.nx_graphs, B)
            Gs = []
            for g in gs[:k]:
                G = nx.Graph()
                G.add_nodes_from(range(int(g.num_nodes)))
                G.add_edges_from(g.edge_index.t().tolist())
                Gs.append(G)
            t = time.perf_counter()
            for G in Gs:
                nx.betweenness_centrality(G), nx.edge_betweenness_centrality(G), nx.closeness_centrality(G), nx.pagerank(G)
            row["networkx_ms_scaled"] = (time.perf_counter() - t) * 1e3 * B / k
            print("   networkx on %d of the graphs, scaled to the batch: %.1f ms" % (k, row["networkx_ms_scaled"]), flush=True)
        out["node_num_%d" % node_num] = row

    # a briefly trained model: the attention's figures beside the structure-only rankings'
    from cal_amd.trainer import CausalTrainer
    args = argparse.Namespace(layers=3, hidden=128, with_random=True, without_node_attention=False,
                              without_edge_attention=False, fc_num="222", cat_or_add="add", c=0.5, o=1.0, co=0.5)
    torch.manual_seed(0)
    m = M.CausalGCN(10, 4, args).to(dev)
    train = spmotif.train_mix(a.graphs * 4, node_num=7, seed=2)
    test = spmotif.train_mix(a.graphs * 2, node_num=7, seed=3)
    if dev != "cpu" and a.train_steps:
        tr = CausalTrainer(m, args, lr=1e-3, use_graph=False)
        step = 0
        while step < a.train_steps:
            for bt in DataLoader(train, batch_size=a.graphs, shuffle=True):
                tr.step(bt.to(dev))
                step += 1
                if step >= a.train_steps:
                    break
    loader = DataLoader(test, batch_size=a.graphs, shuffle=False)
    m.eval()
    t = time.perf_counter()
    base = eval_structural_baseline(m, loader, dev, kinds=KINDS + ("-closeness", "-degree"))    # (the periphery first)
    sync()
    out["eval_structural_baseline_ms"] = (time.perf_counter() - t) * 1e3
    out["eval_explanation"] = eval_explanation(m, loader, dev, k="gt", undirected="mean")
    out["structural_baseline"] = base
    out["locality"] = eval_explanation_locality(m, loader, dev, k="gt")
    print("after %d steps: eval_explanation edge precision@k %.3f  AUC %.3f   (chance %.3f)"
          % (a.train_steps, out["eval_explanation"]["edge_precision"], out["eval_explanation"]["edge_auc"], base["chance"]))
    print("   %-18s precision@k %.3f  recall@k %.3f  AUC %.3f" % ("attention", base["attention"]["precision"],
                                                                  base["attention"]["recall"], base["attention"]["auc"]))
    for kd, d in base["kinds"].items():
        print("   %-18s precision@k %.3f  recall@k %.3f  AUC %.3f   against the attention: rho %+.3f  tau %+.3f  jaccard %.3f"
              % (kd, d["precision"], d["recall"], d["auc"], d["rho"], d["tau"], d["jaccard"]))
    print("   locality of the explanations:", out["locality"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()

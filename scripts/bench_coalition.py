"""ms per call of the coalition operators on one GPU, each beside its yardstick in the same process:

* ``coalition_batch`` (two launches, one read-back) against the composition it replaces -- ``splice_batches(a, a, rep_graph, -1)``,
  a mask from torch ops, ``extract_subgraph`` (four launches, two read-backs, the mask ops) -- at the same list of 512 replicas of
  the headline batch (SPMotif ``node_num`` 7, B 128): edges under keys that give both columns of an undirected edge one position,
  and nodes.  The two are asserted equal before anything is timed, and timed alternately.
* ``shapley(perms=8)`` (undirected edges) and ``perturbation_curve`` (11 ratios, directed edges) at the headline batch against
  the sum of their forwards alone (the same replica batches built once, only the engine's eval forwards timed).

    python scripts/bench_coalition.py [--iters 50] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def composition(b, rg, rrow, rth, key, use):
    """The replica batch from the operators that existed before: replicate, mask, extract."""
    from cal_amd.explain import extract_subgraph
    from cal_amd.splice import splice_batches
    rep = splice_batches(b, b, rg, torch.full_like(rg, -1))
    if use == "edges":
        src = rep.edge_src
        rid = torch.repeat_interleave(torch.arange(rg.numel(), device=rg.device), rep.edge_ptr[1:] - rep.edge_ptr[:-1],
                                      output_size=src.numel())
        return extract_subgraph(rep, edge_mask=key[rrow[rid], src] < rth[rid])
    return extract_subgraph(rep, node_mask=key[rrow[rep.batch], rep.node_src] < rth[rep.batch], relabel=True)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--graphs", type=int, default=128, help="batch size (128: the headline batch)")
    ap.add_argument("--device", default="cuda", help="cpu rehearses the script through libcalhost; its times say nothing")
    a = ap.parse_args()
    from cal_amd import model as M, spmotif
    from cal_amd.coalition import coalition_batch, perturbation_curve, shapley
    from cal_amd.data import Batch
    from cal_amd.explain import _Layout, _log_probs, _scores
    from cal_amd.replica import _grouped, _Players
    dev = a.device
    args = argparse.Namespace(layers=3, hidden=128, with_random=True, without_node_attention=False,
                              without_edge_attention=False, fc_num="222", cat_or_add="add", c=0.5, o=1.0, co=0.5)
    torch.manual_seed(0)
    m = M.CausalGCN(10, 4, args).to(dev).eval()
    b = Batch.from_data_list(spmotif.train_mix(a.graphs, node_num=7, seed=1)).to(dev)
    lay = _Layout(b)
    src = _grouped(b, lay)
    out = {"batch": {"graphs": int(b.num_graphs), "nodes": int(b.batch.numel()), "columns": int(b.edge_index.size(1))}}
    sh = shapley(m, b, undirected="mean", perms=8, generator=torch.Generator().manual_seed(1))

    # 1. the builder against the composition, 512 replicas: graph r % B at a threshold that keeps about half of it
    R = 512
    rg = torch.arange(R, device=dev) % b.num_graphs
    rrow = torch.arange(R, device=dev) % 8
    for use in ("edges", "nodes"):
        if use == "edges":
            key = sh.keys                                                # both columns of an undirected edge: one position
        else:                                                            # a random order of every graph's nodes per row
            P = _Players(b, lay, src, "nodes", None)
            key = torch.stack([P.rank(torch.rand(P.M, device=dev)) for _ in range(8)])
        off = b.edge_ptr if use == "edges" else b.ptr
        n = off[1:] - off[:-1]
        rth = (n[rg] // (4 if use == "edges" else 2)).clamp(min=1)
        one, two = coalition_batch(b, rg, rth, key, rep_row=rrow, use=use), composition(b, rg, rrow, rth, key, use)
        for k in ("edge_index", "ptr", "edge_ptr", "batch", "feat" if one.x is None else "x"):
            assert torch.equal(getattr(one, k), getattr(two, k)), (use, k)
        (t1, t2), (s1, s2) = alternate([lambda: coalition_batch(b, rg, rth, key, rep_row=rrow, use=use),
                                        lambda: composition(b, rg, rrow, rth, key, use)], a.iters, a.repeats)
        out["builder_" + use] = {"replicas": R, "nodes": int(one.batch.numel()), "columns": int(one.edge_index.size(1)),
                                 "coalition_batch_ms": t1, "composition_ms": t2, "spread_ms": [s1, s2]}
        print("builder %-6s R %4d  N' %7d  E' %7d  coalition_batch %7.3f ms (spread %.3f)  composition %7.3f ms (spread %.3f)"
              % (use, R, one.batch.numel(), one.edge_index.size(1), t1, s1, t2, s2), flush=True)

    # 2. shapley(perms=8), undirected, against the sum of its forwards alone
    keys = sh.keys
    P = _Players(b, lay, src, "edges", "mean")
    n = P.count(P.rep)
    g1 = torch.repeat_interleave(torch.arange(b.num_graphs, device=dev), n)
    t1_ = torch.arange(g1.numel(), device=dev) - (torch.cumsum(n, 0) - n)[g1]
    T1 = int(g1.numel())
    ii = torch.arange(8 * T1, device=dev)
    reps = [coalition_batch(src, g1[c % T1], t1_[c % T1], keys, rep_row=c // T1) for c in ii.split(512)]
    assert len(reps) + 1 == sh.forwards and 8 * T1 == sh.replicas

    def forwards():
        with torch.no_grad():
            _log_probs(m, src)
            for r in reps:
                _log_probs(m, r)
    its = max(a.iters // 10, 3)
    (t1, t2), (s1, s2) = alternate([lambda: shapley(m, b, undirected="mean", perms=keys), forwards], its, a.repeats)
    out["shapley_undirected_8"] = {"players": T1, "replicas": sh.replicas, "forwards": sh.forwards, "shapley_ms": t1,
                                   "forwards_alone_ms": t2, "spread_ms": [s1, s2]}
    print("shapley perms=8 undirected  players %6d  replicas %6d  forwards %3d  shapley %8.3f ms (spread %.3f)  its forwards alone "
          "%8.3f ms (spread %.3f)" % (T1, sh.replicas, sh.forwards, t1, s1, t2, s2), flush=True)

    # 3. perturbation_curve, 11 ratios, directed edges under the causal attention, against its forwards alone
    ratios = tuple(i / 10 for i in range(11))
    cur = perturbation_curve(m, b, ratios=ratios)
    with torch.no_grad():
        order = _scores(m, b)[0].clone()
    Pd = _Players(b, lay, src, "edges", None)
    key = Pd.rank(order).view(1, -1)
    nn = Pd.count(torch.ones(Pd.M, dtype=torch.bool, device=dev))
    kk = torch.minimum(torch.ceil(torch.tensor(ratios, dtype=torch.float64, device=dev).view(-1, 1) * nn.double().view(1, -1)).long(),
                       nn.view(1, -1)).view(-1)
    gsel = torch.arange(b.num_graphs, device=dev).repeat(len(ratios))
    creps = [coalition_batch(src, gsel[c], kk[c], key, invert=inv) for inv in (False, True)
             for c in torch.arange(gsel.numel(), device=dev).split(512)]
    assert len(creps) + 2 == cur["forwards"] and 2 * gsel.numel() == cur["replicas"]

    def curve_forwards():
        with torch.no_grad():
            _scores(m, b)
            _log_probs(m, src)
            for r in creps:
                _log_probs(m, r)
    (t1, t2), (s1, s2) = alternate([lambda: perturbation_curve(m, b, ratios=ratios), curve_forwards], its, a.repeats)
    out["perturbation_curve_11"] = {"replicas": cur["replicas"], "forwards": cur["forwards"], "curve_ms": t1, "forwards_alone_ms": t2,
                                    "spread_ms": [s1, s2]}
    print("perturbation_curve 11 ratios  replicas %6d  forwards %3d  curve %8.3f ms (spread %.3f)  its forwards alone %8.3f ms "
          "(spread %.3f)" % (cur["replicas"], cur["forwards"], t1, s1, t2, s2), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

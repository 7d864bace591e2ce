"""ms per call of the noise operators on one GPU, each beside its yardstick in the same process:

* ``noise_batch`` at ``add = 0.1`` -- the public call, which derives the layout and builds the twin map (one more launch) every
  time, and the builder as the drivers call it, with both given -- against ``coalition_batch`` building the same number of
  control replicas of the headline batch (SPMotif ``node_num`` 7, B 128) -- the cost floor of copying the batch -- at 512
  replicas, timed alternately;
* ``noise_curve`` (four levels, four trials) and ``stability`` (``add = 0.1``, four trials) at the headline batch.

The median of ``--repeats`` rounds and the spread (max - min) are reported for each.

    python scripts/bench_noise.py [--iters 50] [--repeats 5]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--graphs", type=int, default=128, help="batch size (128: the headline batch)")
    ap.add_argument("--device", default="cuda", help="cpu rehearses the script through libcalhost; its times say nothing")
    a = ap.parse_args()
    from cal_amd import model as M, spmotif
    from cal_amd.coalition import coalition_batch
    from cal_amd.data import Batch
    from cal_amd.explain import _Layout
    from cal_amd.noise import _noise_build, noise_batch, noise_curve, stability
    from cal_amd.replica import _feature_width, _grouped, _Source
    dev = a.device
    args = argparse.Namespace(layers=3, hidden=128, with_random=True, without_node_attention=False,
                              without_edge_attention=False, fc_num="222", cat_or_add="add", c=0.5, o=1.0, co=0.5)
    torch.manual_seed(0)
    m = M.CausalGCN(10, 4, args).to(dev).eval()
    b = Batch.from_data_list(spmotif.train_mix(a.graphs, node_num=7, seed=1)).to(dev)
    lay = _Layout(b)
    src = _grouped(b, lay)
    out = {"batch": {"graphs": int(b.num_graphs), "nodes": int(b.batch.numel()), "columns": int(b.edge_index.size(1))}}

    # 1. the builder against the control replicas of coalition_batch, 512 replicas (the twin map is the drivers' too: built once)
    R = 512
    rg = torch.arange(R, device=dev) % b.num_graphs
    S = _Source(src)
    F, twin = _feature_width(S, "bench"), lay.twins(b.edge_index)[0]
    zero, minus = torch.zeros(R, dtype=torch.long, device=dev), torch.full((R,), -1, device=dev)
    key = torch.zeros(int(b.edge_index.size(1)), dtype=torch.int32, device=dev)
    noisy = lambda: _noise_build(S, F, twin, lay.max_edges, rg, 0.1, 0.0, 0, 8, "keep")
    public = lambda: noise_batch(b, rg, add=0.1)
    control = lambda: coalition_batch(src, rg, zero, key, rep_row=minus)
    one, two, three = noisy(), control(), public()
    assert torch.equal(one.ptr, two.ptr) and one.short == 0 and int(one.edge_index.size(1)) == int(two.edge_index.size(1)) + 2 * one.n_added
    assert torch.equal(one.edge_index, three.edge_index)
    (t0, t1, t2), (s0, s1, s2) = alternate([public, noisy, control], a.iters, a.repeats)
    out["builder"] = {"replicas": R, "nodes": int(one.batch.numel()), "columns": int(one.edge_index.size(1)), "added": one.n_added,
                      "noise_batch_ms": t0, "noise_build_ms": t1, "control_replicas_ms": t2, "ratio": t0 / t2, "ratio_build": t1 / t2,
                      "spread_ms": [s0, s1, s2]}
    print("builder R %4d  N' %7d  E' %7d  added %5d  noise_batch %7.3f ms (spread %.3f)  with layout and twin map given %7.3f ms "
          "(spread %.3f)  coalition_batch control %7.3f ms (spread %.3f)  ratios %.2f / %.2f"
          % (R, one.batch.numel(), one.edge_index.size(1), one.n_added, t0, s0, t1, s1, t2, s2, t0 / t2, t1 / t2), flush=True)

    # 2. the drivers at the headline batch
    its = max(a.iters // 10, 3)
    cur = noise_curve(m, b)
    st = stability(m, b, ratio=0.3)
    (t1, t2), (s1, s2) = alternate([lambda: noise_curve(m, b), lambda: stability(m, b, ratio=0.3)], its, a.repeats)
    out["noise_curve_4x4"] = {"replicas": sum(l["replicas"] for l in cur["levels"]), "forwards": cur["forwards"], "curve_ms": t1,
                              "spread_ms": s1}
    out["stability_4"] = {"replicas": st["replicas"], "forwards": st["forwards"], "stability_ms": t2, "spread_ms": s2}
    print("noise_curve 4 levels x 4 trials  forwards %3d  %8.3f ms (spread %.3f)   stability 4 trials  forwards %3d  %8.3f ms "
          "(spread %.3f)" % (cur["forwards"], t1, s1, st["forwards"], t2, s2), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

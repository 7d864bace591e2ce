"""ms per call of the gradient attributions on one GPU, each beside its yardsticks in the same process, on the headline batch
(SPMotif ``node_num`` 7, B 128) for CausalGCN / CausalGAT / CausalGIN at H 128:

* ``saliency`` and ``integrated_gradients(steps=32)`` (undirected edges);
* what the masks add: the unmasked operator-level forward + backward of the same batch (eval mode, parameters frozen, the
  gradient taken w.r.t. the input features);
* what the methods replace: ``occlusion`` and ``shapley(perms=8)`` on the same batch;
* the kernels: ``cal_gat_mask_fwd`` + ``_bwd`` at ``m = 1`` against ``cal_gat_fwd`` + ``cal_gat_bwd`` at p = 0 on the same rows
  (K x D = 4 x 32, through the two autograd functions of ``cal_amd.ops``).

Everything is timed in turns.

    python scripts/bench_gradient.py [--iters 20] [--repeats 5]
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
        for _ in range(2):
            fn()
    runs = [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            runs[i].append(timed(fn, iters[i]))
    return [statistics.median(r) for r in runs], [max(r) - min(r) for r in runs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--graphs", type=int, default=128, help="batch size (128: the headline batch)")
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--device", default="cuda", help="cpu rehearses the script through libcalhost; its times say nothing")
    a = ap.parse_args()
    from cal_amd import model as M, ops, spmotif
    from cal_amd.coalition import shapley
    from cal_amd.data import Batch
    from cal_amd.gradient import _frozen, integrated_gradients, saliency
    from cal_amd.occlude import occlusion
    from cal_amd.plan import plan_of
    dev = a.device
    args = argparse.Namespace(layers=3, hidden=128, with_random=True, without_node_attention=False,
                              without_edge_attention=False, fc_num="222", cat_or_add="add", c=0.5, o=1.0, co=0.5)
    b = Batch.from_data_list(spmotif.train_mix(a.graphs, node_num=7, seed=1)).to(dev)
    out = {"batch": {"graphs": int(b.num_graphs), "nodes": int(b.batch.numel()), "columns": int(b.edge_index.size(1))}, "steps": a.steps}
    few = max(a.iters // 10, 1)
    for name in ("CausalGCN", "CausalGAT", "CausalGIN"):
        torch.manual_seed(0)
        m = getattr(M, name)(10, 4, args).to(dev).eval()
        feat = b.x if b.x is not None else b.feat

        def plain():
            """The operator-level forward + backward without a mask: what ``saliency`` costs before the masks."""
            with _frozen(m):
                use_engine, m.use_engine = m.use_engine, False
                try:
                    x = feat.clone().requires_grad_(True)
                    b.x, keep = x, b.x
                    try:
                        lp = m(b, eval_random=False)[1]
                    finally:
                        b.x = keep
                    torch.autograd.grad(lp.max(-1).values.exp().sum(), x)
                finally:
                    m.use_engine = use_engine
        fns = [lambda: saliency(m, b, undirected="mean"), plain, lambda: integrated_gradients(m, b, undirected="mean", steps=a.steps),
               lambda: occlusion(m, b, undirected="mean"), lambda: shapley(m, b, undirected="mean", perms=8)]
        ts, ss = alternate(fns, [a.iters, a.iters, few, few, few], a.repeats)
        keys = ("saliency_ms", "plain_fwd_bwd_ms", "ig_ms", "occlusion_ms", "shapley8_ms")
        out[name] = dict(zip(keys, ts), spread_ms=ss)
        print("%-10s saliency %8.3f  plain fwd+bwd %8.3f  ig(%d) %9.3f  occlusion %9.3f  shapley(8) %9.3f   ms (spreads %s)"
              % (name, ts[0], ts[1], a.steps, ts[2], ts[3], ts[4], " ".join("%.3f" % s for s in ss)), flush=True)

    # the masked GAT kernels at m = 1 against the specialised ones at p = 0, on the batch's own rows
    plan = plan_of(b)
    K, D = 4, 32
    g = torch.Generator().manual_seed(2)
    z = (torch.randn(plan.N, K * D, generator=g) * 0.5).to(dev).requires_grad_(True)
    att = (torch.randn(1, K, 2 * D, generator=g) * 0.3).to(dev)
    bias = torch.randn(K * D, generator=g).to(dev)
    gout = torch.randn(plan.N, K * D, generator=g).to(dev)
    ones = torch.ones(plan.E, device=dev, requires_grad=True)

    def masked():
        torch.autograd.grad(ops.gat_aggregate(z, att, bias, plan, K, relu=True, edge_mask=ones), (z, ones), gout)

    def unmasked():
        torch.autograd.grad(ops.gat_aggregate(z, att, bias, plan, K, relu=True), z, gout)
    (t1, t2), (s1, s2) = alternate([masked, unmasked], [a.iters * 5] * 2, a.repeats)
    out["gat_kernels"] = {"K": K, "D": D, "masked_fwd_bwd_ms": t1, "gat_fwd_bwd_ms": t2, "spread_ms": [s1, s2]}
    print("GAT %dx%d fwd+bwd on N %d E %d: masked (m = 1) %.3f ms (spread %.3f)  cal_gat_fwd + cal_gat_bwd (p = 0) %.3f ms (spread %.3f)"
          % (K, D, plan.N, plan.E, t1, s1, t2, s2), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

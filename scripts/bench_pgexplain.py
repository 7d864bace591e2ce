"""ms per call of the parametric edge explainer on one GPU, each beside its yardsticks in the same process, on the headline batch
(SPMotif ``node_num`` 7, B 128) for CausalGCN / CausalGAT / CausalGIN at H 128, L 3, Hd 64, undirected players:

* one ``ExplainerTrainer.step`` (embeddings, one ``ops.linear``, ONE ``cal_edge_mlp_fwd``, the forward at m = 1, one masked forward,
  one backward through ``cal_edge_mlp_bwd`` and the GEMM, one Adam update);
* one ``explain_edges`` (embeddings, the linear, one launch, two forwards) and one ``MaskOptimizer.step`` -- ``learn_mask(steps=100)``
  costs 102 masked forwards per batch, ``explain_edges`` two and a backbone pass;
* forward + backward of the two new kernels alone (the linear included) against the same quantities composed in torch ops
  (``torch_composed`` below: gather, concat, two ``linear``s, elementwise sampling and regularisers; the comparator lives only in
  this script), both from the same embeddings to the gradients of the four parameters.

Everything is timed in turns; the median of ``--repeats`` rounds with the spread (max - min).

    python scripts/bench_pgexplain.py [--iters 20] [--repeats 5]
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


def torch_composed(ex, x, b, pl, gmask, tau, noise, size_coeff, ent_coeff):
    """What ``cal_edge_mlp_fwd`` / ``_bwd`` and the node projection compute, in torch ops: the [E, 2 H] gather and concat, two
    ``linear``s, the sample, both regularisers, autograd -> the gradients of the four parameters."""
    row, col = b.edge_index
    rep, has = pl.rep.long(), pl.mate >= 0
    mate = torch.where(has, pl.mate, pl.rep).long()
    pg = torch.repeat_interleave(torch.arange(pl.B, device=x.device), pl.pptr[1:] - pl.pptr[:-1])
    ent_w = (ent_coeff / pl.cnt.clamp(min=1.0)).float()[pg]

    def run():
        h = torch.relu(torch.nn.functional.linear(torch.cat([x[row], x[col]], -1), ex.lin1.weight, ex.lin1.bias))
        om_e = torch.nn.functional.linear(h, ex.lin2.weight, ex.lin2.bias).view(-1)
        omega = 0.5 * (om_e[rep] + om_e[mate])
        z = (noise + omega) / tau
        m = torch.sigmoid(z)
        ent = torch.nn.functional.softplus(z) - z * m
        mask = torch.ones_like(gmask).index_put((rep,), m).index_put((mate,), m)
        loss = (gmask * mask).sum() + size_coeff * m.sum() + (ent_w * ent).sum()
        return torch.autograd.grad(loss, list(ex.parameters()))
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--graphs", type=int, default=128, help="batch size (128: the headline batch)")
    ap.add_argument("--hidden", type=int, default=64, help="the explainer's hidden width Hd")
    ap.add_argument("--device", default="cuda", help="cpu rehearses the script through libcalhost; its times say nothing")
    a = ap.parse_args()
    from cal_amd import model as M, spmotif
    from cal_amd.data import Batch
    from cal_amd.maskopt import MaskOptimizer
    from cal_amd.pgexplain import EdgeExplainer, EdgePlayers, ExplainerTrainer, explain_edges
    from cal_amd.plan import plan_of
    dev = a.device
    args = argparse.Namespace(layers=3, hidden=128, with_random=True, without_node_attention=False,
                              without_edge_attention=False, fc_num="222", cat_or_add="add", c=0.5, o=1.0, co=0.5)
    b = Batch.from_data_list(spmotif.train_mix(a.graphs, node_num=7, seed=1)).to(dev)
    out = {"batch": {"graphs": int(b.num_graphs), "nodes": int(b.batch.numel()), "columns": int(b.edge_index.size(1))}, "hidden": a.hidden}
    for name in ("CausalGCN", "CausalGAT", "CausalGIN"):
        torch.manual_seed(0)
        m = getattr(M, name)(10, 4, args).to(dev).eval()
        ex = EdgeExplainer(128, a.hidden, seed=1).to(dev)
        tr = ExplainerTrainer(m, ex, total_steps=10 ** 6)
        opt = MaskOptimizer(m, b, undirected="mean")
        pl, plan = EdgePlayers.of(b, "mean"), plan_of(b)
        out.setdefault("players", pl.P)
        x = m._node_embeddings(b)
        gmask = torch.randn(plan.E, generator=torch.Generator().manual_seed(3)).to(dev) * 0.05
        params = list(ex.parameters())

        def fused():
            with torch.enable_grad():
                mask = ex(x, plan, pl, 2.0, 0, 0, 0.05, 1.0)[0]
                return torch.autograd.grad((gmask * mask).sum(), params)
        composed = torch_composed(ex, x, b, pl, gmask, 2.0, torch.zeros(pl.P, device=dev), 0.05, 1.0)
        # the two compute the same gradients: the largest difference relative to the parameter's largest gradient
        diff = max(((u - v).abs().max() / v.abs().max().clamp(min=1e-30)).item() for u, v in zip(fused(), composed()))
        fns = [lambda: tr.step(b), lambda: explain_edges(m, ex, b), opt.step, fused, composed]
        ts, ss = alternate(fns, [a.iters, a.iters, a.iters, a.iters * 5, a.iters * 5], a.repeats)
        keys = ("trainer_step_ms", "explain_edges_ms", "maskopt_step_ms", "kernels_fwd_bwd_ms", "torch_fwd_bwd_ms")
        out[name] = dict(zip(keys, ts), spread_ms=ss, max_rel_grad_diff=diff)
        print("%-10s trainer step %7.3f  explain_edges %7.3f  MaskOptimizer step %7.3f  kernels fwd+bwd %7.4f  torch-composed fwd+bwd "
              "%7.4f   ms (spreads %s); max |grad fused - composed| / max |grad| per parameter %.2g"
              % (name, ts[0], ts[1], ts[2], ts[3], ts[4], " ".join("%.3f" % s for s in ss), diff), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

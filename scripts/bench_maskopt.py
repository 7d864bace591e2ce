"""ms per call of the learned-mask optimiser on one GPU, each beside its yardsticks in the same process, on the headline batch
(SPMotif ``node_num`` 7, B 128) for CausalGCN / CausalGAT / CausalGIN at H 128, L 3, undirected players:

* one ``MaskOptimizer.step()`` (masked forward + backward + ONE ``cal_mask_step``);
* the same step with the update written in torch ops (``TorchUpdate`` below -- the sigmoid, the twin gather, both regularisers
  with their gradients, the chain rule, Adam's updates with bias correction, the scatter back and the per-graph sums: the
  comparator lives only in this script), and the two updates alone on a fixed gradient;
* one ``saliency`` call (one forward + backward of the same batch and its bookkeeping);
* ``learn_mask(steps=100)`` against ``occlusion`` and ``shapley(perms=8)``.

Everything is timed in turns; the median of ``--repeats`` rounds with the spread (max - min).

    python scripts/bench_maskopt.py [--iters 20] [--repeats 5]
"""
import argparse
import json
import math
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


def torch_update_class():
    from cal_amd.maskopt import MaskOptimizer

    class TorchUpdate(MaskOptimizer):
        """``MaskOptimizer`` with the update of ``cal_mask_step`` written in torch ops on the same state and tables."""

        def _tables(self):
            if not hasattr(self, "_pg"):
                cnt = self.pptr[1:] - self.pptr[:-1]
                self._pg = torch.repeat_interleave(torch.arange(self.B, device=self.theta.device), cnt)
                self._ent_w = (self.ent_coeff / cnt.clamp(min=1).float())[self._pg]
                self._rep = self.rep.long()
                self._has = (self.mate >= 0).nonzero().view(-1)
                self._mate = self.mate.long()[self._has]

        def _kernel(self, step, grad, terms):
            if step == 0:
                return super()._kernel(step, grad, terms)
            self._tables()
            b1, b2 = self.betas
            th = self.theta
            m = torch.sigmoid(th)
            ent = torch.nn.functional.softplus(th) - th * m
            terms.zero_()
            terms[:, 0].index_add_(0, self._pg, m.double())
            terms[:, 1].index_add_(0, self._pg, ent.double())
            g = grad[self._rep]
            g[self._has] += grad[self._mate]
            g = (g + self.size_coeff - self._ent_w * th) * (m * (1 - m))
            self.exp_avg.mul_(b1).add_(g, alpha=1 - b1)
            self.exp_avg_sq.mul_(b2).addcmul_(g, g, value=1 - b2)
            denom = (self.exp_avg_sq.sqrt() / math.sqrt(1 - b2 ** step)).add_(self.eps)
            th.addcdiv_(self.exp_avg, denom, value=-self.lr / (1 - b1 ** step))
            new = torch.sigmoid(th)
            self.mask[self._rep] = new
            self.mask[self._mate] = new[self._has]
    return TorchUpdate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--graphs", type=int, default=128, help="batch size (128: the headline batch)")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--device", default="cuda", help="cpu rehearses the script through libcalhost; its times say nothing")
    a = ap.parse_args()
    from cal_amd import model as M, spmotif
    from cal_amd.coalition import shapley
    from cal_amd.data import Batch
    from cal_amd.gradient import saliency
    from cal_amd.maskopt import MaskOptimizer, learn_mask
    from cal_amd.occlude import occlusion
    TorchUpdate = torch_update_class()
    dev = a.device
    args = argparse.Namespace(layers=3, hidden=128, with_random=True, without_node_attention=False,
                              without_edge_attention=False, fc_num="222", cat_or_add="add", c=0.5, o=1.0, co=0.5)
    b = Batch.from_data_list(spmotif.train_mix(a.graphs, node_num=7, seed=1)).to(dev)
    out = {"batch": {"graphs": int(b.num_graphs), "nodes": int(b.batch.numel()), "columns": int(b.edge_index.size(1))}, "steps": a.steps}
    few = max(a.iters // 10, 1)
    for name in ("CausalGCN", "CausalGAT", "CausalGIN"):
        torch.manual_seed(0)
        m = getattr(M, name)(10, 4, args).to(dev).eval()
        fused, plain = MaskOptimizer(m, b, undirected="mean"), TorchUpdate(m, b, undirected="mean")
        out.setdefault("players", fused.P)
        # the two updates alone, on a fixed gradient and states of their own
        k_f, k_t = MaskOptimizer(m, b, undirected="mean"), TorchUpdate(m, b, undirected="mean")
        grad = torch.randn(k_f.M, generator=torch.Generator().manual_seed(3)).to(dev) * 0.05
        terms = torch.zeros(k_f.B, 2, dtype=torch.float64, device=dev)
        fns = [fused.step, plain.step, lambda: saliency(m, b, undirected="mean"), lambda: k_f._kernel(7, grad, terms),
               lambda: k_t._kernel(7, grad, terms), lambda: learn_mask(m, b, undirected="mean", steps=a.steps),
               lambda: occlusion(m, b, undirected="mean"), lambda: shapley(m, b, undirected="mean", perms=8)]
        ts, ss = alternate(fns, [a.iters, a.iters, a.iters, a.iters * 5, a.iters * 5, few, few, few], a.repeats)
        # the two optimisers ran the same number of steps from the same state: their logits may differ by rounding only
        drift = (fused.theta - plain.theta).abs().max().item()
        keys = ("step_ms", "torch_step_ms", "saliency_ms", "update_ms", "torch_update_ms", "learn_mask_ms", "occlusion_ms", "shapley8_ms")
        out[name] = dict(zip(keys, ts), spread_ms=ss, steps_run=fused.t, max_theta_diff=drift)
        print("%-10s step %7.3f  torch step %7.3f  saliency %7.3f  update alone %7.4f  torch update alone %7.4f  learn_mask(%d) %9.3f  "
              "occlusion %9.3f  shapley(8) %9.3f   ms (spreads %s); |theta fused - torch| %.2g after %d steps"
              % (name, ts[0], ts[1], ts[2], ts[3], ts[4], a.steps, ts[5], ts[6], ts[7], " ".join("%.3f" % s for s in ss), drift, fused.t),
              flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

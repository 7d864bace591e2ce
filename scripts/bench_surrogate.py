"""Two measurements of the surrogate attributions on the GPU (nothing is promised in advance; INTEGRATION.md section 20 records
what came out).

1. ms and peak allocated bytes of ``cal_amd.surrogate.surrogate_fit`` (KernelSHAP's constrained fit) beside the batched torch fp64
   spelling -- the padded design matrix [B, S, n] gathered from the keys, ``Z^T Z`` by ``bmm``, ``cholesky_ex``, ``cholesky_solve``
   of both right-hand sides, the constraint -- on the same device in the same process, alternating the two, at B = 128 graphs
   with n = 45 players and S = 256 samples, and with n = 127 and S = 512; and whether two runs of each give the same bits.
   Times are device-synchronised host clocks over ``--iters`` calls after warm-up; both leave their results on the device.
2. The mean absolute error of ``kernel_shap`` and of ``shapley`` against a converged ``shapley`` (``--orders`` orders) on a small
   batch of SPMotif graphs and a briefly trained model, at equal replica counts (``perms`` orders of n replicas against
   ``samples = perms x n_max``).

    python scripts/bench_surrogate.py [--iters 50] [--rounds 3] [--orders 256]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def paired_inputs(B, n, S, dev, seed=0):
    """B graphs of n players, S paired samples each, a smooth game: the tensors ``surrogate_fit`` takes."""
    g = torch.Generator().manual_seed(seed)
    D = S // 2
    key = torch.stack([torch.cat([torch.randperm(n, generator=g) for _ in range(B)]) for _ in range(D)]).to(torch.int32)
    k = torch.arange(1, n, dtype=torch.float64)
    size = 1 + torch.multinomial(((n - 1) / (k * (n - k))).expand(B, -1), D, replacement=True, generator=g)      # [B, D]
    rep_row = torch.arange(D).repeat_interleave(2).repeat(B)
    rep_thresh = size.repeat_interleave(2, dim=1).reshape(-1)
    rep_invert = torch.tensor([0, 1]).repeat(D * B)
    rep_ptr, pl_ptr, pl_elem = torch.arange(B + 1) * S, torch.arange(B + 1) * n, torch.arange(B * n)
    a = torch.randn(B, n, generator=g, dtype=torch.float64) / n ** 0.5
    z = (key.long()[rep_row.view(B, S, 1), pl_elem.view(B, 1, n)] < rep_thresh.view(B, S, 1)) != rep_invert.view(B, S, 1).bool()
    f = lambda zz: 0.5 + 0.4 * torch.tanh((zz.double() * a.view(B, 1, n)).sum(-1) - 0.3)
    value = f(z).reshape(-1)
    ve, vf = f(torch.zeros(B, 1, n)).view(B), f(torch.ones(B, 1, n)).view(B)
    t = lambda x: x.to(dev)
    return dict(key=t(key), rep_ptr=t(rep_ptr), rep_row=t(rep_row), rep_thresh=t(rep_thresh), rep_invert=t(rep_invert), value=t(value),
                pl_ptr=t(pl_ptr), pl_elem=t(pl_elem), v_empty=t(ve), v_full=t(vf)), (B, n, S)


def torch_spelling(i, shape):
    B, n, S = shape
    z = ((i["key"].long()[i["rep_row"].view(B, S, 1), i["pl_elem"].view(B, 1, n)] < i["rep_thresh"].view(B, S, 1))
         != i["rep_invert"].view(B, S, 1).bool()).double()                                           # the design matrix [B, S, n]
    y = i["value"].view(B, S, 1) - i["v_empty"].view(B, 1, 1)
    A = torch.bmm(z.transpose(1, 2), z)
    rhs = torch.cat([torch.bmm(z.transpose(1, 2), y), torch.ones(B, n, 1, dtype=torch.float64, device=z.device)], 2)
    L, info = torch.linalg.cholesky_ex(A)
    xu = torch.cholesky_solve(rhs, L)
    x, u = xu[:, :, 0], xu[:, :, 1]
    delta = (i["v_full"] - i["v_empty"]).view(B, 1)
    return x - u * ((x.sum(1, keepdim=True) - delta) / u.sum(1, keepdim=True)), info


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - base


def fit_bench(a, out):
    from cal_amd.surrogate import surrogate_fit
    for name, n, S in (("n45_s256", 45, 256), ("n127_s512", 127, 512)):
        i, shape = paired_inputs(128, n, S, "cuda")
        pos = ("key", "rep_ptr", "rep_row", "rep_thresh", "value", "pl_ptr", "pl_elem")
        kw = {k: v for k, v in i.items() if k not in pos}
        ours = lambda: surrogate_fit(*[i[k] for k in pos], **kw)
        ref = lambda: torch_spelling(i, shape)
        r1, r2, t1, t2 = ours(), ours(), ref(), ref()
        out[name + "_status_all_fitted"] = bool((r1[3] == 0).all()) and bool((t1[1] == 0).all())
        out[name + "_max_abs_difference"] = float((r1[0].view(128, n) - t1[0]).abs().max())
        out[name + "_fit_bit_equal"] = bool(torch.equal(r1[0].view(torch.int64), r2[0].view(torch.int64)))
        out[name + "_torch_bit_equal"] = bool(torch.equal(t1[0].view(torch.int64), t2[0].view(torch.int64)))
        del r1, r2, t1, t2
        out[name + "_fit_peak_bytes"] = peak_bytes(ours)
        out[name + "_torch_peak_bytes"] = peak_bytes(ref)
        ms = {"fit": [], "torch": []}
        for _ in range(a.rounds):                                        # alternate: the spread is part of the result
            ms["fit"].append(timed(ours, a.iters))
            ms["torch"].append(timed(ref, a.iters))
        out[name + "_fit_ms"] = [round(v, 4) for v in ms["fit"]]
        out[name + "_torch_ms"] = [round(v, 4) for v in ms["torch"]]


def error_bench(a, out):
    import types
    from cal_amd import model as M
    from cal_amd import spmotif
    from cal_amd.coalition import shapley
    from cal_amd.data import Batch
    from cal_amd.engine import StepEngine
    from cal_amd.surrogate import kernel_shap
    args = types.SimpleNamespace(layers=2, hidden=64, with_random=True, without_node_attention=False, without_edge_attention=False,
                                 fc_num="222", cat_or_add="add")
    torch.manual_seed(1)
    m = M.CausalGCN(10, 4, args).to("cuda")
    train = Batch.from_data_list(spmotif.train_mix(64, seed=3)).to("cuda")
    eng = StepEngine(m, lr=1e-2)
    object.__setattr__(m, "_engine", eng)
    m.train()
    for _ in range(30):
        eng.train_step(train, torch.randperm(64).to("cuda"), adam=True)
    b = Batch.from_data_list(spmotif.train_mix(8, seed=11)).to("cuda")
    ref = shapley(m, b, undirected="mean", perms=a.orders, generator=torch.Generator().manual_seed(0))
    players = ~ref.score.isnan()
    nmax = int(max((ref.keys[0, lo:hi].max() + 1 for lo, hi in zip(b.edge_ptr[:-1].tolist(), b.edge_ptr[1:].tolist()))))
    out["error_players_max"], out["error_orders_converged"] = nmax, a.orders
    out["error_score_mean_abs"] = float(ref.score[players].abs().mean())
    out["error_converged_stderr_mean"] = float(ref.stderr[players].mean())
    for perms in (4, 8):
        sh = shapley(m, b, undirected="mean", perms=perms, generator=torch.Generator().manual_seed(1))
        ks = kernel_shap(m, b, undirected="mean", samples=perms * nmax + (perms * nmax) % 2, generator=torch.Generator().manual_seed(1))
        out["error_perms%d_shapley_replicas" % perms], out["error_perms%d_kernel_shap_replicas" % perms] = sh.replicas, ks.replicas
        out["error_perms%d_shapley_mae" % perms] = float((sh.score - ref.score)[players].abs().mean())
        out["error_perms%d_kernel_shap_mae" % perms] = float((ks.score - ref.score)[players].abs().mean())
        out["error_perms%d_kernel_shap_r2_mean" % perms] = float(ks.r2.nanmean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--orders", type=int, default=256)
    a = ap.parse_args()
    out = {}
    fit_bench(a, out)
    error_bench(a, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

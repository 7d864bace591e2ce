"""ms per Lloyd iteration and peak allocated bytes of ``cal_amd.concepts.kmeans`` beside the torch spelling
(``torch.cdist(X, C).argmin(1)``, ``index_add_``, ``bincount``) on the same device in the same process, alternating the two, at
the batch shape (N 4096, H 128, K 16) and the dataset shape (N 2 000 000, H 128, K 16 and K 64).

Rows are seeded planted clusters, the start is the seeded rows of ``kmeans``; a call runs ``--lloyd`` iterations from there (the
data do not converge within them, so no launch of ours returns early -- ``iters_run`` is reported).  Times are device-synchronised
host clocks over ``--iters`` calls after warm-up, divided by the iterations of a call (no read-back: both leave their results on
the device); peak bytes are ``torch.cuda.max_memory_allocated`` above the inputs.  Also recorded: whether two runs of each give the
same bits, and how many rows the two assign alike after one step.

    python scripts/bench_kmeans.py [--iters 20] [--rounds 3] [--lloyd 5]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_spelling(X, C, iters):
    """Lloyd's iterations as the parent commit spells them: the [N, K] matrix, argmin, floating-point atomics for the sums."""
    K = C.size(0)
    for _ in range(iters):
        a = torch.cdist(X, C).argmin(1)
        sums = torch.zeros_like(C).index_add_(0, a, X)
        n = torch.bincount(a, minlength=K)
        C = torch.where(n[:, None] > 0, sums / n.clamp(min=1)[:, None], C)
    return C, a


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--lloyd", type=int, default=5)
    a = ap.parse_args()
    from cal_amd import _lib
    from cal_amd.concepts import kmeans, seed_rows
    dev = "cuda"
    H = 128
    out = {"H": H, "lloyd": a.lloyd}
    for name, N, K in (("batch_k16", 4096, 16), ("dataset_k16", 2_000_000, 16), ("dataset_k64", 2_000_000, 64)):
        g = torch.Generator(device=dev).manual_seed(0)
        centres = torch.randn(K, H, generator=g, device=dev)
        X = (centres[torch.randint(0, K, (N,), generator=g, device=dev)] + torch.randn(N, H, generator=g, device=dev)).contiguous()
        C0 = X[torch.tensor(seed_rows(N, K, 0), device=dev)].contiguous()
        ours = lambda: kmeans(X, K, iters=a.lloyd, init=C0)
        ref = lambda: torch_spelling(X, C0, a.lloyd)
        r1, r2 = ours(), ours()
        t1, t2 = ref(), ref()
        out[name + "_iters_run"] = int(r1.iters_run)
        out[name + "_kmeans_bit_equal"] = bool(torch.equal(r1.centroids.view(torch.int32), r2.centroids.view(torch.int32)))
        out[name + "_torch_bit_equal"] = bool(torch.equal(t1[0].view(torch.int32), t2[0].view(torch.int32)))
        step_a = kmeans(X, K, iters=1, init=C0).assign.long()
        out[name + "_step_agreement"] = float((step_a == torch.cdist(X, C0).argmin(1)).float().mean())
        out[name + "_ws_bytes"] = _lib.query("cal_kmeans_ws", N, K, H, 0)
        out[name + "_pairs_bytes"] = N * K * 4
        del r1, r2, t1, t2, step_a
        out[name + "_kmeans_peak_bytes"] = peak_bytes(ours)
        out[name + "_torch_peak_bytes"] = peak_bytes(ref)
        iters = a.iters if N > 100_000 else a.iters * 10
        ms = {"kmeans": [], "torch": []}
        for _ in range(a.rounds):                                        # alternate: the spread is part of the result
            ms["kmeans"].append(timed(ours, iters) / a.lloyd)
            ms["torch"].append(timed(ref, iters) / a.lloyd)
        out[name + "_kmeans_ms_per_iteration"] = [round(v, 4) for v in ms["kmeans"]]
        out[name + "_torch_ms_per_iteration"] = [round(v, 4) for v in ms["torch"]]
        del X
    print(json.dumps(out))


if __name__ == "__main__":
    main()

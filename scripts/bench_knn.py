"""ms per call and peak allocated bytes of ``cal_amd.neighbors.knn`` beside ``torch.cdist`` + ``torch.topk`` on the same device in
the same process, alternating the two, at the batch shape (nq 128, M 8000, H 128, k 10) and the dataset shape (nq = M = 8000).

Rows are seeded ``|N(0, 1)|``; times are device-synchronised host clocks over ``--iters`` calls after warm-up (no read-back:
both leave their results on the device); peak bytes are ``torch.cuda.max_memory_allocated`` above the inputs.  The neighbour
sets of the two are compared on the way.

    python scripts/bench_knn.py [--iters 200] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_spelling(Q, X, k):
    """The [nq, M] matrix, then the k smallest of every row (ties in no defined order)."""
    d = torch.cdist(Q, X)
    return d.topk(k, dim=1, largest=False)


def timed(fn, iters):
    for _ in range(10):
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
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    from cal_amd import _lib
    from cal_amd.neighbors import knn
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    H, k = 128, 10
    X = torch.randn(8000, H, generator=g).abs().to(dev)
    out = {"H": H, "k": k}
    for name, nq in (("batch", 128), ("dataset", 8000)):
        Q = X[:nq].contiguous()
        ours = lambda: knn(Q, X, k)
        ref = lambda: torch_spelling(Q, X, k)
        r, t = ours(), ref()
        same = (r.idx.long().sort(1).values == t.indices.sort(1).values).float().mean()
        out[name + "_neighbour_agreement"] = float(same)
        out[name + "_ws_bytes"] = _lib.query("cal_knn_ws", nq, 8000, k, 0)
        out[name + "_pairs_bytes"] = nq * 8000 * 4
        out[name + "_knn_peak_bytes"] = peak_bytes(ours)
        out[name + "_torch_peak_bytes"] = peak_bytes(ref)
        ms = {"knn": [], "torch": []}
        for _ in range(a.rounds):                                        # alternate: the spread is part of the result
            ms["knn"].append(timed(ours, a.iters))
            ms["torch"].append(timed(ref, a.iters))
        out[name + "_knn_ms"] = [round(v, 4) for v in ms["knn"]]
        out[name + "_torch_ms"] = [round(v, 4) for v in ms["torch"]]
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Float64 restatement of cal_knn (include/cal_hip.h): both metrics, the key order, skip, k', the votes, the tolerance of a pair and
the closed rank positions; the contract every implementation is held to; the case table tests/test_knn.py (host twin) and
tests/test_gpu_knn.py (HIP) share; and the probe's counts in plain Python."""
import functools

import numpy as np
import torch

INF = float("inf")


def gamma(H):
    """Forward error bound of an fp32 dot product of length H under any summation order, times the factor 2 in front of it, plus
    the handful of roundings around it."""
    return (H + 8) * 2.0 ** -24


def pair_distances(Q, X, metric):
    """(d64 [nq, M], tol [nq, M]): the fp64 distance of every pair (a non-finite one: +inf) and its tolerance."""
    Q, X = np.asarray(Q, np.float64), np.asarray(X, np.float64)
    qn, xn = (Q * Q).sum(1)[:, None], (X * X).sum(1)[None, :]
    with np.errstate(all="ignore"):
        dot = Q @ X.T
        if metric == "l2":
            d = np.maximum(qn + xn - 2.0 * dot, 0.0)
            tol = gamma(Q.shape[1]) * (qn + xn)
        else:
            d = np.maximum(1.0 - dot / (np.sqrt(qn) * np.sqrt(xn)), 0.0)
            d = np.where((qn == 0) | (xn == 0), 1.0, d)
            tol = np.full(d.shape, gamma(Q.shape[1]))
    bad = ~np.isfinite(d)
    return np.where(bad, INF, d), np.where(bad | ~np.isfinite(tol), 0.0, tol)


def oracle(Q, X, k, metric="l2", skip=None, labels=None, C=0):
    """dict: idx [nq, k] (-1 tail), dist [nq, k] fp64 (+inf tail), kk [nq], votes [nq, C], closed [nq, k] bool, and d64, tol,
    elig [nq, M].  Order: fp64 distance, the lower row on equal distances."""
    nq, M = len(Q), len(X)
    d64, tol = pair_distances(Q, X, metric)
    elig = np.ones((nq, M), bool)
    if skip is not None:
        for q, s in enumerate(np.asarray(skip)):
            if 0 <= s < M:
                elig[q, s] = False
    idx = np.full((nq, k), -1, np.int64)
    dist = np.full((nq, k), INF)
    closed = np.zeros((nq, k), bool)
    votes = np.zeros((nq, C), np.int64)
    kk = np.minimum(k, elig.sum(1))
    for q in range(nq):
        rows = np.flatnonzero(elig[q])
        order = rows[np.argsort(d64[q, rows], kind="stable")]
        n = int(kk[q])
        idx[q, :n], dist[q, :n] = order[:n], d64[q, order[:n]]
        ds, ts = d64[q, order[:n + 1]], tol[q, order[:n + 1]]
        with np.errstate(invalid="ignore"):
            gap_ok = (ds[1:] - ds[:-1]) > (ts[1:] + ts[:-1])          # gap between sorted positions p and p + 1
        for p in range(n):
            lo = p == 0 or gap_ok[p - 1]
            hi = p + 1 >= len(order) or gap_ok[p]
            closed[q, p] = lo and hi and np.isfinite(ds[p])
        if labels is not None:
            for j in order[:n]:
                if 0 <= labels[j] < C:
                    votes[q, labels[j]] += 1
    return dict(idx=idx, dist=dist, kk=kk, votes=votes, closed=closed, d64=d64, tol=tol, elig=elig)


def check_contract(idx, dist, votes, o, k, labels=None, C=0, items=(1, 2, 3, 4, 5, 6)):
    """Assert the six items of the contract for a result (idx int [nq, k], dist fp32 [nq, k], votes [nq, C] or None)."""
    idx, dist = np.asarray(idx, np.int64), np.asarray(dist, np.float32)
    nq, M = o["d64"].shape
    assert idx.shape == (nq, k) and dist.shape == (nq, k)
    for q in range(nq):
        n = int(o["kk"][q])
        got = idx[q, :n]
        if 1 in items:
            assert (got >= 0).all() and (got < M).all(), ("range", q)
            assert len(set(got.tolist())) == n and o["elig"][q, got].all(), ("distinct / eligible", q)
            assert (idx[q, n:] == -1).all() and np.isposinf(dist[q, n:]).all(), ("tail", q)
        d, t = o["d64"][q, got], o["tol"][q, got]
        if 2 in items:
            same_inf = np.isposinf(d) & np.isposinf(dist[q, :n])
            with np.errstate(invalid="ignore"):
                assert (same_inf | (np.abs(dist[q, :n].astype(np.float64) - d) <= t)).all(), ("distance", q)
        if 3 in items:
            assert not np.signbit(dist[q, :n]).any(), ("sign", q)
            keys = (dist[q, :n].view(np.uint32).astype(np.uint64) << np.uint64(32)) | got.astype(np.uint64)
            assert (keys[1:] > keys[:-1]).all(), ("keys ascending", q)
        if 4 in items and n:
            out = o["elig"][q].copy()
            out[got] = False
            with np.errstate(invalid="ignore"):
                nearer = o["d64"][q] < d[-1] - (o["tol"][q] + t[-1])
            assert not (out & nearer).any(), ("a nearer row was left out", q)
        if 5 in items:
            c = o["closed"][q, :n]
            assert (got[c] == o["idx"][q, :n][c]).all(), ("closed positions", q)
        if 6 in items and votes is not None:
            want = np.zeros(C, np.int64)
            for j in got:
                if 0 <= labels[j] < C:
                    want[labels[j]] += 1
            assert (np.asarray(votes)[q] == want).all(), ("votes", q)


# ---- the case table -------------------------------------------------------------------------------------------------------------
def _c(nq, M, H, k, metric="l2", skip=None, C=0, chunk=0, special=None, items=(1, 2, 3, 4, 5, 6)):
    return dict(nq=nq, M=M, H=H, k=k, metric=metric, skip=skip, C=C, chunk=chunk, special=special, items=items)


CASES = [
    _c(1, 1, 1, 1),
    _c(31, 4, 3, 5, C=2),                                             # M = k - 1
    _c(32, 33, 10, 5, "cosine", skip="self", C=2),
    _c(33, 127, 64, 5, C=4, special="label"),                         # a label outside [0, C)
    _c(65, 129, 128, 1, "cosine"),
    _c(33, 129, 129, 5, skip="outside"),
    _c(31, 1000, 10, 5, skip="self", C=4, chunk=32),                  # 32 chunks, the merge, a short last chunk
    _c(32, 1000, 64, 64, "cosine", chunk=32),
    _c(65, 1000, 256, 5),
    _c(1, 1000, 3, 64, "cosine"),
    _c(33, 63, 256, 64, "cosine", C=64),                              # M = k - 1 at the limits
    _c(1, 129, 256, 64, C=64, special="label"),
    _c(32, 127, 1, 5),
    _c(32, 127, 1, 5, "cosine", items=(1, 2, 3, 4, 6)),               # positive rows of width 1: every distance ties
    _c(33, 129, 10, 5, "cosine", special="zero"),
    _c(33, 129, 10, 5, special="nan"),
    _c(33, 129, 10, 5, "cosine", special="nan"),
    _c(65, 129, 129, 64, "cosine", C=2),
    _c(1, 33, 128, 1),
    _c(31, 127, 3, 1, "cosine", skip="self"),
    _c(32, 1000, 128, 5, C=64, chunk=64),
    _c(33, 129, 64, 5, skip=None, special="contains"),                # the bank holds the queries, nothing skipped
]
IDS = ["%d-nq%d-M%d-H%d-k%d-%s%s%s%s%s" % (i, c["nq"], c["M"], c["H"], c["k"], c["metric"], "-skip_" + c["skip"] if c["skip"] else "",
                                           "-C%d" % c["C"] if c["C"] else "", "-chunk%d" % c["chunk"] if c["chunk"] else "",
                                           "-" + c["special"] if c["special"] else "") for i, c in enumerate(CASES)]


def _inputs(c, seed):
    g = torch.Generator().manual_seed(seed)
    nq, M, H = c["nq"], c["M"], c["H"]
    Q = torch.randn(nq, H, generator=g).abs()
    X = torch.randn(M, H, generator=g).abs()
    n = min(nq, M)
    if c["skip"] == "self" or c["special"] == "contains":
        X[:n] = Q[:n]
    if c["special"] == "zero":
        X[M // 2] = 0.0
        Q[0] = 0.0
    if c["special"] == "nan":
        X[M // 3, H // 2] = float("nan")
    skip = None
    if c["skip"] == "self":
        skip = torch.arange(nq)
    elif c["skip"] == "outside":
        skip = torch.where(torch.arange(nq) % 2 == 0, torch.full((nq,), -1), torch.full((nq,), M + 5))
    labels = None
    if c["C"]:
        labels = torch.randint(0, c["C"], (M,), generator=g)
        if c["special"] == "label":
            labels[0], labels[M - 1] = c["C"], -1
    return Q, X, skip, labels


@functools.lru_cache(maxsize=None)
def case(i):
    """(Q, X, skip, labels, oracle) of case i: computed once, shared by the tests, never changed."""
    c = CASES[i]
    Q, X, skip, labels = _inputs(c, 100 + i)
    o = oracle(Q.numpy(), X.numpy(), c["k"], c["metric"], None if skip is None else skip.numpy(),
               None if labels is None else labels.numpy(), c["C"])
    return Q, X, skip, labels, o


# exact cases: integer coordinates in [0, 8], H <= 256: every product and sum is below 2^24, exact in any fp32 order
EXACT = [dict(nq=33, M=200, H=10, k=5, skip=None, chunk=0), dict(nq=65, M=129, H=256, k=64, skip="self", chunk=0),
         dict(nq=32, M=1000, H=3, k=8, skip=None, chunk=32), dict(nq=32, M=1000, H=3, k=8, skip="self", chunk=0)]


@functools.lru_cache(maxsize=None)
def exact_case(i):
    c = EXACT[i]
    g = torch.Generator().manual_seed(500 + i)
    Q = torch.randint(0, 9, (c["nq"], c["H"]), generator=g).float()
    X = torch.randint(0, 9, (c["M"], c["H"]), generator=g).float()
    n = min(c["nq"], c["M"])
    X[:n] = Q[:n]                                                     # the bank holds the queries ...
    X[n:n + 20] = X[:20]                                              # ... and several copied rows
    skip = torch.arange(c["nq"]) if c["skip"] == "self" else None
    o = oracle(Q.numpy(), X.numpy(), c["k"], "l2", None if skip is None else skip.numpy())
    return Q, X, skip, o


# ---- the probe in plain Python ---------------------------------------------------------------------------------------------------
def probe_counts(idx, bank_values, query_values):
    """(acc, purity) of one (space, target): idx [nq, k] lists of bank rows (-1: none), values as Python ints."""
    hits = own = total = 0
    for q, row in enumerate(idx):
        nb = [bank_values[j] for j in row if j >= 0]
        total += len(nb)
        own += sum(1 for v in nb if v == query_values[q])
        if nb:
            counts = {}
            for v in nb:
                counts[v] = counts.get(v, 0) + 1
            best = max(counts.values())
            hits += min(v for v, n in counts.items() if n == best) == query_values[q]
    return hits / len(idx), own / total


def probe_chance(bank_values):
    return max(bank_values.count(v) for v in set(bank_values)) / len(bank_values)


def probe_overlap(idx_o, idx_c):
    s = 0.0
    for a, b in zip(idx_o, idx_c):
        a, b = {j for j in a if j >= 0}, {j for j in b if j >= 0}
        s += len(a & b) / len(a | b) if a | b else 0.0
    return s / len(idx_o)

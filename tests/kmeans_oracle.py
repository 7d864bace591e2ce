"""Float64 restatement of one k-means step (cal_kmeans of include/cal_hip.h): the nearest centroid of every row under the order
(distance, the lower centroid), which rows are *closed*, the fp64 mean of any assignment; the contract every implementation is held
to; the case table tests/test_kmeans.py (host twin) and tests/test_gpu_kmeans.py (HIP) share; the exact cases in integer
arithmetic; and the order of sums of rules.hpp in plain numpy (one sequential float32 chain per superblock)."""
import functools

import numpy as np
import torch

from tests.knn_oracle import gamma, pair_distances

INF = float("inf")


def step_oracle(X, C):
    """dict: d64, tol [N, K] (tests/knn_oracle.pair_distances, squared Euclidean); nearest [N] (-1: unassignable, every distance
    non-finite; the lower centroid on equal fp64 distances); closed [N] bool: the gap between the nearest and the second-nearest
    fp64 distance exceeds the sum of their tolerances (K = 1: the distance is finite)."""
    d64, tol = pair_distances(X, C, "l2")
    N, K = d64.shape
    order = np.argsort(d64, axis=1, kind="stable")
    first = order[:, 0]
    rows = np.arange(N)
    ok = np.isfinite(d64[rows, first])
    nearest = np.where(ok, first, -1)
    if K > 1:
        second = order[:, 1]
        with np.errstate(invalid="ignore"):
            closed = ok & ((d64[rows, second] - d64[rows, first]) > (tol[rows, second] + tol[rows, first]))
    else:
        closed = ok.copy()
    return dict(d64=d64, tol=tol, nearest=nearest, closed=closed)


def mean_of(X, assign, K):
    """(mean fp64 [K, H] (nan rows for empty clusters), mean |x| fp64 [K, H], counts [K]) of the rows by an assignment."""
    X = np.asarray(X, np.float64)
    mean, mabs, counts = np.full((K, X.shape[1]), np.nan), np.zeros((K, X.shape[1])), np.zeros(K, np.int64)
    for c in range(K):
        rows = X[assign == c]
        counts[c] = len(rows)
        if len(rows):
            mean[c], mabs[c] = rows.mean(0), np.abs(rows).mean(0)
    return mean, mabs, counts


def check_step(res, X, C, o, items=(1, 2, 3, 4, 5, 6)):
    """Assert the six items of the contract for one step from the centroids C.  res: dict of numpy arrays centroids [K, H] fp32,
    assign [N], counts [K], inertia (float), moved (int)."""
    X, C = np.asarray(X, np.float32), np.asarray(C, np.float32)
    N, K = o["d64"].shape
    a = np.asarray(res["assign"], np.int64)
    rows = np.arange(N)
    assert a.shape == (N,)
    if 1 in items:
        assert ((a >= -1) & (a < K)).all(), "range"
        assert ((a == -1) == (o["nearest"] == -1)).all(), "-1 exactly on the unassignable rows"
    live = a >= 0
    if 2 in items:
        assert (a[o["closed"]] == o["nearest"][o["closed"]]).all(), "closed rows"
    if 3 in items:
        j = rows[live]
        best = o["nearest"][j]
        with np.errstate(invalid="ignore"):
            assert (o["d64"][j, a[j]] <= o["d64"][j, best] + o["tol"][j, a[j]] + o["tol"][j, best]).all(), "a nearer centroid was left out"
    if 4 in items:
        assert np.array_equal(np.asarray(res["counts"], np.int64), np.bincount(a[live], minlength=K)), "counts"
    if 5 in items:
        mean, mabs, counts = mean_of(X, a, K)
        got = np.asarray(res["centroids"], np.float32)
        for c in range(K):
            if counts[c]:
                assert (np.abs(got[c].astype(np.float64) - mean[c]) <= gamma(counts[c] + 2) * mabs[c]).all(), ("centroid", c)
            else:
                assert np.array_equal(got[c].view(np.uint32), C[c].view(np.uint32)), ("an empty cluster keeps its bits", c)
    if 6 in items:
        want, slack = o["d64"][rows[live], a[live]].sum(), o["tol"][rows[live], a[live]].sum()
        assert abs(float(res["inertia"]) - want) <= slack, ("inertia", float(res["inertia"]), want, slack)
        assert int(res["moved"]) == int(live.sum()), "moved[0] is the number of assigned rows"


# ---- the case table -------------------------------------------------------------------------------------------------------------
def _c(N, H, K, kind="planted", span=0, special=None, tie=False):
    return dict(N=N, H=H, K=K, kind=kind, span=span, special=special, tie=tie)


CASES = [
    _c(1, 1, 1, "bank"),
    _c(31, 3, 2),
    _c(129, 1, 5, "bank"),
    _c(127, 64, 33),
    _c(1000, 64, 5),
    _c(1000, 129, 33, "bank"),
    _c(300, 256, 64, "bank"),
    _c(4097, 256, 64),
    _c(127, 10, 5, span=128),                                         # one short superblock
    _c(128, 10, 5, span=128),                                         # one full superblock
    _c(129, 10, 5, "bank", span=128),                                 # a last superblock of one row
    _c(1000, 10, 64, "bank", span=128),                               # eight superblocks, a short last one
    _c(33, 8, 33, "bank", special="k_is_n"),                          # K = N: every row is a centroid
    _c(200, 8, 4, special="twin_centroids", tie=True),                # two identical centroids: the second stays empty
    _c(130, 5, 3, special="identical", tie=True),                     # every row identical: every distance ties
    _c(300, 16, 5, special="copies"),                                 # copied rows
    _c(129, 10, 5, special="nan"),                                    # a row with a NaN
    _c(129, 10, 5, "bank", special="zero"),                           # a zero row
    _c(1000, 10, 5, "bank", span=256, special="nan"),
    _c(300, 192, 5),                                                  # a wide tile: 64 rows of 192 columns
]
IDS = ["%d-N%d-H%d-K%d-%s%s%s" % (i, c["N"], c["H"], c["K"], c["kind"], "-span%d" % c["span"] if c["span"] else "",
                                  "-" + c["special"] if c["special"] else "") for i, c in enumerate(CASES)]


def _inputs(c, seed):
    """(X [N, H], init): init int64 [K] rows (bank cases: the centroids are bank rows) or float32 [K, H] centroids."""
    g = torch.Generator().manual_seed(seed)
    N, H, K = c["N"], c["H"], c["K"]
    if c["kind"] == "planted":
        centres = 4.0 * torch.randn(K, H, generator=g)
        X = centres[torch.randint(0, K, (N,), generator=g)] + 0.5 * torch.randn(N, H, generator=g)
        init = centres + 0.3 * torch.randn(K, H, generator=g)
    else:
        X = torch.randn(N, H, generator=g).abs()
        init = torch.randperm(N, generator=g)[:K].sort().values
    sp = c["special"]
    if sp == "k_is_n":
        init = torch.arange(N)
    if sp == "twin_centroids":
        init[2] = init[1]
    if sp == "identical":
        X[:] = X[0].clone()
        init[:] = init[0].clone()
    if sp == "copies":
        X[50:70] = X[:20]
    if sp == "nan":
        X[N // 3, H // 2] = float("nan")
        if init.dtype == torch.int64:                                # no NaN centroid: the row is not one of the initial rows
            init = torch.tensor([r for r in range(N) if r != N // 3][:K])
    if sp == "zero":
        X[5] = 0.0
    return X, init


def centroids_of(X, init):
    return init if init.dtype == torch.float32 else X[init]


@functools.lru_cache(maxsize=None)
def case(i):
    """(X, init, C, oracle) of case i: computed once, shared by the tests, never changed."""
    X, init = _inputs(CASES[i], 700 + i)
    C = centroids_of(X, init).clone()
    return X, init, C, step_oracle(X.numpy(), C.numpy())


# ---- exact cases: integer coordinates in [0, 8], integer centroids, H <= 256: every product, norm and distance is an integer
# below 2^24 and every cluster sum stays below 2^24 (N <= 1000): exact in fp32 in any order; the mean is one rounded division ------
EXACT = [dict(N=200, H=10, K=5), dict(N=1000, H=3, K=8), dict(N=129, H=256, K=64)]
EXACT_SPANS = (0, 128)


@functools.lru_cache(maxsize=None)
def exact_case(i):
    """(X, C, want): want = assign, counts, inertia (float), centroids fp32 from integer arithmetic."""
    c = EXACT[i]
    g = torch.Generator().manual_seed(900 + i)
    X = torch.randint(0, 9, (c["N"], c["H"]), generator=g).float()
    C = torch.randint(0, 9, (c["K"], c["H"]), generator=g).float()
    C[1] = C[0]                                                       # a twin centroid: stays empty
    X[10:20] = X[:10]                                                 # copied rows
    xi, ci = X.numpy().astype(np.int64), C.numpy().astype(np.int64)
    d = ((xi[:, None, :] - ci[None, :, :]) ** 2).sum(2)
    a = d.argmin(1)                                                   # the first minimum: the lower centroid
    counts = np.bincount(a, minlength=c["K"])
    sums = np.zeros((c["K"], c["H"]), np.int64)
    np.add.at(sums, a, xi)
    assert sums.max() < 2 ** 24 and d.max() < 2 ** 24
    with np.errstate(invalid="ignore", divide="ignore"):
        cen = sums.astype(np.float32) / counts.astype(np.float32)[:, None]
    cen = np.where(counts[:, None] > 0, cen, C.numpy())
    return X, C, dict(assign=a, counts=counts, inertia=float(d[np.arange(len(a)), a].sum()), centroids=cen.astype(np.float32))


# ---- order cases: well-separated clusters of rows with full fp32 mantissas: the assignment is beyond doubt, and the centroids'
# BITS follow from the order of sums alone -------------------------------------------------------------------------------------
ORDER = [dict(N=1000, H=7, K=3, span=128), dict(N=1000, H=7, K=3, span=0), dict(N=700, H=130, K=5, span=256)]


def ordered_means(X, a, C, span):
    """The rule in numpy: per superblock and cluster one sequential float32 chain in ascending row order from +0 (np.cumsum is
    sequential), the superblocks in ascending order, one rounded division; an empty cluster keeps its centroid."""
    X, C = np.asarray(X, np.float32), np.asarray(C, np.float32)
    N, K = len(X), len(C)
    total, counts = None, np.zeros(K, np.int64)
    for s0 in range(0, N, span):
        part = np.zeros_like(C)
        for c in range(K):
            rows = X[s0:s0 + span][a[s0:s0 + span] == c]
            counts[c] += len(rows)
            if len(rows):
                part[c] = np.cumsum(np.concatenate([np.zeros((1, X.shape[1]), np.float32), rows]), axis=0, dtype=np.float32)[-1]
        total = part if total is None else (total + part).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = total / counts.astype(np.float32)[:, None]
    return np.where(counts[:, None] > 0, mean, C).astype(np.float32), counts


def default_span(N):
    """kmeans_span(N, 0) of rules.hpp."""
    pieces = (N + 127) // 128
    return max(1, (pieces + 511) // 512) * 128


@functools.lru_cache(maxsize=None)
def order_case(i):
    c = ORDER[i]
    g = torch.Generator().manual_seed(950 + i)
    centres = 100.0 * torch.eye(c["K"], c["H"])
    lab = torch.randint(0, c["K"], (c["N"],), generator=g)
    X = centres[lab] + torch.randn(c["N"], c["H"], generator=g)
    C = centres + 0.25
    o = step_oracle(X.numpy(), C.numpy())
    assert o["closed"].all() and np.array_equal(o["nearest"], lab.numpy())
    want, counts = ordered_means(X.numpy(), lab.numpy(), C.numpy(), c["span"] or default_span(c["N"]))
    return X, C, lab.numpy(), want, counts

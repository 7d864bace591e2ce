"""The oracle and the case table of cal_surrogate_fit (tests/test_surrogate.py: the host twin; tests/test_gpu_surrogate.py: HIP).

The oracle works from the fp64 inputs as exact rationals.  For d <= 33 everything is ``fractions.Fraction``: the Gram matrix, the
LDL^T pivots (the Cholesky pivot d_j of the rule IS the LDL^T pivot, a rational), the two solves, the constraint, SSR and SST.
Above that the Gram matrix is formed in numpy ``longdouble`` (exact for the table's integer weights; the right-hand side to
2^-64) and solved by a longdouble Cholesky with one step of iterative refinement; ``test_surrogate.py`` ties that path to the
rational one on the small cases.

The bound on phi and phi0 is ``8 d kappa_inf(A) 2^-53 max(|phi*|_inf, |Delta|)`` (mode 1: ``|phi0*|`` in Delta's place): the
standard forward error of a Cholesky solve is d u kappa, the factor 8 is the margin.  kappa is computed per graph.

The bound on r2 follows from SSR and SST.  With e the bound on a coefficient, a fitted value is off by at most
``delta = (n + 1) e + (n + 2) u (max|v| + |phi0*| + sum|phi*|)`` (the coefficients' errors, then the chain of n + 1 additions),
so SSR is off by at most ``dSSR = sum w (2 |r_s| delta + delta^2) + (S + 2) u sum w (|r_s| + delta)^2``; the weighted mean is off
by ``dm = (S + 2) u max|v|``, SST by ``dSST = sum w (2 |v_s - m| dm + dm^2) + (S + 2) u SST``; and
``|r2 - r2*| <= 2 (dSSR + (SSR / SST) dSST) / SST + 4 u (1 + SSR / SST)``, the 2 covering the second-order terms.
"""
import itertools
import math
from fractions import Fraction

import numpy as np
import torch

U = 2.0 ** -53
PIVOT = Fraction(1, 2 ** 30)
EXACT_MAX_D = 33
KAPPA_MAX = 1e6
GPU_MAX_PLAYERS = 127


# ---- graphs and batches ----------------------------------------------------------------------------------------------------------
class G:
    """One graph of a case: ``keys`` int [Kg, m] over its m elements, ``players`` (local elements), the samples (``row``, ``th``,
    ``inv`` or None, ``val``, ``wt`` or None) and ``ve`` / ``vf``."""

    def __init__(self, keys, players, row, th, val, inv=None, wt=None, ve=0.0, vf=0.0):
        self.keys = np.asarray(keys, dtype=np.int64)
        assert self.keys.ndim == 2
        self.players, self.row, self.th = list(players), list(row), list(th)
        self.val = [float(v) for v in val]
        self.inv = None if inv is None else [int(i) for i in inv]
        self.wt = None if wt is None else [float(w) for w in wt]
        self.ve, self.vf = float(ve), float(vf)


def members(keys, players, row, th, inv):
    """bool [S, n]: the membership rule in numpy (a row outside [0, K): every player)."""
    S, n, K = len(row), len(players), keys.shape[0]
    z = np.ones((S, n), dtype=bool)
    for s in range(S):
        if 0 <= row[s] < K:
            z[s] = (keys[row[s], players] < th[s]) != bool(inv[s] if inv is not None else 0)
    return z


def quant(v):
    """Values on a 2^-24 grid: the rationals stay small."""
    return np.round(np.asarray(v, dtype=np.float64) * 2.0 ** 24) / 2.0 ** 24


def game(n, seed):
    """A smooth non-additive game on n players -> f(z [S, n] bool) -> values [S]."""
    a = np.random.default_rng(seed).uniform(-1.0, 1.0, size=max(n, 1)) / math.sqrt(max(n, 1))

    def f(z):
        z = np.asarray(z, dtype=np.float64).reshape(-1, n)
        pair = z[:, 0] * z[:, -1] if n >= 2 else 0.0
        return quant(0.5 + 0.4 * np.tanh(z @ a[:n] * 2.0 - 0.3) + 0.05 * pair)
    return f


def shapley_size(rng, n):
    k = np.arange(1, n)
    p = (n - 1) / (k * (n - k))
    return int(rng.choice(k, p=p / p.sum()))


def paired(n, S, seed, f=None, twins=False, extra=0):
    """A graph of n players under KernelSHAP's paired sampling: S / 2 random orders, a Shapley-kernel size each, the prefix and its
    complement.  ``twins``: every player has two columns with the same key, the even one its representative.  ``extra``:
    elements that are no player (key -1)."""
    rng = np.random.default_rng(seed)
    f = f or game(n, seed + 1000)
    D = S // 2
    pos = np.stack([rng.permutation(n) for _ in range(D)]) if D else np.zeros((0, n), np.int64)
    if twins:
        keys = np.repeat(pos, 2, axis=1)
        players = list(range(0, 2 * n, 2))
    else:
        keys, players = pos, list(range(n))
    if extra:
        keys = np.concatenate([keys, -np.ones((D, extra), np.int64)], axis=1)
    row, th, inv = [], [], []
    for q in range(D):
        k = shapley_size(rng, n)
        row += [q, q]
        th += [k, k]
        inv += [0, 1]
    z = members(keys, players, row, th, inv)
    return G(keys, players, row, th, f(z), inv=inv, ve=f(np.zeros((1, n)))[0], vf=f(np.ones((1, n)))[0])


def binomial(n, S, seed, f=None, keep=0.5, width=0.75):
    """A graph of n players under LIME's sampling: S orders, Binomial sizes, locality weights."""
    rng = np.random.default_rng(seed)
    f = f or game(n, seed + 1000)
    keys = np.stack([rng.permutation(n) for _ in range(S)]) if S else np.zeros((0, n), np.int64)
    th = [int(rng.binomial(n, keep)) for _ in range(S)]
    row = list(range(S))
    z = members(keys, list(range(n)), row, th, None)
    wt = [math.exp(-((1.0 - k / n) ** 2) / width ** 2) for k in th]
    return G(keys, list(range(n)), row, th, f(z), wt=wt)


def explicit(n, sets, f, wt=None, ve=None, vf=None):
    """A graph whose samples are the given subsets of its n players: one key row each (0 for members, 1 else), threshold 1."""
    keys = np.array([[0 if p in s else 1 for p in range(n)] for s in sets], dtype=np.int64).reshape(len(sets), n)
    z = np.array([[p in s for p in range(n)] for s in sets], dtype=bool).reshape(len(sets), n)
    return G(keys, list(range(n)), list(range(len(sets))), [1] * len(sets), f(z) if len(sets) else [], wt=wt,
             ve=f(np.zeros((1, n)))[0] if ve is None else ve, vf=f(np.ones((1, n)))[0] if vf is None else vf)


def batch(name, graphs, mode, ridge=0.0, tol=True, status=None, gpu_status=None):
    """The tensors ``surrogate_fit`` takes.  ``status``: what the table expects (None: all fitted); ``gpu_status``: where the device
    library's limit makes it differ.  ``tol``: phi / phi0 / r2 are held to the oracle's bounds (and kappa <= KAPPA_MAX)."""
    K = max([g.keys.shape[0] for g in graphs] + [1])
    M = sum(g.keys.shape[1] for g in graphs)
    key = np.zeros((K, M), dtype=np.int32)
    rep_ptr, pl_ptr, row, th, inv, val, wt, pel, ve, vf = [0], [0], [], [], [], [], [], [], [], []
    col = 0
    any_inv, any_wt = any(g.inv is not None for g in graphs), any(g.wt is not None for g in graphs)
    for g in graphs:
        m = g.keys.shape[1]
        key[:g.keys.shape[0], col:col + m] = g.keys
        pel += [col + p for p in g.players]
        row += g.row
        th += g.th
        inv += g.inv if g.inv is not None else [0] * len(g.row)
        wt += g.wt if g.wt is not None else [1.0] * len(g.row)
        val += g.val
        ve.append(g.ve)
        vf.append(g.vf)
        rep_ptr.append(len(row))
        pl_ptr.append(len(pel))
        col += m
    i64 = lambda v: torch.tensor(v, dtype=torch.long)
    f64 = lambda v: torch.tensor(v, dtype=torch.float64)
    B = len(graphs)
    return {"name": name, "graphs": graphs, "mode": mode, "ridge": float(ridge), "tol": tol,
            "status": [0] * B if status is None else list(status),
            "gpu_status": None if gpu_status is None else list(gpu_status),
            "key": torch.from_numpy(key), "rep_ptr": i64(rep_ptr), "rep_row": i64(row), "rep_thresh": i64(th),
            "rep_invert": i64(inv) if any_inv else None, "value": f64(val), "weight": f64(wt) if any_wt else None,
            "pl_ptr": i64(pl_ptr), "pl_elem": i64(pel), "v_empty": f64(ve), "v_full": f64(vf)}


def fit_args(c, dev="cpu"):
    """-> (args, kwargs) of ``surrogate_fit`` for case ``c`` on ``dev``."""
    t = lambda x: None if x is None else x.to(dev)
    args = [t(c[k]) for k in ("key", "rep_ptr", "rep_row", "rep_thresh", "value", "pl_ptr", "pl_elem")]
    kw = {"rep_invert": t(c["rep_invert"]), "weight": t(c["weight"]), "mode": "lime" if c["mode"] else "shap", "ridge": c["ridge"]}
    if c["mode"] == 0:
        kw["v_empty"], kw["v_full"] = t(c["v_empty"]), t(c["v_full"])
    return args, kw


# ---- the table -------------------------------------------------------------------------------------------------------------------
def linear_game(n, c, seed):
    a = quant(np.random.default_rng(seed).uniform(-0.25, 0.25, size=n))

    def f(z):
        return c + np.asarray(z, dtype=np.float64).reshape(-1, n) @ a
    f.a = a
    return f


def shapley_weights(n):
    return {k: (n - 1) / (math.comb(n, k) * k * (n - k)) for k in range(1, n)}


def table_game5():
    """A game on 5 players given as a table over the 32 subsets."""
    tab = quant(np.random.default_rng(55).uniform(0.0, 1.0, size=32))

    def f(z):
        z = np.asarray(z).reshape(-1, 5).astype(np.int64)
        return tab[(z << np.arange(5)).sum(1)]
    f.tab = tab
    return f


def brute_force_shapley5(tab):
    """Shapley values of the table game over all 120 orders, in Fractions."""
    phi = [Fraction(0)] * 5
    for order in itertools.permutations(range(5)):
        m = 0
        for p in order:
            phi[p] += Fraction(float(tab[m | (1 << p)])) - Fraction(float(tab[m]))
            m |= 1 << p
    return [x / 120 for x in phi]


def _cases():
    C = []
    f1 = game(1, 7)
    one = explicit(1, [], f1)
    C.append(batch("n1-defined", [one, G(np.zeros((1, 1)), [0], [0, 0], [1, 0], [f1([[1]])[0], f1([[0]])[0]], ve=one.ve, vf=one.vf)], 0))
    f2, f3 = game(2, 8), game(3, 9)
    C.append(batch("n2-minimal", [explicit(2, [{0}, {1}], f2)], 0))
    C.append(batch("n3-minimal", [explicit(3, [{0}, {1, 2}, {1}, {0, 2}], f3)], 0))
    C.append(batch("n2-lime-minimal", [explicit(2, [{0}, {1}, {0, 1}], f2)], 1))
    f5 = table_game5()
    sets = [set(s) for k in range(1, 5) for s in itertools.combinations(range(5), k)]
    w5 = shapley_weights(5)
    C.append(batch("enum5-shapley", [explicit(5, sets, f5, wt=[w5[len(s)] for s in sets])], 0))
    lin = linear_game(6, 0.375, 21)
    C.append(batch("linear-shap", [paired(6, 24, 31, f=lin)], 0))
    C.append(batch("linear-lime", [binomial(6, 24, 32, f=lin)], 1, ridge=0.0))
    for n in (63, 64, 65):
        C.append(batch("lanes-n%d" % n, [paired(n, 4 * n, 100 + n)], 0))
    C.append(batch("lanes-lime-n63-n64", [binomial(63, 256, 163), binomial(64, 260, 164)], 1, ridge=1e-3))
    C.append(batch("limit-n127-shap", [paired(127, 512, 127)], 0))
    C.append(batch("limit-n127-lime", [binomial(127, 600, 128)], 1, ridge=1e-3))
    C.append(batch("over-n128", [paired(128, 512, 129), paired(5, 20, 130)], 0, gpu_status=[2, 0]))
    C.append(batch("undirected-twins", [paired(7, 28, 41, twins=True, extra=3), paired(4, 16, 42, twins=True)], 0))
    # sample flags: no invert at all, all zero, mixed, a control row (outside [0, K): every player, whatever invert says)
    g = paired(6, 24, 51)
    plain = G(g.keys, g.players, g.row, g.th, game(6, 1051)(members(g.keys, g.players, g.row, g.th, None)), ve=g.ve, vf=g.vf)
    C.append(batch("invert-null", [plain], 0))
    C.append(batch("invert-zeros", [G(plain.keys, plain.players, plain.row, plain.th, plain.val, inv=[0] * 24, ve=g.ve, vf=g.vf)], 0))
    C.append(batch("invert-mixed", [g], 0))
    ctl = G(g.keys, g.players, g.row + [-1, 99], g.th + [0, 0], g.val + [g.vf, g.vf], inv=g.inv + [0, 1], ve=g.ve, vf=g.vf)
    C.append(batch("control-rows", [ctl], 0))
    C.append(batch("weights-ones", [G(g.keys, g.players, g.row, g.th, g.val, inv=g.inv, wt=[1.0] * 24, ve=g.ve, vf=g.vf)], 0))
    # the pivot rule is relative to A_jj: weights of 2^-40 leave a full-rank system full rank
    C.append(batch("tiny-weights", [G(g.keys, g.players, g.row, g.th, g.val, inv=g.inv, wt=[2.0 ** -40] * 24, ve=g.ve, vf=g.vf)], 0))
    # ridge: S < n is deficient, ridge cures it; in mode 1 the intercept carries none
    few = paired(8, 6, 61)
    C.append(batch("ridge-cures", [few], 0, ridge=0.25))
    C.append(batch("ridge-lime", [binomial(5, 12, 62)], 1, ridge=0.5))
    # rank-deficient inputs
    f6 = game(6, 71)
    dup = explicit(6, [{0}, {1, 2}] * 6, f6)
    C.append(batch("deficient", [explicit(6, [], f6), paired(8, 6, 72), dup, paired(9, 2 * 8 - 2, 73)], 0, tol=False, status=[1, 1, 1, 1]))
    C.append(batch("deficient-lime", [binomial(6, 4, 74), binomial(3, 0, 75)], 1, tol=False, status=[1, 1]))
    # bad values: that graph only
    good = lambda s: paired(5, 20, s)
    nanv, negw, infw = good(81), good(82), good(83)
    nanv.val[3] = float("nan")
    negw.wt = [1.0] * 20
    negw.wt[7] = -0.5
    infw.wt = [1.0] * 20
    infw.wt[19] = float("inf")
    C.append(batch("bad-values", [good(80), nanv, negw, good(84), infw], 0, status=[0, 3, 3, 0, 3]))
    # batch edges: a graph without a player, a graph without a replica between two that have them
    nop = G(np.full((2, 3), -1), [], [0, 1], [0, 1], [0.5, 0.25], ve=0.5, vf=0.5)
    C.append(batch("no-player-no-replica", [paired(4, 16, 91), nop, explicit(3, [], f3), paired(3, 12, 92)], 0, status=[0, 0, 1, 0]))
    C.append(batch("no-player-lime", [nop, binomial(4, 20, 93)], 1))
    return C


CASES = _cases()
IDS = [c["name"] for c in CASES]


def case(name):
    return CASES[IDS.index(name)]


def single(c, g):
    """Graph g of case c as a batch of its own."""
    return batch(c["name"] + "-alone", [c["graphs"][g]], c["mode"], c["ridge"])


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
def _design(c, g):
    """-> (z bool [S, d] with the intercept column, w [S], v [S], n, d) of graph g."""
    gr, mode = c["graphs"][g], c["mode"]
    n, S = len(gr.players), len(gr.row)
    z = members(gr.keys, gr.players, gr.row, gr.th, gr.inv)
    if mode == 1:
        z = np.concatenate([z, np.ones((S, 1), dtype=bool)], axis=1)
    w = np.array(gr.wt if gr.wt is not None else [1.0] * S, dtype=np.float64)
    return z, w, np.array(gr.val, dtype=np.float64), n, n + mode


def _status3(c, g):
    gr = c["graphs"][g]
    w = gr.wt if gr.wt is not None else []
    bad = any(not math.isfinite(v) for v in gr.val) or any(not math.isfinite(x) or x < 0 for x in w)
    return bad or (c["mode"] == 0 and not (math.isfinite(gr.ve) and math.isfinite(gr.vf)))


def _exact(c, g):
    """The rational path -> dict(status, phi [n] Fractions, phi0, r2 (Fraction or None), A as floats)."""
    gr, mode, ridge = c["graphs"][g], c["mode"], Fraction(c["ridge"])
    z, w, v, n, d = _design(c, g)
    S = len(v)
    wq, vq = [Fraction(float(x)) for x in w], [Fraction(float(x)) for x in v]
    ve, vf = Fraction(gr.ve), Fraction(gr.vf)
    y = [x - ve for x in vq] if mode == 0 else vq
    A = [[sum((wq[s] for s in range(S) if z[s, i] and z[s, j]), Fraction(0)) for j in range(d)] for i in range(d)]
    for i in range(n):
        A[i][i] += ridge
    b = [sum((wq[s] * y[s] for s in range(S) if z[s, i]), Fraction(0)) for i in range(d)]
    out = {"A": np.array([[float(x) for x in r] for r in A], dtype=np.float64).reshape(d, d), "n": n, "d": d}
    phi, phi0 = [Fraction(0)] * n, ve
    deficient = False
    if mode == 0 and n == 1:
        phi = [vf - ve]
    elif d > 0:
        L = [[Fraction(0)] * d for _ in range(d)]
        piv = [Fraction(0)] * d
        for j in range(d):
            piv[j] = A[j][j] - sum((L[j][k] * L[j][k] * piv[k] for k in range(j)), Fraction(0))
            if not piv[j] > A[j][j] * PIVOT:
                deficient = True
                break
            for i in range(j + 1, d):
                L[i][j] = (A[i][j] - sum((L[i][k] * L[j][k] * piv[k] for k in range(j)), Fraction(0))) / piv[j]

        def solve(r):
            t = list(r)
            for i in range(d):
                t[i] -= sum((L[i][k] * t[k] for k in range(i)), Fraction(0))
            t = [t[i] / piv[i] for i in range(d)]
            for i in range(d - 1, -1, -1):
                t[i] -= sum((L[k][i] * t[k] for k in range(i + 1, d)), Fraction(0))
            return t
        if not deficient:
            x = solve(b)
            if mode == 0:
                u = solve([Fraction(1)] * d)
                cc = (sum(x) - (vf - ve)) / sum(u)
                phi = [x[i] - u[i] * cc for i in range(n)]
            else:
                phi, phi0 = x[:n], x[n]
    if deficient and n > 0:
        out["status"] = 1
        return out
    out["status"] = 0
    out["phi"], out["phi0"] = phi, (None if deficient else phi0)
    out["r2"] = None
    sw = sum(wq, Fraction(0))
    if sw > 0 and not deficient:
        mean = sum((wq[s] * vq[s] for s in range(S)), Fraction(0)) / sw
        res = [vq[s] - phi0 - sum((phi[p] for p in range(n) if z[s, p]), Fraction(0)) for s in range(S)]
        ssr = sum((wq[s] * res[s] ** 2 for s in range(S)), Fraction(0))
        sst = sum((wq[s] * (vq[s] - mean) ** 2 for s in range(S)), Fraction(0))
        out["ssr"], out["sst"], out["res"], out["mean"] = ssr, sst, res, mean
        if sst > 0:
            out["r2"] = 1 - ssr / sst
    return out


def _chol_ld(A):
    """Left-looking Cholesky in longdouble -> (L, deficient)."""
    d = A.shape[0]
    L = np.zeros_like(A)
    for j in range(d):
        dj = A[j, j] - L[j, :j] @ L[j, :j]
        if not dj > A[j, j] * np.longdouble(2.0 ** -30):
            return L, True
        L[j, j] = np.sqrt(dj)
        if j + 1 < d:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L, False


def _solve_ld(L, A, r):
    def once(t):
        t = t.copy()
        d = len(t)
        for i in range(d):
            t[i] = (t[i] - L[i, :i] @ t[:i]) / L[i, i]
        for i in range(d - 1, -1, -1):
            t[i] = (t[i] - L[i + 1:, i] @ t[i + 1:]) / L[i, i]
        return t
    x = once(r)
    return x + once(r - A @ x)                                   # one step of refinement


def _longdouble(c, g):
    """The longdouble path: the same dict with longdouble entries."""
    gr, mode = c["graphs"][g], c["mode"]
    z, w, v, n, d = _design(c, g)
    ld = np.longdouble
    zl, wl, vl = z.astype(ld), w.astype(ld), v.astype(ld)
    ve, vf = ld(gr.ve), ld(gr.vf)
    y = vl - ve if mode == 0 else vl
    A = (zl * wl[:, None]).T @ zl if len(v) else np.zeros((d, d), dtype=ld)
    A[np.arange(n), np.arange(n)] += ld(c["ridge"])
    b = zl.T @ (wl * y) if len(v) else np.zeros(d, dtype=ld)
    out = {"A": A.astype(np.float64), "n": n, "d": d}
    phi, phi0, deficient = np.zeros(n, dtype=ld), ve, False
    if mode == 0 and n == 1:
        phi = np.array([vf - ve], dtype=ld)
    elif d > 0:
        L, deficient = _chol_ld(A)
        if not deficient:
            x = _solve_ld(L, A, b)
            if mode == 0:
                u = _solve_ld(L, A, np.ones(d, dtype=ld))
                phi = x - u * ((x.sum() - (vf - ve)) / u.sum())
            else:
                phi, phi0 = x[:n], x[n]
    if deficient and n > 0:
        out["status"] = 1
        return out
    out["status"], out["phi"], out["phi0"], out["r2"] = 0, phi, (None if deficient else phi0), None
    sw = wl.sum() if len(v) else ld(0)
    if sw > 0 and not deficient:
        mean = (wl * vl).sum() / sw
        res = vl - phi0 - zl[:, :n] @ phi
        out["ssr"], out["sst"], out["res"], out["mean"] = (wl * res * res).sum(), (wl * (vl - mean) ** 2).sum(), res, mean
        if out["sst"] > 0:
            out["r2"] = 1 - out["ssr"] / out["sst"]
    return out


def oracle_graph(c, g, path=None, limit=None):
    """The oracle for graph g of case c: ``status``; for status 0 ``phi`` (float64 [n]), ``phi0``, ``r2`` (NaN where undefined) with
    the bounds ``tol_phi`` / ``tol_r2`` and ``kappa``.  ``path``: "exact" / "longdouble" (default by d); ``limit``: the player
    limit of the library under test."""
    gr = c["graphs"][g]
    n = len(gr.players)
    if limit is not None and n > limit:
        return {"status": 2, "n": n}
    if _status3(c, g):
        return {"status": 3, "n": n}
    d = n + c["mode"]
    path = path or ("exact" if d <= EXACT_MAX_D else "longdouble")
    o = _exact(c, g) if path == "exact" else _longdouble(c, g)
    if o["status"]:
        return o
    f = lambda x: float("nan") if x is None else float(x)
    o["phi"] = np.array([f(x) for x in o["phi"]], dtype=np.float64)
    o["phi0"], o["r2"] = f(o["phi0"]), f(o["r2"])
    solved = d > 0 and not (c["mode"] == 0 and n == 1) and not math.isnan(o["phi0"])
    o["kappa"] = float(np.linalg.cond(o["A"], np.inf)) if solved else 1.0
    delta = abs(gr.vf - gr.ve) if c["mode"] == 0 else abs(o["phi0"]) if not math.isnan(o["phi0"]) else 0.0
    scale = max([abs(x) for x in o["phi"]] + [delta])
    o["tol_phi"] = 8.0 * max(d, 1) * o["kappa"] * U * scale
    o["tol_r2"] = float("nan")
    if "sst" in o and float(o["sst"]) > 0:
        S = len(gr.val)
        w = np.array(gr.wt if gr.wt is not None else [1.0] * S, dtype=np.float64)
        v = np.array(gr.val, dtype=np.float64)
        res = np.array([abs(float(x)) for x in o["res"]], dtype=np.float64)
        ssr, sst, mean = float(o["ssr"]), float(o["sst"]), float(o["mean"])
        vmax = float(np.abs(v).max())
        dl = (n + 1) * o["tol_phi"] + (n + 2) * U * (vmax + abs(o["phi0"]) + float(np.abs(o["phi"]).sum()))
        dssr = float((w * (2 * res * dl + dl * dl)).sum() + (S + 2) * U * (w * (res + dl) ** 2).sum())
        dm = (S + 2) * U * vmax
        dsst = float((w * (2 * np.abs(v - mean) * dm + dm * dm)).sum() + (S + 2) * U * sst)
        o["tol_r2"] = 2.0 * (dssr + (ssr / sst) * dsst) / sst + 4.0 * U * (1.0 + ssr / sst)
    return o


_ORACLE = {}


def oracle(name, limit=None):
    """The oracle of every graph of a case, computed once."""
    k = (name, limit)
    if k not in _ORACLE:
        c = case(name)
        _ORACLE[k] = [oracle_graph(c, g, limit=limit) for g in range(len(c["graphs"]))]
    return _ORACLE[k]


# ---- the restatement, with seeded defects ----------------------------------------------------------------------------------------
DEFECTS = ("ignore-invert", "le-for-lt", "weights-dropped", "no-correction", "delta-is-v-full", "ridge-on-intercept",
           "intercept-first", "pivot-without-ajj", "twins-as-two-players")


def restate(c, defect=None):
    """The rules restated in numpy fp64 -> (phi [P], phi0 [B], r2 [B], status [B]).  ``defect``: one of DEFECTS, seeded."""
    mode, ridge = c["mode"], c["ridge"]
    phis, phi0s, r2s, sts = [], [], [], []
    for gr in c["graphs"]:
        players = list(gr.players)
        if defect == "twins-as-two-players":
            players = [e for e in range(gr.keys.shape[1]) if (gr.keys[:, e] >= 0).all()] if gr.keys.shape[0] else players
        n, S = len(players), len(gr.row)
        nan = float("nan")
        w = np.array(gr.wt if gr.wt is not None else [1.0] * S, dtype=np.float64)
        v = np.array(gr.val, dtype=np.float64)
        ve, vf = gr.ve, gr.vf
        if not (np.isfinite(v).all() and np.isfinite(w).all() and (w >= 0).all()):
            phis += [nan] * len(gr.players)
            phi0s.append(nan), r2s.append(nan), sts.append(3)
            continue
        if defect == "weights-dropped":
            w = np.ones(S)
        inv = None if defect == "ignore-invert" else gr.inv
        th = [t + 1 for t in gr.th] if defect == "le-for-lt" else gr.th
        z = members(gr.keys, players, gr.row, th, inv).astype(np.float64).reshape(S, n)
        if mode == 1:
            one = np.ones((S, 1))
            z = np.concatenate([one, z] if defect == "intercept-first" else [z, one], axis=1)
        d = n + mode
        y = v - ve if mode == 0 else v
        delta = vf if defect == "delta-is-v-full" else vf - ve
        A = (z * w[:, None]).T @ z
        rd = np.arange(d if defect == "ridge-on-intercept" else n)
        A[rd, rd] += ridge
        b = z.T @ (w * y)
        phi, phi0, deficient = np.zeros(n), ve, False
        if mode == 0 and n == 1:
            phi = np.array([delta])
        elif d > 0:
            L = np.zeros((d, d))
            for j in range(d):
                dj = A[j, j] - L[j, :j] @ L[j, :j]
                if not dj > (1.0 if defect == "pivot-without-ajj" else A[j, j]) * 2.0 ** -30:
                    deficient = True
                    break
                L[j, j] = math.sqrt(dj)
                L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
            if not deficient:
                def solve(r):
                    t = r.copy()
                    for i in range(d):
                        t[i] = (t[i] - L[i, :i] @ t[:i]) / L[i, i]
                    for i in range(d - 1, -1, -1):
                        t[i] = (t[i] - L[i + 1:, i] @ t[i + 1:]) / L[i, i]
                    return t
                x = solve(b)
                if mode == 0:
                    u = solve(np.ones(d))
                    phi = x if defect == "no-correction" else x - u * ((x.sum() - delta) / u.sum())
                elif defect == "intercept-first":
                    phi, phi0 = x[:n], x[n]                     # (reads the unknowns where the rule puts them)
                else:
                    phi, phi0 = x[:n], x[n]
        if deficient and n > 0:
            phis += [nan] * len(gr.players)
            phi0s.append(nan), r2s.append(nan), sts.append(1)
            continue
        if deficient:
            phi0 = nan
        zp = z[:, 1:] if (mode == 1 and defect == "intercept-first") else z[:, :n]
        res = v - phi0 - zp @ phi
        sw = w.sum()
        mean = (w * v).sum() / sw if sw > 0 else nan
        sst = (w * (v - mean) ** 2).sum() if S else 0.0
        ssr = (w * res * res).sum() if S else 0.0
        phis += list(phi[:len(gr.players)]) + [nan] * (len(gr.players) - len(phi))
        phi0s.append(phi0), r2s.append(1.0 - ssr / sst if sst > 0 else nan), sts.append(0)
    return np.array(phis, dtype=np.float64), np.array(phi0s), np.array(r2s), np.array(sts, dtype=np.int64)

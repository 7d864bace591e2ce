"""Plain-Python restatement of cal_centrality, written from the contract in include/cal_hip.h, and the case table the CPU and the
GPU tests share.

Integers are Python ints.  sigma is a Python int, delta, bc and ebc are ``fractions.Fraction``: EXACT, so what the libraries are
held to is the value itself, not another rounding of it.  PageRank has two restatements: ``pagerank_exact`` -- the stationary
vector from a dense fp64 solve of (I - alpha M) x = (1 - alpha) / n 1 with the dangling columns uniform, the yardstick of ``pr`` --
and ``pagerank_steps`` -- the iteration of the contract in Python floats (IEEE doubles, no contraction) in the contract's order of
every sum, which gives ``pr_iters``.

``defect=`` seeds one of DEFECTS into the restatement; tests/test_centrality.py shows that its inputs and bounds notice each.
"""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
MAX_NODES = 256
LDS_COLS = 768
W = 4

DEFECTS = ("sigma skips the last word of a row", "backward starts one level too high", "the s = v term left in",
           "reverse orientation of ebc dropped", "dangling mass dropped", "closeness without its reach factor", "hop seeded with 1")


def adjacency(n, cols):
    """-> (sorted neighbour lists, ignored columns) of the simple undirected graph the columns make."""
    adj = [set() for _ in range(n)]
    ignored = 0
    for u, v in cols:
        if not (0 <= u < n and 0 <= v < n):
            ignored += 1
        elif u != v:
            adj[u].add(v)
            adj[v].add(u)
    return [sorted(a) for a in adj], ignored


def _levels(adj, seeds):
    """-> (dist, -1 unreached; the nodes level by level) of a search from ``seeds``."""
    dist = [-1] * len(adj)
    for s in seeds:
        dist[s] = 0
    levels, cur = [], sorted(seeds)
    while cur:
        levels.append(cur)
        nxt = []
        for v in cur:
            for w in adj[v]:
                if dist[w] < 0:
                    dist[w] = dist[v] + 1
                    nxt.append(w)
        cur = sorted(nxt)
    return dist, levels


def brandes(n, cols, sources=None, defect=None):
    """-> dict: far, reach, ecc, deg (ints), bc (Fractions, raw), ebc (Fractions per column, raw), hop (ints or None),
    ignored."""
    adj, ignored = adjacency(n, cols)
    far, reach, ecc = [0] * n, [0] * n, [0] * n
    bc = [Fraction(0)] * n
    edge = {}                                             # (a, b), a < b -> Fraction
    for s in range(n):
        dist, levels = _levels(adj, [s])
        sigma = [0] * n
        sigma[s] = 1
        for lev in levels[1:]:
            for v in lev:
                up = [u for u in adj[v] if dist[u] == dist[v] - 1]
                if defect == DEFECTS[0]:
                    up = [u for u in up if u >> 6 != (n - 1) >> 6 or n <= 64]
                sigma[v] = sum(sigma[u] for u in up)
        delta = [Fraction(0)] * n
        q = [Fraction(0)] * n
        deaf = len(levels) - 2 if defect == DEFECTS[1] else -1          # the level that does not hear the deepest one
        for L in range(len(levels) - 1, -1, -1):
            for v in levels[L]:
                if L != deaf and sigma[v]:
                    acc = Fraction(0)
                    for w in adj[v]:
                        if dist[w] == L + 1 and sigma[w]:
                            t = sigma[v] * q[w]
                            acc += t
                            key = (v, w) if v < w else (w, v)
                            edge[key] = edge.get(key, 0) + t
                    delta[v] = acc
                if sigma[v]:
                    q[v] = (1 + delta[v]) / sigma[v]
        for v in range(n):
            if dist[v] >= 0:
                far[v] += dist[v]
                reach[v] += 1
                ecc[v] = max(ecc[v], dist[v])
                if v != s or defect == DEFECTS[2]:
                    bc[v] += delta[v]
    ebc = []
    for u, v in cols:
        if not (0 <= u < n and 0 <= v < n) or u == v:
            ebc.append(Fraction(0))
        elif defect == DEFECTS[3] and u > v:
            ebc.append(Fraction(0))
        else:
            ebc.append(Fraction(edge.get((min(u, v), max(u, v)), 0)))
    hop = None
    if sources is not None:
        hop = _levels(adj, [v for v in range(n) if sources[v]])[0]
        if defect == DEFECTS[6]:
            hop = [h + 1 if h >= 0 else h for h in hop]
    return dict(far=far, reach=reach, ecc=ecc, deg=[len(a) for a in adj], bc=bc, ebc=ebc, hop=hop, ignored=ignored, adj=adj)


def closeness(far, reach, n, defect=None):
    """Wasserman-Faust, as networkx: ((reach - 1) / far) * ((reach - 1) / (n - 1)); 0 where far == 0."""
    out = []
    for f, r in zip(far, reach):
        if f == 0:
            out.append(0.0)
        elif defect == DEFECTS[5]:
            out.append((r - 1) / f)
        else:
            out.append(((r - 1) / f) * ((r - 1) / (n - 1)))
    return out


def pagerank_exact(adj, alpha, defect=None):
    n = len(adj)
    if n == 0:
        return np.zeros(0)
    M = np.zeros((n, n))
    for u, a in enumerate(adj):
        if a:
            M[a, u] = 1.0 / len(a)
        elif defect != DEFECTS[4]:
            M[:, u] = 1.0 / n
    return np.linalg.solve(np.eye(n) - alpha * M, np.full(n, (1.0 - alpha) / n))


def _tree_sum(vals):
    s = [0.0] * 256
    for i, v in enumerate(vals):
        s[i & 255] += v
    h = 128
    while h:
        for i in range(h):
            s[i] += s[i + h]
        h >>= 1
    return s[0]


def pagerank_steps(adj, alpha, tol, max_iter):
    """The iteration of the contract, in its order of every sum -> (x, steps)."""
    n = len(adj)
    if n == 0:
        return [], 0
    x = [1.0 / n] * n
    it = 0
    dn = float(n)
    dsum = _tree_sum([0.0 if adj[v] else x[v] for v in range(n)])
    while it < max_iter:
        xd = [x[v] / float(len(adj[v])) if adj[v] else 0.0 for v in range(n)]
        xn = []
        for v in range(n):
            pull = 0.0
            for u in adj[v]:
                pull += xd[u]
            t = pull + dsum / dn
            a = alpha * t
            b = (1.0 - alpha) / dn
            xn.append(a + b)
        err = _tree_sum([abs(xn[v] - x[v]) for v in range(n)])
        x = xn
        dsum = _tree_sum([0.0 if adj[v] else x[v] for v in range(n)])
        it += 1
        if err < tol:
            break
    return x, it


# ---- the bounds -------------------------------------------------------------------------------------------------------------------
def gamma(k):
    return k * U / (1.0 - k * U)


def bc_bound(n):
    """Relative error of bc and ebc against the exact rationals: gamma_k, k = 2 n (n + 3).  Every output is a sum of non-negative
    terms (no cancellation); a value depends on a chain of at most n levels forward and n back, each with at most n - 1 adds and
    three operations per term, plus n adds over the sources."""
    return gamma(2 * n * (n + 3))


def pr_bound(n, alpha, tol):
    """L1 distance of pr from the exact stationary vector: alpha / (1 - alpha) tol, the contraction bound of the iteration
    (||x_k - x*|| <= alpha / (1 - alpha) ||x_k - x_{k-1}||, and the step stops below tol), plus n k' u for the rounding with
    k' = (n + 8) / (1 - alpha): a step's component carries at most deg <= n adds and a handful of other operations, (n + 8) u
    relative, the components sum to 1, so a step adds at most (n + 8) u in L1 and the contraction accumulates that to
    (n + 8) u / (1 - alpha); the factor n covers the dense solve of the yardstick itself (backward stable, condition at most
    (1 + alpha) / (1 - alpha))."""
    return alpha / (1.0 - alpha) * tol + n * (n + 8) / (1.0 - alpha) * U


def frac_err(got, exact):
    """|got - exact| / exact as a float, exactly formed (0 for 0 against 0, inf for a non-zero against 0 or a NaN)."""
    if got != got:
        return math.inf
    d = abs(Fraction(got) - exact)
    if d == 0:
        return 0.0
    return math.inf if exact == 0 else float(d / exact)


# ---- the cases --------------------------------------------------------------------------------------------------------------------
def both(edges):
    return list(edges) + [(v, u) for u, v in edges]


def path(n):
    return both([(i, i + 1) for i in range(n - 1)])


def star(n):
    return both([(0, i) for i in range(1, n)])


def cycle(n):
    return both([(i, (i + 1) % n) for i in range(n)])


def complete(n):
    return [(i, j) for i in range(n) for j in range(n) if i != j]


def grid(r, c):
    e = [(i * c + j, i * c + j + 1) for i in range(r) for j in range(c - 1)]
    e += [(i * c + j, (i + 1) * c + j) for i in range(r - 1) for j in range(c)]
    return both(e)


def cube(d):
    return both([(v, v ^ (1 << b)) for v in range(1 << d) for b in range(d) if v < v ^ (1 << b)])


def ba(n, m, seed):
    """a preferential-attachment graph from a small LCG (no dependence on a library's generator)"""
    state = [seed * 2654435761 % (1 << 32) or 1]

    def rnd(k):
        state[0] = (state[0] * 1664525 + 1013904223) % (1 << 32)
        return (state[0] >> 8) % k
    ends, edges = list(range(m)), []
    for v in range(m, n):
        picked = set()
        while len(picked) < m:
            picked.add(ends[rnd(len(ends))])
        for u in picked:
            edges.append((u, v))
            ends += [u, v]
    return both(edges)


HOUSE = both([(0, 1), (1, 2), (2, 3), (3, 0), (0, 4), (1, 4)])


def _case(name, n, cols, sources=None):
    return dict(name=name, n=n, cols=list(cols), sources=sources)


def _mask(n, on):
    return [1 if v in on else 0 for v in range(n)]


def cases():
    """The smallest shapes at which the kernel can still go wrong (see tests/test_gpu_centrality.py for why each is here)."""
    two_comp = both([(0, 1), (1, 2), (2, 0), (3, 4), (4, 5)])                         # a triangle, a path of 3, node 6 isolated
    messy = [(0, 1), (0, 1), (1, 2), (2, 2), (3, 2), (1, 7), (-1, 0), (9, 9), (3, 4), (4, 3), (4, 3)]   # one-way, duplicates,
    #                                                                                   self loops, columns that leave (n = 5)
    out = [
        _case("n0", 0, []), _case("n1", 1, []), _case("n2", 2, both([(0, 1)])), _case("n3", 3, path(3)),
        _case("no-columns", 5, [], _mask(5, {2})),
        _case("path7", 7, path(7), _mask(7, {0})), _case("star6", 6, star(6), _mask(6, {3})),
        _case("cycle6", 6, cycle(6), _mask(6, {})), _case("cycle7", 7, cycle(7), _mask(7, set(range(7)))),
        _case("house", 5, HOUSE, _mask(5, {4})), _case("k4", 4, complete(4)),
        _case("two-components", 7, two_comp, _mask(7, {3})),
        _case("messy", 5, messy, _mask(5, {0})),
    ]
    for n in (63, 64, 65, 127, 128, 129):
        out.append(_case("ba%d" % n, n, ba(n, 2, n), _mask(n, {n - 1})))
    out += [
        _case("path256", 256, path(256), _mask(256, {255})),
        _case("star256", 256, star(256), _mask(256, {17})),
        _case("k64", 64, complete(64)),                                               # 4032 columns: above the LDS cap of ebc
        _case("grid16", 256, grid(16, 16), _mask(256, {0, 255})),
        _case("q6", 64, cube(6), _mask(64, {63})),
        _case("cycle200", 200, cycle(200)),                                           # a long cycle: two shortest paths at the far end
    ]
    return out


_ORACLE = {}


def oracle(case, alpha=0.85, tol=1e-12, max_iter=1000):
    """The exact outputs of a case, computed once: ``brandes`` plus ``pr`` (exact), ``pr_iters``, ``closeness``."""
    key = (case["name"], alpha, tol, max_iter)
    if key not in _ORACLE:
        o = brandes(case["n"], case["cols"], case["sources"])
        o["pr"] = pagerank_exact(o["adj"], alpha)
        o["pr_iters"] = pagerank_steps(o["adj"], alpha, tol, max_iter)[1]
        o["closeness"] = closeness(o["far"], o["reach"], case["n"])
        _ORACLE[key] = o
    return _ORACLE[key]


def batch_arrays(cs, big=None):
    """The cases as one batch -> (edge_index [2, E] int64, ptr, edge_ptr [B + 1], batch [N], sources uint8 [N]) as numpy arrays.
    Local ids outside a graph stay outside it (they land in a neighbour's range or outside the batch)."""
    ptr, eptr, src, rows = [0], [0], [], []
    for c in cs:
        lo = ptr[-1]
        rows += [(lo + u, lo + v) for u, v in c["cols"]]
        ptr.append(lo + c["n"])
        eptr.append(len(rows))
        src += c["sources"] if c["sources"] is not None else [0] * c["n"]
    ei = np.asarray(rows, dtype=np.int64).reshape(-1, 2).T.copy()
    batch = np.repeat(np.arange(len(cs)), np.diff(ptr))
    return ei, np.asarray(ptr, np.int64), np.asarray(eptr, np.int64), batch.astype(np.int64), np.asarray(src, np.uint8)


def judge(cs, got, alpha=0.85, tol=1e-12, max_iter=1000, exact=None):
    """``got``: dict of numpy arrays of a whole batch of the cases ``cs`` (far reach ecc deg hop pr_iters int; bc ebc pr
    float64; ignored, skipped) -> the list of what misses the contract (empty: all is well).  ``exact``: per case, the dict to
    hold it to (default: ``oracle``)."""
    bad = []
    no = eo = 0
    ign = 0
    for i, c in enumerate(cs):
        n, m = c["n"], len(c["cols"])
        o = exact[i] if exact is not None else oracle(c, alpha, tol, max_iter)
        ign += o["ignored"]
        for key in ("far", "reach", "ecc", "deg"):
            if list(got[key][no:no + n]) != o[key]:
                bad.append("%s: %s" % (c["name"], key))
        if o["hop"] is not None and list(got["hop"][no:no + n]) != o["hop"]:
            bad.append("%s: hop" % c["name"])
        if int(got["pr_iters"][i]) != o["pr_iters"]:
            bad.append("%s: pr_iters %d != %d" % (c["name"], int(got["pr_iters"][i]), o["pr_iters"]))
        if int(got["skipped"][i]) != 0:
            bad.append("%s: skipped" % c["name"])
        bound = bc_bound(n)
        e1 = max([frac_err(float(g), x) for g, x in zip(got["bc"][no:no + n], o["bc"])], default=0.0)
        e2 = max([frac_err(float(g), x) for g, x in zip(got["ebc"][eo:eo + m], o["ebc"])], default=0.0)
        if e1 > bound:
            bad.append("%s: bc %.3e > %.3e" % (c["name"], e1, bound))
        if e2 > bound:
            bad.append("%s: ebc %.3e > %.3e" % (c["name"], e2, bound))
        l1 = float(np.abs(np.asarray(got["pr"][no:no + n], dtype=np.float64) - o["pr"]).sum()) if n else 0.0
        if not l1 <= pr_bound(n, alpha, tol):
            bad.append("%s: pr %.3e > %.3e" % (c["name"], l1, pr_bound(n, alpha, tol)))
        if "closeness" in got and not np.allclose(got["closeness"][no:no + n], o["closeness"], rtol=4 * U, atol=0.0):
            bad.append("%s: closeness" % c["name"])
        no, eo = no + n, eo + m
    if int(got["ignored"]) != ign:
        bad.append("ignored %d != %d" % (int(got["ignored"]), ign))
    return bad

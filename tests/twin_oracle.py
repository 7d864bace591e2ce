"""numpy / torch-CPU oracle of the reverse-edge map (cal_edge_twin) and of the ranking of edge pairs
(cal_explain_rank_pairs), written from the contract in include/cal_hip.h, and the edge batches both test files share."""
import numpy as np
import torch

from tests.explain_oracle import rank_oracle


def twin_oracle(edge_index, ptr, edge_ptr, max_edges=None):
    """-> (twin int32 [E], (columns with twin < 0, self loops)).  Per graph a dict of per-key column lists: the j-th column
    equal to (u, v) pairs with the j-th column equal to (v, u)."""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    ptr, edge_ptr = np.asarray(ptr, dtype=np.int64), np.asarray(edge_ptr, dtype=np.int64)
    E = ei.shape[1]
    twin = np.full(E, -1, dtype=np.int32)
    n_self = 0
    for g in range(ptr.size - 1):
        lo, hi = int(edge_ptr[g]), int(edge_ptr[g + 1])
        if max_edges is not None and hi - lo > max_edges:
            continue
        nlo, nhi = int(ptr[g]), int(ptr[g + 1])
        cols = {}
        for e in range(lo, hi):
            u, v = int(ei[0, e]), int(ei[1, e])
            if not (nlo <= u < nhi and nlo <= v < nhi):
                continue
            if u == v:
                twin[e] = e
                n_self += 1
                continue
            cols.setdefault((u, v), []).append(e)
        for (u, v), es in cols.items():
            back = cols.get((v, u), [])
            for j, e in enumerate(es):
                if j < len(back):
                    twin[e] = back[j]
    return twin, (int((twin < 0).sum()), n_self)


def symmetrise(score, twin, reduce):
    """torch fp32: (a + b) * 0.5, maximum or minimum of a column's score and its twin's; an unpaired column keeps its own."""
    s = torch.as_tensor(np.asarray(score, dtype=np.float32))
    t = torch.as_tensor(np.asarray(twin, dtype=np.int64))
    o = s[t.clamp(min=0)]
    both = {"mean": (s + o) * 0.5, "max": torch.maximum(s, o), "min": torch.minimum(s, o)}[reduce]
    return torch.where(t >= 0, both, s).numpy()


def pair_rank_oracle(score, seg_ptr, twin, reduce, k=None, ratio=None, gt=None, max_seg=None):
    """-> (mask bool [M], rank int32 [M], metrics float64 [B, 4], symmetrised score float32 [M]): rank_oracle over each
    segment's representatives (the lower column of a pair, every unpaired column and self loop), scattered to both columns."""
    seg_ptr = np.asarray(seg_ptr, dtype=np.int64)
    twin = np.asarray(twin, dtype=np.int64)
    M, B = twin.size, seg_ptr.size - 1
    sym = symmetrise(score, twin, reduce)
    idx = np.arange(M)
    rep = np.where((twin >= 0) & (twin < idx), twin, idx)
    pos = np.zeros(M, dtype=bool) if gt is None else np.asarray(gt, dtype=bool).copy()
    paired = twin >= 0
    pos[paired] |= pos[twin[paired]]
    mask, rank = np.zeros(M, dtype=bool), np.full(M, -1, dtype=np.int32)
    met = np.full((B, 4), np.nan)
    for g in range(B):
        lo, hi = int(seg_ptr[g]), int(seg_ptr[g + 1])
        if max_seg is not None and hi - lo > max_seg:
            continue
        reps = [e for e in range(lo, hi) if rep[e] == e]
        m_, r_, t_ = rank_oracle(sym[reps], [0, len(reps)], k=k, ratio=ratio, gt=None if gt is None else pos[reps])
        row = dict(zip(reps, range(len(reps))))
        for e in range(lo, hi):
            mask[e], rank[e] = m_[row[rep[e]]], r_[row[rep[e]]]
        met[g] = t_[0]
    return mask, rank, met, sym


# ---- shared edge batches ---------------------------------------------------------------------------------------------------
def make_batch(sizes, seed=0, stray=True):
    """A batch with ``sizes[g]`` edge columns in graph g, shuffled inside each segment -> (edge_index [2, E], ptr, edge_ptr).
    Every graph mixes symmetric pairs, duplicated edges with unequal multiplicities in the two directions (3 x (u, v) against
    1 x (v, u)), self loops (some duplicated) and purely directed columns over few nodes, so equal keys abound; with ``stray``
    one column of the first graph with >= 4 columns points into another graph's node range."""
    rng = np.random.default_rng(seed)
    ptr, eptr, cols = [0], [0], []
    for m in sizes:
        n = max(2, int(np.sqrt(m)) + 2)
        lo = ptr[-1]
        seg = []
        while len(seg) < m:
            u, v = (int(x) for x in rng.choice(n, 2, replace=False))
            kind, left = rng.random(), m - len(seg)
            if kind < 0.6 and left >= 2:
                seg += [(u, v), (v, u)]
            elif kind < 0.7 and left >= 4:
                seg += [(u, v)] * 3 + [(v, u)]
            elif kind < 0.8:
                seg += [(u, u)] * min(left, 1 + int(rng.integers(0, 2)))
            else:
                seg.append((u, v))
        seg = [seg[i] for i in rng.permutation(m)]
        cols += [(lo + u, lo + v) for u, v in seg]
        ptr.append(lo + n)
        eptr.append(eptr[-1] + m)
    ei = np.array(cols, dtype=np.int64).reshape(-1, 2).T.copy()
    if stray and len(sizes) > 1:
        for g, m in enumerate(sizes):
            if m >= 4:
                other = (g + 1) % len(sizes)
                ei[1, eptr[g] + m // 2] = ptr[other]
                break
    return ei, np.array(ptr, dtype=np.int64), np.array(eptr, dtype=np.int64)


def make_scores(twin, seed=0):
    """Scores with ties (a grid of sixteenths), a NaN on one side of some pairs and on some unpaired columns, and a ground
    truth of about a fifth of the columns."""
    rng = np.random.default_rng(seed + 1)
    M = len(twin)
    s = (np.round(rng.standard_normal(M) * 4) / 16 + 2.0).astype(np.float32)      # positive: no signed zeros
    one_side = (rng.random(M) < 0.05) & (np.asarray(twin) != np.arange(M))
    s[one_side] = np.nan
    return s, rng.random(M) < 0.2

"""Plain-int restatement of exact motif matching (cal_motif_match), written from the contract in include/cal_hip.h -- match order,
parents, roots, steps and budget, the smallest embedding -- on Python sets and lists, and the brute-force counter over all
injective maps that the restatement is checked against."""
from itertools import permutations

import numpy as np

MAX_PATTERN = 8
MAX_NODES = 256


def simple_graph(edge_index, nlo, nhi, elo, ehi):
    """-> (neighbour sets by local id, ignored columns) of the graph that owns the nodes [nlo, nhi) and the columns [elo, ehi)."""
    n = nhi - nlo
    nb = [set() for _ in range(n)]
    ignored = 0
    for e in range(elo, ehi):
        u, v = int(edge_index[0][e]) - nlo, int(edge_index[1][e]) - nlo
        if not (0 <= u < n and 0 <= v < n):
            ignored += 1
        elif u != v:
            nb[u].add(v)
            nb[v].add(u)
    return nb, ignored


def match_order(nb):
    """-> (pi, parent): pi[0] the node of the largest degree, then always the unplaced node with the most placed neighbours, the
    lowest id on ties; parent[d] the earliest position whose node is adjacent to pi[d].  ValueError for a bad pattern."""
    k = len(nb)
    if not 1 <= k <= MAX_PATTERN:
        raise ValueError("a pattern has 1 to 8 nodes")
    pi = [max(range(k), key=lambda i: (len(nb[i]), -i))]
    while len(pi) < k:
        rest = [i for i in range(k) if i not in pi]
        best = max(rest, key=lambda i: (len(nb[i] & set(pi)), -i))
        if not nb[best] & set(pi):
            raise ValueError("a pattern must be connected")
        pi.append(best)
    parent = [None] + [min(j for j in range(d) if pi[j] in nb[pi[d]]) for d in range(1, k)]
    return pi, parent


def search(tnb, pnb, tlab=None, plab=None, induced=False, budget=1 << 17):
    """One pattern in one graph -> (count, truncated roots, smallest embedding by pattern node or None, the steps of every root
    as {(u, w): steps})."""
    n, k = len(tnb), len(pnb)
    pi, parent = match_order(pnb)

    def label_ok(v, d):
        return tlab is None or int(tlab[v]) == int(plab[pi[d]])
    found, steps_of = [], {}
    if k == 1:
        found = [[v] for v in range(n) if label_ok(v, 0)]
        return len(found), 0, (min(found) if found else None), steps_of
    truncated = 0

    class Stop(Exception):
        pass

    for u in range(n):
        for w in sorted(tnb[u]):
            if not (label_ok(u, 0) and label_ok(w, 1)):
                continue
            img = [u, w]
            steps = [0]

            def emb():
                f = [None] * k
                for d in range(k):
                    f[pi[d]] = img[d]
                return f

            def go(d):
                if d == k:
                    found.append(emb())
                    return
                for v in sorted(tnb[img[parent[d]]]):
                    if steps[0] == budget:
                        raise Stop()
                    steps[0] += 1
                    if v in img or not label_ok(v, d):
                        continue
                    good = True
                    for j in range(d):
                        a = img[j] in tnb[v]
                        if pi[j] in pnb[pi[d]]:
                            good = good and a
                        elif induced:
                            good = good and not a
                    if good:
                        img.append(v)
                        go(d + 1)
                        img.pop()
            try:
                go(2)
            except Stop:
                truncated += 1
            steps_of[(u, w)] = steps[0]
    return len(found), truncated, (min(found) if found else None), steps_of


def brute_force(tnb, pnb, tlab=None, plab=None, induced=False):
    """Count over ALL injective maps (small graphs only) -> (count, smallest embedding or None)."""
    n, k = len(tnb), len(pnb)
    cnt, best = 0, None
    for f in permutations(range(n), k):
        ok = all(tlab is None or int(tlab[f[i]]) == int(plab[i]) for i in range(k))
        for i in range(k):
            for j in range(i + 1, k):
                a = f[j] in tnb[f[i]]
                if j in pnb[i]:
                    ok = ok and a
                elif induced:
                    ok = ok and not a
        if ok:
            cnt += 1
            best = list(f) if best is None else min(best, list(f))
    return cnt, best


def motif_match_oracle(edge_index, ptr, edge_ptr, pat_edge_index, pat_ptr, pat_edge_ptr, labels=None, pat_labels=None,
                       induced=False, budget=1 << 17):
    """-> (count int64 [B, P], first int32 [B, P, 8], truncated int64 [B, P], tgt_edges [B], pat_edges [P], ignored)."""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    pei = np.asarray(pat_edge_index, dtype=np.int64).reshape(2, -1)
    B, P = len(ptr) - 1, len(pat_ptr) - 1
    pats = []
    for p in range(P):
        lo, hi = int(pat_ptr[p]), int(pat_ptr[p + 1])
        nb, _ = simple_graph(pei, lo, hi, int(pat_edge_ptr[p]), int(pat_edge_ptr[p + 1]))
        match_order(nb)                                                   # (raises for a bad pattern)
        pats.append((nb, None if pat_labels is None else [int(x) for x in pat_labels[lo:hi]]))
    count = np.zeros((B, P), dtype=np.int64)
    trunc = np.zeros((B, P), dtype=np.int64)
    first = np.full((B, P, MAX_PATTERN), -1, dtype=np.int32)
    ran = B > 0 and P > 0
    tgt = np.full(B, -1, dtype=np.int64)
    pat = np.array([sum(len(s) for s in nb) // 2 for nb, _ in pats], dtype=np.int64) if ran else np.full(P, -1, dtype=np.int64)
    ignored = 0
    for g in range(B if ran else 0):
        lo, hi = int(ptr[g]), int(ptr[g + 1])
        nb, ign = simple_graph(ei, lo, hi, int(edge_ptr[g]), int(edge_ptr[g + 1]))
        ignored += ign
        if hi - lo > MAX_NODES:
            count[g] = -1
            continue
        tgt[g] = sum(len(s) for s in nb) // 2
        tl = None if labels is None else [int(x) for x in labels[lo:hi]]
        for p, (pnb, pl) in enumerate(pats):
            c, t, f, _ = search(nb, pnb, tl, pl, induced, budget)
            count[g, p], trunc[g, p] = c, t
            if f is not None:
                first[g, p, :len(f)] = f
    return count, first, trunc, tgt, pat, ignored

"""Plain-int restatement of the Weisfeiler-Lehman refinement (cal_wl_refine) and of the WL subtree kernel (cal_wl_match), written
from the contract in include/cal_hip.h: Python ints reduced mod 2^64, dicts and Counters, no torch arithmetic."""
from collections import Counter

import numpy as np

M64 = (1 << 64) - 1
C_INIT = 0xD6E8FEB86659FD93
C_SELF = 0xC2B2AE3D27D4EB4F
C_OUT = 0x165667B19E3779F9
C_IN = 0x27D4EB2F165667C5
C_NODE = 0x85EBCA77C2B2AE63
C_GRAPH = 0xFF51AFD7ED558CCD


def sm(x):
    """splitmix64 on a Python int."""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def signed(x):
    """the int64 that carries the uint64 bit pattern x"""
    return x - (1 << 64) if x >= (1 << 63) else x


def wl_refine_oracle(edge_index, ptr, edge_ptr, N, T, init=None, max_nodes=None):
    """-> (colors int64 [T + 1, N], hash int64 [B, T + 1], ignored)."""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    ptr = [int(p) for p in ptr]
    eptr = [int(p) for p in edge_ptr]
    B = len(ptr) - 1
    colors = [[0] * N for _ in range(T + 1)]
    hashes = [[0] * (T + 1) for _ in range(B)]
    ignored = 0
    for g in range(B):
        nlo, nhi = ptr[g], ptr[g + 1]
        cols = []
        for e in range(eptr[g], eptr[g + 1]):
            u, v = int(ei[0, e]), int(ei[1, e])
            if nlo <= u < nhi and nlo <= v < nhi:
                cols.append((u, v))
            else:
                ignored += 1
        n = nhi - nlo
        if max_nodes is not None and n > max_nodes:
            continue
        c = {v: sm(((0 if init is None else int(init[v])) & M64) ^ C_INIT) for v in range(nlo, nhi)}
        h = sm(n ^ C_GRAPH)
        for t in range(T + 1):
            if t:
                out = dict.fromkeys(c, 0)
                inn = dict.fromkeys(c, 0)
                for u, v in cols:
                    out[u] = (out[u] + sm(c[v] ^ C_OUT)) & M64
                    inn[v] = (inn[v] + sm(c[u] ^ C_IN)) & M64
                c = {v: sm((sm((sm((c[v] + C_SELF) & M64) + out[v]) & M64) + inn[v]) & M64) for v in c}
            for v in c:
                colors[t][v] = c[v]
            h = sm((h + sum(sm(c[v] ^ C_NODE) for v in c)) & M64)
            hashes[g][t] = h
    col = np.array([[signed(x) for x in row] for row in colors], dtype=np.int64).reshape(T + 1, N)
    hs = np.array([[signed(x) for x in row] for row in hashes], dtype=np.int64).reshape(B, T + 1)
    return col, hs, ignored


def wl_match_oracle(colors_a, ptr_a, colors_p, ptr_p, max_nodes_a=None):
    """-> (K int64 [A, P, T + 1], self int64 [A, T + 1]) from the two colour arrays [T + 1, Na] / [T + 1, Np]."""
    ca, cp = np.asarray(colors_a, dtype=np.int64), np.asarray(colors_p, dtype=np.int64)
    T1 = ca.shape[0]
    A, P = len(ptr_a) - 1, len(ptr_p) - 1
    K = np.zeros((A, P, T1), dtype=np.int64)
    own = np.zeros((A, T1), dtype=np.int64)
    for a in range(A):
        lo, hi = int(ptr_a[a]), int(ptr_a[a + 1])
        if max_nodes_a is not None and hi - lo > max_nodes_a:
            continue
        for t in range(T1):
            cnt = Counter(int(x) for x in ca[t, lo:hi])
            own[a, t] = sum(v * v for v in cnt.values())
            for p in range(P):
                K[a, p, t] = sum(cnt.get(int(x), 0) for x in cp[t, int(ptr_p[p]):int(ptr_p[p + 1])])
    return K, own


def wl_similarity_oracle(K, self_a, self_p, depths=None):
    """fp64 [A, P]: sum_t K / sqrt(sum_t self_a * sum_t self_p) over the chosen depths, 0 where a graph has no node."""
    K, sa, sp = np.asarray(K), np.asarray(self_a), np.asarray(self_p)
    d = list(range(K.shape[2])) if depths is None else list(depths)
    out = np.zeros(K.shape[:2], dtype=np.float64)
    for a in range(K.shape[0]):
        for p in range(K.shape[1]):
            den = int(sa[a, d].sum()) * int(sp[p, d].sum())
            out[a, p] = float(K[a, p, d].sum()) / np.sqrt(float(den)) if den else 0.0
    return out


def both_directions(edges):
    """both directions of every undirected edge, grouped by source -> [2, 2 |edges|] int64"""
    cols = sorted([(a, b) for a, b in edges] + [(b, a) for a, b in edges])
    return np.array(cols, dtype=np.int64).reshape(-1, 2).T.copy()

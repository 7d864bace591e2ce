"""numpy oracle of per-segment explanation ranking (cal_explain_rank): order, selection count, metrics."""
import math

import numpy as np


def rank_oracle(score, seg_ptr, k=None, ratio=None, gt=None):
    """-> (mask bool [M], rank int32 [M], metrics float64 [B, 4]) for k >= 0, k == "gt" or a ratio."""
    score = np.asarray(score, dtype=np.float32)
    seg_ptr = np.asarray(seg_ptr, dtype=np.int64)
    M, B = score.size, seg_ptr.size - 1
    mask = np.zeros(M, dtype=bool)
    rank = np.zeros(M, dtype=np.int32)
    met = np.zeros((B, 4), dtype=np.float64)
    for g in range(B):
        lo, hi = int(seg_ptr[g]), int(seg_ptr[g + 1])
        m = hi - lo
        s = score[lo:hi].astype(np.float64)
        idx = np.arange(m)
        order = np.lexsort((idx, -s))                 # score descending (NaN last), then index ascending
        r = np.empty(m, dtype=np.int64)
        r[order] = np.arange(m)
        pos = np.zeros(m, dtype=bool) if gt is None else np.asarray(gt[lo:hi], dtype=bool)
        P = int(pos.sum())
        if k == "gt":
            kg = P
        elif k is not None:
            kg = min(int(k), m)
        else:
            kg = min(m, int(math.ceil(ratio * m)))
        sel = r < kg
        mask[lo:hi] = sel
        rank[lo:hi] = r
        # ascending average ranks (1-based), NaN lowest, ties share the mean
        key = np.where(np.isnan(s), -np.inf, s)
        nan = np.isnan(s)
        avg = np.empty(m, dtype=np.float64)
        for i in range(m):
            if nan[i]:
                less, eq = 0, int(nan.sum())
            else:
                less = int(nan.sum() + ((~nan) & (key < key[i])).sum())
                eq = int(((~nan) & (key == key[i])).sum())
            avg[i] = less + (eq + 1) / 2.0
        auc = float("nan")
        if 0 < P < m:
            auc = (avg[pos].sum() - P * (P + 1) / 2.0) / (P * (m - P))
        met[g] = (kg, int((sel & pos).sum()), P, auc)
    return mask, rank, met

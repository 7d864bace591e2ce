"""Float64 restatement of the operator-level launchers of csrc/gcn.hip, csrc/attn.hip and csrc/plan.hip -- what each one is
documented to return, written from the formulas and not from the kernels -- with the per-element error bound that goes with
every float output.  tests/test_ops_contract_ref.py ties it to oracle.cal_oracle, torch autograd and numpy's stable argsort;
tests/ops_contract_cases.py holds the cases and the judge that applies the bounds; tests/test_gpu_ops_contract.py runs them on
the device.  torch float64 on the CPU, index arrays numpy.  The aggregation and the SDDMM are tests/sparse_contract_ref.py's
(`aggregate` with unit outer scale, per-slot coefficient norm_e and per-row loop coefficient dis^2 loop_w; `sddmm` as it is).

Bounds, u = 2^-24, SLACK = 1 + 1e-3 for the second-order terms; none is fitted to an output.  Two rules carry all of them: an
fp32 sum of n terms in any order is within (n - 1) u sum |terms|; a dot of H products is within (H + 1) u sum |a_k b_k|.  A
stored coefficient carries the roundings counted from its expression, and two more are allowed for a multiply that is not fused
into its add.  A multi-stage launcher that hands its intermediates back is judged stage by stage, each stage against fp64 on the
kernel's OWN stored inputs to it, so no bound is composed along a chain.

  dis       d = sum of `slots` weights + loop_w, dis = d^-1/2.  The sum is off by at most slots u M, M = sum |w| + |loop_w|
            (= d for positive weights); the power halves a relative error; eight roundings of slack and two for the square
            root and the reciprocal: relative ((slots + 8) u M / |d| + 2 u).  d == 0: exactly 0.  d < 0: NaN where fp64 has it.
  norm_e    against fp64 on the stored dis: two multiplies + 2: 4 u |ref|; self-loop columns exactly 0.
  out       cal_spmm_fwd: n = slots + 1 terms; the loop coefficient d * loop_w * d carries two roundings, the bias add one, two
            of slack: (n + 5) u T, T = sum |norm_e| |h_j| + d^2 |loop_w| |h_i| + |bias|.  |relu(a) - relu(b)| <= |a - b|.
  dz        exact (a select).  dbias: column sum of N rows in parts, order arbitrary: (N - 1) u sum |dz|.
  gn, gself (H + 1) u sum |a_k b_k|.
  ddeg      against fp64 on the stored gn_e, gself: acc has n = slots_src + slots_dst + 1 terms of two or three multiplies, then
            -0.5 d d d acc is three more (the -0.5 is exact): (n - 1 + 3 + 3 + 2) u M = (slots_src + slots_dst + 8) u M,
            M = 0.5 |d|^3 sum |terms|.
  dw        against fp64 on the stored gn_e, ddeg: two multiplies, one add, + 2: 5 u (|gn dis_r dis_c| + |ddeg_r|); self-loop
            columns exactly 0.
  pq        (H + 1) u sum |x_k W_k|.
  att       the derivation of tests/test_gpu_sparse_contract.py (`att`): a_k = e_k / (e_0 + e_1), e_k = expf(l_k - max l).  With
            |dl_k| <= r u L_k the nonzero argument is off by d = r u (L_0 + L_1) + u |l_0 - l_1|, expf adds its own relative
            error x (measured by the caller against fp64 exp, at least 2 u), h = d + x: |got - ref| <= ref (2 h + 3 u).
            Edge attention, against the stored pq: l_k = (p_k + q_k) + b_k, r = 3 as there, L_k = |p_k| + |q_k| + |b_k|.
            Node attention, against the inputs: l_k = dot_H + b_k, r = H + 2, L_k = sum |x W_k| + |b_k|.
  xc, xo    against fp64 on the stored att_n: one multiply: u |ref|.
  edge att  backward, end to end (the intermediates live in the opaque workspace).  dl_e = a0 a1 (g0 - g1): three roundings,
            |err| <= 3 u A_e, A_e = a0 a1 (|g0| + |g1|).  sp_v = sum of n_v of them: (n_v - 1) u + 3 u <= (n_v + 2) u SA_v,
            SA_v = sum A_e; sq alike over the by-destination slots.  dx = base + sp wp + sq wq with wp = W0 - W1 (one rounding,
            |wp| <= Wp = |W0| + |W1|) and two multiply-adds (2 + 2): u ((n_v + 7) SAp_v Wp + (m_v + 7) SAq_v Wq + 4 |base|).
            dW = sum over N rows of sp_v x_v in parts: (N - 1) u + the error of sp + 2: sum_v (N + n_v + 4) u SA_v |x_v|;
            db = sum_v sp_v: sum_v (N + n_v + 2) u SA_v.  Row 1 of dW and db is minus row 0.
  node att  backward, end to end from the given att_n.  d0 = <x, dxc>, d1 = <x, dxo>: (H + 1) u M0, M1.  dl = a0 a1 (d0 - d1):
            |err| <= (H + 4) u a0 a1 (M0 + M1) =: (H + 4) u Q.  dx = a0 dxc + a1 dxo + dl w0, w0 = Wn0 - Wn1, three
            multiply-adds (3 + 2): u (5 (a0 |dxc| + a1 |dxo|) + (H + 10) Q Wm), Wm = |Wn0| + |Wn1|.
            dWn = sum_v dl_v x_v: sum_v (N + H + 7) u Q_v |x_v|; dbn = sum_v dl_v: sum_v (N + H + 5) u Q_v.
  pooled    a sum of the n rows of a graph in any order, slices included: (n - 1) u sum |x|; one row exact, none: exactly 0.
  add-pool backward, the plan, graph_ptr, every count: exact.
"""
import numpy as np
import torch

from tests import sparse_contract_ref as sref

F64 = torch.float64
U = 2.0 ** -24
SLACK = 1 + 1e-3


def _ix(a):
    return torch.from_numpy(np.asarray(a, np.int64))


def _seg(ptr, vals):
    """sum of vals (per slot) over the slots of every row"""
    n = len(ptr) - 1
    shape = (n,) + tuple(vals.shape[1:])
    return torch.zeros(shape, dtype=F64).index_add_(0, sref.slot_rows(ptr), vals)


def slots(ptr):
    return _ix(np.diff(np.asarray(ptr, np.int64))).to(F64)


# ---- cal_gcn_norm_fwd ---------------------------------------------------------------------------------------------------
def norm_fwd(ptr_src, eid_src, row, col, w, loop_w):
    """-> dis [N], norm_e [E], deg [N], M [N] (sum |w| + |loop_w| of the row)"""
    N, E = len(ptr_src) - 1, len(row)
    ws = (w.to(F64) if w is not None else torch.ones(E, dtype=F64))[_ix(eid_src)]
    deg = _seg(ptr_src, ws) + float(loop_w)
    M = _seg(ptr_src, ws.abs()) + abs(float(loop_w))
    dis = torch.where(deg == 0, torch.zeros_like(deg), deg ** -0.5)
    return dis, norm_e_from(dis, row, col, w), deg, M


def dis_bound(dis, deg, M, nslots):
    rel = ((nslots + 8) * U * M / deg.abs().clamp_min(1e-300) + 2 * U) * SLACK
    return torch.where(deg == 0, torch.zeros_like(deg), dis.abs() * rel)


def norm_e_from(dis, row, col, w):
    r, c = _ix(row), _ix(col)
    dis = dis.to(F64)
    we = w.to(F64) if w is not None else torch.ones(len(row), dtype=F64)
    return torch.where(r != c, dis[r] * we * dis[c], torch.zeros(len(row), dtype=F64))


# ---- cal_spmm_fwd -------------------------------------------------------------------------------------------------------
def spmm(ptr, nbr, eid, norm_e, dis, loop_w, h, bias, relu):
    """-> out, T, n.  out[i] = act(sum_s norm_e[eid[s]] h[nbr[s]] + dis[i] loop_w dis[i] h[i] + bias)"""
    N = len(ptr) - 1
    d = dis.to(F64)
    return sref.aggregate(ptr, nbr, eid, h, torch.ones(N, dtype=F64), norm_e, d * d * float(loop_w), bias, relu)


def spmm_bound(T, n):
    return (n + 5).to(F64)[:, None] * U * T * SLACK


# ---- cal_relu_bwd_colsum ------------------------------------------------------------------------------------------------
def relu_bwd_colsum(dout, y):
    """-> dz (exact), dbias, sum |dz| per column"""
    g = dout.to(F64)
    dz = g if y is None else torch.where(y > 0, g, torch.zeros_like(g))
    return dz, dz.sum(0), dz.abs().sum(0)


def colsum_bound(mag, N):
    return max(N - 1, 0) * U * mag * SLACK


# ---- cal_gcn_norm_bwd ---------------------------------------------------------------------------------------------------
def sddmm(ptr_dst, nbr_dst, eid_dst, h, dz, E):
    """-> gn [E] (NaN where an edge has no slot), gself [N], and their sums of |a_k b_k|"""
    return sref.sddmm(ptr_dst, nbr_dst, eid_dst, h, dz, E)


def dot_bound(mag, H):
    return (H + 1) * U * mag * SLACK


def norm_bwd_node(src, dst, w, dis, loop_w, gn_e, gself):
    """src, dst: (ptr, nbr, eid).  -> ddeg [N], its bound"""
    d, gn = dis.to(F64), gn_e.to(F64)
    acc = mag = 0.0
    for ptr, nbr, eid in (src, dst):
        e = _ix(eid)
        t = gn[e] * (w.to(F64)[e] if w is not None else 1.0) * d[_ix(nbr)]
        acc, mag = acc + _seg(ptr, t), mag + _seg(ptr, t.abs())
    own = 2.0 * gself.to(F64) * d * float(loop_w)
    ddeg = -0.5 * d * d * d * (acc + own)
    M = 0.5 * d.abs() ** 3 * (mag + own.abs())
    return ddeg, (slots(src[0]) + slots(dst[0]) + 8) * U * M * SLACK


def norm_bwd_edge(row, col, dis, gn_e, ddeg):
    """-> dw [E] (0 on the self-loop columns), its bound"""
    r, c = _ix(row), _ix(col)
    d, z = dis.to(F64), torch.zeros(len(row), dtype=F64)
    p = gn_e.to(F64) * d[r] * d[c]
    keep = r != c
    dw = torch.where(keep, p + ddeg.to(F64)[r], z)
    return dw, torch.where(keep, 5 * U * (p.abs() + ddeg.to(F64)[r].abs()) * SLACK, z)


def norm_bwd(src, dst, row, col, w, dis, loop_w, h, dz):
    """the whole launcher in fp64 -> gn_e, gself, ddeg, dw"""
    gn, gself, _, _ = sddmm(*dst, h, dz, len(row))
    ddeg, _ = norm_bwd_node(src, dst, w, dis, loop_w, gn, gself)
    return gn, gself, ddeg, norm_bwd_edge(row, col, dis, gn, ddeg)[0]


# ---- two-class softmax --------------------------------------------------------------------------------------------------
def softmax2_bound(a, logits, L, nround, x):
    """a, logits, L: [..., 2] (the reference, its logits, the magnitudes behind the logits); x: relative error of expf"""
    gap = (logits[..., 0] - logits[..., 1]).abs()
    h = nround * U * L.sum(-1) + U * gap + x
    return a * (2 * h + 3 * U)[..., None] * SLACK


# ---- cal_edge_att_fwd / _bwd --------------------------------------------------------------------------------------------
def edge_proj(x, W):
    """-> pq [N, 4] = (x.W[0,:H], x.W[1,:H], x.W[0,H:], x.W[1,H:]), sum |x_k W_k|"""
    x, W = x.to(F64), W.to(F64)
    H = x.shape[1]
    Wm = torch.stack([W[0, :H], W[1, :H], W[0, H:], W[1, H:]], 1)            # [H, 4]
    return x @ Wm, x.abs() @ Wm.abs()


def edge_att_from_pq(pq, b, row, col):
    """-> att [E, 2], logits [E, 2], L [E, 2] (every input edge, self loops included: the kernel is per edge)"""
    pq, b = pq.to(F64), b.to(F64)
    r, c = _ix(row), _ix(col)
    logits = pq[r, 0:2] + pq[c, 2:4] + b
    L = pq[r, 0:2].abs() + pq[c, 2:4].abs() + b.abs()
    return torch.softmax(logits, -1), logits, L


def edge_att_bwd(x, W, att, datt, src, dst, base):
    """att, datt [2, E]; src, dst: (ptr, eid); base: dx before the call (accumulate) or None.
    -> (dx, dW [2, 2H], db [2]), their bounds"""
    x, W, att, datt = x.to(F64), W.to(F64), att.to(F64), datt.to(F64)
    N, H = x.shape
    dl = att[0] * att[1] * (datt[0] - datt[1])
    A = att[0] * att[1] * (datt[0].abs() + datt[1].abs())
    (ps, es), (pd, ed) = src, dst
    sp, SAp, n = _seg(ps, dl[_ix(es)]), _seg(ps, A[_ix(es)]), slots(ps)
    sq, SAq, m = _seg(pd, dl[_ix(ed)]), _seg(pd, A[_ix(ed)]), slots(pd)
    wp, wq = W[0, :H] - W[1, :H], W[0, H:] - W[1, H:]
    Wp, Wq = W[0, :H].abs() + W[1, :H].abs(), W[0, H:].abs() + W[1, H:].abs()
    b0 = torch.zeros(N, H, dtype=F64) if base is None else base.to(F64)
    dx = b0 + sp[:, None] * wp + sq[:, None] * wq
    bdx = U * (((n + 7) * SAp)[:, None] * Wp + ((m + 7) * SAq)[:, None] * Wq + 4 * b0.abs()) * SLACK
    ax = x.abs()
    dW0 = torch.cat([sp @ x, sq @ x])
    bW0 = U * torch.cat([((N + n + 4) * SAp) @ ax, ((N + m + 4) * SAq) @ ax]) * SLACK
    db0 = sp.sum()
    bb0 = U * ((N + n + 2) * SAp).sum() * SLACK
    return ((dx, torch.stack([dW0, -dW0]), torch.stack([db0, -db0])),
            (bdx, torch.stack([bW0, bW0]), torch.stack([bb0, bb0])))


# ---- cal_node_att_split_fwd / _bwd --------------------------------------------------------------------------------------
def node_att(x, Wn, bn):
    """-> att_n [N, 2], logits, L"""
    x, Wn, bn = x.to(F64), Wn.to(F64), bn.to(F64)
    logits = x @ Wn.t() + bn
    return torch.softmax(logits, -1), logits, x.abs() @ Wn.abs().t() + bn.abs()


def node_split_from(att_n, x):
    """-> xc, xo in fp64 on the given (stored) att_n; bound u |ref|"""
    a, x = att_n.to(F64), x.to(F64)
    return a[:, 0:1] * x, a[:, 1:2] * x


def node_att_bwd(x, Wn, att_n, dxc, dxo):
    """-> (dx, dWn [2, H], dbn [2]), their bounds"""
    x, Wn, a, dxc, dxo = (t.to(F64) for t in (x, Wn, att_n, dxc, dxo))
    N, H = x.shape
    a0, a1 = a[:, 0], a[:, 1]
    d0, d1 = (x * dxc).sum(1), (x * dxo).sum(1)
    Q = a0 * a1 * ((x * dxc).abs().sum(1) + (x * dxo).abs().sum(1))
    dl = a0 * a1 * (d0 - d1)
    w0, Wm = Wn[0] - Wn[1], Wn[0].abs() + Wn[1].abs()
    dx = a0[:, None] * dxc + a1[:, None] * dxo + dl[:, None] * w0
    bdx = U * (5 * (a0[:, None] * dxc.abs() + a1[:, None] * dxo.abs()) + (H + 10) * Q[:, None] * Wm) * SLACK
    dW0, bW0 = dl @ x, U * (N + H + 7) * (Q @ x.abs()) * SLACK
    db0, bb0 = dl.sum(), U * (N + H + 5) * Q.sum() * SLACK
    return ((dx, torch.stack([dW0, -dW0]), torch.stack([db0, -db0])),
            (bdx, torch.stack([bW0, bW0]), torch.stack([bb0, bb0])))


# ---- cal_add_pool_fwd / _bwd --------------------------------------------------------------------------------------------
def add_pool(x, gptr):
    """-> out [B, H], its bound"""
    s, mag, _, n = sref.pool(x, gptr)
    return s, (n.to(F64) - 1).clamp_min(0)[:, None] * U * mag * SLACK


def add_pool_bwd(dout, batch):
    return dout[_ix(batch)]


# ---- cal_plan_build / cal_graph_ptr -------------------------------------------------------------------------------------
PLAN_KEYS = ("rowptr_dst", "nbr_dst", "eid_dst", "rowptr_src", "nbr_src", "eid_src", "row32", "col32")


def plan(ei, N):
    """stable counting sort of the edges by destination and by source, self loops dropped; an edge with an index outside
    [0, N) sets status bit 0 and becomes the dropped self loop (0, 0)"""
    ei = np.asarray(ei, np.int64)
    bad = ((ei < 0) | (ei >= N)).any(0)
    ei = np.where(bad[None, :], 0, ei)
    out = {"row32": ei[0].astype(np.int32), "col32": ei[1].astype(np.int32), "status": int(bad.any())}
    for name, key in (("dst", 1), ("src", 0)):
        out["rowptr_" + name], out["nbr_" + name], out["eid_" + name] = sref.csr_view(ei, N, key)
    return out


def graph_ptr(batch, B):
    """gptr[b] = first node whose graph id is >= b (batch sorted, ids in [0, B))"""
    return np.searchsorted(np.asarray(batch, np.int64), np.arange(B + 1), side="left").astype(np.int32)


def graph_ptr_valid(batch, B):
    b = np.asarray(batch, np.int64)
    return bool((np.diff(b) >= 0).all() and (b >= 0).all() and (b < B).all())


# ---- the comparison every judge uses ------------------------------------------------------------------------------------
def compare(name, got, want, bound, rat, fails, tag=""):
    """got within bound of want, NaN exactly where want has NaN; a bound of 0 asks for equality.  Records the worst
    err / bound under rat[name]."""
    got, want, bound = got.to(F64).reshape(-1), want.to(F64).reshape(-1), bound.to(F64).reshape(-1)
    assert got.shape == want.shape == bound.shape, (name, got.shape, want.shape, bound.shape)
    if got.numel() == 0:
        rat.setdefault(name, 0.0)
        return
    gn, wn = torch.isnan(got), torch.isnan(want)
    if not torch.equal(gn, wn):
        fails.append("%s %s: NaN in %d places where the reference has none, missing in %d" % (tag, name, int((gn & ~wn).sum()), int((wn & ~gn).sum())))
        rat[name] = float("inf")
        return
    ok = ~wn
    if not bool(torch.isfinite(got[ok]).all()):
        fails.append("%s %s: %d infinite entries" % (tag, name, int((~torch.isfinite(got[ok])).sum())))
        rat[name] = float("inf")
        return
    err, bnd = (got[ok] - want[ok]).abs(), bound[ok]
    bad = err > bnd
    pos = bnd > 0
    r = float((err[pos] / bnd[pos]).max()) if bool(pos.any()) else 0.0
    if bool((~pos & (err > 0)).any()):
        r = float("inf")
    rat[name] = max(rat.get(name, 0.0), r)
    if bool(bad.any()):
        fails.append("%s %s: err/bound %.3e, %d entries over, largest error %.3e" % (tag, name, r, int(bad.sum()), float(err.max())))


def exact(name, got, want, rat, fails, tag=""):
    """bitwise equal as values (NaN matches NaN)"""
    same = torch.equal(torch.nan_to_num(got.reshape(-1).to(F64), nan=1.25e300), torch.nan_to_num(want.reshape(-1).to(F64), nan=1.25e300))
    rat[name] = max(rat.get(name, 0.0), 0.0 if same else float("inf"))
    if not same:
        fails.append("%s %s: not exactly the reference" % (tag, name))

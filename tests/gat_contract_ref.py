"""Float64 restatement of the GATConv kernels of csrc/gat.hip over the kernels' own operands -- CSR views (self loops of the
input dropped: they carry no slot; one loop per node added, slot id E + i), z [N, K D], att [K, 2 D] (first D: target half),
bias, relu, slope, p and a keep mask [(E + N), K] -- and the error bounds tests/test_gpu_gat_contract.py holds the kernels to.
tests/test_gat_contract_ref.py ties it to oracle.cal_oracle.gat_conv, to torch autograd and to libcalhost's dropout mask, and
shows that the bounds notice ten seeded defects.  Vectorised torch on the CPU; index arrays are numpy.

  forward   l_s = lrelu(a_dst[i] + a_src[j_s]); alpha_s = exp(l_s - mx_i) / den_i, den_i = sum_s exp(l_s - mx_i) + 1e-16 over the
            row's slots and the node's own loop; out_i = sum_s alpha_s keep_s / (1 - p) z[j_s] + bias (ReLU).
  backward  takes the state (a_dst, a_src, mx, den) AS GIVEN -- the test passes the fp32 arrays the backward kernels read; the
            sign of an fp32 a_dst + a_src is the sign of the exact sum, so the LeakyReLU derivative is decided identically --:
            dalpha_s = keep_s / (1 - p) <g_i, z_j>, S_i = sum_s alpha_s dalpha_s, draw_s = alpha_s (dalpha_s - S_i) lrelu'(raw_s),
            dadst_i = sum over the row, dasrc_j = sum over the slots that gather j (and j's loop),
            dz_j = sum alpha~_s g[dst_s] + dadst_j att_d + dasrc_j att_s, datt = (sum_v dadst_v z_v, sum_v dasrc_v z_v).
  keep_mask mix32 / keep_scale of csrc/gat_common.hpp in numpy uint32 arithmetic (exact), step_seed in Python integers.

Bounds (class Judge), u = 2^-24, x = the relative error of the device's exponential (measured by the GPU test, at least one
ulp = 2 u); every constant counts roundings of the kernels, none is fitted to an output.  Per row i and head: n = deg + 1 terms,
nb = ceil(deg / 4) batches of the online softmax, A_d[i] = sum_d |z att_d|, A_s[j] = sum_d |z att_s|.

  adst, asrc  an fp32 dot of D products in any order: (D + 1) u A.
  logit       E = (D + 3) u A for a score as a kernel uses it (the dot; in the wave family also the log2(e) pre-scaling of att_s
              and the scaling of the finished a_dst), then the add and the slope multiply:
              dl_s = E_d[i] + E_s[j] + 2 u |l_s|.
  mx          within the largest logit error of the row, plus the log2(e) scaling and un-scaling with rounded constants:
              max_s dl_s + 3 u |mx|.
  term        exp(l_s - m) as a relative error t_i: the logit error, the roundings of the exponent -- scaling by log2(e), the
              subtraction, the un-scaled stored maximum: at most 10 u M_i, M_i = max_s |l_s| --, the exponential x, and for every
              batch one rescale by exp2(m - m') (x, one multiply, one add: x + 2 u; the roundings of the exponents m - m' add
              up to at most u times the total rise, inside the 10 u M):  t_i = max_s dl_s + 10 u M_i + x + nb (x + 2 u).
  den         against the fp64 sum of exp(l_s - mx) formed from the kernel's OWN stored adst, asrc, mx, so the error of the
              maximum does not enter twice; a stored and a recomputed score are each within E of the exact one, so dl'_s =
              2 (E_d[i] + E_s[j]) + 2 u |l_s|:  den' (t'_i + (n + 1) u) + n 2^-126.  The last term is the wave forward's bare
              v_exp_f32, which flushes a term below 2^-126 of the row maximum (exp2f returns the subnormal): at most 2^-126 per
              term against a denominator >= 1.
  out         alpha_s carries the term's error and the denominator's (t + n u), the sum of n products n u, and six more
              roundings (1 / den, the scale, keep / (1 - p), the coefficient product, the bias add, one spare):
              T (2 t_i + (2 n + 6) u) + n 2^-126 max|z| / (1 - p), T = sum alpha~ |z_j| + |bias|.  ReLU needs no exclusion.
  draw        on the fp32 state: alpha_s is off by r_s = u (|raw_s| + |l_s| + 3 |l_s - m|) + x + 3 u relatively (the add, the slope,
              the subtraction, the scaling, exp2, 1 / den or v_rcp_f32, the product), dalpha_s by Da_s = (D + 2) u keep/(1-p)
              sum_d |g z|, S by DS = sum_s alpha_s (|dalpha_s| (r_s + (n + 1) u) + Da_s); the cancellation in dalpha - S enters
              as an absolute term:  lrelu' (alpha_s (Da_s + DS) + |alpha_s (dalpha_s - S)| (r_s + 3 u)).
  dadst, dasrc  the sum of those bounds over the row (dst / src view) plus (n - 1) u sum |draw_s| for the order of the sum.
  dz          against the reference formed from the kernel's OWN dadst, dasrc: sum alpha~ |g| (r_s + 2 u) + (n_src + 3) u (sum alpha~
              |g| + |dadst att_d| + |dasrc att_s|).
  datt        an fp32 sum over N rows in blocks, then over blocks, against fp64 from the kernel's OWN dadst, dasrc:
              N u sum_v |dadst z|.
  underflow   the backward's alpha of a slot far below the row maximum (the ascending set) is below 2^-126 and may arrive as 0,
              as may a product of it: 2^-126 per such value, carried through the same formulas (fl_e / fl_l in Judge.grads; one
              per output element of dadst, dasrc, dz's coefficients and the N products of datt).  Relative to the bounds above
              it only matters where the exact result is itself in the subnormal range.
"""
import types

import numpy as np
import torch

from tests import sparse_contract_ref as sref

F64 = torch.float64
U = 2.0 ** -24
FLUSH = 2.0 ** -126
GOLDEN = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1


def _idx(a):
    return torch.from_numpy(np.asarray(a, np.int64))


def _lrelu(v, slope):
    return torch.where(v > 0, v, slope * v)


def _seg_max(own, ri, per_slot):
    """max over the node's own value and its slots' values; [N, K]"""
    return own.scatter_reduce(0, ri[:, None].expand(-1, own.shape[1]), per_slot, "amax", include_self=True)


def _seg_sum(n_rows, idx, per_slot):
    return torch.zeros((n_rows,) + tuple(per_slot.shape[1:]), dtype=F64).index_add_(0, idx, per_slot)


# ---- the dropout mask ------------------------------------------------------------------------------------------------------
def step_seed(seed, ctr):
    """step_seed of csrc/gat_common.hpp: the seed a launch with the device counter at `ctr` uses"""
    return (seed + ctr * GOLDEN) & M64


def _mix32(x):
    x = x ^ (x >> np.uint32(16)); x = x * np.uint32(0x21F0AAAD)
    x = x ^ (x >> np.uint32(15)); x = x * np.uint32(0x735A2D97)
    return x ^ (x >> np.uint32(15))


def keep_mask(seed, E, N, K, p):
    """-> float32 [(E + N), K] of 1 / 0: keep_scale(seed, id, k, K, p, 1) for every slot id (edge e, loop E + i) and head"""
    n = (E + N) * K
    if p <= 0:
        return np.ones((E + N, K), np.float32)
    seed &= M64
    key = np.arange(n, dtype=np.uint64).astype(np.uint32)                 # id * K + k, truncated to 32 bits
    r = _mix32(_mix32(key + np.uint32(seed & 0xFFFFFFFF)) ^ np.uint32(seed >> 32))
    val = r.astype(np.float32) * np.float32(2.0 ** -32)
    return (val >= np.float32(p)).astype(np.float32).reshape(E + N, K)


# ---- the reference ---------------------------------------------------------------------------------------------------------
def forward(ptr, nbr, eid, z, att, bias, relu, slope, p, keep, K, D, E):
    """-> namespace: out [N, K D], adst, asrc, mx, den [N, K], alpha [(E + N), K] per slot id (NaN where an edge has no slot),
    and what the bounds need (T, the logits le [nnz, K] / ll [N, K], pre = out before the ReLU)"""
    N = len(ptr) - 1
    z3, a = z.to(F64).reshape(N, K, D), att.to(F64).reshape(K, 2 * D)
    ri, nb, ed = sref.slot_rows(ptr), _idx(nbr), _idx(eid)
    adst, asrc = (z3 * a[:, :D]).sum(-1), (z3 * a[:, D:]).sum(-1)
    le, ll = _lrelu(adst[ri] + asrc[nb], slope), _lrelu(adst + asrc, slope)
    mx = _seg_max(ll, ri, le)
    pe, pl = torch.exp(le - mx[ri]), torch.exp(ll - mx)
    den = pl + _seg_sum(N, ri, pe) + 1e-16
    inv = 1.0 / (1.0 - p) if p > 0 else 1.0
    kf = torch.ones(E + N, K, dtype=F64) if keep is None else torch.as_tensor(keep).to(F64).reshape(E + N, K)
    ae, al = pe / den[ri], pl / den
    ce, cl = ae * kf[ed] * inv, al * kf[E:] * inv
    pre = _seg_sum(N, ri, ce[:, :, None] * z3[nb]) + cl[:, :, None] * z3
    T = _seg_sum(N, ri, ce.abs()[:, :, None] * z3[nb].abs()) + cl.abs()[:, :, None] * z3.abs()
    if bias is not None:
        pre = pre + bias.to(F64).reshape(K, D)
        T = T + bias.to(F64).reshape(K, D).abs()
    alpha = torch.full((E + N, K), float("nan"), dtype=F64)
    alpha[ed] = ae
    alpha[E:] = al
    pre = pre.reshape(N, K * D)
    return types.SimpleNamespace(out=torch.relu(pre) if relu else pre, adst=adst, asrc=asrc, mx=mx, den=den, alpha=alpha,
                                 T=T.reshape(N, K * D), le=le, ll=ll, pre=pre)


def backward(ptr, nbr, eid, z, att, adst, asrc, mx, den, gout, slope, p, keep, K, D, E):
    """by-destination CSR (the by-source view holds the same slots); the state as given.
    -> namespace: draw [(E + N), K] per slot id (NaN where an edge has no slot), dadst, dasrc [N, K], dz [N, K D], datt [K, 2 D],
    dbias [K D], and the per-slot pieces (a_e / a_l, dal_e / dal_l, S, lr_e / lr_l, raw_e / raw_l, le / ll)"""
    N = len(ptr) - 1
    z3, a, g = z.to(F64).reshape(N, K, D), att.to(F64).reshape(K, 2 * D), gout.to(F64).reshape(N, K, D)
    adst, asrc, mx, den = (t.to(F64).reshape(N, K) for t in (adst, asrc, mx, den))
    ri, nb, ed = sref.slot_rows(ptr), _idx(nbr), _idx(eid)
    inv = 1.0 / (1.0 - p) if p > 0 else 1.0
    kf = torch.ones(E + N, K, dtype=F64) if keep is None else torch.as_tensor(keep).to(F64).reshape(E + N, K)
    raw_e, raw_l = adst[ri] + asrc[nb], adst + asrc
    le, ll = _lrelu(raw_e, slope), _lrelu(raw_l, slope)
    a_e, a_l = torch.exp(le - mx[ri]) / den[ri], torch.exp(ll - mx) / den
    dal_e, dal_l = (g[ri] * z3[nb]).sum(-1) * kf[ed] * inv, (g * z3).sum(-1) * kf[E:] * inv
    S = a_l * dal_l + _seg_sum(N, ri, a_e * dal_e)
    one = torch.ones((), dtype=F64)
    lr_e, lr_l = torch.where(raw_e > 0, one, one * slope), torch.where(raw_l > 0, one, one * slope)
    dr_e, dr_l = a_e * (dal_e - S[ri]) * lr_e, a_l * (dal_l - S) * lr_l
    draw = torch.full((E + N, K), float("nan"), dtype=F64)
    draw[ed] = dr_e
    draw[E:] = dr_l
    dadst, dasrc = dr_l + _seg_sum(N, ri, dr_e), dr_l + _seg_sum(N, nb, dr_e)
    ce, cl = a_e * kf[ed] * inv, a_l * kf[E:] * inv
    dz = _seg_sum(N, nb, ce[:, :, None] * g[ri]) + cl[:, :, None] * g + dadst[:, :, None] * a[:, :D] + dasrc[:, :, None] * a[:, D:]
    datt = torch.cat([(dadst[:, :, None] * z3).sum(0), (dasrc[:, :, None] * z3).sum(0)], -1)
    return types.SimpleNamespace(draw=draw, dadst=dadst, dasrc=dasrc, dz=dz.reshape(N, K * D), datt=datt,
                                 dbias=gout.to(F64).reshape(N, K * D).sum(0), a_e=a_e, a_l=a_l, dal_e=dal_e, dal_l=dal_l, S=S,
                                 lr_e=lr_e, lr_l=lr_l, raw_e=raw_e, raw_l=raw_l, le=le, ll=ll, ce=ce, cl=cl)


# ---- the bounds ------------------------------------------------------------------------------------------------------------
class Judge:
    """the reference and the bounds of one operand set (module docstring); every method -> {name: (|got - want|, bound)}"""

    def __init__(self, ptr, nbr, eid, z, att, bias, relu, slope, p, keep, K, D, E, x):
        self.a = (ptr, nbr, eid)
        self.z, self.att, self.slope, self.p, self.keep, self.K, self.D, self.E, self.x = z, att, slope, p, keep, K, D, E, max(x, 2 * U)
        N = self.N = len(ptr) - 1
        self.f = forward(ptr, nbr, eid, z, att, bias, relu, slope, p, keep, K, D, E)
        self.z3, self.a2 = z.to(F64).reshape(N, K, D), att.to(F64).reshape(K, 2 * D)
        self.ri, self.nb, self.ed = sref.slot_rows(ptr), _idx(nbr), _idx(eid)
        self.Ad, self.As = (self.z3 * self.a2[:, :D]).abs().sum(-1), (self.z3 * self.a2[:, D:]).abs().sum(-1)
        deg = _idx(np.diff(np.asarray(ptr, np.int64)))
        self.n = (deg + 1).to(F64)[:, None]
        self.nbat = ((deg + 3) // 4).to(F64)[:, None]
        self.inv = 1.0 / (1.0 - p) if p > 0 else 1.0
        self.kf = torch.ones(E + N, K, dtype=F64) if keep is None else torch.as_tensor(keep).to(F64).reshape(E + N, K)

    def _term(self, le, ll, scores):
        """(max_s dl_s, t_i) from the logits; scores: how often the dot bound E enters a logit"""
        ri, nb = self.ri, self.nb
        Ed, Es = (self.D + 3) * U * self.Ad, (self.D + 3) * U * self.As
        dl = _seg_max(scores * (Ed + Es) + 2 * U * ll.abs(), ri, scores * (Ed[ri] + Es[nb]) + 2 * U * le.abs())
        M = _seg_max(ll.abs(), ri, le.abs())
        return dl, dl + 10 * U * M + self.x + self.nbat * (self.x + 2 * U)

    def state(self, adst, asrc, mx, den):
        f, ri, nb = self.f, self.ri, self.nb
        adst, asrc, mx, den = (t.to(F64).reshape(self.N, self.K) for t in (adst, asrc, mx, den))
        dl, _ = self._term(f.le, f.ll, 1)
        r = {"adst": ((adst - f.adst).abs(), (self.D + 1) * U * self.Ad), "asrc": ((asrc - f.asrc).abs(), (self.D + 1) * U * self.As),
             "mx": ((mx - f.mx).abs(), dl + 3 * U * f.mx.abs())}
        le, ll = _lrelu(adst[ri] + asrc[nb], self.slope), _lrelu(adst + asrc, self.slope)       # from the kernel's own state
        want = torch.exp(ll - mx) + _seg_sum(self.N, ri, torch.exp(le - mx[ri]))
        _, t = self._term(le, ll, 2)
        r["den"] = ((den - want).abs(), want * (t + (self.n + 1) * U) + self.n * FLUSH)
        return r

    def out(self, out):
        f = self.f
        _, t = self._term(f.le, f.ll, 1)
        rel = (2 * t + (2 * self.n + 6) * U).repeat_interleave(self.D, 1)
        flush = (self.n * FLUSH * float(self.z3.abs().max()) * self.inv).expand(-1, self.K * self.D)
        return {"out": ((out.to(F64).reshape(self.N, -1) - f.out).abs(), f.T * rel + flush)}

    def reference_backward(self, adst, asrc, mx, den, gout):
        ptr, nbr, eid = self.a
        return backward(ptr, nbr, eid, self.z, self.att, adst, asrc, mx, den, gout, self.slope, self.p, self.keep, self.K, self.D, self.E)

    def grads(self, state, gout, draw, dadst, dasrc, dz, datt):
        """state: the fp32 (adst, asrc, mx, den) the backward kernels read; draw [(E + N), K] (NaN = never written)"""
        N, K, D, E, x, ri, nb, ed = self.N, self.K, self.D, self.E, self.x, self.ri, self.nb, self.ed
        b = self.reference_backward(*state, gout)
        g = gout.to(F64).reshape(N, K, D)
        m = state[2].to(F64).reshape(N, K)
        draw, dadst, dasrc = draw.to(F64).reshape(E + N, K), dadst.to(F64).reshape(N, K), dasrc.to(F64).reshape(N, K)
        r_e = U * (b.raw_e.abs() + b.le.abs() + 3 * (b.le - m[ri]).abs()) + x + 3 * U
        r_l = U * (b.raw_l.abs() + b.ll.abs() + 3 * (b.ll - m).abs()) + x + 3 * U
        Da_e = (D + 2) * U * self.kf[ed] * self.inv * (g[ri] * self.z3[nb]).abs().sum(-1)
        Da_l = (D + 2) * U * self.kf[E:] * self.inv * (g * self.z3).abs().sum(-1)
        n = self.n
        DS = b.a_l * (b.dal_l.abs() * (r_l + (n + 1) * U) + Da_l) + \
            _seg_sum(N, ri, b.a_e * (b.dal_e.abs() * (r_e + (n[ri] + 1) * U) + Da_e))
        # fp32 underflow: an alpha below 2^-126 may arrive as 0, and so may each of the three products behind a d(raw logit)
        sumdal = b.dal_l.abs() + _seg_sum(N, ri, b.dal_e.abs())
        fl_e = FLUSH * ((b.dal_e - b.S[ri]).abs() + b.a_e * sumdal[ri] + 3)
        fl_l = FLUSH * ((b.dal_l - b.S).abs() + b.a_l * sumdal + 3)
        b_e = b.lr_e * (b.a_e * (Da_e + DS[ri]) + (b.a_e * (b.dal_e - b.S[ri])).abs() * (r_e + 3 * U) + fl_e)
        b_l = b.lr_l * (b.a_l * (Da_l + DS) + (b.a_l * (b.dal_l - b.S)).abs() * (r_l + 3 * U) + fl_l)
        slots = torch.cat([ed, E + torch.arange(N)])
        bound = torch.cat([b_e, b_l])
        r = {"draw": ((draw[slots] - b.draw[slots]).abs(), bound)}
        dabs_e, dabs_l = b.draw[ed].abs(), b.draw[E:].abs()
        nsrc = 1 + torch.bincount(nb, minlength=N).to(F64)[:, None]
        r["dadst"] = ((dadst - b.dadst).abs(), b_l + _seg_sum(N, ri, b_e) + (n - 1) * U * (dabs_l + _seg_sum(N, ri, dabs_e)) + FLUSH)
        r["dasrc"] = ((dasrc - b.dasrc).abs(), b_l + _seg_sum(N, nb, b_e) + (nsrc - 1) * U * (dabs_l + _seg_sum(N, nb, dabs_e)) + FLUSH)
        # dz and datt against fp64 over the kernel's OWN dadst / dasrc
        ad, as_ = self.a2[:, :D], self.a2[:, D:]
        agg = _seg_sum(N, nb, b.ce[:, :, None] * g[ri]) + b.cl[:, :, None] * g
        want = agg + dadst[:, :, None] * ad + dasrc[:, :, None] * as_
        mag = _seg_sum(N, nb, b.ce[:, :, None] * g[ri].abs()) + b.cl[:, :, None] * g.abs()
        magr = _seg_sum(N, nb, (b.ce * (r_e + 2 * U))[:, :, None] * g[ri].abs()) + (b.cl * (r_l + 2 * U))[:, :, None] * g.abs()
        tot = mag + (dadst[:, :, None] * ad).abs() + (dasrc[:, :, None] * as_).abs()
        gsum = _seg_sum(N, nb, g[ri].abs()) + g.abs()
        r["dz"] = ((dz.to(F64).reshape(N, K, D) - want).abs(), magr + (nsrc[:, :, None] + 3) * U * tot + FLUSH * (self.inv * gsum + 4))
        want = torch.cat([(dadst[:, :, None] * self.z3).sum(0), (dasrc[:, :, None] * self.z3).sum(0)], -1)
        mag = torch.cat([(dadst[:, :, None] * self.z3).abs().sum(0), (dasrc[:, :, None] * self.z3).abs().sum(0)], -1)
        r["datt"] = ((datt.to(F64).reshape(K, 2 * D) - want).abs(), N * U * mag + N * FLUSH)
        return r, b


def datt_bound(z, dadst, dasrc, N, K, D):
    """(want, bound) of d att from given dadst / dasrc (the `part_out` rows are judged against the public call's datt)"""
    z3 = z.to(F64).reshape(N, K, D)
    dadst, dasrc = dadst.to(F64).reshape(N, K), dasrc.to(F64).reshape(N, K)
    want = torch.cat([(dadst[:, :, None] * z3).sum(0), (dasrc[:, :, None] * z3).sum(0)], -1)
    mag = torch.cat([(dadst[:, :, None] * z3).abs().sum(0), (dasrc[:, :, None] * z3).abs().sum(0)], -1)
    return want, N * U * mag + N * FLUSH


def worst(results, rat=None, fails=None, tag=""):
    """largest err / bound over a dict of (err, bound); a non-finite error or an error over a zero bound counts as inf.
    Fills rat {name: worst ratio} and fails [messages]."""
    top = 0.0
    for name, (err, bound) in results.items():
        if not bool(torch.isfinite(err).all()):
            r = float("inf")
        else:
            pos = bound > 0
            r = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
            if bool((err[~pos] > 0).any()):
                r = float("inf")
        if rat is not None:
            rat[name] = max(rat.get(name, 0.0), r)
        if fails is not None and not r <= 1.0:
            over = int((~(err <= bound)).sum())
            fails.append("%s: %s err/bound %.3e (%d entries over)" % (tag, name, r, over))
        top = max(top, r)
    return top

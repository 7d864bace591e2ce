"""fp64 contract of the step's Adam update -- TEST INFRASTRUCTURE, independent of cal_amd: the reference formula, its fp32
restatement, a derived per-element error bound, seeded defects and the case table tests/test_adam_oracle.py (CPU) and
tests/test_gpu_adam_contract.py (HIP: ``adam_update`` inside ``k_finish``, ``k_adam``) share.

The update (engine_kernels.hpp: ``adam_update`` / ``k_adam``; torch.optim.Adam semantics), per element, ``t`` = the step count
AFTER the advance:

    gi    = g * gscale + wd * p
    m1    = b1 * m0 + (1 - b1) * gi                v1 = b2 * v0 + (1 - b2) * gi * gi
    bc1   = 1 - b1^t                               bc2 = 1 - b2^t
    denom = sqrt(v1) / sqrt(bc2) + eps             p1 = p - (lr / bc1) * (m1 / denom)          (D = p1 - p, "the update")

``adam_ref`` evaluates it in fp64 on the fp32 inputs with the hyper-parameters AS THE ENGINE HOLDS THEM (fp32 values: the
C entry points take ``float``), so that ``bound`` measures arithmetic only; the distance to torch's Python-double
hyper-parameters is the representation gap below.

The bound (``bound``) -- derived by counting the roundings of ``adam_update``, not fitted.  u = 2^-24 is half an fp32 ulp
relative, h = 2^-150 half the subnormal ulp (a result below 2^-126 is rounded to a multiple of 2^-149; gfx950 code built by
hipcc keeps fp32 subnormals).  Every +, -, * and fmaf is correctly rounded: u |result| + h.  The library is built without
-ffast-math and without -fno-hip-fp32-correctly-rounded-divide-sqrt, so hipcc's default holds: fp32 ``/`` and ``sqrtf`` are
correctly rounded too (the disassembly of k_adam shows, for each of its three divisions, the v_div_scale / v_div_fmas /
v_div_fixup sequence and, for each of its two roots, a scaled v_sqrt_f32 followed by the two fma residuals that pick among
the neighbouring values -- not a bare v_rcp_f32 / v_sqrt_f32) -- u each.  ``powf`` is OCML's, documented
at 1 ulp = 2u.  Contraction to fma (-ffp-contract=on) only removes roundings.  With A' = 1 + 2^-12 covering the products of
two relative errors (each link of the chain is below 2^-13, see rho below):

    E_gi  = u (|g gscale| + |wd p| + |gi|) + 3h                                (product, product, sum; fmaf has one fewer)
    E_m1  = A' [ 2u |b1 m0| + 3u |(1-b1) gi| + (1-b1) E_gi + 3h ]              (1-b1, two products, sum -- in terms of the two
                                                                                terms, not of m1: they may cancel)
    E_v1  = A' [ 2u b2 v0 + 4u (1-b2) gi^2 + (1-b2)(2 |gi| E_gi + E_gi^2) + 3h ]
    e_bc  = (2 k(b,t) + 1) u + h / bc,     k(b,t) = b^t / (1 - b^t)            (powf's 2u on b^t, magnified by the condition
                                                                                number of 1 - x at x = b^t; the subtraction)
    E_sq  = min(E_v1 / sqrt(v1), sqrt(E_v1)) + u sqrt(v1) + h                  (|sqrt a - sqrt b| <= both; the second when v1
                                                                                underflowed to 0)
    E_den = E_sq / sqrt(bc2) + (sqrt(v1)/sqrt(bc2)) (e_bc2 / 2 + 2u) + h + u denom + h
    E_D   = A' [ |D| (e_bc1 + 3u + E_den / denom) + (lr / bc1) E_m1 / denom + 2h max(1, lr / bc1) ]
    E_p1  = ulp(p1) / 2 + E_D

that is ``ulp(p1)/2 + |D| rho`` with rho = e_bc1 + 3u + E_den/denom + E_m1/|m1|: the first two terms depend on (b1, t) only,
the last two are the element's own (E_m1 / |m1| is unbounded where the two terms of m1 cancel, so it is carried as the
product (lr/bc1) E_m1 / denom).  The uniform part of rho, (2 k(b1,t) + 4 + k(b2,t) + 4.5) u, is

    t = 1:      (b1, b2) = (0.9, 0.999): 1026 u = 6.1e-5     (0.8, 0.99): 116 u     (0, 0.999): 1008 u
    t = 10:     (0.9, 0.999): 109 u      t = 1000: 9.1 u     t = 2^20: 8.5 u

(at t = 1 almost all of it is the allowance for powf(b2, 1) being one ulp off b2, which the subtraction 1 - b2 magnifies
999 times).  Measured on the CPU over every case of ``CASES`` at 3000 elements (tests/test_adam_oracle.py prints both):

    fp32 restatement (``adam_fp32``, numpy float32 operation by operation, np.power in float32) against ``adam_ref``,
    largest error / bound:   m1 0.94   v1 0.99   p1 1.00
    (the bound is sharp: v1's 0.99 is an element whose product b2 v0 and whose sum are both rounded by almost half an ulp, p1's
    1.00 an element whose update is 0.99999 of half an ulp of p and is rounded away)

The representation gap (``gap_bound``): the same chain with the roundings switched off and the hyper-parameters perturbed by
their actual fp32 representation errors d_x = |fp32(x) - x|: E_gi = d_gscale |g| + d_wd |p|, E_m1 = d_b1 (|m0| + |gi|) +
(1-b1) E_gi, E_v1 = d_b2 (v0 + gi^2) + ..., e_bc = k(b,t) ((1 + d_b/b)^t - 1) ~ t k(b,t) d_b / b, E_eps = d_eps,
e_lr = d_lr / lr.  Measured on the CPU over every case of ``CASES``: |adam_ref(fp32-held) - adam_ref(double)| reaches but
never exceeds ``gap_bound`` (largest ratio 1.00 on m1, v1 and p1: the bound uses the actual d_x), and the largest gap of an
update, |D_fp32 - D_double| / |D|, over the elements and cases without a cancellation (m0 gi >= 0, wd = 0) is

    (b1, b2) = (0.9, 0.999):  6.7e-6 at t = 1, 2, 3;  6.5e-6 at t = 10;  3.7e-6 at t = 1000;  6.7e-6 at t = 2^20
    (0, 0.999):               6.4e-6 at t <= 10;      3.7e-6 at t = 1000;  6.5e-6 at t = 2^20
    (0.8, 0.99):              4.3e-7 at t = 1;        5.4e-7 at t >= 1000

(fp32(0.999) is 1.3e-8 above 0.999, which is 1.3e-5 of 1 - b2: at t = 1 that is the error of bc2, at large t the error of the
weight of gi^2 in v1, and the root halves it either way; lr, b1 and eps add the remaining 1e-7.)  With a cancellation the gap
of an update is unbounded relative to the update and stays inside ``gap_bound``.

-- the project's distance from torch's Python-double bias corrections.

The defects (``DEFECTS``) are wrong variants of ``adam_ref``; ``EXPOSES`` says for each on which cases it MUST leave the bound on
at least one output of at least one element and on which it CANNOT (there it is the same function); tests/test_adam_oracle.py
asserts both on the reference alone and prints the table.  No element is masked: the bound holds on all of them.
"""
import itertools

import numpy as np

U = 2.0 ** -24
H = 2.0 ** -150
A2 = 1.0 + 2.0 ** -12


def f32(x):
    """The fp32 value a C ``float`` argument holds, as a Python float."""
    return float(np.float32(x))


def half_ulp32(x):
    """ulp(x) / 2 of fp32 at ``x`` (fp64 array): 2^(e - 24) for 2^e <= |x| < 2^(e+1), 2^-150 below 2^-126."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    _, e = np.frexp(x)                       # x = f 2^e, f in [0.5, 1)
    return np.ldexp(1.0, np.maximum(e - 1, -126) - 24)


def kappa(b, t):
    """Condition number of the bias correction 1 - b^t with respect to b^t."""
    bt = float(b) ** float(t)
    return bt / (1.0 - bt) if bt < 1.0 else np.inf


# ---- the reference and its seeded defects ----------------------------------------------------------------------------------------
DEFECTS = ("t_minus_1", "t_plus_1", "adamw", "wd_updated_p", "eps_in_sqrt", "eps_before_bc2", "gscale_missing",
           "gscale_squared", "gscale_on_wd", "v_unscaled", "betas_swapped", "lr_prev", "one_skipped", "one_twice")


def adam_ref(p, g, m, v, t, lr, b1, b2, eps, wd, gscale, defect=None, lr_prev=None, elem=None):
    """fp64 Adam step -> ``(p1, m1, v1)``; ``defect`` selects a wrong variant (``lr_prev``: the stale learning rate of
    "lr_prev", ``elem``: the element "one_skipped" / "one_twice" act on)."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    t, lr, b1, b2, eps, wd, gs = (float(a) for a in (t, lr, b1, b2, eps, wd, gscale))
    if defect == "one_twice":
        p1, m1, v1 = adam_ref(p, g, m, v, t, lr, b1, b2, eps, wd, gs)
        q1, n1, w1 = adam_ref(p1, g, m1, v1, t, lr, b1, b2, eps, wd, gs)
        p1[elem], m1[elem], v1[elem] = q1[elem], n1[elem], w1[elem]
        return p1, m1, v1
    if defect == "t_minus_1":
        t -= 1.0
    if defect == "t_plus_1":
        t += 1.0
    if defect == "lr_prev":
        lr = float(lr_prev)
    gg = g if defect == "gscale_missing" else g * gs * (gs if defect == "gscale_squared" else 1.0)
    if defect == "adamw":
        gi = gg
    elif defect == "gscale_on_wd":
        gi = (g + wd * p) * gs
    elif defect == "wd_updated_p":
        gi = gg + wd * adam_ref(p, g, m, v, t, lr, b1, b2, eps, 0.0, gs)[0]
    else:
        gi = gg + wd * p
    m1 = b1 * m + (1.0 - b1) * gi
    gv = g if defect == "v_unscaled" else gi
    v1 = b2 * v + (1.0 - b2) * gv * gv
    c1, c2 = (b2, b1) if defect == "betas_swapped" else (b1, b2)
    with np.errstate(divide="ignore", invalid="ignore"):
        bc1, bc2 = np.float64(1.0 - c1 ** t), np.float64(1.0 - c2 ** t)         # (t - 1 = 0: 0, and the update is not finite)
        if defect == "eps_in_sqrt":
            denom = np.sqrt(v1 / bc2 + eps)
        elif defect == "eps_before_bc2":
            denom = (np.sqrt(v1) + eps) / np.sqrt(bc2)
        else:
            denom = np.sqrt(v1) / np.sqrt(bc2) + eps
        p1 = (p * (1.0 - lr * wd) if defect == "adamw" else p) - (lr / bc1) * m1 / denom
    if defect == "one_skipped":
        p1[elem], m1[elem], v1[elem] = p[elem], m[elem], v[elem]
    return p1, m1, v1


def adam_fp32(p, g, m, v, t, lr, b1, b2, eps, wd, gscale):
    """The same formula in numpy float32, operation by operation in ``adam_update``'s order (no fma) -> ``(p1, m1, v1)``."""
    F = np.float32
    p, g, m, v = (np.asarray(a, dtype=F) for a in (p, g, m, v))
    t, lr, b1, b2, eps, wd, gs = (F(a) for a in (t, lr, b1, b2, eps, wd, gscale))
    gi = g * gs
    if wd != 0:
        gi = wd * p + gi
    one = F(1)
    m1 = b1 * m + (one - b1) * gi
    v1 = b2 * v + ((one - b2) * gi) * gi
    bc1, bc2 = one - np.power(b1, t), one - np.power(b2, t)
    denom = np.sqrt(v1) / np.sqrt(bc2) + eps
    p1 = p - (lr / bc1) * (m1 / denom)
    assert p1.dtype == F and m1.dtype == F and v1.dtype == F
    return p1, m1, v1


# ---- the bounds ------------------------------------------------------------------------------------------------------------------
def _chain(p, g, m, v, t, lr, b1, b2, eps, wd, gs, E_m1, E_v1, e_bc1, e_bc2, E_eps, e_lr, a):
    """Error of (p1) from the errors of m1, v1, the bias corrections, eps and lr; ``a`` = 1 adds the roundings of the chain."""
    p1, m1, v1 = adam_ref(p, g, m, v, t, lr, b1, b2, eps, wd, gs)
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    sq = np.sqrt(v1)
    with np.errstate(divide="ignore", invalid="ignore"):
        d_sq = np.where(sq > 0, np.minimum(E_v1 / np.where(sq > 0, sq, 1.0), np.sqrt(E_v1)), np.sqrt(E_v1))
    E_sq = d_sq + a * (U * sq + H)
    q = sq / np.sqrt(bc2)
    den = q + eps
    E_den = E_sq / np.sqrt(bc2) + q * (e_bc2 / 2 + a * 2 * U) + a * H + E_eps + a * (U * den + H)
    D = np.abs(p1 - np.asarray(p, dtype=np.float64))
    scale = lr / bc1
    with np.errstate(divide="ignore", invalid="ignore"):
        E_D = A2 * (D * (e_lr + e_bc1 + a * 3 * U + E_den / den) + scale * E_m1 / den + a * 2 * H * max(1.0, scale))
    return a * half_ulp32(p1) + E_D


def bound(p, g, m, v, t, lr, b1, b2, eps, wd, gscale):
    """Largest |fp32 evaluation - adam_ref| a correct ``adam_update`` may show, per element -> ``dict(p=, m=, v=)`` (fp64 arrays);
    the derivation is the module docstring's."""
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    gi = g * gscale + wd * p
    E_gi = U * (np.abs(g * gscale) + np.abs(wd * p) + np.abs(gi)) + 3 * H
    E_m1 = A2 * (2 * U * np.abs(b1 * m) + 3 * U * np.abs((1 - b1) * gi) + (1 - b1) * E_gi + 3 * H)
    E_v1 = A2 * (2 * U * b2 * v + 4 * U * (1 - b2) * gi * gi + (1 - b2) * (2 * np.abs(gi) * E_gi + E_gi * E_gi) + 3 * H)
    e_bc1 = (2 * kappa(b1, t) + 1) * U + H / (1.0 - b1 ** t)
    e_bc2 = (2 * kappa(b2, t) + 1) * U + H / (1.0 - b2 ** t)
    E_p = _chain(p, g, m, v, t, lr, b1, b2, eps, wd, gscale, E_m1, E_v1, e_bc1, e_bc2, 0.0, 0.0, 1.0)
    return dict(p=E_p, m=E_m1, v=E_v1)


def rho_uniform(b1, b2, t):
    """The part of rho (module docstring) that depends on (b1, b2, t) only, in units of u."""
    return (2 * kappa(b1, t) + 1) + 3 + (2 * kappa(b2, t) + 1) / 2 + 2 + 1 + 1


def gap_bound(p, g, m, v, t, hp64, hp32):
    """Largest |adam_ref(fp32-held hyper-parameters) - adam_ref(double ones)| per element: the chain of ``bound`` without its
    roundings, perturbed by the actual representation errors.  ``hp64`` / ``hp32``: (lr, b1, b2, eps, wd, gscale)."""
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    lr, b1, b2, eps, wd, gs = (float(x) for x in hp64)
    d_lr, d_b1, d_b2, d_eps, d_wd, d_gs = (abs(float(a) - float(b)) for a, b in zip(hp32, hp64))
    gi = g * gs + wd * p
    E_gi = d_gs * np.abs(g) + d_wd * np.abs(p)
    E_m1 = A2 * (d_b1 * (np.abs(m) + np.abs(gi)) + (1 - b1) * E_gi)
    E_v1 = A2 * (d_b2 * (v + gi * gi) + (1 - b2) * (2 * np.abs(gi) * E_gi + E_gi * E_gi))
    e_bc1 = kappa(b1, t) * ((1 + d_b1 / b1) ** t - 1) if b1 > 0 else 0.0
    e_bc2 = kappa(b2, t) * ((1 + d_b2 / b2) ** t - 1) if b2 > 0 else 0.0
    E_p = _chain(p, g, m, v, t, lr, b1, b2, eps, wd, gs, E_m1, E_v1, A2 * e_bc1, A2 * e_bc2, d_eps, d_lr / lr, 0.0)
    return dict(p=E_p, m=E_m1, v=E_v1)


# ---- the cases -------------------------------------------------------------------------------------------------------------------
LR, LR_PREV = 1e-3, 1.1e-3
BETAS = ((0.9, 0.999), (0.8, 0.99), (0.0, 0.999))
EPS = (1e-8, 1e-3)
WD = (0.0, 1e-3)
GSCALE = (1.0, 0.5, 0.125)
T = (1, 2, 3, 10, 1000, 2 ** 20)
#: indices of the special elements of every state draw
SPECIAL = dict(zero=0, neg_zero=1, denormal=2, p_zero=3)
#: the element "one_skipped" / "one_twice" act on
ELEM = 11


def _cases():
    out = []
    for i, ((b1, b2), eps, wd, gs, t) in enumerate(itertools.product(BETAS, EPS, WD, GSCALE, T)):
        out.append(dict(id=i, t=t, dbl=(LR, b1, b2, eps, wd, gs), lr=f32(LR), lr_prev=f32(LR_PREV), b1=f32(b1), b2=f32(b2),
                        eps=f32(eps), wd=f32(wd), gscale=f32(gs)))
    return out


CASES = _cases()


def hp(case):
    """``(t, lr, b1, b2, eps, wd, gscale)`` of a case as the engine holds them -- the trailing arguments of adam_ref / bound."""
    return (case["t"], case["lr"], case["b1"], case["b2"], case["eps"], case["wd"], case["gscale"])


def draw_state(case, n):
    """fp32 ``(p, g, m0, v0)`` [n] of a case: |g| log-uniform over 1e-9 .. 1e1 with random signs; m0 a third each of either sign at
    the gradient's scale, within rounding of -(1-b1) gi / b1 (the two terms of m1 cancel) and 0; v0 >= 0, a quarter exactly 0;
    then the special elements (``SPECIAL``)."""
    assert n >= 16
    rng = np.random.default_rng(1000 + case["id"])
    p = (0.1 * rng.standard_normal(n)).astype(np.float32)
    g = (10.0 ** rng.uniform(-9, 1, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    gi = g.astype(np.float64) * case["gscale"] + case["wd"] * p.astype(np.float64)
    kind = rng.integers(0, 3, n)
    m = 3.0 * rng.standard_normal(n) * np.abs(g)
    if case["b1"] > 0:
        m = np.where(kind == 1, -(1.0 - case["b1"]) * gi / case["b1"], m)
    m = np.where(kind == 2, 0.0, m).astype(np.float32)
    v = (g.astype(np.float64) ** 2 * 10.0 ** rng.uniform(-1, 1, n) * (rng.integers(0, 4, n) > 0)).astype(np.float32)
    z = SPECIAL["zero"]
    g[z] = 0.0; m[z] = 0.0; v[z] = 0.0
    g[SPECIAL["neg_zero"]] = -0.0
    d = SPECIAL["denormal"]
    g[d] = 1e-40; m[d] = 0.0; v[d] = 0.0
    p[SPECIAL["p_zero"]] = 0.0
    assert g[d] != 0 and abs(float(g[d])) < 2.0 ** -126 and np.signbit(g[SPECIAL["neg_zero"]])
    return p, g, m, v


# ---- which case exposes which defect -----------------------------------------------------------------------------------------------
def _small_t(c):
    return c["t"] <= 10          # both bias corrections are far from 1 and move by >= 0.1 % per step


def _sat_t(c):
    return c["t"] == 2 ** 20     # b^t underflows for every b of BETAS: the bias corrections are exactly 1, whatever t +- 1


def _always(c):
    return True


def _never(c):
    return False


#: defect -> (must expose, cannot expose), predicates of a case; a case satisfying neither may go either way (t = 1000: b2^t
#: has left 1 - b2^t by less than some bounds) and is only printed
EXPOSES = {
    "t_minus_1": (_small_t, _sat_t),
    "t_plus_1": (_small_t, _sat_t),
    "adamw": (lambda c: c["wd"] > 0, lambda c: c["wd"] == 0),
    "wd_updated_p": (lambda c: c["wd"] > 0, lambda c: c["wd"] == 0),
    "eps_in_sqrt": (_always, _never),
    "eps_before_bc2": (_small_t, _sat_t),
    "gscale_missing": (lambda c: c["gscale"] != 1, lambda c: c["gscale"] == 1),
    "gscale_squared": (lambda c: c["gscale"] != 1, lambda c: c["gscale"] == 1),
    "gscale_on_wd": (lambda c: c["gscale"] != 1 and c["wd"] > 0, lambda c: c["gscale"] == 1 or c["wd"] == 0),
    "v_unscaled": (lambda c: c["gscale"] != 1 or c["wd"] > 0, lambda c: c["gscale"] == 1 and c["wd"] == 0),
    "betas_swapped": (_small_t, _sat_t),
    "lr_prev": (_always, _never),
    "one_skipped": (_always, _never),
    "one_twice": (_always, _never),
}


def errors(got, ref):
    """|got - ref| per output in fp64, non-finite differences as +inf -> dict(p=, m=, v=); ``got`` / ``ref``: (p1, m1, v1)."""
    out = {}
    for k, a, b in zip(("p", "m", "v"), got, ref):
        with np.errstate(invalid="ignore"):
            d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
        out[k] = np.where(np.isfinite(d), d, np.inf)
    return out


def worst_ratio(err, bnd):
    """max over the elements of error / bound per output (0 / 0 = 0) -> dict(p=, m=, v=)."""
    out = {}
    for k in ("p", "m", "v"):
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err[k] == 0, 0.0, err[k] / bnd[k])
        out[k] = float(np.max(r))
    return out


# ---- judging an engine's step ----------------------------------------------------------------------------------------------------
def snapshot(eng):
    """Host copies of an engine's flat parameter / moment buffers, its step counter and learning rate (synchronising)."""
    return dict(p=eng.flat_p.detach().cpu().numpy().copy(), m=eng.exp_avg.cpu().numpy().copy(),
                v=eng.exp_avg_sq.cpu().numpy().copy(), t=float(eng.step_count.item()), lr=float(eng.lr.item()))


def check_step(eng, before, t, b1, b2, eps, wd, gscale, label="", extra=None):
    """The contract of one applied update: from ``before`` (``snapshot``) and the gradient the engine holds now, EVERY element of
    the new flat buffers lies within ``bound`` (plus ``extra``, a dict like ``bound``'s, e.g. ``gap_bound``) of ``adam_ref`` at
    exactly this ``t`` with the learning rate ``before`` held, and the counter is exactly ``t``.  The hyper-parameters are given
    as the caller passed them to the engine (doubles); they are judged as the fp32 values it holds.  Returns the per-element
    error / bound (largest of the three outputs) for per-site figures."""
    after = snapshot(eng)
    g = eng.flat_g.detach().cpu().numpy()
    args = (before["p"], g, before["m"], before["v"], t, before["lr"], f32(b1), f32(b2), f32(eps), f32(wd), f32(gscale))
    ref = adam_ref(*args)
    bnd = bound(*args)
    if extra is not None:
        bnd = {k: bnd[k] + extra[k] for k in bnd}
    err = errors((after["p"], after["m"], after["v"]), ref)
    assert after["t"] == float(t), (label, "step counter", after["t"], t)
    ratio = np.zeros(g.shape[0])
    for k in ("p", "m", "v"):
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err[k] == 0, 0.0, err[k] / bnd[k])
        i = int(np.argmax(r))
        assert r[i] <= 1.0, (label, k, "element", i, "error", float(err[k][i]), "bound", float(bnd[k][i]), "p0 g m0 v0",
                             [float(a[i]) for a in args[:4]], "t", t, "outside", int((r > 1).sum()))
        ratio = np.maximum(ratio, r)
    return ratio

"""The whole operand and epilogue contract of engine.hpp (GemmArgs / GemmProb / Xform / BNRef) on every kernel of gemm.hip,
gemm_big.hip, gemm_ks.hip and gemm_wres.hip, through the test hook cal_gemm_probe (csrc/gemm_probe.hip), against the float64
restatement in tests/gemm_contract_ref.py (itself tied to torch by tests/test_gemm_contract_ref.py).

Every case: outputs NaN-filled before the launch, a canary block behind EVERY buffer, operands from a seeded generator, the
BatchNorm arena sums taken from the real operand (column means within two standard deviations of zero), row scales in
(0.05, 1) read with stride 2 (the slots between them hold NaN, so a stride of 1 poisons C), non-trivial gamma / beta.

Bounds (none of them fitted to a kernel's output):

  C         max |C - ref| / max |ref| < 2e-5, the suite's GEMM bound (tests/test_gpu_gemm.py).  Split-K slabs are summed here
            in float64.
  st        the sums are compared with float64 sums over the kernel's OWN stored C, so the product's rounding does not
            enter.  v and v * v are exact in fp64 (24-bit significands), so the only error is the order of n fp64 additions:
            each of the n - 1 additions rounds by at most 2^-53 of a partial sum that is at most S = sum |v|, hence
            |got - sum| <= (n - 1) 2^-53 S < n 2^-52 S (n rows; v^2 and S = sum v^2 for st_sq).  In atomic and striped mode the
            kernel adds onto a non-zero starting value s0, one more term: n + 1 and S + |s0| there.  dot_sum is the same sum.
  dot_prod  the kernel forms aux_n = (aux_rs * aux - mean) * rstd in fp32 from a float mean and rstd: 8 fp32 roundings --
            aux_rs * aux, the mean cast to float, the subtraction, the variance cast to float, var + eps, sqrtf, the
            reciprocal, and the final product.  With |aux_rs aux| rstd <= |aux_n| + |mean| rstd each of them moves aux_n by
            at most 2^-24 (|aux_n| + |mean| rstd), so |got - sum v aux_n| <= 8 * 2^-24 * sum |v| (|aux_n| + |mean| rstd), plus
            the fp64 order term above.  The product v * aux_n itself is formed in fp64.
  C null    the sums against the reference sums, under the C bound times the row count: 2e-5 * max |ref| * n.
  running   run_mean / run_var against one reference update to 1e-6 (max-norm relative); num_batches_tracked + 1 exactly;
            with update = 0 all three bit-identical.

k_wres used to add each lane's 16 values of a row block in fp32 before they entered the fp64 sums; its st_sum / st_sq /
dot_sum then missed the st bound 1.1e3 to 1.5e3 times (4e-9 of sum |v|).  It now adds every value in fp64 like the tile
kernels; test_wres_plain_column_sums_within_fp64_order is the regression case.

Worst printed ratios on MI355X (this commit) are recorded per test in the docstrings below.
"""
import ctypes

import pytest
import torch

from tests import gemm_contract_ref as ref
from tests.helpers import Buf, pool_intact as _pool_intact

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUND = 2e-5
U24, U52 = 2.0 ** -24, 2.0 ** -52
SEL_GEMM, SEL_KS, SEL_BIG, SEL_WRES, SEL_DUAL = range(5)
IV_PROB, PV_PROB = 24, 40            # per-problem strides of the description (csrc/gemm_probe.hip)
NAN = float("nan")


def _plan(M, N, K, nbatch=1, hasC=True):
    from cal_amd import _lib
    out = (ctypes.c_int64 * 6)()
    _lib.call("cal_gemm_probe_plan", M, N, K, nbatch, int(hasC), out)
    return {"S": out[0], "nsplit": out[1], "kchunk": out[2], "rt": out[3], "rt_ks": out[4], "nstripe": out[5]}


def _colmatrix(g, rows, cols):
    """random matrix whose columns have their own scale and a mean within two standard deviations of zero"""
    sig = 0.5 + torch.rand(cols, generator=g)
    mu = sig * (3.6 * torch.rand(cols, generator=g) - 1.8)
    return torch.randn(rows, cols, generator=g) * sig + mu


class RowScale:
    """values in (0.05, 1) at stride 2; NaN in the slots between"""

    def __init__(self, pool, g, rows):
        self.v = 0.05 + 0.95 * torch.rand(rows, generator=g)
        inter = torch.full((rows, 2), NAN)
        inter[:, 0] = self.v
        self.buf = Buf(pool, 2 * rows, data=inter)
        self.stride = 2


class BN:
    """one BatchNorm: arena sums of a real matrix (optionally spread over the NSTRIPE planes), parameters, running statistics"""

    def __init__(self, pool, g, x64, striped, nstripe):
        self.n, self.W = x64.shape
        self.s, self.q = x64.sum(0), (x64 * x64).sum(0)
        if striped:
            self.ss = (self.W + 3) // 4 * 4 + 4
            frac = torch.rand(nstripe, self.W, generator=g).double() + 0.1
            frac = frac / frac.sum(0, keepdim=True)
            planes = []
            for src in (self.s, self.q):
                p = torch.zeros(nstripe, self.ss, dtype=torch.float64)
                p[:, :self.W] = frac * src
                planes.append(p)
            self.s, self.q = planes[0][:, :self.W].sum(0), planes[1][:, :self.W].sum(0)     # what a striped reader adds up
            self.sum = Buf(pool, nstripe * self.ss, torch.float64, data=planes[0])
            self.sq = Buf(pool, nstripe * self.ss, torch.float64, data=planes[1])
        else:
            self.ss = 0
            self.sum = Buf(pool, self.W, torch.float64, data=self.s)
            self.sq = Buf(pool, self.W, torch.float64, data=self.q)
        self.gamma_h = 0.5 + torch.rand(self.W, generator=g)
        self.beta_h = 0.5 * torch.randn(self.W, generator=g)
        self.rm_h = 0.3 * torch.randn(self.W, generator=g)
        self.rv_h = 0.5 + torch.rand(self.W, generator=g)
        self.gamma, self.beta = Buf(pool, self.W, data=self.gamma_h), Buf(pool, self.W, data=self.beta_h)
        self.rm, self.rv = Buf(pool, self.W), Buf(pool, self.W)
        self.nbt = Buf(pool, 1, torch.int64)
        self.reset()

    def reset(self):
        self.rm.t.copy_(self.rm_h); self.rv.t.copy_(self.rv_h); self.nbt.t.fill_(3)

    def constants(self, use_running):
        return ref.bn_constants(self.s, self.q, self.n, self.gamma_h, self.beta_h, run_mean=self.rm_h, run_var=self.rv_h,
                                use_running=use_running)

    def ints(self, update, use_running):
        return [1, self.n, int(update), int(use_running), self.ss]

    def ptrs(self):
        return [b.ptr() for b in (self.sum, self.sq, self.gamma, self.beta, self.rm, self.rv, self.nbt)]

    def check_running(self, updated, fails, tag):
        rm, rv, nbt = self.rm.t.cpu(), self.rv.t.cpu(), int(self.nbt.t.item())
        if updated:
            wm, wv, wn = ref.running_update(self.rm_h, self.rv_h, 3, self.s, self.q, self.n)
            em = ((rm.double() - wm).abs().max() / wm.abs().max()).item()
            ev = ((rv.double() - wv).abs().max() / wv.abs().max()).item()
            if not (em < 1e-6 and ev < 1e-6 and nbt == wn):
                fails.append("%s: running statistics mean %.2e var %.2e nbt %d (want %d)" % (tag, em, ev, nbt, wn))
            return max(em, ev)
        if not (torch.equal(rm, self.rm_h) and torch.equal(rv, self.rv_h) and nbt == 3):
            fails.append("%s: running statistics changed without update (nbt %d)" % (tag, nbt))
        return 0.0


# ---- one problem of a launch -------------------------------------------------------------------------------------------
class Prob:
    """operands of one GemmProb, built once; configure() chooses what a launch uses of them and allocates its outputs"""

    def __init__(self, pool, g, ta, tb, M, N, K, striped_bn, nstripe, with_aux=True):
        self.pool, self.ta, self.tb, self.M, self.N, self.K, self.nstripe = pool, ta, tb, M, N, K, nstripe
        self.A = _colmatrix(g, *((K, M) if ta else (M, K)))             # as stored
        self.B = _colmatrix(g, *((N, K) if tb else (K, N)))
        self.dA, self.dB = Buf(pool, self.A.numel(), data=self.A), Buf(pool, self.B.numel(), data=self.B)
        self.rsA = RowScale(pool, g, self.A.shape[0])
        self.bnA = BN(pool, g, self.A.double(), striped_bn, nstripe)
        self.bnB = BN(pool, g, self.B.double(), striped_bn, nstripe)
        self.bias_h = torch.randn(N, generator=g)
        self.bias = Buf(pool, N, data=self.bias_h)
        if with_aux:
            self.aux_h = _colmatrix(g, M, N)
            self.aux = Buf(pool, M * N, data=self.aux_h)
            self.aux_rs = RowScale(pool, g, M)
            self.bn_aux = BN(pool, g, self.aux_h.double(), striped_bn, nstripe)
            self.bn_aux_rs = BN(pool, g, self.aux_rs.v.double()[:, None] * self.aux_h.double(), striped_bn, nstripe)
        self._ref = {}

    def reference(self, xa, xb, use_running, bias_relu):
        """float64 C of the configuration, on the device (computed on the CPU, once)"""
        key = (xa, xb, use_running, bias_relu)
        if key not in self._ref:
            a, b = self.A.double(), self.B.double()
            if xa:
                _, _, sc, sh = self.bnA.constants(use_running)
                a = ref.transform(a, self.rsA.v if xa == 2 else None, sc, sh)
            if xb:
                _, _, sc, sh = self.bnB.constants(use_running)
                b = ref.transform(b, None, sc, sh)
            c = ref.product(a.t() if self.ta else a, b.t() if self.tb else b, self.bias_h if bias_relu else None, bias_relu)
            self._ref[key] = c.to(DEV)
        return self._ref[key]

    def configure(self, xa=0, xb=0, epi="none", mode="atomic", use_running=False, update=True, bias_relu=False, hasC=True,
                  nsplit=1, parts_rows=0, rs_without_bn=False):
        M, N, pool = self.M, self.N, self.pool
        c = {"xa": xa, "xb": xb, "epi": epi, "mode": mode, "use_running": use_running, "update": update and not use_running,
             "bias_relu": bias_relu, "hasC": hasC, "nsplit": nsplit, "parts_rows": parts_rows}
        for bn in (self.bnA, self.bnB):
            bn.reset()
        c["C"] = Buf(pool, nsplit * M * N, fill=NAN)
        iv, pv = [0] * IV_PROB, [0] * PV_PROB
        pv[0], pv[1] = self.dA.ptr(), self.dB.ptr()
        pv[2] = c["C"].ptr() if hasC else 0
        pv[3] = self.bias.ptr() if bias_relu else 0
        if xa == 2 or rs_without_bn:
            pv[4], iv[0] = self.rsA.buf.ptr(), self.rsA.stride
        if xa:
            iv[5:10] = self.bnA.ints(c["update"], use_running); pv[13:20] = self.bnA.ptrs()
        if xb:
            iv[10:15] = self.bnB.ints(c["update"], use_running); pv[20:27] = self.bnB.ptrs()
        if epi != "none":
            ss = 0
            if mode == "striped":
                ss = (N + 3) // 4 * 4 + 4
                n_out = self.nstripe * ss
            else:
                n_out = N
            gen = torch.Generator().manual_seed(99)
            c["s0"] = [torch.randn(n_out, generator=gen).double() for _ in range(2)]
            c["out"] = [Buf(pool, n_out, torch.float64, data=s) for s in c["s0"]]
            c["ss"] = ss
            iv[4] = ss
            if mode == "parts":
                c["parts"] = Buf(pool, parts_rows * 2 * N, torch.float64, fill=NAN)
                pv[12] = c["parts"].ptr()
            if epi == "st":
                pv[6], pv[7] = c["out"][0].ptr(), c["out"][1].ptr()
            else:
                bn = self.bn_aux_rs if epi == "dotrs" else self.bn_aux
                bn.reset()
                c["aux_bn"] = bn
                pv[8] = self.aux.ptr()
                if epi == "dotrs":
                    pv[9], iv[2] = self.aux_rs.buf.ptr(), self.aux_rs.stride
                iv[3] = 1
                iv[15:20] = bn.ints(0, use_running); pv[27:34] = bn.ptrs()
                pv[10], pv[11] = c["out"][0].ptr(), c["out"][1].ptr()
        c["iv"], c["pv"] = iv, pv
        return c

    # -- checks; every violated bound goes to `fails`, every ratio to `rat`
    def check_untouched(self, c, fails, tag):
        if not bool(torch.isnan(c["C"].t).all().item()):
            fails.append(tag + ": C was written")
        if c["epi"] != "none":
            for o, s0 in zip(c["out"], c["s0"]):
                if not torch.equal(o.t.cpu(), s0):
                    fails.append(tag + ": sums were written")
            if c["mode"] == "parts" and not bool(torch.isnan(c["parts"].t).all().item()):
                fails.append(tag + ": partial rows were written")
        for bn in (self.bnA, self.bnB):
            bn.check_running(False, fails, tag)

    def check(self, c, fails, rat, tag):
        M, N = self.M, self.N
        want = self.reference(c["xa"], c["xb"], c["use_running"], c["bias_relu"])
        scale = want.abs().max().item()
        Cs = c["C"].t.view(c["nsplit"], M, N)
        if c["hasC"]:
            if not bool(torch.isfinite(Cs).all().item()):
                fails.append(tag + ": C holds entries the kernel never wrote")
            r = ((Cs.double().sum(0) - want).abs().max() / scale).item()
            rat["C"] = max(rat.get("C", 0.0), r)
            if not r < BOUND:
                fails.append("%s: C ratio %.3e" % (tag, r))
        elif not bool(torch.isnan(Cs).all().item()):
            fails.append(tag + ": the buffer of a null C was written")
        if c["epi"] != "none":
            self._check_sums(c, want, scale, fails, rat, tag)
        if c["xa"]:
            rat["run"] = max(rat.get("run", 0.0), self.bnA.check_running(c["update"], fails, tag + " xa.bn"))
        if c["xb"]:
            rat["run"] = max(rat.get("run", 0.0), self.bnB.check_running(c["update"], fails, tag + " xb.bn"))
        if "aux_bn" in c:
            c["aux_bn"].check_running(False, fails, tag + " aux_bn")

    def _check_sums(self, c, want, scale, fails, rat, tag):
        M, N, n = self.M, self.N, self.M
        out = [o.t.cpu() for o in c["out"]]
        s0 = c["s0"]
        if c["mode"] == "parts":
            P = c["parts_rows"]
            parts = c["parts"].t.view(P, 2, N).cpu()
            if not bool(torch.isfinite(parts).all().item()):
                fails.append("%s: %d values of the %d partial rows were never written" % (tag, int((~torch.isfinite(parts)).sum()), P))
            got = [parts[:, 0].sum(0), parts[:, 1].sum(0)]
            for o, s in zip(out, s0):
                if not torch.equal(o, s):
                    fails.append(tag + ": parts mode also added into the accumulators")
            start = [torch.zeros(N, dtype=torch.float64)] * 2
        elif c["mode"] == "striped":
            ss = c["ss"]
            got = [(o.view(-1, ss) - s.view(-1, ss))[:, :N].sum(0) for o, s in zip(out, s0)]
            pad = [(o.view(-1, ss) - s.view(-1, ss))[:, N:].abs().max().item() for o, s in zip(out, s0)]
            if max(pad) != 0.0:
                fails.append(tag + ": the padding between the planes was written")
            start = [s.view(-1, ss)[:, :N].abs().sum(0) for s in s0]
        else:
            got = [o - s for o, s in zip(out, s0)]
            start = [s.abs() for s in s0]
        terms = n + (0 if c["mode"] == "parts" else 1)
        v = (c["C"].t.view(M, N).double() if c["hasC"] else want)
        av = v.abs()
        if c["epi"] == "st":
            tot = [v.sum(0), (v * v).sum(0)]
            mag = [av.sum(0), (v * v).sum(0)]
            f32 = [0.0 * mag[0], 0.0 * mag[1]]                  # no fp32 arithmetic in these sums
            xn_max = 0.0
        else:
            bn = c["aux_bn"]
            mean, rstd, _, _ = bn.constants(c["use_running"])
            rs = self.aux_rs.v if c["epi"] == "dotrs" else None
            xn = ref.aux_normalised(self.aux_h, rs, mean, rstd).to(DEV)
            env = xn.abs() + (mean.abs() * rstd).to(DEV)[None, :]
            xn_max = xn.abs().max().item()
            tot = [v.sum(0), (v * xn).sum(0)]
            mag = [av.sum(0), (av * xn.abs()).sum(0)]
            f32 = [0.0 * mag[0], (av * env).sum(0) * 8 * U24]   # aux_n: 8 fp32 roundings (module docstring)
        e = BOUND * scale                           # what the C bound allows every entry of a C that is not stored
        null_bound = [n * e, n * (2.0 * scale * e + e * e) if c["epi"] == "st" else n * e * xn_max + f32[1].cpu()]
        for w, name in enumerate(("sum", "sq" if c["epi"] == "st" else "prod")):
            strict = terms * U52 * (mag[w].cpu() + start[w])
            if c["hasC"]:
                bound = strict + f32[w].cpu()
            else:
                bound = strict + null_bound[w]
            err = (got[w] - tot[w].cpu()).abs()
            bad = err > bound
            r = (err / bound.clamp_min(1e-300)).max().item() if bool((bound > 0).any()) else 0.0
            key = ("null_" if not c["hasC"] else "") + name
            rat[key] = max(rat.get(key, 0.0), r)
            if bool(bad.any().item()):
                fails.append("%s: %s err/bound %.3e (%d columns)" % (tag, name, r, int(bad.sum())))


# ---- launches ----------------------------------------------------------------------------------------------------------
def _describe(ta, tb, M, N, K, relu, cfgs, split):
    iv = [int(ta), int(tb), M, N, K, int(relu), len(cfgs), int(split)]
    pv = []
    for c in cfgs:
        iv += c["iv"]
        pv += c["pv"]
    return (ctypes.c_int64 * len(iv))(*iv), (ctypes.c_void_p * len(pv))(*pv)


def _launch(sel, ta, tb, M, N, K, relu, cfgs, split=False, second=None):
    """-> (return code, message)"""
    from cal_amd import _lib
    from cal_amd.plan import _stream
    iv, pv = _describe(ta, tb, M, N, K, relu, cfgs, split)
    iv2, pv2 = _describe(*second) if second else (None, None)
    dv = (ctypes.c_double * 1)(ref.EPS)
    h = _lib.lib()
    rc = h.cal_gemm_probe(sel, iv, pv, iv2, pv2, dv, _stream())
    torch.cuda.synchronize()
    return rc, (h.cal_last_error().decode() if rc else "")


COMBOS = [("none", "atomic")] + [(e, m) for e in ("st", "dot", "dotrs") for m in ("atomic", "striped", "parts")]
COMBOS_NOSTRIPE = [(e, m) for e, m in COMBOS if m != "striped"]


def _report(name, rat, fails):
    print("%s  %s" % (name, "  ".join("%s=%.3e" % kv for kv in sorted(rat.items()))))
    assert not fails, "\n".join(fails)


def _run_family(sel, ta, tb, M, N, K, nbatch, xas, xb, combos, striped_bn, seed, name, rt_key, null_c=True, bn_modes=(False, True)):
    """one set of operands; every (XA, BN mode, epilogue, sum mode) of the family through launcher `sel`"""
    pool, fails, rat = [], [], {}
    g = torch.Generator().manual_seed(seed)
    plan = _plan(M, N, K, nbatch)
    plan_null = _plan(M, N, K, nbatch, hasC=False)
    probs = [Prob(pool, g, ta, tb, M, N, K, striped_bn, plan["nstripe"]) for _ in range(nbatch)]
    for xa in xas:
        for use_running in (bn_modes if (xa or xb) else (False,)):
            runs = [(e, m, True) for e, m in combos]
            if null_c:
                runs += [("st", "atomic", False), ("dotrs", "parts", False)]
            for epi, mode, hasC in runs:
                if (xa or xb) and use_running and mode == "striped":
                    continue                                    # eval mode: one sum mode less, the prologue is what differs
                bias_relu = epi in ("none", "st")
                rows = (plan if hasC else plan_null)[rt_key]
                keep = len(pool)
                cfgs =[p.configure(xa, xb, epi, mode, use_running, True, bias_relu, hasC, 1, rows) for p in probs]
                tag = "%s xa=%d xb=%d run=%d %s/%s C=%d" % (name, xa, xb, use_running, epi, mode, hasC)
                rc, msg = _launch(sel, ta, tb, M, N, K, bias_relu, cfgs)
                if rc:
                    fails.append("%s: rc %d %s" % (tag, rc, msg))
                    continue
                for b, (p, c) in enumerate(zip(probs, cfgs)):
                    p.check(c, fails, rat, "%s p%d" % (tag, b))
                if not _pool_intact(pool):
                    fails.append(tag + ": a canary behind a buffer was overwritten")
                    _report(name, rat, fails)
                del pool[keep:]                                 # the outputs of this launch: checked, the allocator may reuse them
    _report(name, rat, fails)
    return rat


# ---- k_gemm_ks -----------------------------------------------------------------------------------------------------------
KS_CASES = [(32, 32, 128, 1), (33, 31, 10, 1), (70, 40, 200, 1), (130, 128, 128, 3)]


@pytest.mark.parametrize("tb", [0, 1])
@pytest.mark.parametrize("case", KS_CASES, ids=lambda s: "x".join(map(str, s)))
def test_ks_transforms_epilogues_and_sum_modes(case, tb):
    """k_gemm_ks<B_KC, XA>: XA 0 / 1 / 2, every epilogue x sum mode, BN in training (update = 1) and eval mode, C null.
    Worst on MI355X (ratio C = err / max |ref|, bound 2e-5; the others = err / their bound, bound 1): C 3.4e-7, sum 0 (exact),
    sq 4.9e-2, prod 1.9e-1, run 7.2e-8 (bound 1e-6), C null: sum 3.2e-3, sq 1.4e-3, prod 6.4e-4."""
    M, N, K, nb = case
    _run_family(SEL_KS, 0, tb, M, N, K, nb, (0, 1, 2), 0, COMBOS, True, 100 + tb, "k_gemm_ks %dx%dx%d b%d tb=%d" % (M, N, K, nb, tb),
                "rt_ks")


# ---- k_gemm --------------------------------------------------------------------------------------------------------------
SHAPES = [(64, 64, 32), (128, 64, 160), (68, 72, 64), (67, 33, 10), (67, 33, 170)]
# (name, transA, transB, XA classes, XB): every combination launch_gemm instantiates
GEMM_LAYOUTS = [("NN", 0, 0, (0, 1, 2), 0), ("NT", 0, 1, (0, 1), 0), ("TN", 1, 0, (0, 1, 2), 0), ("TNxb", 1, 0, (0,), 1),
                ("TT", 1, 1, (0,), 0)]


@pytest.mark.parametrize("layout", GEMM_LAYOUTS, ids=lambda l: l[0])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gemm_transforms_epilogues_and_sum_modes(shape, layout):
    """k_gemm<A_KC, B_KC, XA, XB> at the three bounds modes and both K loops of the shapes.
    Worst on MI355X (ratio C = err / max |ref|, bound 2e-5; the others = err / their bound, bound 1): C 6.1e-7, sum 0 (exact),
    sq 2.9e-2, prod 1.6e-1, run 7.7e-8 (bound 1e-6), C null: sum 2.1e-3, sq 1.2e-3, prod 5.5e-4."""
    M, N, K = shape
    name, ta, tb, xas, xb = layout
    _run_family(SEL_GEMM, ta, tb, M, N, K, 1, xas, xb, COMBOS, True, 200 + ta * 2 + tb, "k_gemm %s %dx%dx%d" % (name, M, N, K), "rt")


def test_gemm_reads_unstriped_statistics_too():
    """ss = 0: a striped reader adds the same value NSTRIPE times and scales it back (engine.hpp).
    Worst on MI355X: C 2.8e-7, prod 1.2e-1 of its bound."""
    _run_family(SEL_GEMM, 0, 0, 68, 72, 64, 1, (2,), 0, [("dotrs", "atomic")], False, 250, "k_gemm NN ss=0", "rt", null_c=False)
    _run_family(SEL_KS, 0, 1, 33, 31, 10, 1, (2,), 0, [("dotrs", "atomic")], False, 251, "k_gemm_ks ss=0", "rt_ks", null_c=False)


def _split_case(sel, M, N, K, nbatch, xa, seed, name, striped_bn, ta=1, tb=0):
    pool, fails, rat = [], [], {}
    g = torch.Generator().manual_seed(seed)
    plan = _plan(M, N, K, nbatch)
    probs = [Prob(pool, g, ta, tb, M, N, K, striped_bn, plan["nstripe"], with_aux=False) for _ in range(nbatch)]
    cfgs = [p.configure(xa=xa, nsplit=plan["nsplit"]) for p in probs]
    rc, msg = _launch(sel, ta, tb, M, N, K, 0, cfgs, split=True)
    assert rc == 0, (name, rc, msg)
    for b, (p, c) in enumerate(zip(probs, cfgs)):
        p.check(c, fails, rat, "%s p%d" % (name, b))
    if not _pool_intact(pool):
        fails.append(name + ": a canary behind a buffer was overwritten (slabs past the workspace?)")
    rat["slabs"] = plan["nsplit"]
    _report(name, rat, fails)
    return plan


@pytest.mark.parametrize("xa", [1, 2])
@pytest.mark.parametrize("shape", [(64, 64, 4096), (64, 64, 800)], ids=lambda s: "x".join(map(str, s)))
def test_gemm_split_k_with_transformed_operand_three_problems(shape, xa):
    """32 slabs (K = 4096) and the re-cut 7 (K = 800) per problem, three problems, slabs summed here in float64; the running
    statistics are updated by the first slice alone.  Worst on MI355X: C 1.5e-7, run 7.5e-8."""
    plan = _split_case(SEL_GEMM, *shape, 3, xa, 300 + xa, "k_gemm TN split %dx%dx%d xa=%d" % (*shape, xa), True)
    assert plan["nsplit"] > 1


# ---- k_gemm_big ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [64, 132])
@pytest.mark.parametrize("K", [32, 96])
@pytest.mark.parametrize("M", [16384, 16391])
def test_big_rows(M, K, N):
    """k_gemm_big<true, B_KC, XA> through launch_gemm_big alone: a declined launch is return code 3 and fails the case.
    Worst on MI355X (ratio C = err / max |ref|, bound 2e-5; the others = err / their bound, bound 1): C 5.6e-7, sum 5.1e-5,
    sq 3.2e-4, prod 7.5e-2, run 6.6e-8 (bound 1e-6), C null: sum 1.6e-3, sq 3.6e-4, prod 8.9e-5."""
    for name, tb, xas in (("NN", 0, (0, 1, 2)), ("NT", 1, (0, 1))):
        _run_family(SEL_BIG, 0, tb, M, N, K, 1, xas, 0, COMBOS_NOSTRIPE, False, 400 + tb, "k_gemm_big %s %dx%dx%d" % (name, M, N, K),
                    "rt", bn_modes=(False,))


@pytest.mark.parametrize("K", [16384, 16421])
@pytest.mark.parametrize("mn", [(64, 68), (132, 64)], ids=lambda s: "x".join(map(str, s)))
def test_big_gradients_slabs_inside_the_workspace(mn, K):
    """k_gemm_big<false, false, XA>: 16 / 17 slabs of 1024 node rows, the last one ragged.  Worst on MI355X: C 2.9e-7, run 6.1e-8."""
    for xa in (0, 1, 2):
        plan = _split_case(SEL_BIG, mn[0], mn[1], K, 1, xa, 450 + xa, "k_gemm_big TN %dx%dx%d xa=%d" % (*mn, K, xa), False)
        assert plan["nsplit"] > 1


# ---- k_wres / k_tn -------------------------------------------------------------------------------------------------------
WRES_COMBOS = [("none", "atomic")] + [(e, m) for e in ("st", "dot", "dotrs") for m in ("atomic", "parts")]


@pytest.mark.parametrize("tb", [0, 1])
@pytest.mark.parametrize("N", [128, 256])
@pytest.mark.parametrize("K", [128, 256])
@pytest.mark.parametrize("M", [16384, 16415])
def test_wres_all_instantiations(M, K, N, tb):
    """XA 0 / 1 / 2 x EPI 0-3 of k_wres<B_KC, XA, KS, EPI> for one (B_KC, KS), launch_gemm_wres alone.
    Worst on MI355X (ratio C = err / max |ref|, bound 2e-5; the others = err / their bound, bound 1): C 8.0e-7, sum 5.4e-5,
    sq 3.7e-4, prod 7.4e-2, run 6.6e-8 (bound 1e-6)."""
    _run_family(SEL_WRES, 0, tb, M, N, K, 1, (0, 1, 2), 0, WRES_COMBOS, False, 500 + tb, "k_wres %dx%dx%d tb=%d" % (M, N, K, tb), "rt",
                null_c=False, bn_modes=(False,))


@pytest.mark.parametrize("N", [128, 256])
def test_wres_batch_of_two(N):
    """ncol = 2 and 4: both column halves of both problems; each problem's BatchNorm is updated exactly once.
    Worst on MI355X: C 5.8e-7, sum 4.2e-5, sq 2.7e-4, prod 6.2e-2 of their bounds."""
    _run_family(SEL_WRES, 0, 0, 16415, N, 128, 2, (2,), 0, [("st", "atomic"), ("dotrs", "parts")], False, 520, "k_wres batch2 N=%d" % N,
                "rt", null_c=False, bn_modes=(False,))


def test_wres_plain_column_sums_within_fp64_order():
    """Regression case: st_sum / st_sq / dot_sum of k_wres under the fp64-order bound n 2^-52 sum |v| that every kernel meets.
    With a per-lane fp32 pre-sum of the 16 values of a row block (gemm_wres.hip before this test existed) MI355X measured, at
    this shape, err / bound: st_sum 1.15e3, st_sq 1.55e3, dot_sum 8.1e2 -- 3e-9 to 6e-9 of sum |v|, against the 3.6e-12 =
    n 2^-52 of the bound.  With every value added in fp64: sum 0 (exact), sq 2.6e-4, prod 3.0e-2 of their bounds."""
    _run_family(SEL_WRES, 0, 0, 16415, 128, 128, 1, (1,), 0, [("st", "atomic"), ("dot", "parts")], False, 530, "k_wres strict sums", "rt",
                null_c=False, bn_modes=(False,))


@pytest.mark.parametrize("K", [16384, 16391])
def test_tn_direct_operand_gradient(K):
    """k_tn<XA> through launch_gemm_wres alone: 256 / 171 slabs, an odd node count.  Worst on MI355X: C 1.5e-7, run 6.3e-8."""
    for xa in (0, 1, 2):
        plan = _split_case(SEL_WRES, 256, 256, K, 1, xa, 550 + xa, "k_tn 256x256x%d xa=%d" % (K, xa), False)
        assert plan["nsplit"] > 1


# ---- dual launch ---------------------------------------------------------------------------------------------------------
def _dual_case(Mx, Nx, Kx, xa_w, striped_bn, seed, name):
    """ax = dX (NT, [Mx, Nx, Kx], plain) and aw = dW (TN, [Kx, Nx, Mx], XA on the node operand) in one call"""
    pool, fails, rat = [], [], {}
    g = torch.Generator().manual_seed(seed)
    Mw, Nw, Kw = Kx, Nx, Mx
    plan = _plan(Mw, Nw, Kw, 1)
    px = Prob(pool, g, 0, 1, Mx, Nx, Kx, striped_bn, plan["nstripe"], with_aux=False)
    pw = Prob(pool, g, 1, 0, Mw, Nw, Kw, striped_bn, plan["nstripe"], with_aux=False)
    cx, cw = px.configure(), pw.configure(xa=xa_w, nsplit=plan["nsplit"])
    rc, msg = _launch(SEL_DUAL, 0, 1, Mx, Nx, Kx, 0, [cx], second=(1, 0, Mw, Nw, Kw, 0, [cw], True))
    assert rc == 0, (name, rc, msg)
    px.check(cx, fails, rat, name + " dX")
    rx = dict(rat); rat.clear()
    pw.check(cw, fails, rat, name + " dW")
    if not _pool_intact(pool):
        fails.append(name + ": a canary behind a buffer was overwritten")
    _report(name, {"dX": rx["C"], "dW": rat["C"], "run": rat.get("run", 0.0), "slabs": plan["nsplit"]}, fails)


@pytest.mark.parametrize("xa", [1, 2])
def test_dual_64(xa):
    """Worst on MI355X: dX 2.0e-7, dW 1.2e-7, run 7.1e-8."""
    _dual_case(300, 64, 64, xa, True, 600 + xa, "k_gemm_dual xa=%d" % xa)


def test_dual_128():
    """Worst on MI355X: dX 5.0e-7, dW 2.3e-7."""
    _dual_case(16391, 64, 96, 2, False, 610, "k_gemm_big_dual")


def test_dual_weight_resident_pair():
    """launch_gemm_dual hands this pair to k_wres and k_tn, one launch each.  Worst on MI355X: dX 7.0e-7, dW 8.6e-8."""
    _dual_case(16415, 256, 256, 2, False, 620, "k_wres + k_tn pair")


# ---- rejections ----------------------------------------------------------------------------------------------------------
def _rejected(sel, ta, tb, M, N, K, make_cfgs, seed, name, expect_rc=2):
    pool, fails = [], []
    g = torch.Generator().manual_seed(seed)
    plan = _plan(M, N, K)
    probs, cfgs = make_cfgs(pool, g, plan)
    rc, msg = _launch(sel, ta, tb, M, N, K, 0, cfgs)
    print("%s  rc=%d %s" % (name, rc, msg))
    assert rc == expect_rc and msg, (name, rc, msg)
    for p, c in zip(probs, cfgs):
        p.check_untouched(c, fails, name)
    assert _pool_intact(pool)
    assert not fails, "\n".join(fails)


def _one(ta, tb, M, N, K, **kw):
    def make(pool, g, plan):
        p = Prob(pool, g, ta, tb, M, N, K, True, plan["nstripe"])
        return [p], [p.configure(epi="st", mode="parts", parts_rows=max(plan["rt"], plan["rt_ks"]), **kw)]
    return make


@pytest.mark.parametrize("sel", [SEL_GEMM, SEL_KS])
def test_rejects_row_scale_without_bn(sel):
    _rejected(sel, 0, 0, 68, 72, 64, _one(0, 0, 68, 72, 64, rs_without_bn=True), 700, "row scale without BN")


@pytest.mark.parametrize("sel", [SEL_GEMM, SEL_KS])
def test_rejects_mixed_transform_classes(sel):
    def make(pool, g, plan):
        ps = [Prob(pool, g, 0, 0, 68, 72, 64, True, plan["nstripe"]) for _ in range(2)]
        return ps, [ps[0].configure(xa=1), ps[1].configure(xa=2)]
    _rejected(sel, 0, 0, 68, 72, 64, make, 701, "mixed transform classes")


def test_rejects_nt_with_row_scale():
    _rejected(SEL_GEMM, 0, 1, 68, 72, 64, _one(0, 1, 68, 72, 64, xa=2), 702, "NT with XA = 2")


def test_rejects_tt_with_transform():
    _rejected(SEL_GEMM, 1, 1, 68, 72, 64, _one(1, 1, 68, 72, 64, xa=1), 703, "TT with a transform")


@pytest.mark.parametrize("sel", [SEL_GEMM, SEL_KS])
def test_rejects_bn_wider_than_the_table(sel):
    _rejected(sel, 0, 0, 40, 36, 520, _one(0, 0, 40, 36, 520, xa=1), 704, "KC operand with BN over K = 520 > 512")


def test_alone_selectors_report_a_declined_launch():
    """a shape neither special kernel takes: return code 3, nothing written -- never a silent run on the 64 x 64 kernel"""
    for sel in (SEL_BIG, SEL_WRES):
        _rejected(sel, 0, 0, 68, 72, 64, _one(0, 0, 68, 72, 64), 705, "alone selector %d at 68x72x64" % sel, expect_rc=3)


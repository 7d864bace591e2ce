"""The GATConv kernels of csrc/gat.hip path by path -- the wave family (K = 4, D = 64: k_gat_fwd_w, k_gat_bwd_dst_w,
k_gat_bwd_src_w in their DROP and non-DROP builds, k_gat_datt_part_w), k_gat_fwd_fused at every head width LH = 1..64 and group
width G = 8..64, the two-pass forward k_gat_scores + k_gat_fwd<VEC, G> for VEC = 4 and 1, the row backward k_gat_bwd_dst_c /
k_gat_bwd_src<VEC, G> with its read-back path beyond eight slots, k_gat_datt_part at 64..256 threads and k_gat_datt_finish --
through the public cal_gat_fwd / cal_gat_bwd / cal_gat_dropout_mask and, for what those pin to null (the device step counter
`ctr`, `part_out`), through the test hooks cal_gat_probe_* at the end of csrc/gat.hip, against the float64 restatement
tests/gat_contract_ref.py (tied to the oracle, to autograd and to the host library's mask by tests/test_gat_contract_ref.py,
which also shows that these inputs and bounds notice ten seeded defects).

Every case: outputs and the workspace NaN-filled before the launch, a canary block behind (and, for an operand that starts one
float past a 16 B boundary, in front of) EVERY buffer, the workspace exactly cal_gat_bwd_ws floats, operands from a seeded
generator (tests/gat_contract_cases.py), CSR arrays built with numpy.  The batch is the degree ladder of tests/ladder.py
(N = 301: 76 row blocks of the wave grids, 72 of them remapped by xcd_block; 10 blocks of 32 rows for the d att partials, the
last ragged); every case runs twice, on the batch whose by-destination view carries the ladder (forward, by-destination
backward) and on the one whose by-source view does (by-source backward), and every output is judged on both.

Which kernel family a shape reaches is asserted per case: the dispatch rule restated in tests/gat_contract_cases.py says what
it should be, the library's launch-site count and the name of its latest launch site say what it was.

Bounds: module docstring of tests/gat_contract_ref.py.  x, the relative error of the exponential, is measured here through
cal_gat_probe_exp2 against fp64 on 2^20 points of [-126, 0] (exp2f, the bare v_exp_f32) and of [-87, 0] (expf); the larger of
the three and one ulp (2 u = 1.19e-7) is used.  Ascending operand set: see tests/gat_contract_cases.operands; the wave forward's
bare v_exp_f32 flushes the terms below 2^-126 of the row maximum, which adds at most 2^-126 per term against a denominator >= 1.

Measured on MI355X: the x values and the worst ratio of every test are recorded in MEASURED at the end of this file.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import gat_contract_cases as C
from tests import gat_contract_ref as ref
from tests.helpers import Buf, pool_intact
from tests.ladder import N

pytestmark = pytest.mark.gpu
NAN = float("nan")
SEED = 0x5EED0000BEEF0001
OUTS = ("out", "adst", "asrc", "mx", "den", "dz", "datt", "ws")


def _lib():
    from cal_amd import _lib as L
    return L.lib()


def _stream():
    from cal_amd.plan import _stream as s
    return s()


@functools.lru_cache(maxsize=None)
def exp_errors():
    """largest relative errors of exp2f, the bare v_exp_f32 and expf on the device against fp64, 2^20 points each"""
    h, pool, res = _lib(), [], []
    for raw, lo in ((0, -126.0), (1, -126.0), (2, -87.0)):
        x = torch.linspace(lo, 0.0, 1 << 20, dtype=torch.float32)
        src, dst = Buf(pool, x.numel(), data=x), Buf(pool, x.numel(), fill=NAN)
        assert h.cal_gat_probe_exp2(src.ptr(), dst.ptr(), x.numel(), raw, _stream()) == 0
        torch.cuda.synchronize()
        want = torch.exp(x.double()) if raw == 2 else torch.exp2(x.double())
        res.append(float(((dst.t.cpu().double() - want).abs() / want).max()))
    assert pool_intact(pool)
    return tuple(res)


def x_exp():
    return max(max(exp_errors()), 2 * ref.U)


class Run:
    """the buffers of one case on one batch, and its launches"""

    def __init__(self, case, b, ops, seed=SEED, K=None, D=None):
        self.c, self.b, self.ops, self.seed = case, b, ops, seed
        K, D = self.K, self.D = case["K"] if K is None else K, case["D"] if D is None else D
        n, E = self.n, self.E = len(b["dst"][0]) - 1, b["E"]
        mis, pool = case["mis"], []
        self.pool = pool
        off = lambda name: 1 if name in mis else 0
        self.csr = [Buf(pool, len(a), torch.int32, data=torch.from_numpy(a)) for a in b["dst"] + b["src"]]
        self.z, self.att = Buf(pool, ops["z"].numel(), data=ops["z"], off=off("z")), Buf(pool, ops["att"].numel(), data=ops["att"], off=off("att"))
        self.bias = Buf(pool, ops["bias"].numel(), data=ops["bias"], off=off("bias")) if ops["bias"] is not None else None
        self.gout = Buf(pool, ops["gout"].numel(), data=ops["gout"], off=off("gout"))
        H = case["K"] * case["D"]
        self.out, self.dz = Buf(pool, n * H, fill=NAN, off=off("out")), Buf(pool, n * H, fill=NAN, off=off("dz"))
        for name in ("adst", "asrc", "mx", "den"):
            setattr(self, name, Buf(pool, n * case["K"], fill=NAN, off=off(name)))
        self.datt = Buf(pool, 2 * H, fill=NAN)
        h = _lib()
        self.nws = int(h.cal_gat_bwd_ws(n, E, case["K"], case["D"]))
        self.ws = Buf(pool, self.nws, fill=NAN, off=off("ws"))
        self.lay = (ctypes.c_int64 * 4)()
        assert h.cal_gat_probe_ws_layout(n, E, case["K"], case["D"], self.lay) == 0

    def _around(self, fn):
        h = _lib()
        before = h.cal_launch_count()
        rc = fn(h)
        torch.cuda.synchronize()
        self.launches, self.last = h.cal_launch_count() - before, h.cal_gat_probe_last_launch().decode()
        self.msg = h.cal_last_error().decode() if rc else ""
        return rc

    def fwd(self, ctr=None, p=None):
        c, p = self.c, self.c["p"] if p is None else p
        head = [x.ptr() for x in self.csr[:3]] + [self.z.ptr(), self.att.ptr(), self.bias.ptr() if self.bias else None, c["relu"],
                                                 c["slope"], p, self.seed]
        tail = [x.ptr() for x in (self.out, self.adst, self.asrc, self.mx, self.den)] + [self.n, self.E, self.K, self.D, _stream()]
        if ctr is None:
            return self._around(lambda h: h.cal_gat_fwd(*(head + tail)))
        return self._around(lambda h: h.cal_gat_probe_fwd(*(head + [ctr.ptr()] + tail)))

    def bwd(self, ctr=None, part_out=None, p=None, hook=False):
        c, p = self.c, self.c["p"] if p is None else p
        head = [x.ptr() for x in self.csr] + [x.ptr() for x in (self.z, self.att, self.adst, self.asrc, self.mx, self.den, self.gout)] + \
            [c["slope"], p, self.seed]
        mid = [self.dz.ptr(), self.datt.ptr(), self.ws.ptr(), self.n, self.E, self.K, self.D]
        if ctr is None and part_out is None and not hook:
            return self._around(lambda h: h.cal_gat_bwd(*(head + mid + [_stream()])))
        self.nparts = ctypes.c_int(-1)
        return self._around(lambda h: h.cal_gat_probe_bwd(*(head + [ctr.ptr() if ctr else None] + mid +
                                                          [part_out.ptr() if part_out else None, ctypes.byref(self.nparts), _stream()])))

    def bits(self):
        return {k: getattr(self, k).t.view(torch.int32).cpu() for k in OUTS}

    def untouched(self, names=OUTS):
        return all(bool(torch.isnan(getattr(self, k).t).all()) for k in names)

    def piece(self, k, count):
        o = int(self.lay[k])
        return self.ws.t[o:o + count].cpu()

    def judge(self, fails, rat, tag, backward=True, seed=None):
        c, b, o = self.c, self.b, self.ops
        K, D, E, n = c["K"], c["D"], self.E, self.n
        keep = ref.keep_mask(self.seed if seed is None else seed, E, n, K, c["p"])
        J = ref.Judge(*b["dst"], o["z"], o["att"], o["bias"], c["relu"], c["slope"], c["p"], keep, K, D, E, x_exp())
        st = tuple(getattr(self, k).t.cpu() for k in ("adst", "asrc", "mx", "den"))
        res = dict(J.state(*st))
        res.update(J.out(self.out.t.cpu()))
        if backward:
            draw = self.piece(0, (E + n) * K).view(E + n, K)
            if not bool(torch.isnan(draw[:E][torch.from_numpy(~b["slotted"])]).all()):
                fails.append(tag + ": draw of an edge without a slot was written")
            g, _ = J.grads(st, o["gout"], draw, self.piece(1, n * K), self.piece(2, n * K), self.dz.t.cpu(), self.datt.t.cpu())
            res.update(g)
        ref.worst(res, rat, fails, tag)
        if not pool_intact(self.pool):
            fails.append(tag + ": a canary next to a buffer was overwritten")
        return J


FWD_SITE = {"wave": (1, "k_gat_fwd_w"), "fused": (1, "k_gat_fwd_fused"), "twopass4": (2, "k_gat_fwd"), "twopass1": (2, "k_gat_fwd")}
BWD_SITES = {"wave": 3, "rows4": 4, "rows1": 4}


def _report(name, rat, fails):
    print("%s  %s" % (name, "  ".join("%s=%.3e" % kv for kv in sorted(rat.items()))))
    assert not fails, "\n".join(fails)


def _expect_refusal(r, fails, tag, names=("dz", "datt", "ws"), word=None):
    if not (r.rc == 2 and r.msg and r.launches == 0):
        fails.append("%s: expected a refusal before any launch, got rc %d '%s' after %d launches" % (tag, r.rc, r.msg, r.launches))
    if word and word not in r.msg:
        fails.append("%s: the message '%s' does not name '%s'" % (tag, r.msg, word))
    if not r.untouched(names):
        fails.append(tag + ": a refused call wrote an output")
    if not pool_intact(r.pool):
        fails.append(tag + ": a canary next to a buffer was overwritten")


def _run_case(c, fails, rat, wide=False):
    for key in (1, 0):
        b, ops = C.batch_of(c, key), C.operands(c, key)
        tag = "%s key=%d" % (c["name"], key)
        r = Run(c, b, ops)
        rc = r.fwd()
        if rc:
            fails.append("%s: forward rc %d %s" % (tag, rc, r.msg))
            continue
        if (r.launches, r.last) != FWD_SITE[c["fwd"]]:
            fails.append("%s: the forward was meant for %s, the library passed %d launch sites, the last %s" % (tag, c["fwd"], r.launches, r.last))
        fam, _, _, _ = C.bwd_path(c["K"], c["D"], c["mis"])
        if not r.untouched(("dz", "datt", "ws")):
            fails.append(tag + ": the forward wrote a backward buffer")
        r.rc = r.bwd()
        if wide and r.rc == 0:
            print(tag + ": the backward ran")
            fam = "ran"
        if fam == "refuse":
            fr = {}
            r.judge(fails, fr, tag, backward=False)
            rat.update({k: max(rat.get(k, 0.0), v) for k, v in fr.items()})
            _expect_refusal(r, fails, tag, word="64" if wide else None)
            continue
        if r.rc:
            fails.append("%s: backward rc %d %s" % (tag, r.rc, r.msg))
            continue
        if not wide and r.launches != BWD_SITES[c["bwd"]]:
            fails.append("%s: the backward was meant for %s, the library passed %d launch sites" % (tag, c["bwd"], r.launches))
        fr = {}
        J = r.judge(fails, fr, tag)
        rat.update({k: max(rat.get(k, 0.0), v) for k, v in fr.items()})
        if c["asc"] and not float((J.f.le - J.f.mx[J.ri]).min()) < -126 * np.log(2.0):
            fails.append(tag + ": the ascending set does not reach the flush range")


@pytest.mark.parametrize("name", [c["name"] for c in C.CASES])
def test_gat_path(name):
    """forward and backward of one case of the table on both ladder batches: state, out, draw, dadst, dasrc, dz, datt.
    Worst err / bound on MI355X per family: MEASURED at the end of this file."""
    c = C.case_by_name(name)
    fails, rat = [], {}
    _run_case(c, fails, rat)
    _report("gat %s fwd=%s bwd=%s x=%.3e" % (name, c["fwd"], c["bwd"], x_exp()), rat, fails)


@pytest.mark.parametrize("name", [c["name"] for c in C.WIDE])
def test_head_wider_than_a_lane_group(name):
    """D / VEC > 64: the forward runs on the scalar-scores path and is held to its bounds; the backward reduces a head's dot over
    the D / VEC lanes of ONE group of at most 64, so it must either be within its bounds or refuse before any launch with a
    message that names the limit.  MEASURED (end of this file) has the figures of both."""
    c = C.case_by_name(name)
    fails, rat = [], {}
    _run_case(c, fails, rat, wide=True)
    _report("gat wide %s" % name, rat, fails)


def test_exponential_error_is_measured():
    e = exp_errors()
    print("relative error of exp2f %.4e, bare v_exp_f32 %.4e, expf %.4e (one ulp = %.4e); x = %.4e" % (e + (2 * ref.U, x_exp())))
    assert all(0 < v < 1e-5 for v in e)


# ---- exact checks ----------------------------------------------------------------------------------------------------------
def test_device_mask_is_keep_mask_bit_for_bit():
    h = _lib()
    used = sorted({(c["K"], c["p"]) for c in C.CASES + C.WIDE})
    assert any(p == 0 for _, p in used) and any(p > 0 for _, p in used)
    E = C.views(1)["E"]
    for K, p in used:
        for seed in (SEED, ref.step_seed(SEED, (1 << 40) + 5), 77):
            pool = []
            m = Buf(pool, (E + N) * K, fill=NAN)
            assert h.cal_gat_dropout_mask(seed, E, N, K, p, m.ptr(), _stream()) == 0
            torch.cuda.synchronize()
            assert np.array_equal(m.t.cpu().numpy().reshape(E + N, K), ref.keep_mask(seed, E, N, K, p)), (K, p, seed)
            assert pool_intact(pool)


def _full_run(c, b, ops, seed, ctr=None, hook=False):
    r = Run(c, b, ops, seed=seed)
    assert r.fwd(ctr=ctr) == 0, r.msg
    assert r.bwd(ctr=ctr, hook=hook) == 0, r.msg
    assert pool_intact(r.pool)
    return r.bits()


@pytest.mark.parametrize("name", ["fused-4x8", "wave-1", "vec1-7x1"])
def test_step_counter_is_the_seed_offset_and_runs_repeat(name):
    """a hook call with the device counter at c gives, in every output and the whole workspace, the bits of the public call with
    seed + c * 0x9E3779B97F4A7C15 mod 2^64; the same call twice gives the same bits (no atomics); another seed gives other bits"""
    c = C.case_by_name(name)
    assert c["p"] > 0
    b, ops = C.batch_of(c, 1), C.operands(c, 1)
    cnt = (1 << 40) + 5
    pool = []
    ctr = Buf(pool, 1, torch.int64, data=torch.tensor([cnt]))
    eff = ref.step_seed(SEED, cnt)
    assert eff >> 32 != SEED >> 32
    via_ctr = _full_run(c, b, ops, SEED, ctr=ctr)
    direct, again, other = _full_run(c, b, ops, eff), _full_run(c, b, ops, eff), _full_run(c, b, ops, SEED)
    null_ctr = _full_run(c, b, ops, SEED, hook=True)
    for k in OUTS:
        assert torch.equal(via_ctr[k], direct[k]), k
        assert torch.equal(direct[k], again[k]), k
        assert torch.equal(null_ctr[k], other[k]), k
    assert not torch.equal(other["out"], direct["out"]) and not torch.equal(other["dz"], direct["dz"])
    assert pool_intact(pool) and int(ctr.t.item()) == cnt
    # and the bits are the right ones: the run is judged with the mask of the effective seed
    r = Run(c, b, ops, seed=SEED)
    assert r.fwd(ctr=ctr) == 0 and r.bwd(ctr=ctr) == 0
    fails, rat = [], {}
    r.judge(fails, rat, name, seed=eff)
    _report("gat ctr %s" % name, rat, fails)


@pytest.mark.parametrize("name", ["fused-1x4", "wave-0", "vec1-4x1", "twopass-4x12"])
def test_without_dropout_the_seed_does_not_matter(name):
    c = C.case_by_name(name)
    assert c["p"] == 0
    b, ops = C.batch_of(c, 1), C.operands(c, 1)
    runs = []
    for seed in (SEED, 12345):
        r = Run(c, b, ops, seed=seed)
        assert r.fwd() == 0
        if c["bwd"] != "refuse":
            assert r.bwd() == 0
        runs.append(r.bits())
    for k in OUTS:
        assert torch.equal(runs[0][k], runs[1][k]), k


@pytest.mark.parametrize("name", ["fused-1x4", "fused-6x16", "wave-0", "vec1-4x1", "twopass-4x12", "mis-io-4x64"])
def test_batch_without_edges(name):
    """p = 0, no edge: out == z + bias exactly (1 / (1 + 1e-16) is 1 in fp32), den == 1, mx the loop logit -- exactly where the
    kernel stores the logit itself (two-pass forward), within 3 u |mx| where it stores the logit scaled by log2(e) and back
    (fused and wave forward: two multiplications by rounded constants)"""
    c = dict(C.case_by_name(name), p=0.0, relu=0, bias=1)
    n = 7
    z = C.operands(c, 1)["z"][:n].contiguous()
    g = torch.Generator().manual_seed(5)
    ops = {"z": z, "att": C.operands(c, 1)["att"], "bias": torch.randn(c["K"] * c["D"], generator=g), "gout": torch.randn(n, c["K"] * c["D"], generator=g)}
    empty = (np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))
    b = {"dst": empty, "src": empty, "E": 0, "slotted": np.zeros(0, bool)}
    r = Run(c, b, ops)
    assert r.fwd() == 0, r.msg
    out = r.out.t.cpu().view(n, -1)
    assert torch.equal(out, z + ops["bias"])
    assert bool((r.den.t == 1).all())
    adst, asrc, mx = (getattr(r, k).t.cpu() for k in ("adst", "asrc", "mx"))
    raw = adst + asrc
    l = torch.where(raw > 0, raw, torch.tensor(c["slope"], dtype=torch.float32) * raw)
    if c["fwd"].startswith("twopass"):
        assert torch.equal(mx, l)
    else:
        print("%s: %d of %d stored maxima differ from the loop logit" % (name, int((mx != l).sum()), mx.numel()))
        assert bool(((mx.double() - l.double()).abs() <= 3 * ref.U * l.double().abs()).all())
    fails, rat = [], {}
    r.judge(fails, rat, name, backward=False)
    _report("gat edge-free %s" % name, rat, fails)


def test_no_nodes_writes_nothing():
    c = C.case_by_name("fused-4x8")
    b, ops = C.batch_of(c, 1), C.operands(c, 1)
    r = Run(c, b, ops)
    r.n = 0
    assert r.fwd() == 0 and r.launches == 0
    assert r.untouched() and pool_intact(r.pool)


# ---- part_out --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,off", [("wave-1", 0), ("wave-1", 1), ("fused-3x8", 0), ("vec1-40x2", 0)])
def test_partial_rows_handed_to_the_caller(name, off):
    """part_out: the fp64 sum of the nparts rows is d att within the d att bound (against fp64 from the run's own dadst / dasrc), as
    is the public call's datt; datt and the workspace's own partial rows stay untouched; nparts is cal_gat_datt_parts(N).
    off = 1: part_out one float past a 16 B boundary (K = 4, D = 64 then takes the generic partial kernel)."""
    c = C.case_by_name(name)
    b, ops = C.batch_of(c, 0), C.operands(c, 0)
    h = _lib()
    K, D = c["K"], c["D"]
    nparts = int(h.cal_gat_datt_parts(N))
    assert nparts == 10 and h.cal_gat_datt_parts(0) == 0 and h.cal_gat_datt_parts(512 * 32 + 1) == 497
    pub = Run(c, b, ops)
    assert pub.fwd() == 0 and pub.bwd() == 0
    r = Run(c, b, ops)
    part = Buf(r.pool, nparts * 2 * K * D, fill=NAN, off=off)
    assert r.fwd() == 0 and r.bwd(part_out=part) == 0, r.msg
    assert r.nparts.value == nparts and r.launches == BWD_SITES[c["bwd"]] - 1
    assert r.untouched(("datt",)) and bool(torch.isnan(r.ws.t[int(r.lay[3]):]).all()) and pool_intact(r.pool)
    for k in ("dz",):
        assert torch.equal(r.bits()[k], pub.bits()[k])
    got = part.t.cpu().double().view(nparts, K, 2 * D).sum(0)
    want, bound = ref.datt_bound(ops["z"], r.piece(1, N * K), r.piece(2, N * K), N, K, D)
    fails, rat = [], {}
    ref.worst({"parts": ((got - want).abs(), bound), "datt": ((pub.datt.t.cpu().double().view(K, 2 * D) - want).abs(), bound)}, rat, fails, name)
    _report("gat part_out %s off=%d" % (name, off), rat, fails)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals():
    """a non-zero code, a message, every output still NaN, canaries intact, no launch site passed"""
    c = C.case_by_name("fused-4x8")
    b, ops = C.batch_of(c, 1), C.operands(c, 1)
    fails = []
    for what, kw, p in (("K = 0", {"K": 0}, None), ("D = 0", {"D": 0}, None), ("p = 1", {}, 1.0), ("p < 0", {}, -0.25)):
        r = Run(c, b, ops, **kw)
        r.rc = r.fwd(p=p)
        _expect_refusal(r, fails, "forward " + what, names=OUTS)
        r = Run(c, b, ops, **kw)
        r.rc = r.bwd(p=p)
        _expect_refusal(r, fails, "backward " + what, names=OUTS)
    for D in (12, 3, 5):
        cc = dict(c, D=D)
        r = Run(cc, b, C.operands(cc, 1))
        r.rc = r.bwd()
        _expect_refusal(r, fails, "backward D = %d" % D, names=OUTS)
    assert not fails, "\n".join(fails)


MEASURED = """MI355X, this commit; worst err / bound (a bound is 1) over both ladder batches.

x: exp2f 8.30e-8, the bare v_exp_f32 8.30e-8, expf 8.11e-8 -- all three under the one-ulp floor, so x = 2 u = 1.19e-7.

test_gat_path, per family (random operand sets | ascending sets):
  wave family        adst 1.7e-2  asrc 1.8e-2  mx 2.0e-2  den 1.6e-2  out 8.8e-3  draw 4.2e-2  dadst 2.3e-2  dasrc 1.4e-2  dz 0.34  datt 4.2e-3
                     | asrc 6.7e-2  mx 7.7e-2  den 4.0e-2  out 2.7e-2  draw 0.97  dadst 0.22  dasrc 0.59  dz 0.43  datt 1.4e-2
                     (draw 0.97: the backward's bare v_exp_f32 returns 0 for an alpha below 2^-126 -- the underflow term of the bound,
                     nearly in full; without that term the ascending set would not pass, with it the flush is all it allows)
  fused + rows<4>    adst 0.42  asrc 0.43 (D = 4)  mx 0.22  den 7.6e-2  out 4.5e-2  draw 0.27  dadst 0.18  dasrc 0.13  dz 0.41  datt 9.1e-3
                     | mx 0.13  den 4.0e-2  out 4.9e-2  draw 0.44  dadst 0.34  dasrc 0.34  dz 0.38  datt 1.2e-2
  two-pass VEC = 4   adst 0.20  asrc 0.18  mx 9.1e-2  den 4.1e-2  out 2.4e-2 (forward only: the backward refuses)
  VEC = 1 by shape   adst 0.61  asrc 0.60  mx 0.23  den 0.11  out 9.6e-2  draw 0.33  dadst 0.25  dasrc 0.24  dz 0.31  datt 6.4e-3
                     | draw 0.49  dadst 0.42  dasrc 0.38  dz 0.40  datt 8.3e-3
  by alignment       adst 0.14  asrc 0.11  mx 7.4e-2  den 2.7e-2  out 1.4e-2  draw 0.10  dadst 5.3e-2  dasrc 5.0e-2  dz 0.36  datt 3.6e-3
  wave declined      adst 1.6e-2  asrc 1.6e-2  mx 1.6e-2  den 8.8e-3  out 6.6e-3  draw 3.8e-2  dadst 1.1e-2  dasrc 1.8e-2  dz 0.35  datt 5.3e-3
test_step_counter_is_the_seed_offset_and_runs_repeat: bit equality; judged with the effective seed: draw 0.39, dz 0.23, out 9.6e-2.
test_batch_without_edges: out == z + bias and den == 1 exactly on every path; mx is the loop logit exactly on the two-pass path,
  one ulp off in 5 of 42 (fused 6 x 16) and 2 of 28 (wave) stored values: (l * log2 e) * (1 / log2 e) is not l in fp32.
test_partial_rows_handed_to_the_caller: parts 4.5e-3, datt 5.1e-3.
test_head_wider_than_a_lane_group: the forward is within its bounds (out 3.7e-3, den 1.2e-3, mx 9.7e-3).  The backward as it was
  before gat_backward refused these shapes, run once: draw 5.2e3 (1 x 512), 3.9e4 (1 x 128, z misaligned), 2.6e4 (1 x 256, z
  misaligned) times its bound, dadst / dasrc 1.8e3 .. 2.3e4 -- silently wrong gradients; dz and datt, judged against the kernel's own
  dadst / dasrc, stayed inside theirs.  Now: refused before any launch, the message names the limit."""

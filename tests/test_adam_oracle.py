"""The Adam contract's oracle judged on the CPU alone (tests/adam_oracle.py): the fp64 reference equals torch.optim.Adam, the
fp32 restatement lies inside the derived bound on every case, the fp32-held hyper-parameters stay within the derived
representation gap of the double ones, and every seeded defect leaves the bound on exactly the cases it has to -- the condition
under which tests/test_gpu_adam_contract.py means something.  Run with -s for the tables."""
import numpy as np
import pytest
import torch

from tests import adam_oracle as AO

N = 3000          # elements per state draw (not a multiple of 256, like a model's flat buffer)


@pytest.mark.parametrize("wd", [0.0, 1e-3])
def test_adam_ref_equals_torch_adam_in_fp64(wd):
    """Three consecutive steps from zero moments with double hyper-parameters: parameters and both moments to 1e-14 relative."""
    rng = np.random.default_rng(5)
    p0 = 0.1 * rng.standard_normal(N)
    grads = [rng.standard_normal(N) * 10.0 ** rng.uniform(-6, 0, N) for _ in range(3)]
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([tp], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    p, m, v = p0.copy(), np.zeros(N), np.zeros(N)
    for t, g in enumerate(grads, 1):
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        m_in, p_in = m, p
        p, m, v = AO.adam_ref(p, g, m, v, t, lr, b1, b2, eps, wd, 1.0)
        st = opt.state[tp]
        assert float(st["step"]) == t
        # (g and wd * p may cancel in gi, and torch adds them with an fma: the update carries that condition number)
        D, cond = np.abs(p - p_in), (np.abs(g) + wd * np.abs(p_in)) / np.abs(g + wd * p_in)
        assert np.all(np.abs(tp.detach().numpy() - p) <= 1e-14 * (np.abs(p) + D * cond))
        assert np.all(np.abs(st["exp_avg"].numpy() - m) <= 1e-14 * (np.abs(m_in) + np.abs(g) + wd * np.abs(p)))
        # (relative to the terms, not to their sum: g and wd * p may cancel in gi, and torch adds them in another order)
        assert np.all(np.abs(st["exp_avg_sq"].numpy() - v) <= 1e-14 * (v + (1 - b2) * (np.abs(g) + wd * np.abs(p)) ** 2))


def test_cases_cover_what_the_issue_lists():
    assert len(AO.CASES) == 3 * 2 * 2 * 3 * 6
    c = AO.CASES[0]
    p, g, m, v = AO.draw_state(c, N)
    assert all(a.dtype == np.float32 and a.shape == (N,) for a in (p, g, m, v))
    assert np.abs(g[4:]).min() >= 0.9e-9 and np.abs(g).max() <= 10.0 and (g > 0).any() and (g < 0).any()
    assert (v >= 0).all() and (v == 0).sum() > N // 8 and (m > 0).any() and (m < 0).any()
    gi = g.astype(np.float64) * c["gscale"] + c["wd"] * p.astype(np.float64)
    m1 = c["b1"] * m.astype(np.float64) + (1 - c["b1"]) * gi
    cancel = np.abs(m1) <= 2.0 ** -22 * np.abs((1 - c["b1"]) * gi)
    assert (cancel & (g != 0)).sum() > N // 8            # the two terms of m1 cancel to rounding on a third of the elements
    assert float(AO.hp(c)[1]) == float(np.float32(1e-3)) and c["b2"] == float(np.float32(0.999)) != 0.999


def test_fp32_restatement_lies_inside_the_bound_on_every_case():
    worst = dict(p=0.0, m=0.0, v=0.0)
    for c in AO.CASES:
        st = AO.draw_state(c, N)
        ref = AO.adam_ref(*st, *AO.hp(c))
        bnd = AO.bound(*st, *AO.hp(c))
        assert all(np.isfinite(b).all() and (b > 0).all() for b in bnd.values()), c
        r = AO.worst_ratio(AO.errors(AO.adam_fp32(*st, *AO.hp(c)), ref), bnd)
        assert max(r.values()) <= 1.0, (c, r)
        worst = {k: max(worst[k], r[k]) for k in worst}
        z = AO.SPECIAL["zero"]
        if c["wd"] == 0:                                 # g = 0 from zero moments: nothing moves, exactly
            assert ref[0][z] == st[0][z] and ref[1][z] == 0 and ref[2][z] == 0
    print("\nfp32 restatement, largest error / bound over %d cases x %d elements: m1 %.2f  v1 %.2f  p1 %.2f"
          % (len(AO.CASES), N, worst["m"], worst["v"], worst["p"]))
    print("uniform part of rho in u:", {(b, t): round(AO.rho_uniform(AO.f32(b[0]), AO.f32(b[1]), t), 1)
                                        for b in AO.BETAS for t in (1, 10, 1000, 2 ** 20)})
    assert min(worst.values()) > 0.05                    # the bound is within a small factor of what fp32 really does


def test_representation_gap_stays_within_its_derived_bound():
    """fp32-held against double hyper-parameters: the measured distance from torch's Python-double bias corrections."""
    worst = dict(p=0.0, m=0.0, v=0.0)
    rel = {}
    for c in AO.CASES:
        st = AO.draw_state(c, N)
        lr, b1, b2, eps, wd, gs = c["dbl"]
        hp32 = (c["lr"], c["b1"], c["b2"], c["eps"], c["wd"], c["gscale"])
        a = AO.adam_ref(*st, *AO.hp(c))
        b = AO.adam_ref(*st, c["t"], lr, b1, b2, eps, wd, gs)
        gb = AO.gap_bound(*st, c["t"], c["dbl"], hp32)
        gb = {k: gb[k] + 2.0 ** -50 * np.abs(x) for k, x in zip(("p", "m", "v"), b)}      # (both sides are fp64 evaluations)
        r = AO.worst_ratio(AO.errors(a, b), gb)
        assert max(r.values()) <= 1.0, (c, r)
        worst = {k: max(worst[k], r[k]) for k in worst}
        D = np.abs(b[0] - st[0].astype(np.float64))
        key = (c["dbl"][1], c["dbl"][2], c["t"])
        with np.errstate(divide="ignore", invalid="ignore"):
            g = np.where(D > 0, np.abs(a[0] - b[0]) / D, 0.0)
        # (where the two terms of m1 have opposite signs the update is the remainder of a cancellation and its relative gap has
        #  no meaning: those elements are judged by the bound above, not in this figure)
        gi = st[1].astype(np.float64) * gs + wd * st[0].astype(np.float64)
        ok = st[2].astype(np.float64) * gi >= 0
        if wd == 0:                                      # (likewise g and wd * p inside gi)
            rel[key] = max(rel.get(key, 0.0), float(g[ok].max()))
    print("\nrepresentation gap / gap_bound, largest over the cases: m1 %.2f  v1 %.2f  p1 %.2f" % (worst["m"], worst["v"], worst["p"]))
    print("largest |D_fp32 - D_double| / |D| by (b1, b2, t):")
    for key in sorted(rel):
        print("   ", key, "%.2e" % rel[key])
    assert rel[(0.9, 0.999, 1)] < 1e-4                   # (expected from the code alone: about 1e-5)


def test_every_defect_leaves_the_bound_on_the_cases_it_must_and_on_none_it_cannot():
    table = {d: [] for d in AO.DEFECTS}
    assert set(AO.EXPOSES) == set(AO.DEFECTS) and len(AO.DEFECTS) == 14
    for c in AO.CASES:
        st = AO.draw_state(c, N)
        ref = AO.adam_ref(*st, *AO.hp(c))
        bnd = AO.bound(*st, *AO.hp(c))
        for d in AO.DEFECTS:
            bad = AO.adam_ref(*st, *AO.hp(c), defect=d, lr_prev=c["lr_prev"], elem=AO.ELEM)
            err = AO.errors(bad, ref)
            out = {k: int((err[k] > bnd[k]).sum()) for k in ("p", "m", "v")}
            exposed = any(out.values())
            must, cannot = AO.EXPOSES[d]
            assert not (must(c) and cannot(c))
            if must(c):
                assert exposed, (d, c)
            if cannot(c):
                assert not exposed, (d, c, out)
            if exposed:
                table[d].append((c["id"], out))
    print("\ndefect: cases that expose it / required / free (of %d), most elements outside the bound on one case (p, m, v)" % len(AO.CASES))
    for d in AO.DEFECTS:
        must, cannot = AO.EXPOSES[d]
        n_must = sum(1 for c in AO.CASES if must(c))
        n_free = sum(1 for c in AO.CASES if not must(c) and not cannot(c))
        top = max(table[d], key=lambda x: sum(x[1].values()))[1]
        print("    %-16s %3d / %3d / %3d   %s" % (d, len(table[d]), n_must, n_free, (top["p"], top["m"], top["v"])))
        assert table[d] and n_must > 0

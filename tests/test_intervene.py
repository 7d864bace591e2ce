"""All-pairs intervention readout on the CPU: the host twin of cal_intervene_pairs against the fp64 oracle
(tests/intervene_oracle.py), the Python surface (pooled_representations / intervene / trivial_bank / eval_intervention) on CPU
models, and the argument checks."""
import argparse
import copy
import random

import pytest
import torch

from cal_amd import spmotif
from cal_amd.data import Batch
from cal_amd.intervene import (InterventionResult, eval_intervention, intervene, intervention_readout, pooled_representations,
                               trivial_bank)
from tests.intervene_oracle import GAP, Head, oracle, rows

#: absolute bound on log-probabilities, the one tests/test_gpu_engine.py holds the engine's logits to
TOL = 1e-4

# (B, M, H, C, cat, seed, gain): every value of every axis at least once, the corners (B 1 x M 1; H 256 x C 64 x cat; M 4100 x
# H 128: 65 partner chunks of 64, the last one ragged) and one case for each accumulator shape of the pair kernel (C <= 4, 8, 16,
# 32, 64).  The seeds are chosen so that the ORACLE alone has at most 5 % of its graphs with an open hit bracket (asserted).
CASES = [(1, 1, 1, 2, False, 1, 1.0), (3, 5, 4, 3, True, 1, 1.0), (70, 130, 36, 7, False, 27, 1.0),
         (3, 4100, 128, 3, False, 2, 4.0), (3, 130, 256, 64, True, 3, 1.0), (70, 5, 64, 2, True, 1, 1.0),
         (3, 130, 200, 7, False, 2, 1.0), (3, 70, 64, 12, False, 1, 1.0), (3, 70, 36, 20, True, 1, 1.0)]
IDS = ["B%d-M%d-H%d-C%d-%s" % (c[0], c[1], c[2], c[3], "cat" if c[4] else "add") for c in CASES]
_CACHE = {}


def case(i):
    """(head, xo, xc, ref, oracle) of CASES[i], computed once and shared (never modified)."""
    if i not in _CACHE:
        B, M, H, C, cat, seed, gain = CASES[i]
        head = Head(H, C, cat, seed, gain=gain)
        xo, xc = rows(B, H, seed + 100), rows(M, H, seed + 200)
        ref = oracle(head, xo, xc)["p_do"].argmax(-1)
        ref[1::2] = torch.randint(0, C, ref[1::2].shape, generator=torch.Generator().manual_seed(seed))
        o = oracle(head, xo, xc, ref)
        assert o["logits"].abs().max().item() <= 20.0                               # the inputs keep fp64 logits within +-20
        assert int((o["lo"] != o["hi"]).sum()) <= 0.05 * B                          # condition on the oracle, not a measurement
        _CACHE[i] = (head, xo, xc, ref, o)
    return _CACHE[i]


def check_result(r, o, M, C):
    """Checks 1-4 of one result against the oracle; prints each figure before it asserts."""
    lp = r.logp_pairs.cpu().double()
    e1 = (lp - o["logp"]).abs().max().item()
    e2 = (r.p_do.cpu().double() - o["p_do"]).abs().max().item()
    print("max |logp - oracle| %.3g  max |p_do - oracle| %.3g" % (e1, e2))
    assert r.M == M and r.p_do.shape == o["p_do"].shape and r.hits.dtype == torch.int32 and r.j_min.dtype == torch.int32
    assert e1 <= TOL
    assert e2 <= TOL                                         # (against the fp64 mean: accumulation loss over j would show here)
    hits = r.hits.cpu().long()
    assert bool((o["lo"] <= hits).all()) and bool((hits <= o["hi"]).all())
    jm = r.j_min.cpu().long()
    assert bool(((jm >= 0) & (jm < M)).all())
    at = o["p_ref"].gather(1, jm[:, None]).squeeze(1)
    e4 = max((at - o["p_min"]).abs().max().item(), (r.p_min.cpu().double() - o["p_min"]).abs().max().item())
    print("max |p_min - oracle| %.3g" % e4)
    assert e4 <= TOL


def _moved(head, dev):
    return copy.deepcopy(head).to(dev)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_host_readout_matches_oracle(i):
    head, xo, xc, ref, o = case(i)
    r = intervention_readout(head, xo, xc, ref, pairs=True)
    check_result(r, o, CASES[i][1], CASES[i][3])
    r2 = intervention_readout(head, xo, xc, ref, pairs=True)                        # determinism: the same bits
    for f in ("p_do", "hits", "p_min", "j_min", "logp_pairs"):
        assert torch.equal(getattr(r, f), getattr(r2, f)), f
    plain = intervention_readout(head, xo, xc, ref)
    assert plain.logp_pairs is None and torch.equal(plain.p_do, r.p_do) and torch.equal(plain.hits, r.hits)


def test_lowest_partner_and_lowest_class_on_ties():
    head, xo, _, _, _ = case(2)
    B, C = xo.size(0), CASES[2][3]
    xc = rows(1, xo.size(1), 9).expand(6, -1).contiguous()                          # six identical partners
    ref = torch.zeros(B, dtype=torch.long)
    r = intervention_readout(head, xo, xc, ref, pairs=True)
    assert bool((r.j_min == 0).all()) and bool(((r.hits == 0) | (r.hits == 6)).all())
    with torch.no_grad():                                                           # a head whose logits are all equal
        head2 = Head(8, 5, False, 3)
        head2.fc2_co.weight.zero_()
        head2.fc2_co.bias.fill_(0.25)
    r = intervention_readout(head2, rows(4, 8, 1), rows(7, 8, 2), torch.zeros(4, dtype=torch.long))
    assert bool((r.hits == 7).all())                                                # argmax = class 0
    r = intervention_readout(head2, rows(4, 8, 1), rows(7, 8, 2), torch.ones(4, dtype=torch.long))
    assert bool((r.hits == 0).all()) and bool((r.j_min == 0).all())


def check_ref_sentinels(dev):
    head, xo, xc, ref, _ = case(1)
    head, xo, xc = _moved(head, dev), xo.to(dev), xc.to(dev)
    full = intervention_readout(head, xo, xc, ref.to(dev))
    r = intervention_readout(head, xo, xc, None)
    assert bool((r.hits == 0).all()) and bool(torch.isnan(r.p_min).all()) and bool((r.j_min == -1).all())
    assert torch.equal(r.p_do, full.p_do)
    bad = ref.clone()
    bad[0], bad[2] = -1, CASES[1][3]
    r = intervention_readout(head, xo, xc, bad.to(dev))
    assert r.hits[0] == 0 and r.hits[2] == 0 and bool(torch.isnan(r.p_min[[0, 2]]).all()) and r.j_min[0] == -1 and r.j_min[2] == -1
    assert r.hits[1] == full.hits[1] and r.p_min[1] == full.p_min[1] and r.j_min[1] == full.j_min[1]


def test_ref_missing_or_out_of_range():
    check_ref_sentinels("cpu")


def test_errors_and_empty_batch():
    head, xo, xc, ref, _ = case(1)
    with pytest.raises(ValueError, match="M == 0"):
        intervention_readout(head, xo, xc[:0], ref)
    with pytest.raises(ValueError):
        intervention_readout(head, xo, rows(5, 7, 1), ref)                          # another width
    with pytest.raises(ValueError):
        intervention_readout(head, xo, xc, ref[:2])
    r = intervention_readout(head, xo[:0], xc, None, pairs=True)
    assert isinstance(r, InterventionResult) and r.p_do.shape == (0, 3) and r.hits.shape == (0,) and r.logp_pairs.shape == (0, 5, 3)
    # the host library takes sizes beyond the GPU limits
    big = Head(260, 70, False, 1)
    r = intervention_readout(big, rows(2, 260, 1), rows(3, 260, 2), torch.zeros(2, dtype=torch.long), pairs=True)
    assert (r.logp_pairs.double() - oracle(big, rows(2, 260, 1), rows(3, 260, 2))["logp"]).abs().max().item() <= TOL
    m = _model("CausalGCN")
    b = _batch()
    with pytest.raises(ValueError):
        intervene(m, b, ref="x")
    with pytest.raises(ValueError):
        eval_intervention(m, [b], "cpu", bank="all")


def _args(**kw):
    d = dict(layers=2, hidden=64, with_random=True, without_node_attention=False, without_edge_attention=False,
             fc_num="222", cat_or_add="add", c=0.5, o=1.0, co=0.5)
    d.update(kw)
    return argparse.Namespace(**d)


def _model(name, seed=1, **kw):
    from cal_amd import model as M
    torch.manual_seed(seed)
    return getattr(M, name)(10, 4, _args(**kw))


def _batch(B=16, seed=3):
    return Batch.from_data_list(spmotif.train_mix(B, seed=seed))


def train_three_steps(m, b, lr=1e-2):
    """Three Adam steps of the reference's loss on ``b`` (autograd surface: runs on the engine when the model has one)."""
    import torch.nn.functional as F
    m.train()
    opt = torch.optim.Adam(m.parameters(), lr=lr)
    y = b.y.view(-1)
    for _ in range(3):
        opt.zero_grad()
        c, o, co = m(b)
        uni = torch.full_like(c, 1.0 / c.size(1))
        loss = 0.5 * F.kl_div(c, uni, reduction="batchmean") + F.nll_loss(o, y) + 0.5 * F.nll_loss(co, y)
        loss.backward()
        opt.step()
    return m


def check_ties_to_model(m, b):
    """Check 5: with the batch's own bank, pair (g, g) is the model's eval-mode co output under the identity permutation and
    pair (g, perm[g]) the one under ``perm``."""
    B = int(b.num_graphs)
    dev = b.edge_index.device
    r = intervene(m, b, bank=None, pairs=True)
    assert r.M == B and r.logp_pairs.shape == (B, B, m.num_classes)
    was = m.training
    m.eval()
    with torch.no_grad():
        ident = torch.arange(B, device=dev)
        perm = torch.randperm(B, generator=torch.Generator().manual_seed(5)).to(dev)
        co_i = m(b, perm=ident)[2].clone()
        co_p = m(b, perm=perm)[2].clone()
    m.train(was)
    e_i = (r.logp_pairs[ident, ident] - co_i).abs().max().item()
    e_p = (r.logp_pairs[ident, perm] - co_p).abs().max().item()
    print("identity %.3g  perm %.3g" % (e_i, e_p))
    assert e_i <= TOL and e_p <= TOL
    y = b.y.view(-1)
    assert torch.equal(r.hits.long(), (r.logp_pairs.argmax(-1) == y[:, None]).sum(1))
    ro = intervene(m, b, ref="o")
    with torch.no_grad():
        m.eval()
        o_arg = m(b, perm=ident)[1].argmax(-1)
        m.train(was)
    assert torch.equal(ro.hits.long(), (r.logp_pairs.argmax(-1) == o_arg[:, None]).sum(1))
    return r


def snapshot(m):
    return {k: v.clone() for k, v in m.state_dict().items()}


@pytest.mark.parametrize("name,kw", [("CausalGCN", {}), ("CausalGCN", {"cat_or_add": "cat"}), ("CausalGAT", {}), ("CausalGIN", {})],
                         ids=["gcn-add", "gcn-cat", "gat", "gin"])
def test_cpu_intervene_ties_to_the_model_and_leaves_it_alone(name, kw):
    b = _batch()
    m = train_three_steps(_model(name, **kw), b)
    sd0 = snapshot(m)
    py0, t0 = random.getstate(), torch.get_rng_state()
    check_ties_to_model(m, b)
    xc, xo = pooled_representations(m, b)
    assert xc.shape == (16, 64) and xo.shape == (16, 64)
    m.intervene(b, ref=None)
    eval_intervention(m, [b], "cpu")
    trivial_bank(m, [b], "cpu")
    assert m.training and random.getstate() == py0 and torch.equal(torch.get_rng_state(), t0)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd0[k]), k


def rotation_accuracy(m, batches):
    """(mean over graphs of the share of rotations under which the co head is right, number of graphs with an open bracket):
    the co accuracy through ``model(data, perm=...)`` over the rotations perm_r[g] = (g + r) mod B, which cover every pair once.
    A graph is open when one of its pairs has a top-two log-prob gap of at most GAP."""
    total, n, open_ = 0.0, 0, 0
    was = m.training
    m.eval()
    with torch.no_grad():
        for b in batches:
            B = int(b.num_graphs)
            y = b.y.view(-1)
            g = torch.arange(B, device=y.device)
            right = torch.zeros(B, dtype=torch.float64, device=y.device)
            close = torch.zeros(B, dtype=torch.bool, device=y.device)
            for r in range(B):
                co = m(b, perm=(g + r) % B)[2]
                right += (co.argmax(-1) == y).double()
                top = co.topk(2, dim=-1).values
                close |= (top[:, 0] - top[:, 1]) <= GAP
            total += float((right / B).sum())
            open_ += int(close.sum())
            n += B
    m.train(was)
    return total / n, open_, n


def check_eval_intervention(m, batches, dev):
    res = eval_intervention(m, batches, dev)
    want, open_, n = rotation_accuracy(m, batches)
    print("acc_mean %.6f rotations %.6f open graphs %d" % (res["acc_mean"], want, open_))
    assert res["graphs"] == n
    assert abs(res["acc_mean"] - want) <= open_ / n + 1e-12                          # exact up to the graphs with an open bracket
    rs = [intervene(m, b) for b in batches]
    ys = [b.y.view(-1) for b in batches]
    assert abs(res["acc_do"] - sum(float((r.p_do.argmax(-1) == y).sum()) for r, y in zip(rs, ys)) / n) < 1e-12
    assert abs(res["acc_all"] - sum(float((r.hits == r.M).sum()) for r in rs) / n) < 1e-12
    assert abs(res["p_min_mean"] - sum(float(r.p_min.double().sum()) for r in rs) / n) < 1e-9
    bank = trivial_bank(m, batches, dev)
    assert bank.shape == (n, 64)
    assert torch.equal(bank[:int(batches[0].num_graphs)], pooled_representations(m, batches[0])[0])
    assert trivial_bank(m, batches, dev, max_rows=20).shape == (20, 64)
    fixed = eval_intervention(m, batches, dev, bank=bank)
    assert fixed["graphs"] == n and 0.0 <= fixed["acc_all"] <= fixed["acc_mean"] <= 1.0


def test_cpu_eval_intervention_equals_the_rotations():
    m = train_three_steps(_model("CausalGCN"), _batch())
    batches = [_batch(12, seed=7), _batch(12, seed=8), _batch(7, seed=9)]
    check_eval_intervention(m, batches, "cpu")

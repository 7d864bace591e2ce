"""All-pairs intervention readout on the MI355X: cal_intervene_pairs (HIP) against the fp64 oracle and the host twin at every
accumulator shape, across partner chunks and at the limits; its launch count and determinism; and the Python surface on
engine-backed models on every route family, tied to the model's own co head."""
import random

import pytest
import torch

from cal_amd import _lib, spmotif, synth
from cal_amd.data import Batch
from cal_amd.intervene import eval_intervention, intervene, intervention_readout, pooled_representations
from tests.intervene_oracle import Head, rows
from tests.test_intervene import (CASES, IDS, TOL, _args, _moved, case, check_eval_intervention, check_ref_sentinels, check_result,
                                  check_ties_to_model)

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIELDS = ("p_do", "hits", "p_min", "j_min", "logp_pairs")


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_hip_readout_matches_oracle_and_host(i):
    head, xo, xc, ref, o = case(i)
    M, C = CASES[i][1], CASES[i][3]
    hd = _moved(head, DEV)
    r = intervention_readout(hd, xo.to(DEV), xc.to(DEV), ref.to(DEV), pairs=True)
    check_result(r, o, M, C)
    r2 = intervention_readout(hd, xo.to(DEV), xc.to(DEV), ref.to(DEV), pairs=True)
    for f in FIELDS:                                                               # two calls: the same bits
        assert torch.equal(getattr(r, f), getattr(r2, f)), f
    plain = intervention_readout(hd, xo.to(DEV), xc.to(DEV), ref.to(DEV))
    assert plain.logp_pairs is None
    for f in FIELDS[:4]:                                                           # ... with or without the per-pair output
        assert torch.equal(getattr(r, f), getattr(plain, f)), f
    h = intervention_readout(head, xo, xc, ref, pairs=True)                        # the host twin
    assert (r.logp_pairs.cpu() - h.logp_pairs).abs().max().item() <= TOL
    assert (r.p_do.cpu() - h.p_do).abs().max().item() <= TOL
    closed = o["lo"] == o["hi"]
    assert torch.equal(r.hits.cpu()[closed], h.hits[closed])


def test_launch_count_is_three():
    head, xo, xc, ref, _ = case(3)                                                 # 65 partner chunks
    hd, xo, xc, ref = _moved(head, DEV), xo.to(DEV), xc.to(DEV), ref.to(DEV)
    for pairs in (False, True):
        n0 = _lib.query("cal_launch_count")
        intervention_readout(hd, xo, xc, ref, pairs=pairs)
        assert _lib.query("cal_launch_count") - n0 == 3                            # fold, pairs, finish (cal_hip.h)
    n0 = _lib.query("cal_launch_count")
    intervention_readout(hd, xo[:0], xc, None)
    assert _lib.query("cal_launch_count") == n0                                    # B = 0: nothing


def test_ref_missing_or_out_of_range():
    check_ref_sentinels(DEV)


def test_errors_at_the_gpu_limits():
    z = torch.zeros(2, dtype=torch.long, device=DEV)
    with pytest.raises(ValueError, match="H <= 256"):
        intervention_readout(Head(260, 3, False, 1).to(DEV), rows(2, 260, 1).to(DEV), rows(3, 260, 2).to(DEV), z)
    with pytest.raises(ValueError, match="C <= 64"):
        intervention_readout(Head(8, 65, False, 1).to(DEV), rows(2, 8, 1).to(DEV), rows(3, 8, 2).to(DEV), z)
    with pytest.raises(ValueError, match="2 <= C"):
        intervention_readout(Head(8, 1, False, 1).to(DEV), rows(2, 8, 1).to(DEV), rows(3, 8, 2).to(DEV), z)
    with pytest.raises(ValueError, match="M == 0"):
        intervention_readout(Head(8, 3, False, 1).to(DEV), rows(2, 8, 1).to(DEV), rows(0, 8, 2).to(DEV), z)
    with pytest.raises(ValueError):
        intervention_readout(Head(8, 3, False, 1).to(DEV), rows(2, 8, 1).to(DEV), rows(3, 8, 2), z)      # two devices
    r = intervention_readout(Head(256, 64, True, 1).to(DEV), rows(1, 256, 1).to(DEV), rows(1, 256, 2).to(DEV), z[:1])
    assert r.p_do.shape == (1, 64) and abs(float(r.p_do.sum()) - 1.0) < 1e-5        # at the limits


def _gpu_model(name, seed=1, feat=10, ncls=4, **kw):
    from cal_amd import model as M
    torch.manual_seed(seed)
    return getattr(M, name)(feat, ncls, _args(**kw)).to(DEV)


def _train(m, b, steps=3):
    """``steps`` engine train steps on ``b`` (forward, loss, backward, Adam): BatchNorm statistics and weights move."""
    from cal_amd.engine import StepEngine
    m.train()
    eng = StepEngine(m, lr=1e-2)
    object.__setattr__(m, "_engine", eng)
    perm = torch.randperm(int(b.num_graphs), generator=torch.Generator().manual_seed(0)).to(DEV)
    for _ in range(steps):
        eng.train_step(b, perm, adam=True)
    eng.check_status()
    return eng


def _pooled_both_paths(m, b):
    """pooled_representations on the engine and on the operator path agree.  The rows are sums of ReLU outputs over a graph's
    nodes, so the bound is relative to their size: the 1e-4 tests/test_gpu_explain.py allows between the two paths for values
    in [0, 1], times the largest magnitude of the rows (at least 1)."""
    assert m.engine() is not None
    xc, xo = pooled_representations(m, b)
    m.use_engine = False
    try:
        assert m._engine_for(b.x if b.x is not None else b.feat) is None
        yc, yo = pooled_representations(m, b)
    finally:
        m.use_engine = True
    for u, v in ((xc, yc), (xo, yo)):
        bound = TOL * max(1.0, float(v.abs().max()))
        err = float((u - v).abs().max())
        print("pooled: max |engine - operators| %.3g (bound %.3g)" % (err, bound))
        assert u.shape == v.shape and err <= bound
    return xc, xo


@pytest.mark.parametrize("name,kw", [("CausalGCN", {}), ("CausalGCN", {"cat_or_add": "cat"}), ("CausalGAT", {}), ("CausalGIN", {})],
                         ids=["gcn-add", "gcn-cat", "gat", "gin"])
def test_intervene_ties_to_the_model_on_both_paths(name, kw):
    b = Batch.from_data_list(spmotif.train_mix(16, seed=3)).to(DEV)
    m = _gpu_model(name, **kw)
    _train(m, b)
    r = check_ties_to_model(m, b)                                                  # on the engine
    xc, xo = _pooled_both_paths(m, b)
    assert torch.equal(intervention_readout(m, xo, xc, b.y.view(-1)).p_do, r.p_do)
    m.use_engine = False
    try:
        check_ties_to_model(m, b)                                                  # operator path
    finally:
        m.use_engine = True


@pytest.mark.parametrize("route", ["tiles", "wide", "node-level", "big"])
def test_pooled_rows_on_every_route_family(route):
    m = _gpu_model("CausalGCN", feat=109, ncls=2) if route == "tiles" else _gpu_model("CausalGCN")
    eng = m.engine()
    if route == "tiles":
        b = Batch.from_data_list(synth.tu_like(40, kind="mutag", seed=9)).to(DEV)   # small graphs: several per 64-node tile
        eng.tiles = "force"
        assert b.tile_ptr is not None and b.tile_ptr.numel() - 1 < 40
    elif route == "wide":
        b = Batch.from_data_list(spmotif.train_mix(6, node_num=15, seed=11)).to(DEV)          # 129-256-node graphs
        n = b.ptr[1:] - b.ptr[:-1]
        assert int(n.max()) > 128 and int(n.max()) <= 256
    elif route == "node-level":
        b = Batch.from_data_list(spmotif.train_mix(12, seed=11)).to(DEV)
        eng.fused = False                                                          # no layout facts: the node-level chain
    else:
        b = Batch.from_data_list(synth.ba_graphs(3, n=5000, seed=1)).to(DEV)
    _pooled_both_paths(m, b)
    check_ties_to_model(m, b)
    eng.check_status()


def test_calls_leave_the_state_untouched():
    b = Batch.from_data_list(spmotif.train_mix(16, seed=2)).to(DEV)
    m = _gpu_model("CausalGCN")
    eng = _train(m, b, steps=2)
    torch.cuda.synchronize()
    snap = [t.clone() for t in (eng.flat_p, eng.exp_avg, eng.exp_avg_sq, eng.step_count, eng.buffer("status", 4, torch.int32))]
    bn = {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}
    py0, t0, c0 = random.getstate(), torch.get_rng_state(), torch.cuda.get_rng_state()
    m.intervene(b, pairs=True)
    intervene(m, b, ref="o")
    pooled_representations(m, b)
    eval_intervention(m, [b], DEV)
    assert m.engine() is eng and m.training
    after = (eng.flat_p, eng.exp_avg, eng.exp_avg_sq, eng.step_count, eng.buffer("status", 4, torch.int32))
    for u, v in zip(snap, after):
        assert torch.equal(u, v)
    for k, v in m.state_dict().items():
        if k in bn:
            assert torch.equal(v, bn[k]), k
    assert random.getstate() == py0 and torch.equal(torch.get_rng_state(), t0) and torch.equal(torch.cuda.get_rng_state(), c0)
    eng.train_step(b, torch.arange(16, device=DEV), adam=True)                      # training goes on
    eng.check_status()


def test_eval_intervention_equals_the_rotations():
    m = _gpu_model("CausalGCN")
    _train(m, Batch.from_data_list(spmotif.train_mix(16, seed=3)).to(DEV))
    batches = [Batch.from_data_list(spmotif.train_mix(n, seed=s)).to(DEV) for n, s in ((12, 7), (12, 8), (7, 9))]
    check_eval_intervention(m, batches, DEV)

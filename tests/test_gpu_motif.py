"""Exact motif matching on the MI355X: cal_motif_match (csrc/motif.hip) through every case of tests/test_motif.py -- each output
bit-equal to the host twin and the plain-int restatement, one launch per call and none for B = 0 or P = 0 -- identical bits on a
repeated call, the 256-node hub next to a 2-node graph, a 257-node graph beside small ones, model.explanation_motifs of
engine-backed models against motif_census of the same mask on the CPU, and the state a call leaves behind."""
import random

import pytest
import torch

from cal_amd import _lib, spmotif
from cal_amd.data import Batch, DataLoader
from cal_amd.motif import MotifPatterns, eval_explanation_motifs, motif_census, motif_match
from tests.test_gpu_wl import _args, _gpu_model
from tests.test_motif import (CASES, EDGE, PATH3, SQUARE, TRIANGLE, batch_of, boundary_batch, case_word_boundaries, run,  # noqa: F401
                              star, to_dev)

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---- 1. every case of the CPU file through the device ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.__name__[5:])
def test_hip_equals_host_twin_and_restatement(case):
    case(DEV)


def test_hip_word_boundaries_and_a_257_node_graph(boundary_batch):
    case_word_boundaries(DEV, boundary_batch)


# ---- 2. launches, repeated calls -------------------------------------------------------------------------------------------------
def test_one_launch_and_the_same_bits_twice():
    b = Batch.from_data_list(spmotif.train_mix(12, node_num=7, seed=3)).to(DEV)
    pp = MotifPatterns(spmotif.motif_batch(DEV))                             # (a pattern batch on the device is copied once)
    n0 = _lib.query("cal_launch_count")
    m1 = motif_match(b, pp)
    m2 = motif_match(b, pp)
    m3 = motif_match(b, pp, induced=True)
    assert _lib.query("cal_launch_count") - n0 == 3
    for x, y in zip(m1, m2):
        assert x.is_cuda and torch.equal(x, y)
    y = b.y.view(-1)
    assert (m1.count[torch.arange(12, device=DEV), y] > 0).all()             # every graph contains its own label's motif
    assert (m3.count <= m1.count).all() and int(m1.truncated.sum()) == 0
    host = motif_match(b.to("cpu"), spmotif.motif_batch())
    for x, y in zip(m1, host):
        assert torch.equal(x.cpu(), y)


def test_hub_next_to_a_two_node_graph_and_all_patterns():
    """Every root of the star's hub walks 255 neighbours; the lanes of the 2-node graph's workgroup have one root each."""
    tg = batch_of([star(256), EDGE, star(200)])
    res = run(tg, batch_of([PATH3, TRIANGLE, SQUARE, EDGE]), DEV)
    assert res[0].tolist() == [[64770, 0, 0, 510], [0, 0, 0, 2], [199 * 198, 0, 0, 398]]
    res = run(tg, batch_of([star(5)]), DEV, budget=300)                      # a budget that bites below the hub's roots
    assert res[2][0, 0] == 255 and res[2][1, 0] == 0


# ---- 3. the census of engine-backed models ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["CausalGCN", "CausalGAT", "CausalGIN"])
def test_explanation_motifs_of_an_engine_backed_model(name):
    m = _gpu_model(name, _args())
    assert m.engine() is not None
    b = Batch.from_data_list(spmotif.train_mix(6, node_num=7, seed=11))
    bd = to_dev(b, DEV)
    gt = spmotif.ground_truth(b)[1]
    res = m.explanation_motifs(bd, ratio=0.3, edge_gt=gt.to(DEV))
    m.engine().check_status()
    assert res["contains"].is_cuda and res["yhat"].shape == (6,) and torch.equal(res["y"].cpu(), b.y.view(-1))
    mask = res["explanation"].edge_mask.cpu()
    want = motif_census(b, edge_mask=mask, prototypes=spmotif.motif_batch())
    for key in ("contains", "isomorphic", "occurrences", "truncated", "skipped", "nodes", "edges", "match_nodes"):
        assert torch.equal(res[key].cpu(), want[key]), key
    for x, y in zip(res["match"], want["match"]):
        assert torch.equal(x.cpu(), y)
    assert torch.equal(res["planted"].cpu(), motif_census(b, edge_mask=mask & gt, prototypes=spmotif.motif_batch())["contains"])
    assert int(res["nodes"].sum()) > 0 and int(mask.sum()) > 0


def test_the_motif_census_leaves_the_engines_state_untouched():
    from cal_amd.engine import StepEngine
    m = _gpu_model("CausalGCN", _args())
    m.train()
    eng = StepEngine(m, lr=1e-3, deterministic=True)
    object.__setattr__(m, "_engine", eng)
    gs = spmotif.train_mix(12, node_num=7, seed=9)
    tb = Batch.from_data_list(gs).to(DEV)
    perm = torch.randperm(12, device=DEV)
    for _ in range(2):
        eng.train_step(tb, perm, adam=True)
    torch.cuda.synchronize()
    snap = [t.clone() for t in (eng.flat_p, eng.exp_avg, eng.exp_avg_sq, eng.step_count, eng.buffer("status", 4, torch.int32))]
    bn = {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}
    py0, t0, c0 = random.getstate(), torch.get_rng_state(), torch.cuda.get_rng_state()
    res = m.explanation_motifs(Batch.from_data_list(gs[:6]).to(DEV), k=6)
    ev = eval_explanation_motifs(m, DataLoader(gs, batch_size=8, shuffle=False), DEV, k="gt")
    assert res["contains"].shape == (6, 4) and "planted" not in res and ev["graphs"] == 12
    assert ev["skipped"] == 0 and ev["truncated"] == 0
    assert all(0.0 <= ev[key] <= 1.0 for key in ("contain_rate", "iso_rate", "planted_rate", "wl_not_iso"))
    torch.cuda.synchronize()
    assert m.engine() is eng and m.training
    after = (eng.flat_p, eng.exp_avg, eng.exp_avg_sq, eng.step_count, eng.buffer("status", 4, torch.int32))
    for u, v in zip(snap, after):
        assert torch.equal(u, v)
    for k, v in m.state_dict().items():
        if k in bn:
            assert torch.equal(v, bn[k]), k
    assert random.getstate() == py0 and torch.equal(torch.get_rng_state(), t0) and torch.equal(torch.cuda.get_rng_state(), c0)
    eng.train_step(tb, perm, adam=True)                      # training goes on
    eng.check_status()

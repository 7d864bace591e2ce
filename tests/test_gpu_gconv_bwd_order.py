"""The order of the two products behind P1 in the per-graph GCNConv backward (engine_gconv_bwd_body.hpp, -DCAL_GCB_ORDER): with
order 1 all eight waves run dX' = dz W^T, one 32 x 32 tile each, the two BatchNorm-backward column sums cross from the wave of row
tile 0 to the wave of row tile 1 through LDS, and then all eight run dW = x'^T dz.  Whichever order the library was built
with, the step is held here to the same step in fp64 (tests/tools/fuzz_engine.py: logits, losses, every gradient, the Adam update
and -- through the eval-mode forward of the stepped model -- the BatchNorm running statistics, at the bounds of
test_random_shape_sweep_cases_on_the_engine), on the shapes where the tiling changes:

  graphs of 1, 2, 31, 32, 33, 63, 64 nodes   one and two row tiles, the zero-term continuation of the column sums (<= 32 rows),
                                             an edgeless graph (index 1) and two stars whose hubs have 63 and 62 neighbours
  hidden 128 and 64                          K = 128: 2 x 4 tiles of dX', 8 of dW;  K = 64: 2 x 2 and 4
  140 graphs of 3-8 nodes, hidden 128        more workgroups than CUs: the LEAN instantiations (which keep order 0)

each with the attention backward folded into the last layer's launch (k_gconv_bwd_att: the ATT entry of the same body) and as a
launch of its own, which must agree as in test_gpu_att_fold.py.

The seeds: tiny batches can be ill-conditioned (a ReLU input at rounding distance from zero, BatchNorm over few rows).  For the
three cases below the fp32 oracle stays within 0.007 / 0.007 / 0.006 of the judge's floor (1e-4 of each tensor's scale) from the
fp64 step on the CPU, i.e. they are well-conditioned and a miss is the engine's."""
import os
import sys

import pytest
import torch

from tests.test_gpu_att_fold import _batches, _check_on_against_off, _model, _state, _step

pytestmark = pytest.mark.gpu
DEV = "cuda"
NFEAT, NCLS = 10, 4
TILE_EDGES = [31, 2, 64, 32, 33, 1, 63]                   # index 1: edgeless; index 2 and 6: stars (_ragged_batch)
LEAN_SMALL = [3 + i % 6 for i in range(140)]              # 140 graphs x 2 slices > the CUs of the device
CASES = [
    pytest.param(128, TILE_EDGES, 3101, True, id="h128-tile-edges"),
    pytest.param(64, TILE_EDGES, 3104, True, id="h64-tile-edges"),
    pytest.param(128, LEAN_SMALL, 3101, False, id="h128-lean"),
]


def _fuzz():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
    import fuzz_engine
    return fuzz_engine


@pytest.mark.parametrize("fold", ["1", "0"])
@pytest.mark.parametrize("hidden,sizes,seed,folds", CASES)
def test_step_tracks_the_fp64_step(hidden, sizes, seed, folds, fold, monkeypatch):
    monkeypatch.setenv("CAL_AMD_ATT_FOLD", fold)
    if not folds:      # the premise of the LEAN case (Route: lean_bb = workgroups of a one-branch launch > CUs)
        assert len(sizes) * (hidden // 64) > torch.cuda.get_device_properties(0).multi_processor_count
    assert _fuzz().run((hidden, 2, NFEAT, NCLS, sizes), seed) == []


@pytest.mark.parametrize("hidden,sizes,seed,folds", CASES)
def test_folded_and_unfolded_steps_agree_and_launch_the_backward(hidden, sizes, seed, folds, monkeypatch):
    _, bd = _batches(seed, sizes)
    B = len(sizes)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(seed))
    sd = _state("CausalGCN", hidden, 2)
    on = _step(monkeypatch, "1", "CausalGCN", sd, bd, perm, hidden, 2)
    off = _step(monkeypatch, "0", "CausalGCN", sd, bd, perm, hidden, 2)
    _check_on_against_off(on, off, folds)
    for run in (on, off):
        assert "k_gconv_bwd" in run["names"], run["names"]


@pytest.mark.parametrize("fold", ["1", "0"])
@pytest.mark.parametrize("hidden", [128, 64])
def test_deterministic_engine_gives_the_same_bits_twice(hidden, fold, monkeypatch):
    from cal_amd.engine import StepEngine
    monkeypatch.setenv("CAL_AMD_ATT_FOLD", fold)
    _, bd = _batches(3101, TILE_EDGES)
    B = len(TILE_EDGES)
    sd = _state("CausalGCN", hidden, 2)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(3)).to(DEV)
    runs = []
    for _ in range(2):
        m = _model("CausalGCN", sd, hidden, 2)
        eng = StepEngine(m, lr=1e-3, deterministic=True)
        stats = [eng.train_step(bd, perm, adam=True).clone() for _ in range(2)]
        eng.check_status()
        runs.append((eng.buffer("logp", 3 * B * NCLS).clone(), torch.stack(stats), eng.flat_p.detach().clone(),
                     torch.cat([p.grad.detach().flatten() for p in m.parameters()])))
    for u, v in zip(runs[0], runs[1]):
        assert torch.equal(u, v)                           # bit for bit

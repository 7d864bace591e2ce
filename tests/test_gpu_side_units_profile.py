"""The profiled launch of the step engine's side units (engine_unit.hpp: gconv_fwd_att.hip, gconv_bwd_att.hip, gconv_bwd_seq.hip):
inside a single-kernel profiling scope the dispatch carries the scope's two events across to the unit, and the scope keeps its
record only when a kernel used them.  bench.py's roofline block relies on that; nothing else in the suite did.

CausalGCN, hidden 128, two layers, one batch of three graphs (5, 33, 64 nodes), striped sums: two eager training steps under
cal_engine_profile(1), once with both attention folds on (the default: layer 2's forward is k_gconv_fwd_att, its backward
k_gconv_bwd_att) and once with both off (k_gconv_fwd and k_gconv_bwd of engine.hip's own code object, and for the non-LEAN
backward gconv_bwd_seq.hip); layer 1's backward goes through gconv_bwd_seq.hip in both.  Class 2 is the per-graph backbone
forward, class 4 the per-graph backbone backward: one record per layer and step, each with a duration above zero (an event pair
that no dispatch stamped reads -1), and the same number of records per class whichever unit launched the kernel.

The counts are the parent's: this test passed unchanged on the build of the commit before the side units shared one protocol
(c0a4cdd), run once on an MI355X -- class 2 and class 4 with 4 records each over the two steps, folds on and folds off."""
import collections
import ctypes

import numpy as np
import pytest
import torch

from tests.test_gpu_att_fold import _batches, _model, _state
from tests.test_gpu_att_fwd_fold import _folded
from tests.test_gpu_engine import _stage_names

pytestmark = pytest.mark.gpu
DEV = "cuda"
HIDDEN, LAYERS, STEPS = 128, 2, 2
SIZES = [5, 33, 64]


def _profiled_steps(monkeypatch, fold):
    """(launch sites of the last step, {class: [milliseconds of every record]}) of STEPS eager training steps of a fresh engine"""
    from cal_amd import _lib
    from cal_amd.engine import StepEngine
    h = _lib.lib()
    monkeypatch.setenv("CAL_AMD_STRIPED", "1")
    monkeypatch.setenv("CAL_AMD_ATT_FOLD", fold)
    monkeypatch.setenv("CAL_AMD_ATT_FWD_FOLD", fold)
    _, bd = _batches(HIDDEN, SIZES)
    eng = StepEngine(_model("CausalGCN", _state("CausalGCN", HIDDEN, LAYERS), HIDDEN, LAYERS), lr=1e-3)
    perm = torch.tensor([1, 2, 0], device=DEV)
    cap = 64 * STEPS
    buf = (ctypes.c_double * (3 * cap))()
    h.cal_engine_profile(1)
    try:
        for _ in range(STEPS):
            eng.train_step(bd, perm, adam=True)
        torch.cuda.synchronize()
        n = int(h.cal_engine_profile_read(buf, cap))
    finally:
        h.cal_engine_profile(0)
    eng.check_status()
    assert 0 < n < cap
    ms = collections.defaultdict(list)
    for cls, t, _work in np.array(buf[:3 * n], dtype=np.float64).reshape(n, 3):
        ms[int(cls)].append(t)
    return _stage_names(), dict(ms)


def test_profiled_side_unit_launches_keep_their_records(monkeypatch):
    on_names, on = _profiled_steps(monkeypatch, "1")
    off_names, off = _profiled_steps(monkeypatch, "0")
    print("folds on ", on_names, {k: (len(v), min(v)) for k, v in on.items()})
    print("folds off", off_names, {k: (len(v), min(v)) for k, v in off.items()})
    # the launch sites say which units ran: the folded forward replaces k_gconv_fwd + k_att_fwd_graph; the folded backward is the
    # k_att_bwd_graph site, and layer 2 leaves no k_gconv_bwd marks (tests/test_gpu_att_fold.py: _check_on_against_off)
    assert _folded(on_names) and "k_gconv_fwd_att" not in off_names and "k_att_fwd_graph" in off_names
    for names in (on_names, off_names):
        assert "k_att_bwd_graph" in names and "k_gconv_bwd" in names, names
    assert on_names.count("k_gconv_bwd") < off_names.count("k_gconv_bwd"), (on_names, off_names)
    for run in (on, off):
        for cls in (2, 4):
            assert len(run.get(cls, [])) >= LAYERS * STEPS, (cls, run)
            assert all(t > 0 for t in run[cls]), (cls, run[cls])
    assert {k: len(v) for k, v in on.items()} == {k: len(v) for k, v in off.items()}

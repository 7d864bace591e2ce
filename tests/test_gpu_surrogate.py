"""cal_surrogate_fit on the MI355X: the HIP kernel on the case table of tests/surrogate_oracle.py -- statuses everywhere, phi / phi0 /
r2 at the oracle's bounds, the host twin's bits, the same bits on a second call, in another batch and in a graph replay --, the
launch count, and the drivers on engine-backed models."""
import pytest
import torch

from cal_amd import _lib, spmotif
from cal_amd.data import Batch
from cal_amd.surrogate import MAX_PLAYERS, kernel_shap, surrogate_fit
from tests.occlude_oracle import hand_batch
from tests.surrogate_oracle import CASES, IDS, case, fit_args
from tests.test_gpu_intervene import _gpu_model, _train
from tests.test_surrogate import (check_against_shapley, check_case, check_elements_against_shapley, check_flags,
                                  check_independence, check_surface, run_case, same_bits)

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_hip_meets_the_contract(i):
    c = CASES[i]
    r = run_case(c, DEV)
    check_case(c, r, limit=MAX_PLAYERS)
    same_bits(r, run_case(c, DEV))                                                 # two calls: the same bits
    h = run_case(c)                                                                # the host twin: the same bits
    pp = c["pl_ptr"].tolist()
    for g in range(len(c["graphs"])):
        if int(r[3][g]) == int(h[3][g]):                                           # (the twin has no player limit)
            same_bits((r[0][pp[g]:pp[g + 1]], r[1][g:g + 1], r[2][g:g + 1]), (h[0][pp[g]:pp[g + 1]], h[1][g:g + 1], h[2][g:g + 1]))
        else:
            assert c["gpu_status"] is not None and c["gpu_status"][g] == 2


def test_hip_is_independent_of_the_batch_and_of_absent_flags():
    check_independence(DEV)
    check_flags(DEV)


def test_one_launch_per_fit():
    for name in ("n2-minimal", "limit-n127-lime", "bad-values", "over-n128"):
        args, kw = fit_args(case(name), DEV)
        n0 = _lib.query("cal_launch_count")
        surrogate_fit(*args, **kw)
        assert _lib.query("cal_launch_count") - n0 == 1
    args, kw = fit_args(case("n2-minimal"), DEV)
    n0 = _lib.query("cal_launch_count")
    phi, phi0, r2, st = surrogate_fit(args[0], args[1][:1], args[2][:0], args[3][:0], args[4][:0], args[5][:1], args[6][:0],
                                      v_empty=kw["v_empty"][:0], v_full=kw["v_full"][:0])
    assert _lib.query("cal_launch_count") == n0 and phi0.numel() == 0                # B = 0: nothing


def test_a_captured_fit_replays_to_the_same_bits():
    c = case("lanes-lime-n63-n64")
    args, kw = fit_args(c, DEV)
    eager = surrogate_fit(*args, **kw)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        surrogate_fit(*args, **kw)                                                 # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r = surrogate_fit(*args, **kw)                                             # (a read-back inside would end the capture)
    for _ in range(2):
        for t in r:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        same_bits([t.cpu() for t in r], [t.cpu() for t in eager])


def test_surface_on_an_engine_backed_model():
    b = Batch.from_data_list(spmotif.train_mix(3, node_num=6, seed=4)).to(DEV)
    m = _gpu_model("CausalGCN")
    _train(m, b)
    assert m.engine() is not None
    check_surface(m, b, DEV)


def test_kernel_shap_approaches_exact_shapley_on_the_engine():
    m = _gpu_model("CausalGCN", feat=3)
    _train(m, hand_batch([(3, [(0, 1), (1, 0), (1, 2), (2, 1)])] * 4).to(DEV))
    check_against_shapley(m, DEV)


@pytest.mark.parametrize("use", ["edges", "nodes"])
def test_kernel_shap_of_a_restricted_game_approaches_exact_shapley_on_the_engine(use):
    m = _gpu_model("CausalGCN", feat=3)
    _train(m, hand_batch([(3, [(0, 1), (1, 0), (1, 2), (2, 1)])] * 4).to(DEV))
    check_elements_against_shapley(m, DEV, use)


def test_a_graph_over_the_limit_raises_with_the_count():
    ring = lambda n: [p for u in range(n) for p in ((u, (u + 1) % n), ((u + 1) % n, u))]
    b = hand_batch([(5, ring(5)), (70, ring(70)), (66, ring(66))]).to(DEV)           # 10, 140 and 132 columns
    m = _gpu_model("CausalGCN", feat=3)
    with pytest.raises(ValueError, match="2 graphs: more than 127 players"):
        kernel_shap(m, b, samples=300)
    sg = kernel_shap(m, b, undirected="mean", samples=300)                         # 5, 70 and 66 undirected edges
    assert int(sg.status.abs().sum()) == 0 and not bool(sg.score.isnan().any())

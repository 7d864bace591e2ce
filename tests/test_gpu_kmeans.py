"""cal_kmeans on the MI355X: the HIP kernels against the fp64 oracle on the case table of tests/kmeans_oracle.py, bit for bit against
the host twin, the integer oracle and the numpy chain on the exact and the order cases; determinism across calls; cal_kmeans_assign;
the launch count; the early exit; the workspace; the limits; the Python surface on engine-backed models; and a graph capture."""
import random

import numpy as np
import pytest
import torch

from cal_amd import _lib, spmotif
from cal_amd.concepts import assign, eval_concepts, kmeans, node_bank
from cal_amd.data import Batch
from tests.kmeans_oracle import CASES, EXACT, EXACT_SPANS, IDS, ORDER, case, exact_case
from tests.test_gpu_intervene import _gpu_model, _train
from tests.test_kmeans import (check_case, check_exact, check_iterations, check_order, check_surface, planted, run_case, run_exact,
                               run_order, same_bits)

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_hip_meets_the_contract(i):
    r = run_case(i, DEV)
    check_case(i, r)
    same_bits(r, run_case(i, DEV))                                                 # two calls: the same bits
    X, _, C, _ = case(i)
    a, d = assign(X.to(DEV), C.to(DEV))                                            # cal_kmeans_assign: the assignment of a step
    assert torch.equal(a, r.assign)
    live = a >= 0
    assert torch.isposinf(d[~live]).all() and float(d[live].double().sum()) == pytest.approx(float(r.inertia[0]), rel=1e-12, abs=0)
    for span in (128, 256):                                                        # across spans: the same assignment of a step
        s = run_case(i, DEV, span=span)
        assert torch.equal(s.assign, r.assign) and torch.equal(s.counts, r.counts) and torch.equal(s.moved, r.moved)


@pytest.mark.parametrize("span", EXACT_SPANS)
@pytest.mark.parametrize("i", range(len(EXACT)))
def test_hip_is_exact_on_integer_rows(i, span):
    r = run_exact(i, span, DEV)
    check_exact(i, r)
    same_bits(r, run_exact(i, span))                                               # the host twin
    same_bits(r, run_exact(i, span, DEV))


@pytest.mark.parametrize("i", range(len(ORDER)))
def test_hip_sums_in_the_order_of_the_rule(i):
    r = run_order(i, DEV)
    check_order(i, r)
    h = run_order(i)                                                               # the host twin: the same centroid bits
    assert torch.equal(r.centroids.cpu().view(torch.int32), h.centroids.view(torch.int32)) and torch.equal(r.assign.cpu(), h.assign)


@pytest.mark.parametrize("span", [0, 256])
def test_hip_iterations_converge_and_stop(span):
    check_iterations(DEV, span)


def test_launch_count_and_early_exit():
    X, _, init = planted()
    X, init = X.to(DEV), init.to(DEV)
    for iters in (1, 3, 50):
        n0 = _lib.query("cal_launch_count")
        r = kmeans(X, 6, iters=iters, init=init)
        assert _lib.query("cal_launch_count") - n0 == 2 * iters                    # step + update per iteration (cal_hip.h)
    run = int(r.iters_run)
    assert run < 50 and int(r.moved[run - 1]) == 0                                  # the rest of the 100 launches returned at once
    short = kmeans(X, 6, iters=run, init=init)
    assert torch.equal(short.centroids.view(torch.int32), r.centroids.view(torch.int32)) and torch.equal(short.assign, r.assign)
    assert torch.equal(short.counts, r.counts) and torch.equal(short.inertia, r.inertia[:run]) and torch.equal(short.moved, r.moved[:run])
    n0 = _lib.query("cal_launch_count")
    assign(X, r.centroids)
    assert _lib.query("cal_launch_count") - n0 == 1
    n0 = _lib.query("cal_launch_count")
    e = kmeans(X[:0], 6, iters=4, init=r.centroids)                                # N = 0: nothing
    a, d = assign(X[:0], r.centroids)
    assert _lib.query("cal_launch_count") == n0 and int(e.iters_run) == 0 and torch.equal(e.centroids, r.centroids) and a.numel() == 0


def test_workspace_is_partials_not_pairs():
    N, H = 2_000_000, 128
    for K in (16, 64):
        assert 0 < _lib.query("cal_kmeans_ws", N, K, H, 0) < N * K * 4
    assert _lib.query("cal_kmeans_ws", 2 ** 31 - 1, 64, 256, 0) < 40 << 20          # at the limits: tens of MB


def test_errors_at_the_gpu_limits():
    with pytest.raises(ValueError, match="K <= 64"):
        kmeans(torch.rand(100, 8, device=DEV), 65)
    with pytest.raises(ValueError, match="H <= 256"):
        kmeans(torch.rand(100, 257, device=DEV), 3)
    with pytest.raises(ValueError, match="K <= 64"):
        assign(torch.rand(100, 8, device=DEV), torch.rand(65, 8, device=DEV))
    with pytest.raises(ValueError, match="H <= 256"):
        assign(torch.rand(100, 257, device=DEV), torch.rand(3, 257, device=DEV))
    with pytest.raises(ValueError, match="one device"):
        kmeans(torch.rand(100, 8, device=DEV), 3, init=torch.rand(3, 8))
    with pytest.raises(ValueError, match="one device"):
        assign(torch.rand(100, 8, device=DEV), torch.rand(3, 8))
    X = torch.rand(500, 256, device=DEV)
    r = kmeans(X, 64, iters=3)                                                     # at the limits
    assert int(r.counts.sum()) == 500 and int(r.iters_run) >= 1 and torch.isfinite(r.centroids).all()
    same_bits(r, kmeans(X, 64, iters=3))


@pytest.mark.parametrize("name,kw", [("CausalGCN", {}), ("CausalGCN", {"cat_or_add": "cat"}), ("CausalGAT", {}), ("CausalGIN", {})],
                         ids=["gcn-add", "gcn-cat", "gat", "gin"])
def test_surface_on_engine_backed_models(name, kw):
    b = Batch.from_data_list(spmotif.train_mix(16, seed=3)).to(DEV)
    m = _gpu_model(name, **kw)
    _train(m, b)
    assert m.engine() is not None
    check_surface(m, b, DEV)


def test_calls_leave_the_state_untouched():
    b = Batch.from_data_list(spmotif.train_mix(16, seed=2)).to(DEV)
    m = _gpu_model("CausalGCN")
    eng = _train(m, b, steps=2)
    torch.cuda.synchronize()
    snap = [t.clone() for t in (eng.flat_p, eng.exp_avg, eng.exp_avg_sq, eng.step_count, eng.buffer("status", 4, torch.int32))]
    bn = {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}
    py0, t0, c0 = random.getstate(), torch.get_rng_state(), torch.cuda.get_rng_state()
    node_bank(m, [b], DEV)
    con = m.discover_concepts([b], DEV, k=4, iters=5, restarts=2)
    m.assign_concepts(b, con)
    m.concept_report(con, examples=2)
    eval_concepts(m, [b], DEV, k=4, test_loader=[b], iters=5)
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


def test_a_captured_call_replays_to_the_same_bits():
    X, _, init = planted()
    X = X.to(DEV)
    c0 = X[init.to(DEV)].clone()
    eager = kmeans(X, 6, iters=6, init=c0)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        kmeans(X, 6, iters=6, init=c0)                                             # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r = kmeans(X, 6, iters=6, init=c0)
    for _ in range(2):
        r.assign.fill_(-7)
        r.centroids.zero_()
        g.replay()
        torch.cuda.synchronize()
        same_bits(r, eager)

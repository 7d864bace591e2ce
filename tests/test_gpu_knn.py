"""cal_knn on the MI355X: the HIP kernels against the fp64 oracle on the case table of tests/knn_oracle.py, bit for bit against the
oracle and the host twin on the exact cases; determinism across calls, chunkings and outputs; the launch count; the limits; and
the Python surface on engine-backed models."""
import random

import numpy as np
import pytest
import torch

from cal_amd import _lib, spmotif
from cal_amd.data import Batch
from cal_amd.intervene import pooled_representations
from cal_amd.neighbors import embedding_bank, eval_disentanglement, knn, nearest_examples
from tests.knn_oracle import CASES, EXACT, IDS, case, exact_case, gamma, oracle
from tests.test_gpu_intervene import _gpu_model, _pooled_both_paths, _train
from tests.test_intervene import TOL
from tests.test_knn import check_case, check_exact, check_surface, run_case, run_exact

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _same(a, b):
    assert torch.equal(a.idx, b.idx) and torch.equal(a.dist.view(torch.int32), b.dist.view(torch.int32))
    assert (a.votes is None) == (b.votes is None) and (a.votes is None or torch.equal(a.votes, b.votes))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_hip_meets_the_contract(i):
    r = run_case(i, DEV)
    check_case(i, r)
    _same(r, run_case(i, DEV))                                                     # two calls: the same bits
    for chunk in (32, 64, 0):                                                      # ... under every chunking
        _same(r, run_case(i, DEV, chunk=chunk))
    if CASES[i]["C"]:                                                              # ... with or without the votes
        c = CASES[i]
        Q, X, skip, _, _ = case(i)
        plain = knn(Q.to(DEV), X.to(DEV), c["k"], metric=c["metric"], skip=None if skip is None else skip.to(DEV), chunk_rows=c["chunk"])
        assert plain.votes is None and torch.equal(plain.idx, r.idx) and torch.equal(plain.dist, r.dist)


@pytest.mark.parametrize("i", range(len(EXACT)))
def test_hip_is_exact_on_integer_rows(i):
    r = run_exact(i, DEV)
    check_exact(i, r)
    h = run_exact(i)                                                               # the host twin
    assert torch.equal(r.idx.cpu(), h.idx) and torch.equal(r.dist.cpu().view(torch.int32), h.dist.view(torch.int32))
    for chunk in (32, 64, 0):
        _same(r, run_exact(i, DEV, chunk=chunk))


def test_launch_count_is_two():
    for i in (0, 6, 8):                                                            # one chunk; 32 chunks; the plan's chunks
        n0 = _lib.query("cal_launch_count")
        run_case(i, DEV)
        assert _lib.query("cal_launch_count") - n0 == 2                            # select, merge (cal_hip.h)
    Q, X = case(6)[:2]
    n0 = _lib.query("cal_launch_count")
    r = knn(Q[:0].to(DEV), X.to(DEV), 5)
    assert _lib.query("cal_launch_count") == n0 and r.idx.shape == (0, 5)          # nq = 0: nothing


def test_workspace_is_lists_not_pairs():
    nq = M = 8000
    assert 0 < _lib.query("cal_knn_ws", nq, M, 10, 0) < nq * M * 4
    assert _lib.query("cal_knn_ws", 128, M, 10, 0) < 128 * M * 4


def test_errors_at_the_gpu_limits():
    Q, X = torch.rand(2, 8, device=DEV), torch.rand(70, 8, device=DEV)
    with pytest.raises(ValueError, match="k <= 64"):
        knn(Q, X, 65)
    with pytest.raises(ValueError, match="H <= 256"):
        knn(torch.rand(2, 257, device=DEV), torch.rand(70, 257, device=DEV), 5)
    with pytest.raises(ValueError, match="num_classes <= 64"):
        knn(Q, X, 5, labels=torch.zeros(70, dtype=torch.long, device=DEV), num_classes=65)
    with pytest.raises(ValueError, match="one device"):
        knn(Q, X.cpu(), 5)
    with pytest.raises(ValueError, match="one device"):
        knn(Q, X, 5, skip=torch.zeros(2, dtype=torch.long))
    lab = torch.arange(70, device=DEV) % 64
    r = knn(torch.rand(1, 256, device=DEV), torch.rand(70, 256, device=DEV), 64, metric="cosine", labels=lab, num_classes=64)
    assert (r.idx >= 0).all() and int(r.votes.sum()) == 64                         # at the limits


@pytest.mark.parametrize("name,kw", [("CausalGCN", {}), ("CausalGCN", {"cat_or_add": "cat"}), ("CausalGAT", {}), ("CausalGIN", {})],
                         ids=["gcn-add", "gcn-cat", "gat", "gin"])
def test_surface_on_engine_backed_models(name, kw):
    b = Batch.from_data_list(spmotif.train_mix(16, seed=3)).to(DEV)
    m = _gpu_model(name, **kw)
    _train(m, b)
    assert m.engine() is not None
    check_surface(m, b, DEV)
    # engine against the operator path: the rows of the two paths differ by at most the bound of _pooled_both_paths, so a
    # squared distance moves by at most 2 |q - x| (2 e sqrt(H)) + (2 e sqrt(H))^2 on top of the pair's tolerance; positions whose
    # gaps exceed that on both sides must agree
    xc, xo = _pooled_both_paths(m, b)
    on = m.nearest_examples(b, embedding_bank(m, [b], DEV), k=5)
    m.use_engine = False
    try:
        off = m.nearest_examples(b, embedding_bank(m, [b], DEV), k=5)
    finally:
        m.use_engine = True
    rows = xo.double().cpu().numpy()
    e = 2.0 * TOL * max(1.0, float(xo.abs().max())) * np.sqrt(rows.shape[1])
    o = oracle(rows, rows, 5)
    order = np.argsort(o["d64"], axis=1, kind="stable")
    ds = np.take_along_axis(o["d64"], order, 1)[:, :6]
    slack = 2.0 * np.sqrt(ds) * e + e * e + gamma(rows.shape[1]) * 4.0 * (rows * rows).sum(1).max()
    gap = ds[:, 1:] - ds[:, :-1] > slack[:, 1:] + slack[:, :-1]
    closed = np.concatenate([np.ones((len(rows), 1), bool), gap[:, :-1]], 1) & gap
    print("positions closed between the two paths: %d of %d" % (closed.sum(), closed.size))
    assert (on.idx.cpu().numpy()[closed] == off.idx.cpu().numpy()[closed]).all()


def test_calls_leave_the_state_untouched():
    b = Batch.from_data_list(spmotif.train_mix(16, seed=2)).to(DEV)
    m = _gpu_model("CausalGCN")
    eng = _train(m, b, steps=2)
    torch.cuda.synchronize()
    snap = [t.clone() for t in (eng.flat_p, eng.exp_avg, eng.exp_avg_sq, eng.step_count, eng.buffer("status", 4, torch.int32))]
    bn = {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}
    py0, t0, c0 = random.getstate(), torch.get_rng_state(), torch.cuda.get_rng_state()
    bank = embedding_bank(m, [b], DEV)
    m.nearest_examples(b, bank, k=3, space="c")
    m.knn_probe(bank, k=3)
    eval_disentanglement(m, [b], DEV, k=3)
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

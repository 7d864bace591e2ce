"""cal_knn on the host: the libcalhost twin against the fp64 oracle on the shared case table and on the exact cases; the oracle tied
to torch.cdist / torch.topk; seeded defects noticed by the table; spmotif.context_of; and the Python surface on CPU models."""
import random

import numpy as np
import pytest
import torch

from cal_amd import spmotif, synth
from cal_amd.data import Batch
from cal_amd.intervene import pooled_representations
from cal_amd.neighbors import EmbeddingBank, embedding_bank, eval_disentanglement, knn, knn_probe, nearest_examples
from tests.knn_oracle import (CASES, EXACT, IDS, case, check_contract, exact_case, oracle, pair_distances, probe_chance, probe_counts,
                              probe_overlap)
from tests.test_intervene import _batch, _model, snapshot, train_three_steps


def run_case(i, dev="cpu", chunk=None):
    c = CASES[i]
    Q, X, skip, labels, _ = case(i)
    mv = lambda t: None if t is None else t.to(dev)
    return knn(mv(Q), mv(X), c["k"], metric=c["metric"], skip=mv(skip), labels=mv(labels), num_classes=c["C"] or None,
               chunk_rows=c["chunk"] if chunk is None else chunk)


def check_case(i, r):
    c = CASES[i]
    _, _, _, labels, o = case(i)
    check_contract(r.idx.cpu().numpy(), r.dist.cpu().numpy(), None if r.votes is None else r.votes.cpu().numpy(), o, c["k"],
                   None if labels is None else labels.numpy(), c["C"], c["items"])


def run_exact(i, dev="cpu", chunk=None):
    c = EXACT[i]
    Q, X, skip, _ = exact_case(i)
    return knn(Q.to(dev), X.to(dev), c["k"], skip=None if skip is None else skip.to(dev), chunk_rows=c["chunk"] if chunk is None else chunk)


def check_exact(i, r):
    """Bit for bit the oracle: idx, and dist as the fp32 the exact fp64 value is."""
    c = EXACT[i]
    Q, _, skip, o = exact_case(i)
    assert np.array_equal(r.idx.cpu().numpy().astype(np.int64), o["idx"])
    assert np.array_equal(r.dist.cpu().numpy().view(np.uint32), o["dist"].astype(np.float32).view(np.uint32))
    if skip is None:                                                               # the query's own row first, at +0
        assert np.array_equal(r.idx[:, 0].cpu().numpy(), np.arange(c["nq"])) and not r.dist[:, 0].cpu().numpy().view(np.uint32).any()
    else:
        assert not (r.idx.cpu() == torch.arange(c["nq"])[:, None]).any()


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_host_twin_meets_the_contract(i):
    check_case(i, run_case(i))
    c, o = CASES[i], case(i)[4]
    if c["H"] >= 3:                                                                # item 5 is not vacuous
        live = np.arange(c["k"])[None, :] < o["kk"][:, None]
        share = o["closed"][live].mean()
        print("closed positions: %.1f %%" % (100 * share))
        assert share >= 0.9


@pytest.mark.parametrize("i", range(len(EXACT)))
def test_host_twin_is_exact_on_integer_rows(i):
    check_exact(i, run_exact(i))


@pytest.mark.parametrize("i", [3, 6, 7, 9, 14])
def test_oracle_agrees_with_cdist_topk(i):
    c = CASES[i]
    Q, X, skip, _, o = case(i)
    d = torch.cdist(Q.double(), X.double()) ** 2
    if c["metric"] == "cosine":
        qn, xn = Q.double().norm(dim=1, keepdim=True), X.double().norm(dim=1, keepdim=True)
        d = torch.where((qn == 0) | (xn.T == 0), torch.ones_like(d), 1 - (Q.double() @ X.double().T) / (qn * xn.T))
    if skip is not None:
        ok = skip < c["M"]
        d[torch.arange(c["nq"])[ok], skip[ok]] = float("inf")
    kk = min(c["k"], c["M"] - (1 if skip is not None else 0))
    top = d.topk(kk, largest=False)
    closed = o["closed"][:, :kk]
    assert closed.mean() > 0.5
    assert np.array_equal(top.indices.numpy()[closed], o["idx"][:, :kk][closed])
    assert np.allclose(top.values.numpy()[closed], o["dist"][:, :kk][closed], rtol=0, atol=1e-9)


# ---- seeded defects: a float32 model of the operator (chunked selection, merge) with one rule broken at a time ----------------
def model_knn(Q, X, k, metric, skip, labels, C, chunk, defect=None):
    Q, X = Q.numpy(), X.numpy()
    nq, M = len(Q), len(X)
    with np.errstate(all="ignore"):
        qn, xn = (Q * Q).sum(1, dtype=np.float32), np.einsum("ij,ij->i", X, X).astype(np.float32)
        dot = (Q @ X.T).astype(np.float32)
        if metric == "l2":
            d = (qn[:, None] + xn[None, :]) - np.float32(2) * dot
        else:
            d = np.float32(1) - dot / (np.sqrt(qn)[:, None] * np.sqrt(xn)[None, :])
            d = np.where((qn[:, None] == 0) | (xn[None, :] == 0), np.float32(1), d)
    d = np.where(np.isfinite(d), d, np.float32(np.inf)).astype(np.float32)
    if defect != "no_clamp":
        d = np.where(d > 0, d, np.float32(0))
    rows = chunk or 128
    idx = np.full((nq, k), -1, np.int64)
    dist = np.full((nq, k), np.inf, np.float32)
    votes = np.zeros((nq, C), np.int64) if labels is not None else None
    for q in range(nq):
        bits = d[q].view(np.uint32).astype(np.uint64)
        low = np.arange(M, dtype=np.uint64) if defect != "dist_only" else np.uint64(M) - np.arange(M, dtype=np.uint64)
        keys = (bits << np.uint64(32)) | low
        ok = np.ones(M, bool)
        if skip is not None and 0 <= skip[q] < M and defect != "skip_ignored":
            ok[skip[q]] = False
        lists = []
        for j0 in range(0, M, rows):
            js = np.arange(j0, min(M, j0 + rows))[ok[j0:j0 + rows]]
            lists.append(js[np.argsort(keys[js], kind="stable")][:k])
        if defect == "merge_drops_last_chunk" and len(lists) > 1:
            lists.pop()
        js = np.concatenate(lists)
        js = js[np.argsort(keys[js], kind="stable")][:k]
        idx[q, :len(js)], dist[q, :len(js)] = js, d[q, js]
        if labels is not None:
            for j in (idx[q] if defect == "votes_over_k" else js):
                if 0 <= labels[j] < C:
                    votes[q, labels[j]] += 1
    return idx, dist, votes


def _model_passes(defect):
    """The cases (table and exact) the model passes / fails with the defect."""
    failed = []
    for i, c in enumerate(CASES):
        Q, X, skip, labels, o = case(i)
        lab = None if labels is None else labels.numpy()
        got = model_knn(Q, X, c["k"], c["metric"], None if skip is None else skip.numpy(), lab, c["C"], c["chunk"], defect)
        try:
            check_contract(*got, o, c["k"], lab, c["C"], c["items"])
        except AssertionError:
            failed.append(IDS[i])
    for i, c in enumerate(EXACT):
        Q, X, skip, o = exact_case(i)
        idx, dist, _ = model_knn(Q, X, c["k"], "l2", None if skip is None else skip.numpy(), None, 0, c["chunk"], defect)
        if not (np.array_equal(idx, o["idx"]) and np.array_equal(dist.view(np.uint32), o["dist"].astype(np.float32).view(np.uint32))):
            failed.append("exact%d" % i)
    return failed


def test_the_model_itself_passes():
    assert _model_passes(None) == []


@pytest.mark.parametrize("defect", ["dist_only", "skip_ignored", "no_clamp", "merge_drops_last_chunk", "votes_over_k"])
def test_seeded_defects_are_noticed(defect):
    failed = _model_passes(defect)
    print(defect, "->", failed)
    assert failed


# ---- spmotif.context_of ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("node_num", [3, 7, 15])
def test_context_of_reads_the_base(node_num):
    ds = spmotif.generate_dataset(2, node_num=node_num, seed=node_num)
    for value, ctx in enumerate(("tree", "ba")):
        b = Batch.from_data_list([g for s in spmotif.CLASS_LIST for g in ds[ctx][s]])
        keys = set(b.keys()) if callable(getattr(b, "keys", None)) else None
        out = spmotif.context_of(b)
        assert out.dtype == torch.long and out.tolist() == [value] * 8
        assert keys is None or set(b.keys()) == keys                               # nothing added to the batch


def test_context_of_is_unknown_elsewhere():
    b = Batch.from_data_list(synth.tu_like(40, kind="mutag", seed=9))
    assert spmotif.context_of(b).tolist() == [-1] * 40
    b = Batch.from_data_list(spmotif.train_mix(6, seed=1))
    b.y = b.y + 4                                                                  # no class of CLASS_LIST
    assert spmotif.context_of(b).tolist() == [-1] * 6


# ---- errors -----------------------------------------------------------------------------------------------------------------------
def test_errors_and_empty_queries():
    Q, X = torch.rand(3, 8), torch.rand(5, 8)
    for bad in (lambda: knn(Q.double(), X.double(), 2), lambda: knn(Q[0], X, 2), lambda: knn(Q, X[:, :7], 2),
                lambda: knn(Q, X[:0], 2), lambda: knn(Q, X, 0), lambda: knn(Q, X, 2, metric="l1"),
                lambda: knn(Q, X, 2, labels=torch.zeros(5, dtype=torch.long)), lambda: knn(Q, X, 2, chunk_rows=48)):
        with pytest.raises(ValueError):
            bad()
    r = knn(Q[:0], X, 2, labels=torch.zeros(5, dtype=torch.long), num_classes=3)
    assert r.idx.shape == (0, 2) and r.dist.shape == (0, 2) and r.votes.shape == (0, 3)
    r = knn(torch.rand(2, 300), torch.rand(70, 300), 70)                           # the host twin has no limits
    assert r.idx.shape == (2, 70) and (r.idx >= 0).all()


# ---- the Python surface -----------------------------------------------------------------------------------------------------------
def check_surface(m, b, dev):
    """nearest_examples / knn_probe / embedding_bank / eval_disentanglement of a trained model on the batch ``b`` as its own bank."""
    B = int(b.num_graphs)
    bank = embedding_bank(m, [b], dev)
    xc, xo = pooled_representations(m, b)
    assert torch.equal(bank.xc, xc) and torch.equal(bank.xo, xo) and torch.equal(bank.y, b.y.view(-1))
    assert bank.graph.tolist() == list(range(B)) and bank.context is not None
    for space, rows in (("o", xo), ("c", xc)):
        for metric in ("l2", "cosine"):
            o = oracle(rows.cpu().numpy(), rows.cpu().numpy(), 5, metric)
            r = m.nearest_examples(b, bank, k=5, space=space, metric=metric)
            idx = r.idx.cpu().numpy()
            for g in range(B):                                                     # itself first, within the pair's tolerance
                p = int(np.flatnonzero(idx[g] == g)[0])
                assert float(r.dist[g, p]) <= o["tol"][g, g] and (p == 0 or float(r.dist[g, 0]) <= float(r.dist[g, p]))
            assert (idx[o["closed"]] == o["idx"][o["closed"]]).all()
            assert torch.equal(r.y, bank.y[r.idx.long()]) and torch.equal(r.graph, r.idx.long())
            assert torch.equal(r.votes.sum(1), torch.full((B,), 5, dtype=r.votes.dtype, device=r.votes.device))
            ex = nearest_examples(m, b, bank, k=5, space=space, metric=metric, exclude=torch.arange(B, device=rows.device))
            assert not (ex.idx.cpu() == torch.arange(B)[:, None]).any()
            ox = oracle(rows.cpu().numpy(), rows.cpu().numpy(), 5, metric, skip=np.arange(B))
            assert (ex.idx.cpu().numpy()[ox["closed"]] == ox["idx"][ox["closed"]]).all()
    t = m.knn_probe(bank, k=3)
    skip = torch.arange(B, device=xo.device)
    io, ic = (knn(x, x, 3, skip=skip).idx.cpu().tolist() for x in (xo, xc))
    for name, vals in (("y", bank.y.tolist()), ("context", bank.context.tolist())):
        for space, idx in (("o", io), ("c", ic)):
            acc, purity = probe_counts(idx, vals, vals)
            assert t[space][name] == {"acc": acc, "purity": purity}
        assert t["chance"][name] == probe_chance(vals)
    assert abs(t["overlap"] - probe_overlap(io, ic)) < 1e-12 and (t["k"], t["queries"], t["bank"]) == (3, B, B)
    half = EmbeddingBank(bank.xc[:8], bank.xo[:8], bank.y[:8], bank.pred_o[:8], bank.graph[:8], bank.context[:8])
    t2 = knn_probe(bank, queries=half, k=3, targets={"pred": (bank.pred_o, half.pred_o)})      # queries against a bank
    i2 = knn(half.xo, bank.xo, 3).idx.cpu().tolist()
    acc, purity = probe_counts(i2, bank.pred_o.tolist(), half.pred_o.tolist())
    assert t2["o"]["pred"] == {"acc": acc, "purity": purity} and t2["queries"] == 8
    e = eval_disentanglement(m, [b], dev, k=3)
    assert e["graphs"] == B and e["o"] == t["o"] and e["c"] == t["c"]
    return bank


@pytest.mark.parametrize("name,kw", [("CausalGCN", {}), ("CausalGCN", {"cat_or_add": "cat"}), ("CausalGAT", {}), ("CausalGIN", {})],
                         ids=["gcn-add", "gcn-cat", "gat", "gin"])
def test_cpu_surface_and_state(name, kw):
    b = _batch()
    m = train_three_steps(_model(name, **kw), b)
    sd0 = snapshot(m)
    py0, t0 = random.getstate(), torch.get_rng_state()
    check_surface(m, b, "cpu")
    assert m.training and random.getstate() == py0 and torch.equal(torch.get_rng_state(), t0)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd0[k]), k

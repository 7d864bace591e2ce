"""cal_kmeans on the host: the libcalhost twin against the fp64 oracle on the shared case table, on the exact cases and on the
order cases; the oracle tied to brute force and torch; the condition on the table itself; several iterations; seeded defects the
table notices; argument errors; and the Python surface (node_bank, discover_concepts, concept_report) on CPU models against a
plain-Python restatement of every count."""
import random

import numpy as np
import pytest
import torch

from cal_amd import concepts as cc
from cal_amd import spmotif, synth
from cal_amd.concepts import Concepts, NodeBank, assign, concept_report, discover_concepts, eval_concepts, kmeans, node_bank
from cal_amd.data import Batch
from cal_amd.neighbors import knn
from tests.kmeans_oracle import (CASES, EXACT, EXACT_SPANS, IDS, ORDER, case, check_step, default_span, exact_case, mean_of, order_case,
                                 ordered_means, step_oracle)
from tests.knn_oracle import gamma, probe_chance, probe_counts
from tests.test_intervene import _batch, _model, snapshot, train_three_steps


def as_dict(r):
    """A KMeansResult of one step as the numpy dict check_step takes."""
    return dict(centroids=r.centroids.cpu().numpy(), assign=r.assign.cpu().numpy(), counts=r.counts.cpu().numpy(),
                inertia=float(r.inertia[0]), moved=int(r.moved[0]))


def run_case(i, dev="cpu", span=None, iters=1):
    c = CASES[i]
    X, init, _, _ = case(i)
    return kmeans(X.to(dev), c["K"], iters=iters, init=init.to(dev), span_rows=c["span"] if span is None else span)


def check_case(i, r):
    c = CASES[i]
    X, _, C, o = case(i)
    assert int(r.iters_run) == 1
    d = as_dict(r)
    check_step(d, X.numpy(), C.numpy(), o)
    if c["special"] == "twin_centroids":                                           # the second twin stays empty, with its bits
        assert d["counts"][2] == 0 and d["counts"][1] > 0 and np.array_equal(d["centroids"][2].view(np.uint32), C.numpy()[2].view(np.uint32))
    if c["special"] == "identical":
        assert (d["assign"] == 0).all() and d["counts"].tolist() == [c["N"]] + [0] * (c["K"] - 1)
    if c["special"] == "nan":
        assert d["assign"][c["N"] // 3] == -1 and d["counts"].sum() == c["N"] - 1 and np.isfinite(d["centroids"]).all()
    if c["special"] == "k_is_n":
        assert d["assign"].tolist() == list(range(c["N"])) and d["inertia"] <= o["tol"].diagonal().sum()


def same_bits(a, b):
    assert torch.equal(a.assign.cpu(), b.assign.cpu()) and torch.equal(a.counts.cpu(), b.counts.cpu())
    assert torch.equal(a.centroids.cpu().view(torch.int32), b.centroids.cpu().view(torch.int32))
    assert torch.equal(a.inertia.cpu().view(torch.int64), b.inertia.cpu().view(torch.int64))
    assert torch.equal(a.moved.cpu(), b.moved.cpu()) and int(a.iters_run) == int(b.iters_run)


# ---- the table itself --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_the_table_meets_its_condition(i):
    """Outside the tie cases the contract's item 2 leaves out at most 2 % of a case's rows as not closed."""
    c, o = CASES[i], case(i)[3]
    share = 1.0 - o["closed"][o["nearest"] >= 0].mean()
    print("not closed: %.2f %%" % (100 * share))
    assert c["tie"] or share <= 0.02


@pytest.mark.parametrize("i", [1, 3, 5, 11, 16])
def test_oracle_agrees_with_brute_force_and_torch(i):
    X, _, C, o = case(i)
    x, cn = X.numpy().astype(np.float64), C.numpy().astype(np.float64)
    brute = np.array([[((x[j] - cn[k]) ** 2).sum() for k in range(len(cn))] for j in range(len(x))])
    ok = np.isfinite(brute).all(1)
    assert np.allclose(brute[ok], o["d64"][ok], rtol=0, atol=1e-9 * max(1.0, brute[ok].max()))
    assert (o["nearest"][~ok] == -1).all() and np.array_equal(o["nearest"][ok], brute[ok].argmin(1))
    t = torch.cdist(X.double(), C.double()).argmin(1).numpy()
    cl = o["closed"]
    assert cl.mean() > 0.9 and np.array_equal(t[cl], o["nearest"][cl])
    mean, _, counts = mean_of(x, o["nearest"], len(cn))
    s = torch.zeros(len(cn), x.shape[1], dtype=torch.float64).index_add_(0, torch.from_numpy(o["nearest"][ok]), X.double()[torch.from_numpy(ok)])
    assert np.array_equal(counts, np.bincount(o["nearest"][ok], minlength=len(cn)))
    full = counts > 0
    assert np.allclose(s.numpy()[full] / counts[full, None], mean[full], rtol=1e-12, atol=1e-12)


# ---- the host twin -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_host_twin_meets_the_contract(i):
    r = run_case(i)
    check_case(i, r)
    same_bits(r, run_case(i))
    a, d = assign(case(i)[0], case(i)[2])
    assert torch.equal(a, r.assign)                                                # cal_kmeans_assign: the assignment of a step
    live = a >= 0
    assert torch.isposinf(d[~live]).all() and abs(float(d[live].double().sum()) - float(r.inertia[0])) <= 1e-9 * max(1.0, float(r.inertia[0]))


def run_exact(i, span, dev="cpu"):
    X, C, _ = exact_case(i)
    return kmeans(X.to(dev), EXACT[i]["K"], iters=1, init=C.to(dev), span_rows=span)


def check_exact(i, r):
    _, C, want = exact_case(i)
    d = as_dict(r)
    assert np.array_equal(d["assign"], want["assign"]) and np.array_equal(d["counts"], want["counts"])
    assert d["inertia"] == want["inertia"] and d["moved"] == EXACT[i]["N"]
    assert np.array_equal(d["centroids"].view(np.uint32), want["centroids"].view(np.uint32))
    assert d["counts"][1] == 0                                                     # the twin centroid


@pytest.mark.parametrize("span", EXACT_SPANS)
@pytest.mark.parametrize("i", range(len(EXACT)))
def test_host_twin_is_exact_on_integer_rows(i, span):
    check_exact(i, run_exact(i, span))


def run_order(i, dev="cpu"):
    X, C, _, _, _ = order_case(i)
    return kmeans(X.to(dev), ORDER[i]["K"], iters=1, init=C.to(dev), span_rows=ORDER[i]["span"])


def check_order(i, r):
    _, _, lab, want, counts = order_case(i)
    assert np.array_equal(r.assign.cpu().numpy(), lab) and np.array_equal(r.counts.cpu().numpy(), counts)
    assert np.array_equal(r.centroids.cpu().numpy().view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("i", range(len(ORDER)))
def test_host_twin_sums_in_the_order_of_the_rule(i):
    check_order(i, run_order(i))


def test_spans_change_bits_only_within_the_contract():
    """Not promised: the same bits across span_rows.  Promised: the same assignment of a step, centroids within the contract."""
    for i in (4, 11):
        X, _, C, o = case(i)
        rs = [run_case(i, span=s) for s in (0, 128, 256)]
        for r in rs[1:]:
            assert torch.equal(r.assign, rs[0].assign) and torch.equal(r.counts, rs[0].counts)
            check_step(as_dict(r), X.numpy(), C.numpy(), o)


# ---- several iterations ------------------------------------------------------------------------------------------------------------
def planted(N=1500, H=12, K=6, seed=5):
    g = torch.Generator().manual_seed(seed)
    centres = 6.0 * torch.randn(K, H, generator=g)
    lab = torch.randint(0, K, (N,), generator=g)
    lab[:K] = torch.arange(K)
    X = centres[lab] + 0.5 * torch.randn(N, H, generator=g)
    X[N // 2, 1] = float("nan")
    return X, lab, torch.arange(K)                                                 # seeded with one row of each cluster


def check_iterations(dev="cpu", span=0):
    X, lab, init = planted()
    N, H = X.shape
    r = kmeans(X.to(dev), 6, iters=10, init=init.to(dev), span_rows=span)
    run = int(r.iters_run)
    inertia, moved = r.inertia.cpu().numpy(), r.moved.cpu().numpy()
    ok = torch.isfinite(X).all(1)
    xn = (X[ok].double() ** 2).sum(1)
    slack = 2.0 * gamma(H) * float((xn + xn.max()).sum())                          # two steps' pair tolerances, |c|^2 <= max |x|^2
    assert 1 <= run < 10 and (np.diff(inertia[:run]) <= slack).all()
    assert moved[0] == int(ok.sum()) and moved[run - 1] == 0 and (moved[run:] == 0).all() and (inertia[run:] == 0).all()
    assert int(r.counts.sum()) == int(ok.sum())
    a = r.assign.cpu()
    assert torch.equal(a[ok].long(), lab[ok]) and int(a[N // 2]) == -1             # every row in its planted cluster
    again = kmeans(X.to(dev), 6, iters=3, init=r.centroids, span_rows=span)        # a further call moves nothing
    assert int(again.iters_run) == 2 and int(again.moved[1]) == 0 and torch.equal(again.assign, r.assign)
    assert torch.equal(again.centroids.view(torch.int32), r.centroids.view(torch.int32))
    short = kmeans(X.to(dev), 6, iters=run, init=init.to(dev), span_rows=span)     # early exit: the bits of iters = iters_run
    assert torch.equal(short.centroids.view(torch.int32), r.centroids.view(torch.int32)) and torch.equal(short.assign, r.assign)
    assert torch.equal(short.counts, r.counts) and torch.equal(short.inertia, r.inertia[:run]) and torch.equal(short.moved, r.moved[:run])
    return r


@pytest.mark.parametrize("span", [0, 256])
def test_host_iterations_converge_and_stop(span):
    check_iterations(span=span)


def test_restarts_take_the_lowest_inertia_and_the_lower_seed():
    g = torch.Generator().manual_seed(2)
    X = torch.randn(400, 6, generator=g)
    runs = [kmeans(X, 7, iters=8, seed=s) for s in (3, 4, 5, 6)]
    finals = [float(r.inertia[int(r.iters_run) - 1]) for r in runs]
    best = kmeans(X, 7, iters=8, seed=3, restarts=4)
    same_bits(best, runs[int(np.argmin(finals))])
    same_bits(kmeans(torch.ones(20, 2), 2, iters=3, seed=1, restarts=3), kmeans(torch.ones(20, 2), 2, iters=3, seed=1))   # a tie
    r = kmeans(X, 7, iters=2)                                                      # the default start: the seeded rows
    same_bits(r, kmeans(X, 7, iters=2, init=torch.tensor(cc.seed_rows(400, 7, 0))))


# ---- seeded defects: a float32 model of a step with one rule broken at a time ----------------------------------------------------
def model_step(X, C, span, defect=None):
    X, C = np.asarray(X, np.float32), np.asarray(C, np.float32)
    N, K = len(X), len(C)
    with np.errstate(all="ignore"):
        xn, cn = np.einsum("ij,ij->i", X, X).astype(np.float32), np.einsum("ij,ij->i", C, C).astype(np.float32)
        d = (xn[:, None] + cn[None, :]) - np.float32(2) * (X @ C.T).astype(np.float32)
    d = np.where(np.isfinite(d), d, np.float32(np.inf)).astype(np.float32)
    if defect != "no_clamp":
        d = np.where(d > 0, d, np.float32(0))
    low = np.arange(K, dtype=np.uint64) if defect != "tie_high" else np.uint64(K - 1) - np.arange(K, dtype=np.uint64)
    keys = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | low[None, :]
    a = keys.argmin(1)
    dist = d[np.arange(N), a]
    a = np.where(np.isposinf(dist), 0 if defect == "nan_counted" else -1, a)
    span = span or default_span(N)
    Xs = np.where(np.isfinite(X), X, np.float32(1)) if defect == "nan_counted" else X
    if defect == "drop_last_span" and N > span:
        keep = ((N - 1) // span) * span
        cen, _ = ordered_means(Xs[:keep], a[:keep], C, span)
    elif defect == "descending":
        cen, _ = ordered_means(Xs[::-1], a[::-1], C, N)
    else:
        cen, _ = ordered_means(Xs, a, C, span)
    counts = np.bincount(a[a >= 0], minlength=K)
    if defect == "empty_zeroed":
        cen = np.where(counts[:, None] > 0, cen, np.float32(0))
    return dict(centroids=cen, assign=a, counts=counts, inertia=float(dist[a >= 0].astype(np.float64).sum()), moved=int((a >= 0).sum()))


def _model_fails(defect):
    failed = []
    for i, c in enumerate(CASES):
        X, _, C, o = case(i)
        try:
            check_step(model_step(X.numpy(), C.numpy(), c["span"], defect), X.numpy(), C.numpy(), o)
        except AssertionError:
            failed.append(IDS[i])
    for i in range(len(EXACT)):
        X, C, want = exact_case(i)
        for span in EXACT_SPANS:
            got = model_step(X.numpy(), C.numpy(), span, defect)
            if not (np.array_equal(got["assign"], want["assign"]) and np.array_equal(got["counts"], want["counts"])
                    and got["inertia"] == want["inertia"] and np.array_equal(got["centroids"].view(np.uint32), want["centroids"].view(np.uint32))):
                failed.append("exact%d-span%d" % (i, span))
    for i, c in enumerate(ORDER):
        X, C, lab, want, _ = order_case(i)
        got = model_step(X.numpy(), C.numpy(), c["span"], defect)
        if not (np.array_equal(got["assign"], lab) and np.array_equal(got["centroids"].view(np.uint32), want.view(np.uint32))):
            failed.append("order%d" % i)
    return failed


def test_the_model_itself_passes():
    assert _model_fails(None) == []


@pytest.mark.parametrize("defect", ["tie_high", "nan_counted", "empty_zeroed", "drop_last_span", "descending", "no_clamp"])
def test_seeded_defects_are_noticed(defect):
    failed = _model_fails(defect)
    print(defect, "->", failed)
    assert failed


# ---- errors ------------------------------------------------------------------------------------------------------------------------
def test_errors_and_empty_rows():
    X = torch.rand(40, 8)
    C = X[:3].clone()
    bad = [lambda: kmeans(X.double(), 3), lambda: kmeans(X[0], 3), lambda: kmeans(X, 0), lambda: kmeans(X, 3, iters=0),
           lambda: kmeans(X, 3, span_rows=100), lambda: kmeans(X, 3, restarts=0), lambda: kmeans(X, 41),
           lambda: kmeans(X, 3, init=C[:2]), lambda: kmeans(X, 3, init=C[:, :7]), lambda: kmeans(X, 3, init=torch.tensor([0, 1])),
           lambda: kmeans(X, 3, init=torch.tensor([0, 1, 1])), lambda: kmeans(X, 3, init=torch.tensor([0, 1, 40])),
           lambda: kmeans(X, 3, init=C.double()), lambda: kmeans(X, 3, init=C, restarts=2), lambda: kmeans(X[:0], 3),
           lambda: assign(X, C[:, :7]), lambda: assign(X, C[:0]), lambda: assign(X.double(), C.double())]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    r = kmeans(X[:0], 3, iters=4, init=C)                                          # no rows: the centroids stay, nothing runs
    assert int(r.iters_run) == 0 and torch.equal(r.centroids, C) and r.assign.shape == (0,) and r.counts.tolist() == [0, 0, 0]
    a, d = assign(X[:0], C)
    assert a.shape == (0,) and d.shape == (0,)
    r = kmeans(torch.rand(300, 300), 70, iters=2)                                  # the host twin has no limits
    assert r.centroids.shape == (70, 300) and int(r.counts.sum()) == 300


# ---- the Python surface ------------------------------------------------------------------------------------------------------------
def plain_report(bank, asg, centroids, examples, k):
    """concept_report restated with Python lists and loops (knn only for the examples and the completeness neighbours)."""
    K = int(centroids.size(0))
    a, y, g = asg.tolist(), bank.y.tolist(), bank.graph.tolist()
    ctx = bank.context.tolist() if bank.context is not None else None
    gt = bank.node_gt.tolist() if bank.node_gt is not None else None
    att = bank.att.double().tolist()
    first = {}
    for row, gg in enumerate(g):
        first.setdefault(gg, row)
    near = knn(centroids, bank.x, min(examples, len(a)))
    rows = []
    for c in range(K):
        mine = [j for j in range(len(a)) if a[j] == c]
        n = len(mine)
        top = lambda v: max(sum(1 for j in mine if v[j] == u) for u in set(v[j] for j in mine)) / n
        e = [{"row": j, "graph": g[j], "node": j - first[g[j]], "dist": float(dd)}
             for j, dd in zip(near.idx[c].tolist(), near.dist[c].tolist()) if j >= 0]
        rows.append({"size": n, "purity_y": top(y) if n else None, "purity_context": (top(ctx) if n else None) if ctx else None,
                     "motif_share": (sum(gt[j] for j in mine) / n if n else None) if gt else None,
                     "attention": sum(att[j] for j in mine) / n if n else None, "examples": e})
    B = bank.num_graphs
    hist = [[sum(1 for j in range(len(a)) if g[j] == b and a[j] == c) for c in range(K)] for b in range(B)]
    gy = [y[first[b]] for b in range(B)]
    idx = knn(torch.tensor(hist, dtype=torch.float32, device=bank.x.device), torch.tensor(hist, dtype=torch.float32, device=bank.x.device),
              k, skip=torch.arange(B, device=bank.x.device)).idx.cpu().tolist()
    acc, _ = probe_counts(idx, gy, gy)
    motif = [c for c in range(K) if gt and rows[c]["size"] and rows[c]["motif_share"] > 0.5]
    inside = [att[j] for j in range(len(a)) if a[j] in motif]
    outside = [att[j] for j in range(len(a)) if a[j] >= 0 and a[j] not in motif]
    gap = sum(inside) / len(inside) - sum(outside) / len(outside) if inside and outside else None
    return rows, hist, acc, probe_chance(gy), motif, gap, gy


def check_surface(m, b, dev, k=6):
    """node_bank / discover_concepts / assign_concepts / concept_report / eval_concepts of a trained model on the batch ``b``."""
    B, N = int(b.num_graphs), int(b.batch.numel())
    bank = node_bank(m, [b], dev)
    x = m._node_embeddings(b)
    assert torch.equal(bank.x, x) and torch.equal(bank.graph, b.batch) and torch.equal(bank.y, b.y.view(-1)[b.batch])
    assert torch.equal(bank.node_gt, spmotif.ground_truth(b)[0]) and torch.equal(bank.context, spmotif.context_of(b)[b.batch])
    from cal_amd.explain import _eval_mode
    assert bank.num_graphs == B and len(bank) == N and bank.att.shape == (N,) and float(bank.att.min()) >= 0 and float(bank.att.max()) <= 1
    with _eval_mode(m):                                                            # the operator path's causal node attention
        assert torch.equal(bank.att, m._attention_scores(b)[1])
    cut = node_bank(m, [b, b], dev, max_rows=N + 3)                                # a second batch: graph numbers run on
    assert len(cut) == N + 3 and cut.num_graphs == B + 1 and torch.equal(cut.graph[N:], torch.full((3,), B, device=cut.graph.device))
    con = m.discover_concepts([b], dev, k=k, iters=20)
    assert isinstance(con, Concepts) and con.k == k and torch.equal(con.bank.x, bank.x)
    res = con.result
    same = kmeans(bank.x, k, iters=20)
    assert torch.equal(res.centroids, same.centroids) and torch.equal(res.assign, same.assign)
    a2, d2 = m.assign_concepts(b, con)
    ref_a, ref_d = assign(x, res.centroids)
    assert torch.equal(a2, ref_a) and torch.equal(d2, ref_d)
    if int(res.moved[int(res.iters_run) - 1]) == 0:                                # converged: the table places its own rows alike
        assert torch.equal(a2, res.assign)
    rep = m.concept_report(con, examples=3, k=3)
    rows, hist, acc, chance, motif, gap, gy = plain_report(bank, res.assign.cpu(), res.centroids, 3, 3)
    assert (rep["k"], rep["rows"], rep["graphs"], rep["queries"]) == (k, N, B, B)
    for c in range(k):
        got, want = rep["concepts"][c], rows[c]
        assert got["size"] == want["size"] == int(res.counts[c])
        for key in ("purity_y", "purity_context", "motif_share"):
            assert (np.isnan(got[key]) if want[key] is None else got[key] == want[key]), (c, key)
        assert np.isnan(got["attention"]) if want["attention"] is None else abs(got["attention"] - want["attention"]) < 1e-9
        assert got["examples"] == want["examples"] and len(got["examples"]) == 3
    assert rep["completeness"] == acc and rep["chance"] == chance and rep["motif_concepts"] == motif
    assert (np.isnan(rep["attention_gap"]) if gap is None else abs(rep["attention_gap"] - gap) < 1e-9)
    assert torch.equal(cc._histograms(res.assign, bank.graph, B, k).cpu(), torch.tensor(hist))
    e = eval_concepts(m, [b], dev, k=k, examples=3, knn_k=3, iters=20)
    assert e == rep or all(e[key] == rep[key] for key in ("completeness", "chance", "motif_concepts", "graphs"))
    t = eval_concepts(m, [b], dev, k=k, test_loader=[b], knn_k=1, iters=20)        # queries against the table: nothing skipped
    hf = torch.tensor(hist, dtype=torch.float32, device=bank.x.device)
    qf = cc._histograms(assign(bank.x, res.centroids)[0], bank.graph, B, k).float()    # the queries are placed by the final centroids
    assert t["completeness"] == probe_counts(knn(qf, hf, 1).idx.cpu().tolist(), gy, gy)[0] and t["queries"] == B
    return con


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


def test_banks_without_ground_truth():
    b = Batch.from_data_list(synth.tu_like(12, kind="mutag", seed=9))
    torch.manual_seed(0)
    from cal_amd import model as M
    from tests.test_intervene import _args
    m = M.CausalGCN(int(b.x.size(1)), 2, _args())
    bank = node_bank(m, [b], "cpu")
    assert bank.node_gt is None and bank.context is None
    rep = concept_report(Concepts(kmeans(bank.x, 3, iters=5), bank), examples=2)
    assert rep["motif_concepts"] is None and rep["attention_gap"] is None
    assert all(r["motif_share"] is None and r["purity_context"] is None for r in rep["concepts"])
    assert sum(r["size"] for r in rep["concepts"]) == len(bank)

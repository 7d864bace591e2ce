"""Soft edge masks and gradient attributions on the CPU: the oracle restatement (tests/softmask_oracle.py) tied to
``oracle.cal_oracle`` at the corners of the mask cube, the host twins of ``cal_edge_dot`` / ``cal_gat_mask_fwd`` / ``_bwd``
against oracle autograd, and ``masked_log_probs`` / ``saliency`` / ``integrated_gradients`` of CPU-resident models against the
oracle's, with the identities of the scores, the binary masks against ``coalition_batch``'s replicas, the state a call leaves
behind and the argument errors.

Gradient tolerance (``softmask_oracle.SCORE_ATOL``, rtol 1e-3): measured, not guessed -- the fp32 host path against the fp64
oracle over every model-level case below (3 graphs, 17 nodes, 44 columns, H 32, L 2; saliency and 4-step integrated gradients
over edges, undirected pairs, nodes, a subset of the edges and the ``co`` head):

    max |score - oracle|   CausalGCN 1.78e-8   CausalGAT 8.68e-9   CausalGIN 5.91e-8
    max |score| per case   6.0e-3 .. 8.1e-2    2.2e-3 .. 3.6e-2    1.4e-2 .. 2.6e-1
    smallest ReLU |pre|    1.48e-4             1.54e-4             1.20e-4

atol = 4 x the first row per model (the GPU sums in another order than the host).  ``test_the_gradient_checks_are_not_vacuous``
holds the oracle alone to max |score| >= 100 atol and to a smallest ReLU |pre-activation| >= 1e-4 over every differentiated
forward; the seeds of ``softmask_oracle.MODEL_SEED`` were searched on the CPU so that both hold.
"""
import random
import subprocess

import pytest
import torch

from cal_amd import _lib, ops, spmotif
from cal_amd.coalition import coalition_batch, perturbation_curve
from cal_amd.data import Batch
from cal_amd.explain import edge_twins
from cal_amd.gradient import Gradients, gradient_agreement, integrated_gradients, masked_log_probs, saliency
from cal_amd.plan import GraphPlan, _c
from oracle import cal_oracle as O
from tests import softmask_oracle as SO

SYMBOLS = ("cal_edge_dot", "cal_gat_mask_fwd", "cal_gat_mask_bwd_ws", "cal_gat_mask_bwd")
LOGIT_TOL = 1e-4          # operator-level path against the oracle, on a logit (tests/test_host_lib.py)


def test_abi_symbols_are_exported_by_both_libraries():
    protos = _lib.parse_header()
    for path in (_lib.LIB_PATH, _lib.HOST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
        assert set(SYMBOLS) <= exported, path
    assert set(SYMBOLS) <= set(protos) and set(SYMBOLS) <= set(_lib.HOST_SYMBOLS)
    assert len(protos["cal_edge_dot"][1]) == 9 and len(protos["cal_gat_mask_fwd"][1]) == 19 and len(protos["cal_gat_mask_bwd"][1]) == 23


# ---- the oracle restatement at the corners of the cube --------------------------------------------------------------------------
@pytest.mark.parametrize("name", SO.MODELS)
def test_oracle_ties_to_the_causal_forward(name):
    """On six fixture graphs (352 nodes) with one self-loop column added: m = 1 is ``causal_forward(training=False)``, a binary
    edge mask the forward on the graph without those columns, a binary node mask the forward on the graph without those nodes."""
    from tests.helpers import ref_batch
    data = ref_batch([0, 4, 7, 12, 16, 20])
    x, batch, B = data.feat.double(), data.batch, data.num_graphs
    ei = torch.cat([torch.tensor([[3], [3]]), data.edge_index], 1)
    sd = {k: v.double() for k, v in SO.model_state(name, x.size(1)).items()}
    E, N = ei.size(1), x.size(0)
    full = O.causal_forward(name, sd, x, ei, batch, layers=2, heads=4, num_graphs=B)
    for kw in (dict(edge_mask=torch.ones(E, dtype=torch.float64)), dict(node_mask=torch.ones(N, dtype=torch.float64)), {}):
        got = SO.masked_forward(name, sd, x, ei, batch, B, **kw)
        assert max((a - b).abs().max().item() for a, b in zip(got, full)) <= 1e-12
    g = torch.Generator().manual_seed(4)
    keep = torch.rand(E, generator=g) < 0.6
    got = SO.masked_forward(name, sd, x, ei, batch, B, edge_mask=keep.double())
    want = O.causal_forward(name, sd, x, ei[:, keep], batch, layers=2, heads=4, num_graphs=B)
    assert max((a - b).abs().max().item() for a, b in zip(got, want)) <= 1e-12
    nk = torch.rand(N, generator=g) < 0.7
    got = SO.masked_forward(name, sd, x, ei, batch, B, node_mask=nk.double())
    xr, eir, br = SO.remove_nodes(x, ei, batch, nk)
    want = O.causal_forward(name, sd, xr, eir, br, layers=2, heads=4, num_graphs=B)
    assert max((a - b).abs().max().item() for a, b in zip(got, want)) <= 1e-12


# ---- host twins against oracle autograd -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", SO.EDGE_DOT_H)
def test_host_edge_dot(H):
    ei, n, facts, a, b, want = SO.edge_dot_case(H)
    plan = GraphPlan(ei, n)
    deg = plan.rowptr_dst[1:] - plan.rowptr_dst[:-1]
    assert int(deg[facts["hub"]]) >= 70 and int(deg[facts["isolated"]]) == 0
    assert int(((ei[0] == 1) & (ei[1] == 0)).sum()) == 2                  # a duplicated column
    out = torch.full((plan.E,), 7.0)
    _c("cal_edge_dot", plan.row32, plan.col32, a, b, out, n, plan.E, H)
    assert torch.allclose(out.double(), want, **SO.TOL_DW) and out[facts["loop"]].item() == 0.0
    # through the operator: GINConv's weighted sum, its dx and dw
    g = torch.Generator().manual_seed(9)
    w = torch.rand(plan.E, generator=g).requires_grad_(True)
    x = b.clone().requires_grad_(True)
    res = ops.gin_aggregate(x, plan, 0.25, edge_weight=w)
    res.backward(a)
    ro, rx, rw = SO.gin_weight_grad_oracle(b, ei, w.detach(), a, 0.25)
    assert torch.allclose(res.detach().double(), ro, **SO.TOL_OUT) and torch.allclose(x.grad.double(), rx, **SO.TOL_DZ)
    assert torch.allclose(w.grad.double(), rw, **SO.TOL_DW) and w.grad[facts["loop"]].item() == 0.0
    assert torch.equal(ops.gin_aggregate(b, plan, 0.25, edge_weight=torch.ones(plan.E)), ops.gin_aggregate(b, plan, 0.25))


def test_host_edge_dot_without_columns():
    plan = GraphPlan(torch.zeros(2, 0, dtype=torch.long), 4)
    x = torch.randn(4, 8).requires_grad_(True)
    w = torch.zeros(0, requires_grad=True)
    out = ops.gin_aggregate(x, plan, 0.0, edge_weight=w)
    out.sum().backward()
    assert torch.equal(out.detach(), x.detach()) and w.grad.shape == (0,) and torch.equal(x.grad, torch.ones(4, 8))
    _c("cal_edge_dot", plan.row32, plan.col32, x.detach(), x.detach(), torch.zeros(4), 4, 0, 8)


@pytest.mark.parametrize("K,D", SO.GAT_SHAPES)
def test_host_gat_mask(K, D):
    c = SO.gat_case(K, D)
    ei, n, facts = c["ei"], c["N"], c["facts"]
    plan = GraphPlan(ei, n)
    deg = plan.rowptr_dst[1:] - plan.rowptr_dst[:-1]
    assert int(deg[facts["hub"]]) >= 130 and int(deg[facts["isolated"]]) == 0 and int(deg[facts["dark"]]) == 3
    assert bool((c["m"][ei[1] == facts["dark"]] == 0).all()) and {0.0, 1.0} < set(c["m"].tolist())
    z, m = c["z"].clone().requires_grad_(True), c["m"].clone().requires_grad_(True)
    out = ops.gat_aggregate(z, c["att"], c["bias"], plan, K, relu=c["relu"], edge_mask=m)
    out.backward(c["gout"])
    assert torch.allclose(out.detach().double(), c["out"], **SO.TOL_OUT)
    assert torch.allclose(z.grad.double(), c["dz"], **SO.TOL_DZ)
    assert torch.allclose(m.grad.double(), c["dm"], **SO.TOL_DW) and m.grad[facts["loop"]].item() == 0.0
    # m = 1 is the GATConv as it is
    one = ops.gat_aggregate(c["z"], c["att"], c["bias"], plan, K, relu=True, edge_mask=torch.ones(plan.E))
    assert torch.allclose(one, ops.gat_aggregate(c["z"], c["att"], c["bias"], plan, K, relu=True), atol=1e-6, rtol=1e-6)
    # frozen parameters: a backward that would need d att raises
    att = c["att"].clone().requires_grad_(True)
    with pytest.raises(RuntimeError):
        ops.gat_aggregate(c["z"], att, c["bias"], plan, K, edge_mask=c["m"]).sum().backward()


# ---- model level ----------------------------------------------------------------------------------------------------------------
_MODELS = {}


def _model(name):
    if name not in _MODELS:
        data = SO.model_batch()
        sd = SO.model_state(name, data.feat.size(1))
        _MODELS[name] = (SO.build_model(name, sd, data.feat.size(1)), {k: v.double() for k, v in sd.items()}, data)
    return _MODELS[name]


def _err(got, want):
    got, want = got.cpu().double(), want.cpu().double()
    assert torch.equal(got.isnan(), want.isnan())
    ok = ~want.isnan()
    return (got - want)[ok].abs().max().item() if bool(ok.any()) else 0.0


def _close(got, want, name):
    got, want = got.cpu().double(), want.cpu().double()
    assert torch.equal(got.isnan(), want.isnan())
    ok = ~want.isnan()
    return torch.allclose(got[ok], want[ok], atol=SO.SCORE_ATOL[name], rtol=SO.SCORE_RTOL)


@pytest.mark.parametrize("name", SO.MODELS)
def test_masked_log_probs_match_the_oracle(name):
    m, sd, data = _model(name)
    E, N = data.edge_index.size(1), data.feat.size(0)
    g = torch.Generator().manual_seed(1)
    em, nm = torch.rand(E, generator=g), torch.rand(N, generator=g)
    em[::3], nm[::4] = 0.0, 0.0
    x = data.feat.double()
    for kw in (dict(edge_mask=em), dict(node_mask=nm), dict(edge_mask=em, node_mask=nm), {}):
        got = masked_log_probs(m, data, **kw)
        want = SO.masked_forward(name, sd, x, data.edge_index, data.batch, data.num_graphs, **{k: v.double() for k, v in kw.items()})
        err = max((a.double() - b).abs().max().item() for a, b in zip(got, want))
        print("%s %s: max |log p - oracle| = %.3g" % (name, sorted(kw), err))
        assert err < LOGIT_TOL
    with torch.no_grad():                                                 # the caller's grad mode does not matter
        em.requires_grad_(True)
        lp = masked_log_probs(m, data, edge_mask=em)[1]
    assert lp.requires_grad and torch.autograd.grad(lp.exp().sum(), em)[0].shape == (E,)


@pytest.mark.parametrize("case", SO.SCORE_CASES, ids=lambda c: "-".join(str(v) for v in c))
@pytest.mark.parametrize("name", SO.MODELS)
def test_scores_match_the_oracle(name, case):
    use, undirected, subset, head = case
    m, sd, data = _model(name)
    M = data.edge_index.size(1) if use == "edges" else data.feat.size(0)
    el = SO.subset_of(M) if subset else None
    for steps in (None, 4):
        want, _ = SO.oracle_scores(name, case, steps)
        if steps is None:
            got = m.saliency(data, use=use, undirected=undirected, head=head, elements=el)
            assert got.method == "saliency" and got.forwards == 1 and got.gap is None and got.p_baseline is None
        else:
            got = m.integrated_gradients(data, use=use, undirected=undirected, head=head, elements=el, steps=steps)
            assert got.method == "ig" and got.forwards == steps + 2 and got.steps == steps
            assert _err(got.p_baseline, want["p_baseline"]) < LOGIT_TOL and _err(got.gap, want["gap"]) < 4 * LOGIT_TOL
        assert isinstance(got, Gradients) and got.score.dtype == torch.float64 and got.score.shape == (M,)
        assert torch.equal(got.yhat, want["yhat"]) and _err(got.p_full, want["p_full"]) < LOGIT_TOL
        print("%s %s steps=%s: max |score - oracle| = %.3g (max |score| %.3g, atol %.3g)"
              % (name, case, steps, _err(got.score, want["score"]), want["score"].nan_to_num(0).abs().max().item(), SO.SCORE_ATOL[name]))
        assert _close(got.score, want["score"], name)


def test_the_gradient_checks_are_not_vacuous():
    """On the oracle alone: the scores are far above the tolerance, and no ReLU of a differentiated forward sits close enough to
    its kink for an fp32 sign flip to change a gradient."""
    for name in SO.MODELS:
        for case in SO.SCORE_CASES:
            for steps in (None, 4):
                want, min_pre = SO.oracle_scores(name, case, steps)
                assert want["score"].nan_to_num(0).abs().max().item() >= 100 * SO.SCORE_ATOL[name], (name, case, steps)
                assert min_pre >= 1e-4, (name, case, steps, min_pre)


@pytest.mark.parametrize("name", SO.MODELS)
def test_identities_of_the_scores(name):
    m, _, data = _model(name)
    E = data.edge_index.size(1)
    twin = edge_twins(data)[0]
    gid = data.batch[data.edge_index[0]]
    el = SO.subset_of(E)
    one = integrated_gradients(m, data, steps=3)
    pair = integrated_gradients(m, data, steps=3, undirected="mean")
    part = integrated_gradients(m, data, steps=3, elements=el)
    assert one.score[0].item() == 0.0 and pair.score[0].item() == 0.0 and saliency(m, data).score[0].item() == 0.0   # the self loop
    assert torch.equal(pair.twin, twin) and one.twin is None
    # gap = sum of the players' scores - (p_full - p_baseline), per graph
    idx = torch.arange(E)
    paired = (twin >= 0) & (twin != idx)
    rep = ~(paired & (twin < idx))
    for res, r in ((one, torch.ones(E, dtype=torch.bool)), (pair, rep), (part, el)):
        sums = torch.zeros(data.num_graphs, dtype=torch.float64).index_add_(0, gid[r], res.score[r])
        assert (res.gap - (sums - (res.p_full.double() - res.p_baseline.double()))).abs().max().item() <= 2.0 ** -40
    # a pair's score is the sum of its two columns' directed scores; both columns carry it
    t = twin.clamp(min=0).long()
    want = torch.where(paired, one.score + one.score[t], one.score)
    assert (pair.score - want).abs().max().item() <= 2.0 ** -40 and torch.equal(pair.score[paired], pair.score[t[paired]])
    # non-players score NaN, players do not (a subset walks another path, so only the pattern is exact)
    assert torch.equal(part.score.isnan(), ~el) and not bool(one.score.isnan().any())
    # the same call twice: identical bits
    again = integrated_gradients(m, data, steps=3, undirected="mean")
    assert torch.equal(again.score, pair.score) and torch.equal(again.gap, pair.gap) and torch.equal(again.p_baseline, pair.p_baseline)


@pytest.mark.parametrize("name", SO.MODELS)
@pytest.mark.parametrize("use", ["edges", "nodes"])
def test_binary_masks_are_coalition_replicas(name, use):
    b = Batch.from_data_list(spmotif.train_mix(3, node_num=6, seed=4))
    feat = (b.x if b.x is not None else b.feat).size(1)
    m = SO.build_model(name, SO.model_state(name, feat), feat).eval()
    M = b.edge_index.size(1) if use == "edges" else b.batch.numel()
    gid = b.batch[b.edge_index[0]] if use == "edges" else b.batch
    key = torch.randint(0, 10, (M,), generator=torch.Generator().manual_seed(6), dtype=torch.int32)
    rg, rth = torch.tensor([0, 1, 2, 1, 0]), torch.tensor([5, 3, 8, 10, 1])
    reps = coalition_batch(b, rg, rth, key, use=use)
    assert reps.empty_graphs == 0
    with torch.no_grad():
        want = m(reps, eval_random=False)
    for r in range(rg.numel()):
        mask = torch.where((gid == rg[r]) & (key >= rth[r]), 0.0, 1.0)
        got = masked_log_probs(m, b, **{"edge_mask" if use == "edges" else "node_mask": mask})
        for h in range(3):
            assert (got[h][rg[r]].exp() - want[h][r].exp()).abs().max().item() < LOGIT_TOL, (r, h)


def test_a_call_leaves_the_model_as_it_was():
    m, _, data = _model("CausalGAT")
    m.train()
    for p in m.parameters():
        p.grad = None
    m.convs[0].weight.grad = torch.full_like(m.convs[0].weight, 3.0)
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    req0 = [p.requires_grad for p in m.parameters()]
    py0, t0 = random.getstate(), torch.get_rng_state()
    calls0 = m.convs[0]._calls
    saliency(m, data, use="nodes")
    integrated_gradients(m, data, steps=2, undirected="mean")
    masked_log_probs(m, data, edge_mask=torch.ones(data.edge_index.size(1)))
    gradient_agreement(m, data, steps=2, ratio=0.3)
    assert m.training and random.getstate() == py0 and torch.equal(torch.get_rng_state(), t0) and m.convs[0]._calls == calls0
    assert [p.requires_grad for p in m.parameters()] == req0
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd0[k]), k
    for n, p in m.named_parameters():
        assert p.grad is None or (n == "convs.0.weight" and bool((p.grad == 3.0).all())), n
    m.eval()
    # a GAT mask does not go through attention dropout
    m.train()
    with pytest.raises(ValueError):
        m._masked_forward(data, edge_mask=torch.ones(data.edge_index.size(1)))
    m.eval()


def test_argument_errors():
    m, _, data = _model("CausalGCN")
    E, N = data.edge_index.size(1), data.feat.size(0)
    with pytest.raises(ValueError):
        masked_log_probs(m, data, edge_mask=torch.ones(E - 1))
    with pytest.raises(ValueError):
        masked_log_probs(m, data, node_mask=torch.ones(N + 1))
    with pytest.raises(TypeError):
        masked_log_probs(m, data, edge_mask=torch.ones(E, dtype=torch.float64))
    with pytest.raises(TypeError):
        masked_log_probs(m, data, node_mask=torch.ones(N, dtype=torch.bool))
    with pytest.raises(ValueError):
        masked_log_probs(m, data, edge_mask=torch.ones(E, device="meta"))
    for fn in (saliency, integrated_gradients):
        with pytest.raises(ValueError):
            fn(m, data, use="graphs")
        with pytest.raises(ValueError):
            fn(m, data, head="x")
        with pytest.raises(ValueError):
            fn(m, data, use="nodes", undirected="mean")
        with pytest.raises(ValueError):
            fn(m, data, undirected="median")
        with pytest.raises(ValueError):
            fn(m, data, elements=torch.ones(E + 1, dtype=torch.bool))
        with pytest.raises(TypeError):
            fn(m, data, elements=torch.ones(E))
    with pytest.raises(ValueError):
        integrated_gradients(m, data, steps=0)
    with pytest.raises(TypeError):
        integrated_gradients(m, data, steps=2.5)
    with pytest.raises(ValueError):
        gradient_agreement(m, data, method="shap", ratio=0.3)
    with pytest.raises(ValueError):
        gradient_agreement(m, data, steps=0, ratio=0.3)


def test_agreement_and_curves_take_the_scores():
    m, _, _ = _model("CausalGCN")
    from cal_amd.occlude import rank_agreement
    from tests.helpers import ref_batch
    b = ref_batch([0, 4, 7])
    ig = m.integrated_gradients(b, steps=2, undirected="mean")
    res = perturbation_curve(m, b, undirected="mean", ratios=(0.0, 0.5, 1.0), order=ig.score)
    assert bool(torch.isfinite(res["auc_insertion"]).all()) and bool(torch.isfinite(res["auc_deletion"]).all())
    for method, ref in (("ig", ig), ("saliency", m.saliency(b, undirected="mean"))):
        out = gradient_agreement(m, b, method=method, steps=2, undirected="mean", ratio=0.3)
        from cal_amd.explain import explain
        causal = explain(m, b, ratio=0.3, undirected="mean").edge_score
        twin = edge_twins(b)[0]
        sel = ~((twin >= 0) & (twin < torch.arange(twin.numel())))
        counts, met = rank_agreement(causal, ref.score.float(), b.edge_ptr, b.max_edges, sel=sel, ratio=0.3)
        for j, key in enumerate(("rho", "tau", "jaccard")):
            ok = ~met[:, j].isnan()
            assert out[key + "_undefined"] == int((~ok).sum())
            assert abs(out[key] - met[ok, j].mean().item()) < 1e-12 if bool(ok.any()) else out[key] != out[key]
        assert out["graphs"] == b.num_graphs and out["elements"] == int(counts[:, 0].sum()) and out["forwards"] == ref.forwards + 1

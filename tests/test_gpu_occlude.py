"""Occlusion attributions on the MI355X: the HIP replica builder (cal_occlude_count / cal_occlude_write) against the plain-torch
restatement and the host twin bit for bit (the CPU case list; the sizes beyond it: tests/test_gpu_restrict.py), against the composition of splice_batches and extract_subgraph, the HIP
rank-agreement kernel against the numpy counts and the host twin, the replica batch on the engine's per-graph route, occlusion()
against the fp64 oracle, the exact zeros of control replicas on a deterministic engine, and faithfulness() /
eval_faithfulness() recomputed from the engine's own scores, leaving the engine's state untouched."""
import argparse
import random

import pytest
import torch

from cal_amd import _lib, spmotif
from cal_amd.data import Batch, DataLoader
from cal_amd.explain import _Layout, _log_probs, _untiled, edge_twins, explain, extract_subgraph
from cal_amd.occlude import eval_faithfulness, faithfulness, occlude_batch, occlusion, rank_agreement
from cal_amd.splice import splice_batches
from oracle import cal_oracle as O
from tests.occlude_oracle import (AGREE_SPECS, agreement_inputs, check_agreement, check_faith, check_occlude, faith_from_scores,
                                  occlude_cases, occlusion_oracle)

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOGIT_TOL = 1e-4                   # tests/test_gpu_engine.py: the engine's logits against the oracle at these shapes
CASES = occlude_cases()
SEEDS = {"CausalGCN": 2, "CausalGAT": 1, "CausalGIN": 1}                  # tests/test_gpu_splice.py
SHAPES = [("CausalGCN", 128), ("CausalGAT", 64), ("CausalGIN", 64)]


def _dev(b):
    """A device copy of a CPU batch (the case list is shared between tests)."""
    d = Batch()
    for k, v in b.__dict__.items():
        d.__dict__[k] = v.to(DEV) if torch.is_tensor(v) else v
    d._plan = None
    return d


def _m(t):
    return t.to(DEV) if torch.is_tensor(t) else t


def _same(u, v):
    for key in ("edge_index", "ptr", "edge_ptr", "batch", "node_src", "edge_src"):
        assert torch.equal(getattr(u, key).cpu(), getattr(v, key).cpu()), key
    assert (u.max_nodes, u.max_edges, u.empty_graphs) == (v.max_nodes, v.max_edges, v.empty_graphs)


@pytest.mark.parametrize("name", sorted(CASES))
def test_hip_equals_restatement_and_host_twin(name):
    b, rg, re, use, twin = CASES[name]
    res = occlude_batch(_dev(b), _m(rg), _m(re), use=use, twin=_m(twin))
    assert res.edge_index.is_cuda and res.ptr.is_cuda and res.node_src.is_cuda
    check_occlude(res, b, rg, re, use, twin)
    _same(res, occlude_batch(b, rg, re, use=use, twin=twin))


@pytest.mark.parametrize("name", ["spmotif_edges", "spmotif_nodes"])
def test_hip_equals_the_composition_of_splice_and_extract(name):
    b, rg, re, use, twin = CASES[name]
    bd, rg, re = _dev(b), rg.to(DEV), re.to(DEV)
    res = occlude_batch(bd, rg, re, use=use, twin=_m(twin))
    rep = splice_batches(bd, bd, rg, torch.full_like(rg, -1))
    if use == "edges":
        src = rep.edge_src                                                # the source column of every replicated column
        gone = re[torch.repeat_interleave(torch.arange(rg.numel(), device=DEV), rep.edge_ptr[1:] - rep.edge_ptr[:-1])]
        tw = twin.to(DEV).long()[gone.clamp(min=0)]
        comp = extract_subgraph(rep, edge_mask=(src != gone) & ((gone < 0) | (src != tw)))
    else:
        gone = re[rep.batch]
        comp = extract_subgraph(rep, node_mask=rep.node_src != gone, relabel=True)
    for key in ("edge_index", "ptr", "edge_ptr", "batch"):
        assert torch.equal(getattr(res, key), getattr(comp, key)), key
    assert torch.equal(res.feat if res.x is None else res.x, comp.feat if comp.x is None else comp.x)
    assert (res.max_nodes, res.max_edges) == (comp.max_nodes, comp.max_edges)


def test_hip_rank_agreement_equals_the_numpy_counts_and_the_host_twin():
    a, b, seg = check_agreement(DEV)                                       # (2049 and 5000 take the tiled path)
    sel = agreement_inputs()[3]
    for mx, use_sel, kw in AGREE_SPECS:
        s = sel if use_sel else None
        dev = rank_agreement(a.to(DEV), b.to(DEV), seg.to(DEV), mx, sel=_m(s), **kw)
        host = rank_agreement(a, b, seg, mx, sel=s, **kw)
        assert torch.equal(dev[0].cpu(), host[0]) and torch.equal(dev[1].cpu().isnan(), host[1].isnan())
        assert torch.equal(dev[1].cpu().nan_to_num(), host[1].nan_to_num())
    counts, met = rank_agreement(a[:0].to(DEV), b[:0].to(DEV), torch.tensor([0], device=DEV), 0, k=1)
    assert counts.shape == (0, 10) and met.shape == (0, 3)


def _args(**kw):
    d = dict(layers=3, hidden=128, with_random=True, without_node_attention=False, without_edge_attention=False,
             fc_num="222", cat_or_add="add", c=0.5, o=1.0, co=0.5)
    d.update(kw)
    return argparse.Namespace(**d)


def _gpu_model(name, args=None, seed=None, deterministic=False):
    from cal_amd import model as M
    from cal_amd.engine import StepEngine
    args = args or _args()
    torch.manual_seed(SEEDS[name] if seed is None else seed)
    sd = O.init_state(name, 10, 4, hidden=args.hidden, layers=args.layers, heads=4, cat_or_add=args.cat_or_add)
    m = getattr(M, name)(10, 4, args)
    m.load_state_dict(sd, strict=name != "CausalGIN")
    m = m.to(DEV)
    if deterministic:
        object.__setattr__(m, "_engine", StepEngine(m, deterministic=True))
    return m, sd


def _stage_names():
    h = _lib.lib()
    names, k = [], 1
    while True:
        nm = h.cal_engine_stage_name(k)
        nm = nm.decode() if isinstance(nm, bytes) else nm
        if not nm:
            return names
        names.append(nm)
        k += 1


@pytest.mark.parametrize("use", ["edges", "nodes"])
def test_replica_batch_takes_the_per_graph_route(use):
    m, _ = _gpu_model("CausalGCN")
    b = Batch.from_data_list(spmotif.train_mix(16, node_num=7, seed=11)).to(DEV)
    off = b.edge_ptr if use == "edges" else b.ptr
    re = torch.arange(0, int(off[-1]), 3, device=DEV)[:512]
    rg = torch.searchsorted(off, re, right=True) - 1
    rep = occlude_batch(b, rg, re, use=use, twin=edge_twins(b)[0] if use == "edges" else None)
    assert rep.ptr.is_cuda and rep.edge_ptr.is_cuda and rep.max_nodes > 0 and rep.no_self_loops and rep.empty_graphs == 0
    eng = m.engine()
    eng.forward(rep, None, training=False)
    names = _stage_names()
    assert "k_plan_graph" in names and "k_plan_count" not in names, names
    eng.check_status()


@pytest.mark.parametrize("use,undirected", [("edges", None), ("edges", "mean"), ("nodes", None)])
@pytest.mark.parametrize("name,hidden", SHAPES)
def test_occlusion_matches_the_oracle(name, hidden, use, undirected):
    """The engine's log-probabilities are held to LOGIT_TOL of the oracle at these shapes; p <= 1, so each probability is within
    1.0001e-4 and a score, the difference of two, within 2.1 LOGIT_TOL.  The argmax is the engine's, handed to the oracle."""
    m, sd = _gpu_model(name, _args(hidden=hidden))
    b = Batch.from_data_list(spmotif.train_mix(6, node_num=7, seed=11))
    bd = _dev(b)
    occ = occlusion(m, bd, use=use, undirected=undirected, chunk=100)
    m.engine().check_status()
    twin = edge_twins(b)[0] if undirected else None
    M = b.edge_index.size(1) if use == "edges" else b.batch.numel()
    n = int((~((twin >= 0) & (twin < torch.arange(M)))).sum()) if undirected else M
    assert occ.replicas == n and occ.forwards == 1 + -(-n // 100) and occ.forwards >= 3 and n % 100 != 0
    assert (occ.twin is None) == (twin is None) and (twin is None or torch.equal(occ.twin.cpu(), twin))
    want = occlusion_oracle(name, sd, b, occ.yhat, use, twin, layers=3, heads=4)
    got = occ.score.cpu().double()
    assert not bool(want.isnan().any()) and not bool(got.isnan().any())
    err = (got - want).abs().max().item()
    print("%s %s undirected=%s: %d replicas, max |score - oracle| = %.3g (largest |score| %.3g)"
          % (name, use, undirected, n, err, want.abs().max().item()))
    assert err < 2.1 * LOGIT_TOL, err


@pytest.mark.parametrize("name,hidden", SHAPES)
def test_control_replicas_with_a_deterministic_engine(name, hidden):
    m, _ = _gpu_model(name, _args(hidden=hidden), deterministic=True)
    b = Batch.from_data_list(spmotif.train_mix(16, node_num=7, seed=11)).to(DEV)
    B = b.num_graphs
    ctl = occlude_batch(b, torch.arange(B, device=DEV), torch.full((B,), -1, device=DEV))
    for key in ("edge_index", "ptr", "edge_ptr", "batch", "y"):
        assert torch.equal(getattr(ctl, key), getattr(b, key)), key
    assert torch.equal(ctl.feat if ctl.x is None else ctl.x, b.feat if b.x is None else b.x)
    assert (ctl.max_nodes, ctl.max_edges) == (b.max_nodes, b.max_edges)
    m.eval()
    with torch.no_grad():
        full = _log_probs(m, _untiled(b, _Layout(b)))
        again = _log_probs(m, ctl)
    assert torch.equal(full, again)                                       # so those scores are exactly 0
    m.engine().check_status()


def test_faithfulness_from_the_engines_own_scores_and_untouched_state():
    from cal_amd.engine import StepEngine
    args = _args(layers=2, hidden=64)
    m, _ = _gpu_model("CausalGCN", args, seed=0)
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
    for use, undirected in (("edges", "mean"), ("nodes", None)):
        res = eval_faithfulness(m, DataLoader(gs, batch_size=4, shuffle=False), DEV, use=use, undirected=undirected, ratio=0.3)
        parts, singles = [], []
        for i in range(0, 12, 4):
            b = Batch.from_data_list(gs[i:i + 4]).to(DEV)
            singles.append(m.faithfulness(b, use=use, undirected=undirected, ratio=0.3))
            occ = m.occlusion(b, use=use, undirected=undirected)
            ex = explain(m, b, ratio=0.3, undirected=undirected)
            causal, top = (ex.edge_score, ex.edge_mask) if use == "edges" else (ex.node_score, ex.node_mask)
            seg, mx = (b.edge_ptr, b.max_edges) if use == "edges" else (b.ptr, b.max_nodes)
            sel = None
            if undirected:
                sel = ~((occ.twin >= 0) & (occ.twin < torch.arange(occ.twin.numel(), device=DEV)))
            parts.append(faith_from_scores(causal, occ.score, seg, mx, sel, top, ratio=0.3))
            check_faith(singles[-1], parts[-1:])
        check_faith(res, parts)
        assert res["replicas"] == sum(s["replicas"] for s in singles) and res["forwards"] == sum(s["forwards"] for s in singles)
    eng.check_status()
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

"""Subgraph extraction and fidelity on the MI355X: the HIP extraction (cal_subgraph_extract) against the plain-torch
restatement bit for bit (the CPU case list, graphs beyond one chunk of the kernel, 512 small graphs), the extracted batch on
the engine's per-graph route, engine forwards on it and fidelity() / eval_fidelity() against the fp64 oracle, the exact
identities of a deterministic engine, stream order, and fidelity() leaving the engine's state untouched.

Seeds: the oracle alone was checked for these (model seed 2 for CausalGCN, 1 for CausalGAT / CausalGIN at the shapes below): every
head's top-two log-probability gap on the whole batch exceeds 1e-3 and under 1 % of the (head, variant, graph) triples are
near-ties; check_fidelity asserts both again."""
import argparse
import random

import pytest
import torch

from cal_amd import _lib, spmotif, synth
from cal_amd.data import Batch, DataLoader
from cal_amd.explain import eval_fidelity, explain, extract_subgraph, fidelity
from oracle import cal_oracle as O
from tests.subgraph_oracle import (case_batches, check_extraction, check_fidelity, extract_oracle, fidelity_oracle,
                                   oracle_log_probs)

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOGIT_TOL = 1e-4                   # tests/test_gpu_engine.py: the engine's logits against the oracle at these shapes
CASES = case_batches()
SEEDS = {"CausalGCN": 2, "CausalGAT": 1, "CausalGIN": 1}


def _dev(b):
    """A device copy of a CPU batch (the case list is shared between tests)."""
    d = Batch()
    for k, v in b.__dict__.items():
        d.__dict__[k] = v.to(DEV) if torch.is_tensor(v) else v
    d._plan = None
    return d


def _m(t):
    return None if t is None else t.to(DEV)


@pytest.mark.parametrize("relabel", [False, True])
@pytest.mark.parametrize("complement", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_hip_equals_restatement(name, complement, relabel):
    b, em, nm = CASES[name]
    sub = extract_subgraph(_dev(b), edge_mask=_m(em), node_mask=_m(nm), complement=complement, relabel=relabel)
    assert sub.edge_index.is_cuda and sub.ptr.is_cuda
    check_extraction(sub, b, em, nm, complement, relabel)
    host = extract_subgraph(b, edge_mask=em, node_mask=nm, complement=complement, relabel=relabel)
    assert torch.equal(sub.edge_index.cpu(), host.edge_index) and torch.equal(sub.node_map.cpu(), host.node_map)


@pytest.mark.parametrize("which", ["ba5000", "small512"])
def test_hip_beyond_one_chunk_and_many_graphs(which):
    if which == "ba5000":
        b = Batch.from_data_list(synth.ba_graphs(3, n=5000, seed=1))          # thousands of nodes / edges per workgroup
    else:
        b = Batch.from_data_list(spmotif.train_mix(512, node_num=7, seed=6))
    g = torch.Generator().manual_seed(8)
    E, N = b.edge_index.size(1), b.batch.numel()
    em, nm = torch.rand(E, generator=g) < 0.3, torch.rand(N, generator=g) < 0.7
    bd = _dev(b)
    for e_, n_ in ((em, None), (None, nm), (em, nm)):
        for complement in (False, True):
            for relabel in (False, True):
                sub = extract_subgraph(bd, edge_mask=_m(e_), node_mask=_m(n_), complement=complement, relabel=relabel)
                check_extraction(sub, b, e_, n_, complement, relabel)


def test_hip_ungrouped_edge_index():
    b, em, nm = CASES["both"]
    perm = torch.randperm(b.edge_index.size(1), generator=torch.Generator().manual_seed(5))

    class Foreign:
        pass
    f = Foreign()
    f.x, f.feat, f.edge_index, f.batch, f.num_graphs, f.y = b.x.to(DEV), None, b.edge_index[:, perm].to(DEV), b.batch.to(DEV), \
        b.num_graphs, b.y.to(DEV)
    order = torch.argsort(b.batch[b.edge_index[0, perm]], stable=True)
    sub = extract_subgraph(f, edge_mask=em[perm].to(DEV), node_mask=nm.to(DEV), relabel=True)
    r = extract_oracle(b.edge_index[:, perm][:, order], b.ptr, b.edge_ptr, b.batch.numel(), em[perm][order], nm, False, True, b.x)
    assert torch.equal(sub.edge_index.cpu(), r["edge_index"]) and torch.equal(sub.edge_map.cpu(), order[r["edge_map"]])
    assert torch.equal(sub.x.cpu(), r["x"]) and torch.equal(sub.batch.cpu(), r["batch"])


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


def test_extracted_batch_takes_the_per_graph_route():
    m, _ = _gpu_model("CausalGCN")
    b = Batch.from_data_list(spmotif.train_mix(128, node_num=7, seed=11)).to(DEV)          # the headline shape
    ex = explain(m, b, ratio=0.3)
    eng = m.engine()
    for complement in (False, True):
        for relabel in (False, True):
            sub = ex.to_batch(b, complement=complement, relabel=relabel)
            assert sub.ptr.is_cuda and sub.edge_ptr.is_cuda and sub.max_nodes > 0 and sub.no_self_loops
            eng.forward(sub, None, training=False)
            names = _stage_names()
            assert "k_plan_graph" in names and "k_gptr_dis" not in names and "k_plan_count" not in names, names
            eng.check_status()


SHAPES = [("CausalGCN", 128), ("CausalGAT", 64), ("CausalGIN", 64)]       # tests/test_gpu_explain.py's engine shapes


@pytest.mark.parametrize("name,B", SHAPES)
def test_engine_forward_on_extracted_batch_matches_oracle(name, B):
    m, sd = _gpu_model(name)
    b = Batch.from_data_list(spmotif.train_mix(B, node_num=7, seed=11))
    bd = _dev(b)
    ex = explain(m, bd, ratio=0.3)
    em = ex.edge_mask.cpu()
    sd64 = {k: v.double() for k, v in sd.items()}
    eng = m.engine()
    x = b.x if b.x is not None else b.feat
    worst = 0.0
    for complement in (False, True):
        for relabel in (False, True):
            sub = ex.to_batch(bd, complement=complement, relabel=relabel)
            r = check_extraction(sub, b, em, None, complement, relabel)
            assert int(sub.ptr.diff().min()) > 0                  # (zero-node graphs are not the engine's business)
            lp = torch.stack(eng.forward(sub, None, training=False)).cpu().double()
            eng.check_status()
            ref = oracle_log_probs(name, sd64, r["x"], r["edge_index"], r["batch"], B, layers=3, heads=4)
            err = (lp - ref).abs().max().item()
            print("%s complement=%d relabel=%d: max |logp - oracle| = %.3g" % (name, complement, relabel, err))
            worst = max(worst, err)
    assert worst < LOGIT_TOL, worst
    assert x.size(0) == b.batch.numel()


@pytest.mark.parametrize("use", ["edges", "both"])
@pytest.mark.parametrize("name,B", SHAPES)
def test_fidelity_matches_oracle(name, B, use):
    """The selection is the engine's own explanation (its ranking is pinned bit for bit in test_gpu_explain; a score within
    1e-4 of the oracle's may order two near-equal edges differently, which is not what this test is about); the three
    forwards and the metrics are the fp64 oracle's on the restatement's batches."""
    m, sd = _gpu_model(name)
    b = Batch.from_data_list(spmotif.train_mix(B, node_num=7, seed=11))
    bd = _dev(b)
    ex = explain(m, bd, ratio=0.3)
    res = fidelity(m, bd, ratio=0.3, use=use)
    m.engine().check_status()
    ref = fidelity_oracle(name, sd, b, ex.edge_mask.cpu(), ex.node_mask.cpu() if use == "both" else None, layers=3, heads=4)
    check_fidelity(res, ref, LOGIT_TOL)


def test_eval_fidelity_matches_oracle():
    m, sd = _gpu_model("CausalGCN")
    gs = spmotif.train_mix(96, node_num=7, seed=9)
    ratios = (0.2, 0.5)
    res = eval_fidelity(m, DataLoader(gs, batch_size=32, shuffle=False), DEV, ratios=ratios)
    m.engine().check_status()
    for r in ratios:
        refs = []
        for i in range(0, 96, 32):
            b = Batch.from_data_list(gs[i:i + 32])
            ex = explain(m, _dev(b), ratio=r)
            refs.append((fidelity_oracle("CausalGCN", sd, b, ex.edge_mask.cpu(), None, layers=3, heads=4), ex))
        ref = {k: sum(q[k] for q, _ in refs) / len(refs) for k in refs[0][0] if k not in ("hits", "margin", "graphs", "sparsity")}
        ref["graphs"] = 96
        ref["margin"] = torch.cat([q["margin"] for q, _ in refs], -1)
        kept = sum(int(ex.edge_mask.sum()) for _, ex in refs)
        ref["sparsity"] = 1.0 - kept / sum(ex.edge_mask.numel() for _, ex in refs)
        check_fidelity(res[r], ref, LOGIT_TOL)


@pytest.mark.parametrize("name,B", SHAPES)
def test_identities_with_a_deterministic_engine(name, B):
    m, _ = _gpu_model(name, deterministic=True)
    b = Batch.from_data_list(spmotif.train_mix(B, node_num=7, seed=11)).to(DEV)
    one = fidelity(m, b, ratio=1.0)
    zero = fidelity(m, b, k=0)
    for h in ("c", "o", "co"):
        assert one["fid_minus_" + h] == 0.0 and one["acc_keep_" + h] == one["acc_full_" + h], (h, one)
        assert zero["fid_plus_" + h] == 0.0 and zero["acc_drop_" + h] == zero["acc_full_" + h], (h, zero)
    assert one["sparsity"] == 0.0 and zero["sparsity"] == 1.0
    for use in ("edges", "nodes", "both"):
        ex = explain(m, b, ratio=0.3)
        masks = [t for t, u in ((ex.edge_mask, "nodes"), (ex.node_mask, "edges")) if use != u]
        want = 1.0 - sum(int(t.sum()) for t in masks) / sum(t.numel() for t in masks)
        assert fidelity(m, b, ratio=0.3, use=use)["sparsity"] == want
    m.engine().check_status()


def test_extraction_is_stream_ordered():
    m, _ = _gpu_model("CausalGCN")
    b = Batch.from_data_list(spmotif.train_mix(64, node_num=7, seed=11)).to(DEV)
    ex0 = explain(m, b, ratio=0.3)
    ref = ex0.to_batch(b, relabel=True)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ex = explain(m, b, ratio=0.3)                              # the extraction is enqueued behind it, no synchronisation between
        sub = ex.to_batch(b, relabel=True)
    s.synchronize()
    torch.cuda.current_stream().wait_stream(s)
    for key in ("edge_index", "ptr", "edge_ptr", "batch", "node_map", "edge_map"):
        assert torch.equal(getattr(sub, key), getattr(ref, key)), key
    assert torch.equal(sub.feat if sub.x is None else sub.x, ref.feat if ref.x is None else ref.x)
    assert (sub.max_nodes, sub.max_edges) == (ref.max_nodes, ref.max_edges)


def test_fidelity_after_training_leaves_the_engine_state_untouched():
    from cal_amd.engine import StepEngine
    args = _args(layers=2, hidden=64)
    m, _ = _gpu_model("CausalGCN", args, seed=0)
    m.train()
    eng = StepEngine(m, lr=1e-3)
    object.__setattr__(m, "_engine", eng)
    b = Batch.from_data_list(spmotif.train_mix(64, seed=2)).to(DEV)
    perm = torch.randperm(64, device=DEV)
    for _ in range(2):
        eng.train_step(b, perm, adam=True)
    torch.cuda.synchronize()
    snap = [t.clone() for t in (eng.flat_p, eng.exp_avg, eng.exp_avg_sq, eng.step_count, eng.buffer("status", 4, torch.int32))]
    bn = {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}
    py0, t0 = random.getstate(), torch.get_rng_state()
    res = fidelity(m, b, ratio=0.3, use="both")
    assert m.engine() is eng and m.training and res["graphs"] == 64
    after = (eng.flat_p, eng.exp_avg, eng.exp_avg_sq, eng.step_count, eng.buffer("status", 4, torch.int32))
    for u, v in zip(snap, after):
        assert torch.equal(u, v)
    for k, v in m.state_dict().items():
        if k in bn:
            assert torch.equal(v, bn[k]), k
    assert random.getstate() == py0 and torch.equal(torch.get_rng_state(), t0)
    eng.train_step(b, perm, adam=True)                      # training goes on
    eng.check_status()

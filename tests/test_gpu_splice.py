"""Batch splice and structure interventions on the MI355X: the HIP splice (cal_graph_splice_count / cal_graph_splice_write)
against the plain-torch restatement and the host twin bit for bit (the CPU case list, a scan beyond one chunk, parts of very
different sizes, the scalar row copy next to the vector one), the spliced batch on the engine's per-graph route, engine forwards
on it and structure_intervention() / eval_structure_intervention() against the fp64 oracle, the exact identities of a
deterministic engine, stream order, and structure_intervention() leaving the engine's state untouched.

Seeds: the oracle alone was checked on the CPU for these (model seed 2 for CausalGCN, 1 for CausalGAT / CausalGIN, the seeds of
tests/test_gpu_subgraph.py, at the shapes below with the operator-level model's own partition at ratio 0.3 and the partner rows
ROWS): every head's top-two log-probability gap on the whole batch exceeds 1e-3 and under 1 % of the (head, variant, graph)
entries are near-ties, with and without the bridge; check_structure asserts both again."""
import argparse
import random

import pytest
import torch

from cal_amd import _lib, spmotif, synth
from cal_amd.data import Batch, Data, DataLoader
from cal_amd.explain import _Layout, _scores, explain, extract_subgraph
from cal_amd.splice import _structure_forward, eval_structure_intervention, splice_batches, structure_intervention
from oracle import cal_oracle as O
from tests.splice_oracle import HEADS, check_splice, check_structure, splice_cases, structure_oracle
from tests.subgraph_oracle import extract_oracle, oracle_log_probs

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOGIT_TOL = 1e-4                   # tests/test_gpu_engine.py: the engine's logits against the oracle at these shapes
CASES = splice_cases()
SEEDS = {"CausalGCN": 2, "CausalGAT": 1, "CausalGIN": 1}
SHAPES = [("CausalGCN", 128), ("CausalGAT", 64), ("CausalGIN", 64)]       # tests/test_gpu_explain.py's engine shapes


def partner_rows(B, m=2, seed=21):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randperm(B, generator=g) for _ in range(m)])


def _dev(b):
    """A device copy of a CPU batch (the case list is shared between tests)."""
    d = Batch()
    for k, v in b.__dict__.items():
        d.__dict__[k] = v.to(DEV) if torch.is_tensor(v) else v
    d._plan = None
    return d


def _m(t):
    if isinstance(t, (tuple, list)):
        return tuple(_m(v) for v in t)
    return t.to(DEV) if torch.is_tensor(t) else t


def _same(u, v):
    for key in ("edge_index", "ptr", "edge_ptr", "batch", "node_src", "edge_src"):
        assert torch.equal(getattr(u, key).cpu(), getattr(v, key).cpu()), key
    assert (u.max_nodes, u.max_edges, u.empty_graphs, u.bridges_unwritten) == (v.max_nodes, v.max_edges, v.empty_graphs,
                                                                              v.bridges_unwritten)


@pytest.mark.parametrize("name", sorted(CASES))
def test_hip_equals_restatement_and_host_twin(name):
    a, b, ga, gb, bridge = CASES[name]
    res = splice_batches(_dev(a), _dev(b), _m(ga), _m(gb), bridge=_m(bridge))
    assert res.edge_index.is_cuda and res.ptr.is_cuda and res.node_src.is_cuda
    check_splice(res, a, b, ga, gb, bridge)
    _same(res, splice_batches(a, b, ga, gb, bridge=bridge))


def _tiny(n, feat, g, hi=7):
    ds = []
    for _ in range(n):
        k = int(torch.randint(3, hi, (1,), generator=g))
        src = torch.arange(k)
        ei = torch.stack([torch.cat([src, (src + 1) % k]), torch.cat([(src + 1) % k, src])])      # a ring, both directions
        ds.append(Data(x=torch.randn(k, feat, generator=g), edge_index=ei, y=torch.randint(0, 4, (1,), generator=g)))
    return ds


def test_hip_scan_beyond_one_chunk():
    """3000 pairs of 3-6-node graphs, a third of the parts absent (many short and some empty result graphs): every thread of
    the scanning workgroup owns a run of pairs."""
    g = torch.Generator().manual_seed(4)
    a, b = Batch.from_data_list(_tiny(500, 4, g)), Batch.from_data_list(_tiny(300, 4, g))
    ga, gb = torch.randint(-250, 500, (3000,), generator=g).clamp(min=-1), torch.randint(-150, 300, (3000,), generator=g).clamp(min=-1)
    res = splice_batches(_dev(a), _dev(b), ga.to(DEV), gb.to(DEV), bridge="first")
    r = check_splice(res, a, b, ga, gb, "first")
    assert r["totals"][4] > 100 and r["totals"][5] > 500


def test_hip_large_part_next_to_small_ones():
    """One pair of two 5000-node graphs between pairs of 3-node graphs: element loops of thousands of columns in the count, the
    same chunks of the output for everybody in the write."""
    g = torch.Generator().manual_seed(5)
    big = synth.ba_graphs(2, n=5000, seed=1)
    F = int(big[0].x.size(1)) if big[0].x is not None else int(big[0].feat.size(1))
    small = _tiny(6, F, g, hi=4)
    for d in small:
        d.x, d.feat = (d.x, None) if big[0].x is not None else (None, d.x)
    a, b = Batch.from_data_list(small[:2] + [big[0]] + small[2:3]), Batch.from_data_list(small[3:5] + [big[1]] + small[5:])
    res = splice_batches(_dev(a), _dev(b), bridge="first")
    check_splice(res, a, b, None, None, "first")
    assert res.max_nodes == 10000
    # a dropped column in the large part: the compacted path of the count and sel[] in the write
    a.edge_index = a.edge_index.clone()
    lo = int(a.edge_ptr[2])
    a.edge_index[0, lo + 1500] = 0
    a.edge_index[1, lo + 7777] = int(a.ptr[3])
    res = splice_batches(_dev(a), _dev(b), torch.tensor([2, 0, 2], device=DEV), torch.tensor([2, 2, -1], device=DEV))
    r = check_splice(res, a, b, [2, 0, 2], [2, 2, -1], None)
    assert r["totals"][1] == res.edge_index.size(1) and int((res.edge_src >= 0).sum()) == 2 * (int(a.edge_ptr[3]) - lo - 2) + \
        int(a.edge_ptr[1])


@pytest.mark.parametrize("F", [5, 4])
def test_hip_rows_at_odd_offsets(F):
    """Feature matrices that start one float into their storage: F = 5 takes the scalar copy as always, F = 4 takes it because
    the rows are not 16-byte aligned (next to the aligned call, which takes the vector copy)."""
    from tests.splice_oracle import _with_feat
    a0, b0, _, gb, _ = CASES["permutation"]
    a, b = _with_feat(a0, F, 31), _with_feat(b0, F, 32)
    ad, bd = _dev(a), _dev(b)
    for src, d in ((a, ad), (b, bd)):
        flat = torch.empty(src.x.numel() + 1, device=DEV)
        flat[1:] = src.x.to(DEV).view(-1)
        d.x = flat[1:].view(-1, F)
        assert d.x.data_ptr() % 16 == 4 and d.x.is_contiguous()
    check_splice(splice_batches(ad, bd, None, gb.to(DEV)), a, b, None, gb, None)
    check_splice(splice_batches(_dev(a), _dev(b), None, gb.to(DEV)), a, b, None, gb, None)


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


def _parts(m, bd, ratio=0.3):
    ex = explain(m, bd, ratio=ratio)
    return ex, extract_subgraph(bd, node_mask=ex.node_mask, relabel=True), \
        extract_subgraph(bd, node_mask=ex.node_mask, complement=True, relabel=True)


def test_spliced_batch_takes_the_per_graph_route():
    m, _ = _gpu_model("CausalGCN")
    b = Batch.from_data_list(spmotif.train_mix(128, node_num=7, seed=11)).to(DEV)          # the headline shape
    _, causal, trivial = _parts(m, b)
    eng = m.engine()
    perm = partner_rows(128)[0].to(DEV)
    for bridge in (None, "first"):
        sp = splice_batches(causal, trivial, None, perm, bridge=bridge)
        assert sp.ptr.is_cuda and sp.edge_ptr.is_cuda and sp.max_nodes > 0 and sp.no_self_loops and sp.empty_graphs == 0
        eng.forward(sp, None, training=False)
        names = _stage_names()
        assert "k_plan_graph" in names and "k_gptr_dis" not in names and "k_plan_count" not in names, names
        eng.check_status()


@pytest.mark.parametrize("name,B", SHAPES)
def test_engine_forward_on_spliced_batch_matches_oracle(name, B):
    m, sd = _gpu_model(name)
    b = Batch.from_data_list(spmotif.train_mix(B, node_num=7, seed=11))
    bd = _dev(b)
    ex, causal, trivial = _parts(m, bd)
    nm = ex.node_mask.cpu()
    x = b.x if b.x is not None else b.feat
    oc, ot = (extract_oracle(b.edge_index, b.ptr, b.edge_ptr, x.size(0), node_keep=nm, complement=c, relabel=True, x=x)
              for c in (False, True))
    sd64 = {k: v.double() for k, v in sd.items()}
    eng = m.engine()
    perm = partner_rows(B)[0]
    worst = 0.0
    for bridge in (None, "first"):
        sp = splice_batches(causal, trivial, None, perm.to(DEV), bridge=bridge)
        src = [Batch(), Batch()]                              # the restatement's two parts as sources
        for s, r in zip(src, (oc, ot)):
            s.x, s.feat = (r["x"], None) if b.x is not None else (None, r["x"])
            s.edge_index, s.batch, s.ptr, s.edge_ptr, s.num_graphs, s.no_self_loops = r["edge_index"], r["batch"], r["ptr"], \
                r["edge_ptr"], B, True
        src[0].y = b.y
        r = check_splice(sp, src[0], src[1], None, perm, bridge)
        assert int(sp.ptr.diff().min()) > 0                   # (zero-node graphs are not the engine's business)
        lp = torch.stack(eng.forward(sp, None, training=False)).cpu().double()
        eng.check_status()
        ref = oracle_log_probs(name, sd64, r["x"], r["edge_index"], r["batch"], B, layers=3, heads=4)
        err = (lp - ref).abs().max().item()
        print("%s bridge=%s: max |logp - oracle| = %.3g" % (name, bridge, err))
        worst = max(worst, err)
    assert worst < LOGIT_TOL, worst


@pytest.mark.parametrize("bridge", [None, "first"])
@pytest.mark.parametrize("name,B", SHAPES)
def test_structure_intervention_matches_oracle(name, B, bridge):
    """The partition is the engine's own explanation (its ranking is pinned bit for bit in test_gpu_explain); the splices, the
    forwards and the metrics are the fp64 oracle's on the restatement's batches."""
    m, sd = _gpu_model(name)
    b = Batch.from_data_list(spmotif.train_mix(B, node_num=7, seed=11))
    bd = _dev(b)
    rows = partner_rows(B)
    ex = explain(m, bd, ratio=0.3)
    res = structure_intervention(m, bd, ratio=0.3, partners=rows.to(DEV), bridge=bridge)
    m.engine().check_status()
    ref = structure_oracle(name, sd, b, ex.node_mask.cpu(), rows, bridge, layers=3, heads=4)
    check_structure(res, [ref], LOGIT_TOL)


def test_eval_structure_intervention_matches_oracle():
    m, sd = _gpu_model("CausalGCN")
    gs = spmotif.train_mix(96, node_num=7, seed=9)
    rows = partner_rows(32)
    ratios = (0.3, 0.5)
    res = eval_structure_intervention(m, DataLoader(gs, batch_size=32, shuffle=False), DEV, ratios=ratios, partners=rows.to(DEV))
    m.engine().check_status()
    for r in ratios:
        parts = []
        for i in range(0, 96, 32):
            b = Batch.from_data_list(gs[i:i + 32])
            ex = explain(m, _dev(b), ratio=r)
            parts.append(structure_oracle("CausalGCN", sd, b, ex.node_mask.cpu(), rows, None, layers=3, heads=4))
        check_structure(res[r], parts, LOGIT_TOL)


@pytest.mark.parametrize("name,B", SHAPES)
def test_identities_with_a_deterministic_engine(name, B):
    m, _ = _gpu_model(name, deterministic=True)
    b = Batch.from_data_list(spmotif.train_mix(B, node_num=7, seed=11)).to(DEV)
    x = b.x if b.x is not None else b.feat
    none = torch.zeros(0, B, dtype=torch.long, device=DEV)
    m.eval()
    with torch.no_grad():
        lay = _Layout(b)
        edge, node = _scores(m, b)
        sc = (edge.clone(), node.clone())
        for ratio, k in ((1.0, None), (None, 0)):
            full, ident, _, _, _, _, sp = _structure_forward(m, b, lay, sc, ratio, k, "nodes", None, none, None)
            assert torch.equal(sp.edge_index, b.edge_index) and torch.equal(sp.ptr, b.ptr)
            assert torch.equal(sp.x if sp.x is not None else sp.feat, x)
            assert torch.equal(ident, full)
    for kw in (dict(ratio=1.0), dict(k=0)):
        res = structure_intervention(m, b, partners=partner_rows(B, 1).to(DEV), **kw)
        for h in HEADS:
            assert res["acc_self_" + h] == res["acc_full_" + h], (h, res)
    m.engine().check_status()


def test_splice_is_stream_ordered():
    m, _ = _gpu_model("CausalGCN")
    b = Batch.from_data_list(spmotif.train_mix(64, node_num=7, seed=11)).to(DEV)
    perm = partner_rows(64)[0].to(DEV)
    _, causal, trivial = _parts(m, b)
    ref = splice_batches(causal, trivial, None, perm, bridge="first")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _, c2, t2 = _parts(m, b)                               # the splice is enqueued behind them, no synchronisation between
        sp = splice_batches(c2, t2, None, perm, bridge="first")
    s.synchronize()
    torch.cuda.current_stream().wait_stream(s)
    _same(sp, ref)
    assert torch.equal(sp.feat if sp.x is None else sp.x, ref.feat if ref.x is None else ref.x)


def test_structure_intervention_after_training_leaves_the_engine_state_untouched():
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
    py0, t0, c0 = random.getstate(), torch.get_rng_state(), torch.cuda.get_rng_state()
    res = m.structure_intervention(b, ratio=0.3, partners=2, bridge="first")
    assert m.engine() is eng and m.training and res["graphs"] == 64
    after = (eng.flat_p, eng.exp_avg, eng.exp_avg_sq, eng.step_count, eng.buffer("status", 4, torch.int32))
    for u, v in zip(snap, after):
        assert torch.equal(u, v)
    for k, v in m.state_dict().items():
        if k in bn:
            assert torch.equal(v, bn[k]), k
    assert random.getstate() == py0 and torch.equal(torch.get_rng_state(), t0) and torch.equal(torch.cuda.get_rng_state(), c0)
    eng.train_step(b, perm, adam=True)                      # training goes on
    eng.check_status()

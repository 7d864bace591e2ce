"""The step's Adam held to the fp64 contract of tests/adam_oracle.py at every site that applies it: ``k_adam`` alone
(``cal_engine_adam``, ``cal_engine_adam_ticked``, behind ``k_finish`` with CAL_AMD_ADAM_FUSED=0) and ``adam_update`` in the three
branches of ``k_finish`` (slab tasks, commit tasks, update-only ranges), under every protocol that advances the step counter.

The method: ``k_finish`` stores the finished gradient into ``flat_g`` in the thread that applies it, so after a step the exact
relation (P0, M0, V0, G, t) -> (P1, M1, V1) can be judged for EVERY element of the flat buffers (padding included, no mask),
whatever the rest of the step did: ``adam_oracle.check_step``.  ``cal_engine_finish_layout`` says which site updated which
element; every test prints the largest error / bound per site kind (run with -s).  What a wrong update looks like to this
judge is asserted on the CPU (tests/test_adam_oracle.py: 14 seeded defects)."""
import argparse
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import cal_oracle as O
from tests import adam_oracle as AO
from tests.helpers import ref_graphs

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = {0: "slab", 1: "commit", 2: "range"}
#: the hyper-parameters of the real-step cases: both betas off torch's defaults, an eps and a weight decay that matter
HP = dict(b1=0.8, b2=0.99, eps=1e-3, wd=1e-3)


def _args(**kw):
    d = dict(layers=2, hidden=64, with_random=True, without_node_attention=False,
             without_edge_attention=False, fc_num="222", cat_or_add="add", c=0.5, o=1.0, co=0.5)
    d.update(kw)
    return argparse.Namespace(**d)


def _model(name, nfeat=10, ncls=4, seed=3, **kw):
    from cal_amd import model as M
    args = _args(**kw)
    torch.manual_seed(seed)
    sd = O.init_state(name, nfeat, ncls, hidden=args.hidden, layers=args.layers, heads=4, cat_or_add=args.cat_or_add)
    m = getattr(M, name)(nfeat, ncls, args)
    m.load_state_dict(sd, strict=name != "CausalGIN")
    m = m.to(DEV).train()
    if name == "CausalGAT":
        for c in m.convs:
            c.dropout = 0.0
    return m, args


def _engine(name, gscale=0.5, **kw):
    from cal_amd.engine import StepEngine
    m, args = _model(name, **kw)
    eng = StepEngine(m, lr=1e-3, betas=(HP["b1"], HP["b2"]), eps=HP["eps"], weight_decay=HP["wd"])
    eng.set_grad_scale(gscale)
    return m, eng


def _batch(sizes, nfeat=10, seed=0):
    """Random undirected graphs of the given sizes, no self loops, about four neighbours per node."""
    from cal_amd.data import Batch, Data
    g = torch.Generator().manual_seed(seed)
    ds = []
    for n in sizes:
        a = torch.rand(n, n, generator=g) < min(0.3, 4.0 / n)
        a = a | a.t()
        a.fill_diagonal_(False)
        ds.append(Data(x=torch.randn(n, nfeat, generator=g), edge_index=a.nonzero().t().contiguous(),
                       y=torch.randint(0, 4, (1,), generator=g)))
    return Batch.from_data_list(ds).to(DEV)


def _random_moments(eng, t0, seed=1):
    """Non-zero moments of either sign over the parameters (the padding keeps its zeros), the counter at ``t0``."""
    g = torch.Generator().manual_seed(seed)
    n = eng.flat_p.numel()
    live = _padding(eng) == 0
    m = 1e-3 * torch.randn(n, generator=g) * live
    v = (1e-3 * torch.randn(n, generator=g)) ** 2 * live
    eng.exp_avg.copy_(m.to(DEV))
    eng.exp_avg_sq.copy_(v.to(DEV))
    eng.step_count.fill_(float(t0))


def _padding(eng):
    """1 where the flat buffers hold alignment padding, 0 where a parameter lives (CPU tensor)."""
    from cal_amd.trainer import flat_offsets
    params = list(eng.model.parameters())
    pad = torch.ones(eng.flat_p.numel())
    for p, off in zip(params, flat_offsets(params)[0]):
        pad[off:off + p.numel()] = 0
    return pad


def _layout(eng):
    """``[(begin, end, kind)]`` of the latest step's k_finish tasks and the adam_in_finish it ended with."""
    from cal_amd import _lib
    out = (ctypes.c_int64 * (3 * 256))()
    mode = ctypes.c_int64(-1)
    n = _lib.query("cal_engine_finish_layout", eng._h, out, 3 * 256, ctypes.byref(mode))
    assert 0 <= n <= 256
    return [(out[3 * i], out[3 * i + 1], out[3 * i + 2]) for i in range(n)], int(mode.value)


def _stage_names():
    from cal_amd import _lib
    h = _lib.lib()
    names, k = [], 1
    while True:
        nm = h.cal_engine_stage_name(k)
        nm = nm.decode() if isinstance(nm, bytes) else nm
        if not nm:
            return names
        names.append(nm)
        k += 1


def _by_kind(ratio, iv):
    out = {}
    for b, e, k in iv:
        if e > b:
            out[KINDS[k]] = max(out.get(KINDS[k], 0.0), float(ratio[b:e].max()))
    return out


def _assert_partition(iv, n):
    """The tasks' intervals are disjoint and cover [0, n) exactly: every element is updated exactly once."""
    pos = 0
    for b, e, _ in sorted(iv):
        assert b == pos and e >= b, (b, e, pos)
        pos = e
    assert pos == n, (pos, n)


def _assert_padding_zero(eng):
    pad = _padding(eng).bool()
    for t in (eng.flat_p, eng.exp_avg, eng.exp_avg_sq):
        assert not t.detach().cpu()[pad].any()


# ---- a. k_adam alone -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", AO.T)
def test_k_adam_alone_obeys_the_contract_on_every_case(t):
    """``cal_engine_adam`` (k_adam with ticked = 0, then k_adam_tick) on the synthetic states of ``adam_oracle.CASES`` -- special
    elements included -- written over the whole flat buffer of a small model (7884 elements: the last block is ragged).  Every
    element within the bound, the counter exactly t, and two calls from equal state give equal bits."""
    m, eng = _engine("CausalGCN", hidden=32, layers=1)
    n = eng.flat_p.numel()
    assert n % 256 != 0
    eng.train_step(_batch([5, 7, 6]), None, adam=False)          # (the workspace and its status word exist)
    eng.check_status()
    worst = 0.0
    for c in [c for c in AO.CASES if c["t"] == t]:
        lr, b1, b2, eps, wd, gs = c["dbl"]
        eng.set_adam(b1, b2, eps, wd)
        eng.set_grad_scale(gs)
        eng.lr.fill_(lr)
        p, g, m0, v0 = (torch.from_numpy(a) for a in AO.draw_state(c, n))
        bits = []
        for _ in range(2):
            with torch.no_grad():
                eng.flat_p.copy_(p.to(DEV)); eng.flat_g.copy_(g.to(DEV))
            eng.exp_avg.copy_(m0.to(DEV)); eng.exp_avg_sq.copy_(v0.to(DEV))
            eng.step_count.fill_(float(t - 1))
            before = AO.snapshot(eng)
            assert before["lr"] == c["lr"] and before["t"] == t - 1
            eng.adam()
            ratio = AO.check_step(eng, before, t, b1, b2, eps, wd, gs, label=("k_adam", c["id"]))
            bits.append((eng.flat_p.detach().clone(), eng.exp_avg.clone(), eng.exp_avg_sq.clone()))
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*bits))
        z = AO.SPECIAL["zero"]
        if wd == 0:                                              # g = 0 from zero moments: nothing moves
            assert float(bits[0][0][z]) == float(p[z]) and float(bits[0][1][z]) == 0 and float(bits[0][2][z]) == 0
        worst = max(worst, float(ratio.max()))
    eng.check_status()
    print("\nk_adam alone, t = %d: largest error / bound over %d cases x %d elements: %.2f" % (t, len(AO.CASES) // len(AO.T), n, worst))


# ---- b. the three k_finish sites on each route family ----------------------------------------------------------------------------
def _sizes(lo, hi, n, seed):
    rng = np.random.default_rng(seed)
    return [int(x) for x in rng.integers(lo, hi + 1, n)]


FAMILIES = {
    # per-graph kernels, both attention folds
    "gcn_h128_l2": ("CausalGCN", dict(hidden=128, layers=2), _sizes(5, 24, 8, 1)),
    "gcn_h64_l1": ("CausalGCN", dict(hidden=64, layers=1), _sizes(5, 24, 8, 2)),
    "gat_h128_k4": ("CausalGAT", dict(hidden=128, layers=2), _sizes(5, 24, 8, 3)),
    "gin_h64": ("CausalGIN", dict(hidden=64, layers=2), _sizes(5, 24, 8, 4)),
    # one 300-node graph among small ones: the node-level chain
    "gcn_node_level": ("CausalGCN", dict(hidden=64, layers=2), [12, 300, 9, 20, 7]),
    # graphs of 130 .. 200 nodes: the wide per-graph kernels
    "gcn_wide": ("CausalGCN", dict(hidden=64, layers=2), [130, 200, 161, 177]),
    # the 2H-wide co head: the readout as GEMMs
    "gcn_cat": ("CausalGCN", dict(hidden=64, layers=2, cat_or_add="cat"), _sizes(5, 24, 8, 5)),
    "gcn_l0": ("CausalGCN", dict(hidden=64, layers=0), _sizes(5, 24, 8, 6)),
    # the deepest models the engine accepts (MAX_LAYERS = 6): the most gaps between the tasks
    "gcn_l6_node_level": ("CausalGCN", dict(hidden=64, layers=6), [12, 300, 9, 20, 7]),
    "gin_l6_node_level": ("CausalGIN", dict(hidden=64, layers=6), [12, 300, 9, 20, 7]),
    "gat_l6_node_level": ("CausalGAT", dict(hidden=64, layers=6), [12, 300, 9, 20, 7]),
    "gin_l6_cat": ("CausalGIN", dict(hidden=64, layers=6, cat_or_add="cat"), _sizes(5, 24, 8, 7)),
    # more than 512 graphs: no one-launch readout, no per-graph backward
    "gin_l6_b600": ("CausalGIN", dict(hidden=64, layers=6), _sizes(3, 6, 600, 8)),
}


@functools.lru_cache(maxsize=None)
def _run_family(family):
    """-> (site kinds seen, update-only ranges, adam_in_finish) of the family's steps; every assertion of the contract inside."""
    name, kw, sizes = FAMILIES[family]
    m, eng = _engine(name, **kw)
    bd = _batch(sizes, seed=len(sizes))
    n = eng.flat_p.numel()
    seen = set()
    for t0 in (0, 7):
        _random_moments(eng, t0, seed=11 + t0)
        before = AO.snapshot(eng)
        eng.train_step(bd, None, adam=True)
        names = _stage_names()
        iv, mode = _layout(eng)
        ratio = AO.check_step(eng, before, t0 + 1, gscale=0.5, label=(family, t0), **HP)
        eng.check_status()
        _assert_padding_zero(eng)
        assert names[-1] == "k_finish" and "k_adam" not in names and mode == 1, (names, mode)
        _assert_partition(iv, n)
        per = _by_kind(ratio, iv)
        nranges = sum(1 for _, _, k in iv if k == 2)
        assert nranges <= 24
        seen |= set(per)
        print("\n%-18s t0 = %d  nparam %6d  tasks: %2d slab %2d commit %2d range   error / bound: %s"
              % (family, t0, n, sum(1 for x in iv if x[2] == 0), sum(1 for x in iv if x[2] == 1), nranges,
                 "  ".join("%s %.2f" % kv for kv in sorted(per.items()))))
    return seen, nranges, mode


@pytest.mark.parametrize("family", list(FAMILIES))
def test_k_finish_sites_obey_the_contract_on_each_route_family(family):
    """One fused step per t0 in {0, 7} at wd = 1e-3, gscale = 0.5 from random non-zero moments.  The layout reader's intervals
    are disjoint and cover [0, nparam) exactly, no k_adam launch follows, every element of P, M, V is within the bound at
    t = t0 + 1, the padding stays exactly 0 and the counter is exactly t.

    The fallback to a separate k_adam (``adam_in_finish == 2``: more than MAX_ADAM_RANGES = 24 gaps, or overlapping tasks) is
    NOT reachable from any shape StepEngine accepts, so it has no case here: the tasks never overlap (asserted), and the number
    of update-only ranges does not grow with the depth -- on every family here the backbone's weight gradients arrive as slab
    tasks.  Counts seen: 11 on every GCN / GAT / GIN family, the 6-layer backbones (MAX_LAYERS) on the node-level chain
    included; 10 without a backbone layer; 5 for the 600-graph batch (printed with the others).  Even if no weight were
    summed from slabs, a model has at most 21 runs of weights between its bias / BatchNorm commit tasks (CausalGIN,
    6 layers: 1 + 12 + 2 + 6)."""
    _run_family(family)


def test_all_three_site_kinds_occur_over_the_families():
    seen = {f: _run_family(f) for f in FAMILIES}          # (cached when the cases above ran in this process)
    kinds = set().union(*(s[0] for s in seen.values()))
    assert kinds == set(KINDS.values()), kinds
    assert all(s[2] == 1 for s in seen.values())
    print("\nupdate-only ranges per family:", {f: s[1] for f, s in seen.items()})


# ---- c. every counter protocol, three consecutive steps --------------------------------------------------------------------------
def _three_steps(eng, bd, run, label, gscale=0.5, site="k_finish"):
    """Steps t = 1, 2, 3 from a fresh engine: contract and counter after each; returns the stage names per step."""
    names = []
    for t in (1, 2, 3):
        before = AO.snapshot(eng)
        assert before["t"] == t - 1
        run()
        names.append(_stage_names())
        ratio = AO.check_step(eng, before, t, gscale=gscale, label=(label, t), **HP)
        eng.check_status()
        print("\n%-12s t = %d  %s  largest error / bound %.2f" % (label, t, site, float(ratio.max())))
    _assert_padding_zero(eng)
    return names


@pytest.mark.parametrize("env", [None, "CAL_AMD_ADAM_FUSED", "CAL_AMD_FOLD_ZERO"])
def test_counter_protocols_of_the_one_call_step(env, monkeypatch):
    """t = 1, 2, 3 -- where an off-by-one of the bias corrections is largest -- through the fused default (the counter advanced by
    k_zero_f64 in the first step of a fresh engine, inside k_plan_graph from the second), CAL_AMD_ADAM_FUSED=0 (advanced by
    k_finish through fa.tick, k_adam follows) and CAL_AMD_FOLD_ZERO=0 (always k_zero_f64)."""
    if env:
        monkeypatch.setenv(env, "0")
    m, eng = _engine("CausalGCN", hidden=128, layers=2)
    bd = _batch(_sizes(5, 24, 8, 1), seed=8)
    names = _three_steps(eng, bd, lambda: eng.train_step(bd, None, adam=True), env or "fused",
                         site="k_adam" if env == "CAL_AMD_ADAM_FUSED" else "k_finish")
    iv, mode = _layout(eng)
    assert "k_zero_f64" in names[0]                                         # the first step of an engine keeps the launch
    assert ("k_zero_f64" in names[2]) == (env == "CAL_AMD_FOLD_ZERO")
    if env == "CAL_AMD_ADAM_FUSED":
        assert mode == 0 and all(nm[-2:] == ["k_finish", "k_adam"] for nm in names) and not any(k == 2 for _, _, k in iv)
    else:
        assert mode == 1 and all("k_adam" not in nm for nm in names)


def test_counter_protocols_of_the_separate_update():
    """``train_step(adam=False, tick=True)`` + ``adam_ticked()`` (the counter advanced by k_finish, k_adam with ticked = 1) and
    ``train_step(adam=False)`` + ``adam()`` (k_adam with ticked = 0, advanced by k_adam_tick behind it)."""
    bd = _batch(_sizes(5, 24, 8, 1), seed=8)
    for label in ("ticked", "adam"):
        m, eng = _engine("CausalGCN", hidden=64, layers=2)

        def run():
            p0, t0 = eng.flat_p.detach().clone(), float(eng.step_count.item())
            eng.train_step(bd, None, adam=False, tick=label == "ticked")
            assert torch.equal(eng.flat_p.detach(), p0)
            assert float(eng.step_count.item()) == t0 + (1 if label == "ticked" else 0)
            (eng.adam_ticked if label == "ticked" else eng.adam)()
        _three_steps(eng, bd, run, label, site="k_adam")
        assert _layout(eng)[1] == 0


def test_counter_protocol_of_the_module_surface():
    """``EngineAdam.step()`` after ``loss.backward()`` through the engine's autograd node: one k_adam launch per step."""
    from cal_amd.optim import EngineAdam
    from cal_amd.train_causal import causal_loss
    m, args = _model("CausalGCN", hidden=64, layers=2)
    bd = _batch(_sizes(5, 24, 8, 1), seed=8)
    opt = EngineAdam(m.parameters(), lr=1e-3, betas=(HP["b1"], HP["b2"]), eps=HP["eps"], weight_decay=HP["wd"])
    eng = m.engine()
    eng.set_grad_scale(0.5)
    perm = torch.arange(8)
    for t in (1, 2, 3):
        opt.zero_grad()
        c, o, co = m(bd, eval_random=True, perm=perm)
        causal_loss(c, o, co, bd.y, 4, args)[0].backward()
        before = AO.snapshot(eng)
        opt.step()
        ratio = AO.check_step(eng, before, t, gscale=0.5, label=("module", t), **HP)
        eng.check_status()
        print("\nmodule       t = %d  k_adam  largest error / bound %.2f" % (t, float(ratio.max())))
    assert opt._cal_binding is not None and all(float(s["step"]) == 3.0 for s in opt.state_dict()["state"].values())


def test_bound_torch_adam_and_the_engine_share_moments_and_counters():
    """A plain ``torch.optim.Adam`` attached by ``optim.bind``, stepped alternately the engine's way (one call, Adam inside
    k_finish) and torch's way (module forward, backward, ``optimizer.step()``): the shared moments obey the contract whichever
    ran -- torch's own fp32 kernels with Python-double hyper-parameters within bound + representation gap -- and both counters
    read t after every step."""
    from cal_amd.optim import bind
    from cal_amd.train_causal import causal_loss
    m, args = _model("CausalGCN", hidden=64, layers=2)
    bd = _batch(_sizes(5, 24, 8, 1), seed=8)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, betas=(HP["b1"], HP["b2"]), eps=HP["eps"], weight_decay=HP["wd"])
    b = bind(opt, m)
    assert b is not None
    eng = b.engine
    perm = torch.arange(8)
    hp64 = (1e-3, HP["b1"], HP["b2"], HP["eps"], HP["wd"], 1.0)
    for t in (1, 2, 3, 4):
        if t % 2:
            b.resync()
            assert float(eng.step_count.item()) == t - 1
            before = AO.snapshot(eng)
            eng.train_step(bd, perm.to(DEV), adam=True)
            b.stepped()
            b.flush()
            ratio = AO.check_step(eng, before, t, gscale=1.0, label=("bound/engine", t), **HP)
        else:
            opt.zero_grad()
            c, o, co = m(bd, eval_random=True, perm=perm)
            causal_loss(c, o, co, bd.y, 4, args)[0].backward()
            before = AO.snapshot(eng)
            opt.step()
            b.resync()                                           # the engine's counter follows the optimizer's
            g = eng.flat_g.detach().cpu().numpy()
            gap = AO.gap_bound(before["p"], g, before["m"], before["v"], t, hp64, tuple(AO.f32(x) for x in hp64))
            ratio = AO.check_step(eng, before, t, gscale=1.0, label=("bound/torch", t), extra=gap, **HP)
        eng.check_status()
        assert all(float(opt.state[p]["step"]) == t for p in m.parameters()) and float(eng.step_count.item()) == t
        print("\nbound        t = %d  %s  largest error / bound %.2f" % (t, "engine" if t % 2 else "torch ", float(ratio.max())))


# ---- d. a captured step replayed -------------------------------------------------------------------------------------------------
def test_captured_step_replayed_obeys_the_contract_at_each_replays_t_and_lr():
    m, eng = _engine("CausalGCN", hidden=128, layers=2)
    bd = _batch(_sizes(5, 24, 8, 1), seed=8)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eng.train_step(bd, None, adam=True)                      # (warm-up: the workspace exists, the arena is known)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.train_step(bd, None, adam=True)
    torch.cuda.synchronize()
    assert float(eng.step_count.item()) == 1.0                   # capturing ran nothing
    for k, lr in enumerate((1e-3, 2.5e-3, 4e-4)):
        eng.lr.fill_(lr)
        before = AO.snapshot(eng)
        assert before["lr"] == AO.f32(lr)
        g.replay()
        torch.cuda.synchronize()
        ratio = AO.check_step(eng, before, 2 + k, gscale=0.5, label=("replay", k), **HP)
        eng.check_status()
        print("\nreplay %d      t = %d  lr %.1e  largest error / bound %.2f" % (k, 2 + k, lr, float(ratio.max())))


# ---- e. a flagged step -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("protocol", ["fused", "CAL_AMD_ADAM_FUSED", "CAL_AMD_FOLD_ZERO", "ticked", "adam"])
def test_flagged_step_leaves_parameters_moments_and_counter_bit_identical(protocol, monkeypatch):
    """The bad-bounds batch of test_flagged_step_leaves_the_parameters_alone on every protocol that can be flagged: the flagged
    step and a valid one behind it (the word is sticky) leave P, M, V and the step counter bit-identical; after check_status
    has raised, the next step obeys the contract at t0 + 1."""
    from cal_amd import _lib
    from cal_amd.data import Batch
    if protocol.startswith("CAL_"):
        monkeypatch.setenv(protocol, "0")
    good = Batch.from_data_list(ref_graphs(list(range(8)))).to(DEV)
    bad = Batch.from_data_list(ref_graphs([24, 25])).to(DEV)
    bad.max_nodes, bad.max_edges = 50, 100
    m, eng = _engine("CausalGCN", hidden=64, layers=2)

    def run(b):
        if protocol in ("ticked", "adam"):
            eng.train_step(b, None, adam=False, tick=protocol == "ticked")
            (eng.adam_ticked if protocol == "ticked" else eng.adam)()
        else:
            eng.train_step(b, None, adam=True)
    run(good)
    eng.check_status()
    _random_moments(eng, 7)
    before = AO.snapshot(eng)
    keep = [t.detach().clone() for t in (eng.flat_p, eng.exp_avg, eng.exp_avg_sq, eng.step_count)]
    for b in (bad, good):
        run(b)
        now = (eng.flat_p.detach(), eng.exp_avg, eng.exp_avg_sq, eng.step_count)
        assert all(torch.equal(a.view(torch.int32), k.view(torch.int32)) for a, k in zip(now, keep)), protocol
    with pytest.raises(_lib.CalError, match="per-graph bounds"):
        eng.check_status()
    run(good)
    AO.check_step(eng, before, 8, gscale=0.5, label=("after the flag", protocol), **HP)
    eng.check_status()


# ---- f. against torch's semantics ------------------------------------------------------------------------------------------------
def test_three_steps_equal_torch_adam_fed_the_same_gradients():
    """CausalGCN with ``without_node_attention``: the read-back G as ``.grad`` of ``torch.optim.Adam`` on fp64 CPU copies, step by
    step from the engine's state before each step, Python-double hyper-parameters: every parameter with a gradient path within
    bound + representation gap.  The switched-off attention MLP and conv_feat.bias have no gradient path: the reference leaves
    their ``.grad`` None and torch skips them; the engine updates every element of the flat buffer and gives them a ZERO
    gradient ("Adam on parameters without a gradient path"): with weight decay their moments and weights move as
    torch's would under ``zero_grad(set_to_none=False)``.  Both halves are asserted."""
    from cal_amd.engine import StepEngine
    from cal_amd.trainer import flat_offsets
    m, args = _model("CausalGCN", hidden=64, layers=2, without_node_attention=True)
    eng = StepEngine(m, lr=1e-3, betas=(HP["b1"], HP["b2"]), eps=HP["eps"], weight_decay=HP["wd"])
    bd = _batch(_sizes(5, 24, 8, 1), seed=8)
    names = [k for k, _ in m.named_parameters()]
    params = list(m.parameters())
    offs = flat_offsets(params)[0]
    dead = {"node_att_mlp.weight", "node_att_mlp.bias", "conv_feat.bias"}
    tp = [torch.nn.Parameter(p.detach().cpu().double().clone()) for p in params]
    opt = torch.optim.Adam(tp, lr=1e-3, betas=(HP["b1"], HP["b2"]), eps=HP["eps"], weight_decay=HP["wd"], foreach=False)
    hp64 = (1e-3, HP["b1"], HP["b2"], HP["eps"], HP["wd"], 1.0)
    moved = False
    for t in (1, 2, 3):
        before = AO.snapshot(eng)
        eng.train_step(bd, None, adam=True)
        AO.check_step(eng, before, t, gscale=1.0, label=("torch semantics", t), **HP)      # zero-gradient semantics everywhere
        eng.check_status()
        after = AO.snapshot(eng)
        g = eng.flat_g.detach().cpu().numpy()
        bnd = AO.bound(before["p"], g, before["m"], before["v"], t, before["lr"], *(AO.f32(x) for x in hp64[1:]))
        gap = AO.gap_bound(before["p"], g, before["m"], before["v"], t, hp64, tuple(AO.f32(x) for x in hp64))
        worst = 0.0
        for k, q, p, off in zip(names, tp, params, offs):
            sl = slice(off, off + p.numel())
            with torch.no_grad():
                q.copy_(torch.from_numpy(before["p"][sl]).double().view(q.shape))
            if k in dead:
                assert not g[sl].any(), k
                q.grad = None
                continue
            if t > 1:
                opt.state[q]["exp_avg"].copy_(torch.from_numpy(before["m"][sl]).double().view(q.shape))
                opt.state[q]["exp_avg_sq"].copy_(torch.from_numpy(before["v"][sl]).double().view(q.shape))
            q.grad = torch.from_numpy(g[sl]).double().view(q.shape)
        opt.step()
        for k, q, p, off in zip(names, tp, params, offs):
            sl = slice(off, off + p.numel())
            if k in dead:
                assert q not in opt.state and np.array_equal(q.detach().numpy().reshape(-1), before["p"][sl].astype(np.float64))
                moved |= bool((after["p"][sl] != before["p"][sl]).any())
                continue
            assert float(opt.state[q]["step"]) == t
            for key, got, ref in (("p", after["p"][sl], q.detach().numpy()), ("m", after["m"][sl], opt.state[q]["exp_avg"].numpy()),
                                  ("v", after["v"][sl], opt.state[q]["exp_avg_sq"].numpy())):
                err = np.abs(got.astype(np.float64) - ref.reshape(-1))
                lim = bnd[key][sl] + gap[key][sl]
                assert np.all(err <= lim), (k, key, t, float((err / lim).max()))
                worst = max(worst, float((err / lim).max()))
        print("\ntorch fp64   t = %d  largest |engine - torch| / (bound + gap) %.2f" % (t, worst))
    assert moved          # the dead attention MLP decays with wd > 0 where torch would have skipped it

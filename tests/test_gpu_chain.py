"""Chained train steps: the commit of step i and the graph plan of batch i + 1 in one launch (k_finish_plan, finish_plan.hip).

Every test compares bits: a chained step does the same work in the same order, only in another launch.  The batches of a chain
differ in B, N and E, so the merged launch's grid composition and every plan block's share of the arena change from step to step.
"""
import argparse
import random

import pytest
import torch

from oracle import cal_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
MERGED, FINISH_ONLY, PLAN = "k_finish_plan", "k_finish_plan(finish)", "k_plan_graph"


def _args(**kw):
    d = dict(layers=2, hidden=64, with_random=True, without_node_attention=False, without_edge_attention=False, fc_num="222",
             cat_or_add="add", c=0.5, o=1.0, co=0.5)
    d.update(kw)
    return argparse.Namespace(**d)


def _graph(n, gen, chords):
    """A ring of n nodes with `chords` random chords, both directions of every edge, no self loops."""
    from cal_amd.data import Data
    und = {(i, (i + 1) % n) for i in range(n)}
    while len(und) < n + chords:
        a, b = (int(v) for v in torch.randint(0, n, (2,), generator=gen))
        if a != b and (b, a) not in und:
            und.add((a, b))
    und = sorted(und)
    ei = torch.tensor([[a for a, b in und] + [b for a, b in und], [b for a, b in und] + [a for a, b in und]], dtype=torch.long)
    return Data(x=torch.randn(n, 10, generator=gen), edge_index=ei, y=torch.randint(0, 4, (1,), generator=gen))


def _batch(sizes, seed, pack=False):
    from cal_amd.data import Batch
    gen = torch.Generator().manual_seed(seed)
    return Batch.from_data_list([_graph(n, gen, chords=n // 3 + k) for k, n in enumerate(sizes)], pack=pack).to(DEV)


def _three(pack_second=False):
    """Three batches of 3-6 graphs of 8-40 nodes: B, N and E all differ."""
    return [_batch([8, 40, 17, 23], 1), _batch([33, 9, 12, 40, 26, 15], 2, pack=pack_second), _batch([21, 38, 11], 3)]


def _trainer(name, batches, chain=True, tiles=None):
    from cal_amd import model as M
    from cal_amd.trainer import CausalTrainer
    torch.manual_seed(3)
    sd = O.init_state(name, 10, 4, hidden=64, layers=2, heads=4)
    random.seed(7)
    m = getattr(M, name)(10, 4, _args())
    m.load_state_dict({k: v.clone() for k, v in sd.items()})
    tr = CausalTrainer(m.to(DEV), _args(), lr=1e-2, use_graph=True)
    if not chain:
        tr.engine.set_chain(False)
    if tiles is not None:
        tr.engine.tiles = tiles
    tr.reserve_for(batches)
    for b in batches:
        tr.prepare(b)
    return m, tr


def _rewind(m, tr, snap):
    m.load_state_dict(snap)
    tr.engine.exp_avg.zero_(); tr.engine.exp_avg_sq.zero_(); tr.engine.step_count.zero_()
    tr._perm_counter.zero_()
    if tr.engine.heads:
        tr.engine.gat_ctr.zero_()


def _state(m, tr, stats):
    out = {"stats": stats.clone(), "p": tr.flat_p.clone(), "m1": tr.engine.exp_avg.clone(), "m2": tr.engine.exp_avg_sq.clone(),
           "step": tr.engine.step_count.clone(), "ctr": tr._perm_counter.clone()}
    for k, v in m.state_dict().items():
        if "running_" in k or "num_batches_tracked" in k:
            out["bn." + k] = v.clone()
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _run(name, batches, seq, chain=True, passes=1, tiles=None):
    """`passes` passes over the batches from a fresh model: one step_sequence launch per pass, or single steps.  Returns the
    final state and the launch names of the sequence's capture."""
    m, tr = _trainer(name, batches, chain=chain, tiles=tiles)
    snap = {k: v.clone() for k, v in m.state_dict().items()}
    _rewind(m, tr, snap)
    log = []
    if seq:
        tr.engine.launch_log = log
        tr.step_sequence(batches)              # the capture (and one real pass): rewind what it changed
        tr.engine.launch_log = None
        _rewind(m, tr, snap)
    for _ in range(passes):
        if seq:
            stats = tr.step_sequence(batches)
        else:
            for b in batches:
                stats = tr.step(b)
    torch.cuda.synchronize()
    tr.check_status()
    return _state(m, tr, stats), [n for names in log for n in names]


def _counts(names):
    return names.count(PLAN), names.count(MERGED), names.count(FINISH_ONLY), names.count("k_finish")


def test_chain_equals_single_steps():
    """Three chained steps against the same three step() calls, and what was launched: one stand-alone plan, two merged launches,
    one finish-only launch -- so the test cannot pass by not chaining."""
    bs = _three()
    assert len({b.num_graphs for b in bs}) == 3 and len({b.x.size(0) for b in bs}) == 3 and len({b.edge_index.size(1) for b in bs}) == 3
    ref, _ = _run("CausalGCN", bs, seq=False)
    got, names = _run("CausalGCN", bs, seq=True)
    assert _counts(names) == (1, 2, 1, 0), names
    assert float(got["step"]) == 3.0 and int(got["ctr"]) == 3
    _same(ref, got)


def test_chain_replayed_twice():
    """The captured chain replayed twice equals two passes of single steps: nothing survives a replay in the words between the steps."""
    bs = _three()
    ref, _ = _run("CausalGCN", bs, seq=False, passes=2)
    got, _ = _run("CausalGCN", bs, seq=True, passes=2)
    assert float(got["step"]) == 6.0 and int(got["ctr"]) == 6
    _same(ref, got)


def test_chain_self_loop_in_the_middle_batch():
    """A self loop in batch 2 (which declares none): found by the plan part of step 1's last launch.  Step 1 still updates, steps 2
    and 3 do not, and the counter, the message and the parameters are the unchained run's."""
    from cal_amd._lib import CalError
    res = []
    for chain in (True, False):
        bs = _three()
        ei = bs[1].edge_index
        ei[1, 5] = ei[0, 5]
        m, tr = _trainer("CausalGCN", bs, chain=chain)          # (the warm-up steps of batch 2 are flagged, and restored)
        with pytest.raises(CalError):
            tr.check_status()
        snap = {k: v.clone() for k, v in m.state_dict().items()}
        _rewind(m, tr, snap)
        p0 = tr.flat_p.clone()
        log = tr.engine.launch_log = []
        stats = tr.step_sequence(bs)
        torch.cuda.synchronize()
        with pytest.raises(CalError) as exc:
            tr.check_status()
        res.append((_state(m, tr, stats), str(exc.value), [n for names in log for n in names], p0))
        tr.check_status()                                       # cleared: the pending words too
    (a, msg_a, names_a, p0), (b, msg_b, names_b, _) = res
    assert _counts(names_a) == (1, 2, 1, 0) and _counts(names_b) == (3, 0, 0, 3)
    assert "self loops" in msg_a and msg_a == msg_b
    assert float(a["step"]) == 1.0 and not torch.equal(a["p"], p0)
    for k in ("p", "m1", "m2", "step", "ctr"):
        assert torch.equal(a[k], b[k]), k
    # step 1 alone leaves the same parameters: steps 2 and 3 changed nothing
    one, _ = _run("CausalGCN", _three()[:1], seq=False)
    assert torch.equal(one["p"], a["p"]) and torch.equal(one["m1"], a["m1"]) and torch.equal(one["m2"], a["m2"])


def test_chain_packed_second_member():
    """A packed batch (tiles of consecutive graphs) as the chain's second member."""
    def batches():
        bs = _three(pack_second=True)
        assert bs[1].tile_ptr is not None
        bs[0].tile_ptr = None; bs[2].tile_ptr = None            # only the second member runs on tiles
        return bs
    ref, _ = _run("CausalGCN", batches(), seq=False, tiles="force")
    got, names = _run("CausalGCN", batches(), seq=True, tiles="force")
    assert _counts(names) == (1, 2, 1, 0), names
    _same(ref, got)


def test_chain_gat():
    """CausalGAT: the plan part also moves the attention-dropout tick."""
    bs = _three()
    ref, _ = _run("CausalGAT", bs, seq=False)
    got, names = _run("CausalGAT", bs, seq=True)
    assert _counts(names) == (1, 2, 1, 0), names
    _same(ref, got)


def test_chain_falls_back_for_the_wide_plan():
    """A successor with a graph above 128 nodes takes the 1024-thread plan, which stays a launch of its own: same bits, and no
    merged launch towards it (the step behind it starts a chain of its own)."""
    bs = [_batch([8, 40, 17, 23], 1), _batch([140, 9, 12], 2), _batch([21, 38, 11], 3)]
    ref, _ = _run("CausalGCN", bs, seq=False)
    got, names = _run("CausalGCN", bs, seq=True)
    assert _counts(names) == (2, 1, 1, 1), names               # step 1: k_finish; batch 2: its own plan, then chained to batch 3
    assert names.index("k_finish") < names.index(MERGED)
    _same(ref, got)


def test_chain_switched_off(monkeypatch):
    """CAL_AMD_CHAIN=0: no merged launch, same bits."""
    bs = _three()
    ref, _ = _run("CausalGCN", bs, seq=False)
    monkeypatch.setenv("CAL_AMD_CHAIN", "0")
    got, names = _run("CausalGCN", bs, seq=True)
    assert _counts(names) == (3, 0, 0, 3), names
    _same(ref, got)


def test_chain_refuses_another_step():
    """After a step that planned its successor, a call for any other batch is refused and enqueues nothing; the announced step
    then runs, ends the chain, and the three steps equal unchained ones."""
    from cal_amd import _lib, model as M
    from cal_amd.engine import StepEngine
    bs = _three()
    res = []
    for chain in (True, False):
        torch.manual_seed(3)
        sd = O.init_state("CausalGCN", 10, 4, hidden=64, layers=2)
        m = M.CausalGCN(10, 4, _args())
        m.load_state_dict({k: v.clone() for k, v in sd.items()})
        eng = StepEngine(m.to(DEV).train(), lr=1e-2)
        eng.reserve(max(b.x.size(0) for b in bs), max(b.edge_index.size(1) for b in bs), 6)
        eng.launch_log = []
        eng.train_step(bs[0], next_batch=bs[1] if chain else None)
        if chain:
            assert eng.launch_log[-1][-1] == MERGED
            before = _lib.query("cal_launch_count")
            with pytest.raises(_lib.CalError, match="planned another batch"):
                eng.train_step(bs[2])
            assert _lib.query("cal_launch_count") == before
        eng.train_step(bs[1])
        if chain:
            assert eng.launch_log[-1][-1] == FINISH_ONLY and PLAN not in eng.launch_log[-1]
        eng.train_step(bs[2])
        torch.cuda.synchronize()
        eng.check_status()
        res.append((eng.flat_p.clone(), eng.exp_avg.clone(), eng.exp_avg_sq.clone(), eng.step_count.clone()))
    for x, y in zip(*res):
        assert torch.equal(x, y)
    assert float(res[0][3]) == 3.0

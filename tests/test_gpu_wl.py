"""Weisfeiler-Lehman signatures on the MI355X: cal_wl_refine / cal_wl_match (csrc/wl.hip) against the plain-int restatement and
the host twin bit for bit -- the sizes of the CPU tests, node counts at the LDS cap and one above it (the rounds through global
memory), a three-node hub of 5000 columns (contended LDS atomics), max_nodes below a graph, the empty shapes -- the launch
counts, identical bits on a repeated call, explanation_census of engine-backed models against the census of the same mask on the
CPU, and the state a call leaves behind."""
import argparse
import random

import numpy as np
import pytest
import torch

from cal_amd import _lib, spmotif
from cal_amd.data import Batch
from cal_amd.wl import eval_explanation_census, subgraph_census, wl_match, wl_refine, wl_similarity
from oracle import cal_oracle as O
from tests.test_wl import SIZES, check_match, check_refine, graphs_batch, labels_for, raw_batch, sqrt_samples
from tests.twin_oracle import make_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(b):
    d = Batch()
    for k, v in b.__dict__.items():
        d.__dict__[k] = v.to(DEV) if torch.is_tensor(v) else v
    d._plan = None
    return d


def sized_graphs(ns, seed):
    """Graphs of ``ns[g]`` nodes: a ring in both directions, n // 3 chords in one direction, a few duplicates and self loops,
    columns shuffled -> (edge_index, ptr, edge_ptr)."""
    rng = np.random.default_rng(seed)
    gs = []
    for n in ns:
        cols = []
        if n >= 2:
            cols += [(i, (i + 1) % n) for i in range(n)] + [((i + 1) % n, i) for i in range(n)]
            cols += [tuple(int(x) for x in rng.integers(0, n, 2)) for _ in range(n // 3)]
            cols += cols[:3] + [(0, 0), (n - 1, n - 1)]
        ei = np.array(cols, dtype=np.int64).reshape(-1, 2)
        gs.append((n, ei[rng.permutation(len(cols))].T.copy()))
    return graphs_batch(gs)


def both(ei, ptr, eptr, T, init=None, max_nodes=None):
    """The device result against the restatement and the host twin, for both entry points -> the device ``WLColors``."""
    lab = None if init is None else torch.as_tensor(init)
    b = raw_batch(ei, ptr, eptr, max_nodes=max_nodes)
    before = _lib.query("cal_launch_count")
    res = wl_refine(_dev(b), iters=T, labels=None if lab is None else lab.to(DEV))
    assert _lib.query("cal_launch_count") - before == (1 if len(ptr) > 1 else 0)
    assert res.colors.is_cuda and res.hash.is_cuda and res.ignored.is_cuda
    check_refine(res, ei, ptr, eptr, T, init=init, max_nodes=max_nodes)
    host = wl_refine(b, iters=T, labels=lab)
    assert torch.equal(res.colors.cpu(), host.colors) and torch.equal(res.hash.cpu(), host.hash)
    assert torch.equal(res.ignored.cpu(), host.ignored)
    return res, host


PROTO = make_batch([5, 0, 12, 40], seed=9, stray=False)


def match_both(res, host, T, with_init, max_nodes_a=None):
    pinit = labels_for(int(PROTO[1][-1]), 6) if with_init else None
    lab = None if pinit is None else torch.as_tensor(pinit)
    pb = raw_batch(*PROTO)
    pd, ph = wl_refine(_dev(pb), iters=T, labels=None if lab is None else lab.to(DEV)), wl_refine(pb, iters=T, labels=lab)
    assert torch.equal(pd.colors.cpu(), ph.colors)
    before = _lib.query("cal_launch_count")
    K, own = check_match(res, pd, max_nodes_a=max_nodes_a)
    assert _lib.query("cal_launch_count") - before == (1 if int(res.ptr.numel()) > 1 else 0)
    Kh, ownh = wl_match(host, ph)
    assert K.is_cuda and torch.equal(K.cpu(), Kh) and torch.equal(own.cpu(), ownh)
    return K, own


# ---- 1. bit for bit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [0, 3, 8])
@pytest.mark.parametrize("with_init", [False, True])
def test_hip_equals_restatement_and_host_twin(T, with_init):
    ei, ptr, eptr = make_batch(SIZES, seed=T)
    init = labels_for(int(ptr[-1]), 5) if with_init else None
    res, host = both(ei, ptr, eptr, T, init=init)
    assert int(res.ignored.cpu()[0]) == 1
    K, _ = match_both(res, host, T, with_init)
    assert int(K.sum()) > 0


@pytest.mark.parametrize("ns", [[2048, 5, 300], [5, 2049, 100]], ids=["at_cap", "above_cap"])
def test_hip_at_the_lds_cap_and_above(ns):
    """2048 nodes: the four LDS arrays are full; 2049: that graph's rounds run through the rows of colors and the workspace,
    beside graphs that stay in LDS in the same launch; the match sorts 2048 colours in LDS / compares every pair of 2049."""
    assert _lib.query("cal_explain_lds_cap") == 2048
    ei, ptr, eptr = sized_graphs(ns, seed=3)
    init = labels_for(int(ptr[-1]), 8) % 2
    for T, lab in ((3, None), (2, init)):
        res, host = both(ei, ptr, eptr, T, init=lab)
        match_both(res, host, T, lab is not None)
    again = wl_refine(_dev(raw_batch(ei, ptr, eptr)), iters=2, labels=torch.as_tensor(init).to(DEV))
    assert torch.equal(again.colors, res.colors) and torch.equal(again.hash, res.hash)      # (the workspace is reused)


def test_hip_hub_contention_and_small_next_to_large_instantiation():
    """Three nodes, 5000 columns (self loops included): every atomic of a round lands on one of six words."""
    rng = np.random.default_rng(1)
    hub = rng.integers(0, 3, (2, 5000)).astype(np.int64)
    for extra in ([], [(300, np.zeros((2, 0)))]):                          # 256-thread and 1024-thread workgroups
        ei, ptr, eptr = graphs_batch([(3, hub), (2, np.array([[0], [1]]))] + extra)
        res, host = both(ei, ptr, eptr, 3)
        match_both(res, host, 3, False)


def test_hip_max_nodes_below_a_graph():
    ei, ptr, eptr = make_batch([30, 200, 8], seed=2)
    cut = int(np.diff(ptr).max()) - 1
    res, host = both(ei, ptr, eptr, 2, max_nodes=cut)
    assert int(res.hash[1].abs().sum()) == 0 and int(res.hash[0].abs().min()) > 0
    full, fhost = both(ei, ptr, eptr, 2)
    match_both(full._replace(max_nodes=cut), fhost._replace(max_nodes=cut), 2, False, max_nodes_a=cut)


def test_hip_empty_shapes():
    none = np.zeros((2, 0), dtype=np.int64)
    both(none, [0], [0], 2)                                                 # B = 0: nothing is launched
    res, host = both(none, [0, 0, 0], [0, 0, 0], 2)                         # N = 0: the empty graph's hash, twice
    assert int(res.hash[0, 2]) & ((1 << 64) - 1) == 0x706430794531A862
    match_both(res, host, 2, False)
    res, host = both(none, [0, 4, 4, 9], [0, 0, 0, 0], 8)                   # E = 0
    K, own = match_both(res, host, 8, False)
    assert own.cpu().tolist() == [[16] * 9, [0] * 9, [25] * 9]


# ---- 2. / 3. launches and repeated calls --------------------------------------------------------------------------------------
def test_one_launch_each_and_the_same_bits_twice():
    b = _dev(Batch.from_data_list(spmotif.train_mix(12, node_num=7, seed=3)))
    protos = spmotif.motif_batch(DEV)
    n0 = _lib.query("cal_launch_count")
    a1, p1 = wl_refine(b, iters=3, labels="argmax"), wl_refine(protos, iters=3)
    n1 = _lib.query("cal_launch_count")
    a0 = wl_refine(b, iters=3)
    m1, m2 = wl_match(a0, p1), wl_match(a0, p1)
    n2 = _lib.query("cal_launch_count")
    assert (n1 - n0, n2 - n1) == (2, 3)
    a2 = wl_refine(b, iters=3, labels="argmax")
    assert torch.equal(a1.colors, a2.colors) and torch.equal(a1.hash, a2.hash) and torch.equal(a1.ignored, a2.ignored)
    assert torch.equal(m1[0], m2[0]) and torch.equal(m1[1], m2[1])
    lab = b.feat.argmax(1)
    assert torch.equal(wl_refine(b, iters=3, labels=lab).hash, a1.hash) and not torch.equal(a1.hash, a0.hash)
    assert torch.equal(wl_similarity(a0, p1).cpu(), wl_similarity(wl_refine(b.to("cpu"), iters=3), wl_refine(spmotif.motif_batch(), iters=3)))


def test_the_similaritys_root_has_the_cpus_bits():
    from cal_amd.wl import _sqrt_rounded
    d = sqrt_samples()
    assert np.array_equal(_sqrt_rounded(torch.as_tensor(d).to(DEV)).cpu().numpy(), np.sqrt(d))


# ---- 4. / 5. the census of engine-backed models -------------------------------------------------------------------------------
def _args(**kw):
    d = dict(layers=2, hidden=32, with_random=True, without_node_attention=False, without_edge_attention=False,
             fc_num="222", cat_or_add="add", c=0.5, o=1.0, co=0.5)
    d.update(kw)
    return argparse.Namespace(**d)


def _gpu_model(name, args, seed=0):
    from cal_amd import model as M
    torch.manual_seed(seed)
    sd = O.init_state(name, 10, 4, hidden=args.hidden, layers=args.layers, heads=4, cat_or_add=args.cat_or_add)
    m = getattr(M, name)(10, 4, args)
    m.load_state_dict(sd, strict=name != "CausalGIN")
    return m.to(DEV)


@pytest.mark.parametrize("name", ["CausalGCN", "CausalGAT", "CausalGIN"])
def test_explanation_census_of_an_engine_backed_model(name):
    m = _gpu_model(name, _args())
    assert m.engine() is not None
    b = Batch.from_data_list(spmotif.train_mix(6, node_num=7, seed=11))
    bd = _dev(b)
    protos = spmotif.motif_batch()
    res = m.explanation_census(bd, ratio=0.3, prototypes=spmotif.motif_batch(DEV))
    m.engine().check_status()
    assert res["hash"].is_cuda and res["sim"].is_cuda and res["yhat"].shape == (6,) and torch.equal(res["y"].cpu(), b.y.view(-1))
    mask = res["explanation"].edge_mask.cpu()
    want = subgraph_census(b, edge_mask=mask, prototypes=protos)
    for key in ("hash", "nodes", "edges", "exact", "nearest", "sim"):
        assert torch.equal(res[key].cpu(), want[key]), key
    assert res["sim"].dtype == torch.float64 and int(res["edges"].sum()) == int(mask.sum()) > 0


def test_the_census_leaves_the_engines_state_untouched():
    from cal_amd.data import DataLoader
    from cal_amd.engine import StepEngine
    m = _gpu_model("CausalGCN", _args())
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
    protos = spmotif.motif_batch(DEV)
    res = m.explanation_census(Batch.from_data_list(gs[:6]).to(DEV), k=6, prototypes=protos)
    ev = eval_explanation_census(m, DataLoader(gs, batch_size=8, shuffle=False), DEV, k="gt", prototypes=protos)
    assert res["exact"].shape == (6, 4) and ev["graphs"] == 12 and 0.0 <= ev["exact_rate"] <= 1.0
    assert sum(c["graphs"] for c in ev["by_label"].values()) == 12 == sum(c["graphs"] for c in ev["by_prediction"].values())
    torch.cuda.synchronize()
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

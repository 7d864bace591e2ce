"""Weisfeiler-Lehman signatures on the CPU: the host twins of cal_wl_refine / cal_wl_match against the plain-int restatement bit
for bit, the known answers of the restatement, the invariances of the contract, the motif hashes and the limit of 1-WL, the census
on SPMotif's ground truth (a condition, not a tolerance), wl_similarity of the prototypes and eval_explanation_census against the
tally of its per-batch calls."""
import argparse
import subprocess

import numpy as np
import pytest
import torch

from cal_amd import _lib, spmotif, wl
from cal_amd.data import Batch, Data, DataLoader
from cal_amd.wl import eval_explanation_census, subgraph_census, wl_match, wl_refine, wl_similarity
from oracle import cal_oracle as O
from tests import wl_oracle as WO
from tests.twin_oracle import make_batch
from tests.wl_oracle import both_directions, wl_match_oracle, wl_refine_oracle, wl_similarity_oracle

SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257]
SYMBOLS = ("cal_wl_ws", "cal_wl_refine", "cal_wl_match")
M64 = (1 << 64) - 1


def raw_batch(ei, ptr, eptr, max_nodes=None):
    """A ``Batch`` over the arrays of ``make_batch`` (no features): the layout facts as given."""
    ptr, eptr = np.asarray(ptr, dtype=np.int64), np.asarray(eptr, dtype=np.int64)
    b = Batch()
    b.edge_index = torch.as_tensor(np.asarray(ei, dtype=np.int64).reshape(2, -1)).contiguous()
    b.ptr, b.edge_ptr = torch.as_tensor(ptr), torch.as_tensor(eptr)
    b.num_graphs = len(ptr) - 1
    n = np.diff(ptr)
    b.batch = torch.repeat_interleave(torch.arange(b.num_graphs), torch.as_tensor(n))
    b.max_nodes = int(n.max()) if max_nodes is None and n.size else int(max_nodes or 0)
    b.max_edges = int(np.diff(eptr).max()) if eptr.size > 1 else 0
    return b


def graphs_batch(graphs):
    """``graphs``: a list of (n, [2, m] local columns) -> (edge_index, ptr, edge_ptr)."""
    ptr, eptr, cols = [0], [0], []
    for n, ei in graphs:
        ei = np.asarray(ei, dtype=np.int64).reshape(2, -1)
        cols.append(ei + ptr[-1])
        ptr.append(ptr[-1] + n)
        eptr.append(eptr[-1] + ei.shape[1])
    return np.concatenate(cols, 1) if cols else np.zeros((2, 0), dtype=np.int64), np.array(ptr), np.array(eptr)


def motif(name):
    n, edges = spmotif._MOTIFS[name]
    return n, both_directions(edges)


def check_refine(res, ei, ptr, eptr, T, init=None, max_nodes=None):
    """``res`` (a ``WLColors`` on any device) against the restatement, bit for bit -> the restatement's (colors, hash)."""
    N = int(ptr[-1])
    col, hs, ign = wl_refine_oracle(ei, ptr, eptr, N, T, init=init, max_nodes=max_nodes)
    assert res.colors.shape == (T + 1, N) and res.hash.shape == (len(ptr) - 1, T + 1)
    assert np.array_equal(res.colors.cpu().numpy(), col)
    assert np.array_equal(res.hash.cpu().numpy(), hs)
    assert int(res.ignored.cpu()[0]) == ign
    return col, hs


def check_match(a, p, max_nodes_a=None):
    K, own = wl_match(a, p)
    wantK, want_own = wl_match_oracle(a.colors.cpu().numpy(), a.ptr.cpu().numpy(), p.colors.cpu().numpy(), p.ptr.cpu().numpy(),
                                      max_nodes_a=max_nodes_a)
    assert np.array_equal(K.cpu().numpy(), wantK) and np.array_equal(own.cpu().numpy(), want_own)
    return K, own


def labels_for(N, seed):
    return np.random.default_rng(seed).integers(-3, 4, N).astype(np.int64)


# ---- 1. host == restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [0, 1, 3, 8])
@pytest.mark.parametrize("with_init", [False, True])
def test_host_twin_equals_restatement(T, with_init):
    ei, ptr, eptr = make_batch(SIZES, seed=T)
    b = raw_batch(ei, ptr, eptr)
    init = labels_for(int(ptr[-1]), 5) if with_init else None
    res = wl_refine(b, iters=T, labels=None if init is None else torch.as_tensor(init))
    check_refine(res, ei, ptr, eptr, T, init=init)
    assert int(res.ignored[0]) == 1                                         # make_batch's one stray column
    pei, pptr, peptr = make_batch([5, 0, 12, 40], seed=9, stray=False)
    pinit = labels_for(int(pptr[-1]), 6) if with_init else None
    protos = wl_refine(raw_batch(pei, pptr, peptr), iters=T, labels=None if pinit is None else torch.as_tensor(pinit))
    K, own = check_match(res, protos)
    assert int(K.sum()) > 0 and torch.equal(check_match(res, res)[1], own)


def test_abi_symbols_and_constants():
    protos = _lib.parse_header()
    for path in (_lib.LIB_PATH, _lib.HOST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
        assert set(SYMBOLS) <= exported, path
    assert set(SYMBOLS) <= set(protos) and set(SYMBOLS) <= set(_lib.HOST_SYMBOLS)
    assert len(protos["cal_wl_refine"][1]) == 15 and len(protos["cal_wl_match"][1]) == 15 and len(protos["cal_wl_ws"][1]) == 3
    text = open(_lib.HEADER).read()
    for name in ("INIT", "SELF", "OUT", "IN", "NODE", "GRAPH"):
        assert "#define CAL_WL_C_%s 0x%016XULL" % (name, getattr(WO, "C_" + name)) in text
        assert getattr(wl, "C_" + name) == getattr(WO, "C_" + name)
    assert WO.sm(0) == 0xE220A8397B1DCDAF                                   # the published first output of splitmix64 from state 0


def test_max_nodes_below_a_graph_and_the_prototype_limit():
    ei, ptr, eptr = make_batch([30, 200, 8], seed=2)
    n = np.diff(ptr)
    cut = int(n.max()) - 1
    res = wl_refine(raw_batch(ei, ptr, eptr, max_nodes=cut), iters=2)
    _, hs = check_refine(res, ei, ptr, eptr, 2, max_nodes=cut)
    assert (hs[1] == 0).all() and (hs[0] != 0).all()
    full = wl_refine(raw_batch(ei, ptr, eptr), iters=2)
    check_match(full._replace(max_nodes=cut), full, max_nodes_a=cut)
    big = wl_refine(raw_batch(np.zeros((2, 0)), [0, 4097], [0, 0]), iters=2)
    with pytest.raises(_lib.CalError, match="4096"):
        wl_match(full, big)
    with pytest.raises(ValueError):
        wl_match(full, wl_refine(raw_batch(ei, ptr, eptr), iters=3))


# ---- 2. the known answers -----------------------------------------------------------------------------------------------------
def test_known_answers():
    one = wl_refine(raw_batch(np.zeros((2, 0)), [0, 1], [0, 0]), iters=0)
    assert int(one.hash[0, 0]) & M64 == 0xA3DC1D888C9A744B
    ei, ptr, eptr = graphs_batch([(0, np.zeros((2, 0))), motif("house"), (0, np.zeros((2, 0)))])
    res = wl_refine(raw_batch(ei, ptr, eptr), iters=3)
    assert int(res.hash[0, 2]) & M64 == 0x706430794531A862 and torch.equal(res.hash[0], res.hash[2])
    assert [int(h) & M64 for h in res.hash[1]] == [0x5B23C9FF36BEFE7B, 0x5FD635CED7D1A7C3, 0xD53F6B1F5291D717, 0xB159AD2DCBE99EE8]
    none = wl_refine(raw_batch(np.zeros((2, 0)), [0, 0, 0], [0, 0, 0]), iters=3)     # N = 0, B = 2
    assert [int(h) & M64 for h in none.hash[:, 2]] == [0x706430794531A862] * 2 and none.colors.shape == (4, 0)
    empty = wl_refine(raw_batch(np.zeros((2, 0)), [0], [0]), iters=2)                 # B = 0
    assert empty.hash.shape == (0, 3) and int(empty.ignored[0]) == 0
    K, own = wl_match(none, res)
    assert K.shape == (2, 3, 4) and int(K.abs().sum()) == 0 and int(own.abs().sum()) == 0
    assert wl_similarity(none, res).tolist() == [[0.0] * 3] * 2


# ---- 3. invariances -----------------------------------------------------------------------------------------------------------
def test_invariances():
    rng = np.random.default_rng(4)
    ei, ptr, eptr = make_batch([40, 7, 90, 0, 33], seed=11)
    N, T = int(ptr[-1]), 3
    init = labels_for(N, 1)
    base = wl_refine(raw_batch(ei, ptr, eptr), iters=T, labels=torch.as_tensor(init))
    # shuffled columns inside every graph
    sh = ei.copy()
    for g in range(len(ptr) - 1):
        lo, hi = int(eptr[g]), int(eptr[g + 1])
        sh[:, lo:hi] = ei[:, lo + rng.permutation(hi - lo)]
    res = wl_refine(raw_batch(sh, ptr, eptr), iters=T, labels=torch.as_tensor(init))
    assert torch.equal(res.colors, base.colors) and torch.equal(res.hash, base.hash)
    # permuted nodes inside every graph: new id of node v is perm[v]
    perm = np.arange(N)
    for g in range(len(ptr) - 1):
        lo, hi = int(ptr[g]), int(ptr[g + 1])
        perm[lo:hi] = lo + rng.permutation(hi - lo)
    ok = (ei >= 0) & (ei < N)
    pe = np.where(ok, perm[np.clip(ei, 0, N - 1)], ei)
    pinit = np.empty_like(init)
    pinit[perm] = init
    res = wl_refine(raw_batch(pe, ptr, eptr), iters=T, labels=torch.as_tensor(pinit))
    assert torch.equal(res.hash, base.hash) and torch.equal(res.colors[:, torch.as_tensor(perm)], base.colors)
    # a graph alone (graph 2; its stray-free columns)
    g = 2
    lo, hi, nlo, nhi = int(eptr[g]), int(eptr[g + 1]), int(ptr[g]), int(ptr[g + 1])
    alone = wl_refine(raw_batch(ei[:, lo:hi] - nlo, [0, nhi - nlo], [0, hi - lo]), iters=T, labels=torch.as_tensor(init[nlo:nhi]))
    assert torch.equal(alone.hash[0], base.hash[g]) and torch.equal(alone.colors, base.colors[:, nlo:nhi])
    # ungrouped columns: a foreign batch (edge_index, batch, num_graphs) with the columns of all graphs interleaved
    ei, ptr, eptr = make_batch([40, 7, 90, 0, 33], seed=11, stray=False)
    grouped = wl_refine(raw_batch(ei, ptr, eptr), iters=T, labels=torch.as_tensor(init))
    mixed = Data(edge_index=torch.as_tensor(ei[:, rng.permutation(ei.shape[1])]).contiguous())
    mixed.batch, mixed.num_graphs = torch.repeat_interleave(torch.arange(len(ptr) - 1), torch.as_tensor(np.diff(ptr))), len(ptr) - 1
    res = wl_refine(mixed, iters=T, labels=torch.as_tensor(init))
    assert torch.equal(res.hash, grouped.hash) and torch.equal(res.colors, grouped.colors)


# ---- 4. the motifs, and what 1-WL cannot see ----------------------------------------------------------------------------------
def test_motif_hashes_and_the_limit_of_1wl():
    mb = spmotif.motif_batch()
    assert mb.num_graphs == 4 and mb.ptr.tolist() == [0, 5, 11, 17, 23] and mb.edge_ptr.tolist() == [0, 12, 24, 38, 54]
    for c, s in enumerate(spmotif.CLASS_LIST):
        lo, hi = int(mb.edge_ptr[c]), int(mb.edge_ptr[c + 1])
        assert np.array_equal((mb.edge_index[:, lo:hi] - int(mb.ptr[c])).numpy(), motif(s)[1])
    res = wl_refine(mb, iters=3)
    check_refine(res, mb.edge_index.numpy(), mb.ptr.numpy(), mb.edge_ptr.numpy(), 3)
    for t in (1, 2, 3):
        assert len(set(res.hash[:, t].tolist())) == 4
    assert len(set(res.hash[1:, 0].tolist())) == 1 and int(res.hash[0, 0]) != int(res.hash[1, 0])
    tri = [(0, 1), (1, 2), (2, 0)]
    ei, ptr, eptr = graphs_batch([motif("cycle"), (6, both_directions(tri + [(a + 3, b + 3) for a, b in tri]))])
    two = wl_refine(raw_batch(ei, ptr, eptr), iters=8)
    assert torch.equal(two.hash[0], two.hash[1])                            # WL-equivalent, not isomorphic
    assert wl_similarity(two, two).tolist() == [[1.0, 1.0], [1.0, 1.0]]


# ---- 5. the census on the ground truth ----------------------------------------------------------------------------------------
def _spmotif_batch(per_class=3, seed=5):
    ds = spmotif.generate_dataset(per_class, node_num=4, seed=seed)
    gs = [g for ctx in ("tree", "ba") for s in spmotif.CLASS_LIST for g in ds[ctx][s]]
    return Batch.from_data_list(gs)


def test_census_of_the_ground_truth_is_the_motif():
    b = _spmotif_batch()
    B = b.num_graphs
    gt = spmotif.ground_truth(b)[1]
    protos = spmotif.motif_batch()
    res = subgraph_census(b, edge_mask=gt, prototypes=protos)
    y = b.y.view(-1)
    assert res["exact"].shape == (B, 4) and res["exact"][torch.arange(B), y].all()
    assert int(res["exact"].sum()) == B                                     # ... and to no other prototype
    assert torch.equal(res["nearest"], y)
    assert (res["sim"][torch.arange(B), y] == 1.0).all()
    sizes = torch.tensor([spmotif._MOTIFS[s][0] for s in spmotif.CLASS_LIST])
    edges = torch.tensor([2 * len(spmotif._MOTIFS[s][1]) for s in spmotif.CLASS_LIST])
    assert torch.equal(res["nodes"], sizes[y]) and torch.equal(res["edges"], edges[y])
    assert torch.equal(res["hash"], wl_refine(protos, iters=3).hash[y, -1])
    # one ground-truth undirected edge removed from every graph's mask
    cut = gt.clone()
    ei = b.edge_index
    for g in range(B):
        lo, hi = int(b.edge_ptr[g]), int(b.edge_ptr[g + 1])
        e = lo + int(gt[lo:hi].nonzero()[0])
        u, v = int(ei[0, e]), int(ei[1, e])
        cut[e] = False
        cut[lo + int(((ei[0, lo:hi] == v) & (ei[1, lo:hi] == u)).nonzero()[0])] = False
    res = subgraph_census(b, edge_mask=cut, prototypes=protos)
    assert not res["exact"][torch.arange(B), y].any() and (res["sim"][torch.arange(B), y] < 1.0).all()
    # nothing kept: no node, no nearest prototype, similarity 0
    res = subgraph_census(b, edge_mask=torch.zeros_like(gt), prototypes=protos)
    assert (res["nearest"] == -1).all() and int(res["sim"].abs().sum()) == 0 and not res["exact"].any()
    assert int(res["nodes"].sum()) == 0 and len(set(res["hash"].tolist())) == 1


# ---- 6. similarity of the prototypes ------------------------------------------------------------------------------------------
def test_similarity_of_the_prototypes():
    res = wl_refine(spmotif.motif_batch(), iters=3)
    sim = wl_similarity(res, res)
    assert sim.dtype == torch.float64 and torch.equal(sim, sim.t()) and torch.equal(sim.diagonal(), torch.ones(4, dtype=torch.float64))
    K, own = check_match(res, res)
    want = wl_similarity_oracle(K.numpy(), own.numpy(), own.numpy())
    assert np.array_equal(sim.numpy(), want)
    assert round(float(sim[0, 2]), 3) == 0.900 and round(float(sim[1, 3]), 3) == 0.408
    part = wl_similarity(res, res, depths=(0, 2))
    assert np.array_equal(part.numpy(), wl_similarity_oracle(K.numpy(), own.numpy(), own.numpy(), depths=(0, 2)))
    assert float(part[1, 2]) != float(sim[1, 2])


def sqrt_samples():
    rng = np.random.default_rng(0)
    return np.concatenate([rng.integers(1, 1 << 20, 100000), rng.integers(1, 1 << 52, 100000), np.arange(1, 3000) ** 2]).astype(np.float64)


def test_the_similaritys_root_is_correctly_rounded_from_either_neighbour():
    """fp64 sqrt differs by an ulp between devices; ``_sqrt_rounded`` must give numpy's (correctly rounded) root whether it
    starts from that root or from the float on either side of it."""
    d = sqrt_samples()
    t, want = torch.as_tensor(d), np.sqrt(d)
    for to in (None, float("inf"), 0.0):
        x = None if to is None else torch.nextafter(t.sqrt(), torch.tensor(to, dtype=torch.float64))
        assert np.array_equal(wl._sqrt_rounded(t, x).numpy(), want)


# ---- 7. the drivers -----------------------------------------------------------------------------------------------------------
def _args(**kw):
    d = dict(layers=2, hidden=32, with_random=True, without_node_attention=False, without_edge_attention=False,
             fc_num="222", cat_or_add="add")
    d.update(kw)
    return argparse.Namespace(**d)


def _cpu_model(name, feat=10, seed=3):
    from cal_amd import model as M
    torch.manual_seed(seed)
    sd = O.init_state(name, feat, 4, hidden=32, layers=2, heads=4)
    m = getattr(M, name)(feat, 4, _args())
    m.load_state_dict(sd, strict=name != "CausalGIN")
    return m


def test_eval_explanation_census_is_the_tally_of_its_batches():
    import random
    m = _cpu_model("CausalGCN")
    m.train()
    gs = spmotif.train_mix(10, node_num=5, seed=4)
    protos = spmotif.motif_batch()
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    py0, t0 = random.getstate(), torch.get_rng_state()
    ev = eval_explanation_census(m, DataLoader(gs, batch_size=6, shuffle=False), "cpu", k="gt", prototypes=protos, top=2)
    parts = []
    for i in (0, 6):
        b = Batch.from_data_list(gs[i:i + 6])
        ngt, egt = spmotif.ground_truth(b)
        parts.append(m.explanation_census(b, k="gt", prototypes=protos, edge_gt=egt, node_gt=ngt))
    assert m.training and random.getstate() == py0 and torch.equal(torch.get_rng_state(), t0)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd0[k]), k
    hashes = [int(h) & M64 for p in parts for h in p["hash"].tolist()]
    ys = [int(v) for p in parts for v in p["y"].tolist()]
    yh = [int(v) for p in parts for v in p["yhat"].tolist()]
    where = [(b, g) for b, p in enumerate(parts) for g in range(int(p["hash"].numel()))]
    assert ev["graphs"] == 10 and ev["shapes"] == len(set(hashes))
    for key, cls in (("by_label", ys), ("by_prediction", yh)):
        assert sorted(ev[key]) == sorted(set(cls))
        for c, rep in ev[key].items():
            mine = [i for i, v in enumerate(cls) if v == c]
            cnt = {}
            for i in mine:
                cnt.setdefault(hashes[i], []).append(i)
            order = sorted(cnt.items(), key=lambda kv: (-len(kv[1]), kv[1][0]))[:2]
            assert rep["graphs"] == len(mine) and rep["shapes"] == len(cnt)
            assert [(t["hash"], t["count"], t["example"]) for t in rep["top"]] == [(h, len(v), where[v[0]]) for h, v in order]
            assert all(t["share"] == t["count"] / len(mine) for t in rep["top"])
    exact = torch.cat([p["exact"] for p in parts])
    sim = torch.cat([p["sim"] for p in parts])
    assert ev["exact"] == (exact.sum(0).double() / 10).tolist()
    assert max(abs(a - b) for a, b in zip(ev["sim"], sim.mean(0).tolist())) < 1e-12
    assert ev["exact_rate"] == sum(bool(exact[i, ys[i]]) for i in range(10)) / 10
    # the explanation at k = "gt" has as many undirected edges as the motif: its subgraph has the motif's column count
    for p in parts:
        want = torch.tensor([2 * len(spmotif._MOTIFS[s][1]) for s in spmotif.CLASS_LIST])[p["y"]]
        assert torch.equal(p["edges"], want) and p["explanation"].edge_mask.dtype == torch.bool

"""Exact motif matching on the CPU: the host twin of cal_motif_match against the plain-int restatement bit for bit and the
restatement against brute force over all injective maps; the fixed tables of the contract (automorphisms, the motifs in each
other, hexagon against two triangles, the star), the word boundaries of the bit rows, labels and the unsigned key, an 8-node
pattern, rejected patterns, the budget's edges, column order and batch layout, the empty shapes, the census on a hand-made mask
and eval_explanation_motifs on a CPU model.  Every case is a function of the device, so tests/test_gpu_motif.py runs the same
cases through the kernel."""
import subprocess

import numpy as np
import pytest
import torch

from cal_amd import _lib, motif, spmotif
from cal_amd.data import Batch, Data, DataLoader
from cal_amd.motif import (MotifPatterns, automorphisms, contains, eval_explanation_motifs, isomorphic, motif_census,
                           motif_match)
from cal_amd.wl import wl_refine
from tests import motif_oracle as MO
from tests.test_wl import _cpu_model, graphs_batch, raw_batch
from tests.wl_oracle import both_directions

NAMES = spmotif.CLASS_LIST                                                   # house, cycle, grid, diamond
TRI = [(0, 1), (1, 2), (2, 0)]
HEXAGON = (6, both_directions([(i, (i + 1) % 6) for i in range(6)]))
TWO_TRIANGLES = (6, both_directions(TRI + [(a + 3, b + 3) for a, b in TRI]))
TRIANGLE = (3, both_directions(TRI))
K4 = (4, both_directions([(a, b) for a in range(4) for b in range(a + 1, 4)]))
PATH3 = (3, both_directions([(0, 1), (1, 2)]))
EDGE = (2, both_directions([(0, 1)]))
DOT = (1, np.zeros((2, 0), dtype=np.int64))
SQUARE = (4, both_directions([(0, 1), (1, 2), (2, 3), (3, 0)]))
PATH8 = (8, both_directions([(i, i + 1) for i in range(7)]))
SIZES = [1, 2, 63, 64, 65, 128, 129, 255, 256]


def mot(name):
    n, edges = spmotif._MOTIFS[name]
    return n, both_directions(edges)


def star(n):
    return n, both_directions([(0, i) for i in range(1, n)])


def batch_of(graphs):
    return raw_batch(*graphs_batch(graphs))


def sparse_graph(n, rng):
    """A ring in both directions, n // 3 chords in one direction, a few duplicates and self loops, columns shuffled."""
    cols = []
    if n >= 2:
        cols += [(i, (i + 1) % n) for i in range(n)] + [((i + 1) % n, i) for i in range(n)]
        cols += [tuple(int(x) for x in rng.integers(0, n, 2)) for _ in range(n // 3)]
        cols += cols[:3] + [(0, 0), (n - 1, n - 1)]
    ei = np.array(cols, dtype=np.int64).reshape(-1, 2)
    return n, ei[rng.permutation(len(cols))].T.copy()


def to_dev(b, dev):
    """``b`` with its tensors on ``dev`` (``None``: as it is)."""
    if dev is None:
        return b
    d = type(b)()
    for k, v in b.__dict__.items():
        d.__dict__[k] = v.to(dev) if torch.is_tensor(v) else v
    if "_plan" in d.__dict__:
        d._plan = None
    return d


def as_np(m):
    return tuple(t.cpu().numpy() for t in m)


def run(b, pb, dev=None, labels=None, pattern_labels=None, induced=False, budget=motif.DEFAULT_BUDGET, oracle=True):
    """``motif_match`` of the CPU batch ``b`` against the CPU pattern batch ``pb`` by the host twin, checked against the
    restatement (grouped batches only); with ``dev`` also by the device, bit-equal to the host twin, with its launch count.
    -> the numpy arrays (count, first, truncated, tgt_edges, pat_edges, ignored) of the device's result (else the host's)."""
    kw = dict(induced=induced, budget=budget)
    lab = None if labels is None else torch.as_tensor(labels)
    plab = None if pattern_labels is None else torch.as_tensor(pattern_labels)
    host = as_np(motif_match(b, pb, labels=lab, pattern_labels=plab, **kw))
    B, P = int(b.num_graphs), int(pb.num_graphs)
    assert host[0].shape == (B, P) and host[1].shape == (B, P, 8) and host[2].shape == (B, P)
    assert host[1].dtype == np.int32 and host[0].dtype == np.int64
    if oracle:
        want = MO.motif_match_oracle(b.edge_index.numpy(), b.ptr.numpy(), b.edge_ptr.numpy(), pb.edge_index.numpy(), pb.ptr.numpy(),
                                     pb.edge_ptr.numpy(), labels=labels, pat_labels=pattern_labels, **kw)
        for name, got, exp in zip(motif.MotifMatch._fields, host, want):
            assert np.array_equal(got, np.asarray(exp).reshape(got.shape)), name
    if dev is None:
        return host
    before = _lib.query("cal_launch_count")
    res = motif_match(to_dev(b, dev), pb, labels=None if lab is None else lab.to(dev),
                      pattern_labels=None if plab is None else plab.to(dev), **kw)
    assert _lib.query("cal_launch_count") - before == (1 if B and P else 0)
    assert all(t.is_cuda for t in res)
    got = as_np(res)
    for name, x, y in zip(motif.MotifMatch._fields, got, host):
        assert x.dtype == y.dtype and np.array_equal(x, y), name
    return got


# ---- the cases: each a function of the device (None: the host twin alone) ------------------------------------------------------
AUT = [2, 12, 4, 4]
NON_INDUCED = [[2, 0, 0, 0], [0, 12, 0, 0], [0, 12, 4, 0], [4, 12, 0, 4]]      # rows: targets, columns: patterns


def case_motif_tables(dev):
    mb = batch_of([mot(s) for s in NAMES])
    count = run(mb, mb, dev)[0]
    assert count.tolist() == NON_INDUCED
    ind = run(mb, mb, dev, induced=True)
    want = [row[:] for row in NON_INDUCED]
    want[2][1] = want[3][1] = 0                                              # grid and diamond hold no INDUCED 6-cycle
    assert ind[0].tolist() == want and np.diag(ind[0]).tolist() == AUT
    assert ind[4].tolist() == [6, 6, 7, 8] and ind[3].tolist() == [6, 6, 7, 8]
    assert ind[1][0, 0].tolist() == [0, 1, 2, 3, 4, -1, -1, -1] and (ind[1][0, 1] == -1).all()
    if dev is None:
        assert automorphisms(spmotif.motif_batch()).tolist() == AUT


def case_hexagon_and_triangles(dev):
    tg = batch_of([HEXAGON, TWO_TRIANGLES, K4])
    pb = batch_of([HEXAGON, TRIANGLE])
    for induced in (False, True):
        count = run(tg, pb, dev, induced=induced)[0]
        assert count.tolist() == [[12, 0], [0, 12], [0, 24]]
    two = wl_refine(batch_of([HEXAGON, TWO_TRIANGLES]), iters=8)
    assert torch.equal(two.hash[0], two.hash[1])                            # 1-WL cannot tell them apart
    m = motif_match(to_dev(batch_of([HEXAGON, TWO_TRIANGLES]), dev), batch_of([HEXAGON]))
    iso = isomorphic(m, torch.tensor([0, 6, 12]), torch.tensor([0, 6]))
    assert iso.cpu().tolist() == [[True], [False]] and contains(m).cpu().tolist() == [[True], [False]]


def case_star(dev):
    nb, _ = MO.simple_graph(PATH3[1], 0, 3, 0, 4)
    assert MO.match_order(nb) == ([1, 0, 2], [None, 0, 0])
    tg = batch_of([star(256), EDGE])                                         # a hub next to a 2-node graph
    pb = batch_of([PATH3])
    for induced in (False, True):
        res = run(tg, pb, dev, induced=induced)
        assert res[0].tolist() == [[64770], [0]] and res[2].tolist() == [[0], [0]]
        assert res[1][0, 0].tolist() == [1, 0, 2, -1, -1, -1, -1, -1]


def case_budget_edges(dev):
    tg, pb = batch_of([star(256)]), batch_of([PATH3])
    nb, _ = MO.simple_graph(tg.edge_index.numpy(), 0, 256, 0, 510)
    steps = MO.search(nb, [{1}, {0, 2}, {1}])[3]
    assert steps[(0, 7)] == 255 and steps[(7, 0)] == 1 and len(steps) == 510
    res = run(tg, pb, dev, budget=0)
    assert (res[0][0, 0], res[2][0, 0]) == (0, 510) and (res[1] == -1).all()
    res = run(tg, pb, dev, budget=1)
    assert (res[0][0, 0], res[2][0, 0]) == (254, 255)                        # a leaf root takes one step and is done; a hub
                                                                             # root tries leaf 1 and stops
    res = run(tg, pb, dev, budget=255)
    assert (res[0][0, 0], res[2][0, 0]) == (64770, 0)                        # exactly what a hub root needs
    res = run(tg, pb, dev, budget=254)
    assert (res[0][0, 0], res[2][0, 0]) == (254 * 253 + 254, 255)            # one less: every hub root stops before leaf 255
    assert run(batch_of([K4]), batch_of([EDGE]), dev, budget=0)[0].tolist() == [[12]]     # two nodes: roots take no step


@pytest.fixture(scope="module")
def boundary_batch():
    rng = np.random.default_rng(7)
    return [sparse_graph(n, rng) for n in SIZES + [257]]


def case_word_boundaries(dev, graphs):
    pb = batch_of([PATH3, TRIANGLE, SQUARE, mot("house"), DOT])
    alone = run(batch_of(graphs[:-1]), pb, dev)
    res = run(batch_of(graphs[:4] + [graphs[-1]] + graphs[4:-1]), pb, dev)   # the 257-node graph in the middle
    assert (res[0][4] == -1).all() and (res[2][4] == 0).all() and (res[1][4] == -1).all() and res[3][4] == -1
    keep = [0, 1, 2, 3, 5, 6, 7, 8, 9]
    for i in range(4):
        assert np.array_equal(res[i][keep], alone[i])                         # the others are unaffected
    assert alone[0][:, 4].tolist() == SIZES and alone[0][2:, 0].min() > 0
    assert res[5][0] == alone[5][0] == 0
    ind = run(batch_of(graphs[:-1]), pb, dev, induced=True)
    assert (ind[0] <= alone[0]).all() and (ind[0] < alone[0]).any()


def case_labels(dev):
    rng = np.random.default_rng(3)
    graphs = [sparse_graph(n, rng) for n in (9, 40, 130)]
    tg = batch_of(graphs)
    pb = batch_of([PATH3, TRIANGLE, EDGE, DOT])
    lab = rng.integers(0, 3, int(tg.ptr[-1]))
    plab = rng.integers(0, 3, int(pb.ptr[-1]))
    res = run(tg, pb, dev, labels=lab, pattern_labels=plab)
    free = run(tg, pb, dev)
    assert (res[0] <= free[0]).all() and 0 < res[0].sum() < free[0].sum()
    # the key is compared unsigned: the two embeddings of a labelled edge start at node 5 and at node 200
    cols = both_directions([(5, 6), (200, 201), (6, 200)])
    lab = np.zeros(256, dtype=np.int64)
    lab[[5, 200]], lab[[6, 201]] = -7, 1 << 40
    res = run(batch_of([(256, cols)]), batch_of([EDGE]), dev, labels=lab, pattern_labels=np.array([-7, 1 << 40]))
    assert res[0].tolist() == [[3]] and res[1][0, 0, :2].tolist() == [5, 6]
    res = run(batch_of([(256, cols)]), batch_of([EDGE]), dev, labels=lab, pattern_labels=np.array([1 << 40, -7]))
    assert res[0].tolist() == [[3]] and res[1][0, 0, :2].tolist() == [6, 5]
    with pytest.raises(ValueError):
        motif_match(tg, pb, labels=torch.zeros(int(tg.ptr[-1]), dtype=torch.long))
    with pytest.raises(TypeError):
        motif_match(tg, pb, labels=torch.zeros(3, dtype=torch.long), pattern_labels=torch.as_tensor(plab))


def case_eight_node_path(dev):
    ring10 = (10, both_directions([(i, (i + 1) % 10) for i in range(10)]))
    rng = np.random.default_rng(5)
    res = run(batch_of([PATH8, ring10, sparse_graph(200, rng)]), batch_of([PATH8]), dev)
    assert res[0][:2, 0].tolist() == [2, 20] and res[0][2, 0] > 400
    assert res[1][0, 0].tolist() == list(range(8)) and (res[1][2, 0] >= 0).all() and len(set(res[1][2, 0].tolist())) == 8
    assert run(batch_of([PATH8, ring10]), batch_of([PATH8]), dev, induced=True)[0][:, 0].tolist() == [2, 20]


def case_columns_and_layout(dev):
    rng = np.random.default_rng(11)
    graphs = [sparse_graph(n, rng) for n in (40, 7, 90, 33)]
    ei, ptr, eptr = graphs_batch(graphs)
    pb = batch_of([PATH3, TRIANGLE, mot("diamond")])
    base = run(raw_batch(ei, ptr, eptr), pb, dev)
    assert base[5][0] == 0
    stray = ei.copy()
    stray[1, int(eptr[1])] = int(ptr[2]) + 3                                 # graph 1's first column now ends in graph 2
    stray[0, int(eptr[2]) - 1] = -5                                          # ... and its last one starts nowhere
    res = run(raw_batch(stray, ptr, eptr), pb, dev)
    assert res[5][0] == 2 and np.array_equal(res[0][[0, 2, 3]], base[0][[0, 2, 3]])
    # ungrouped columns: a foreign batch (edge_index, batch, num_graphs) with the columns of all graphs interleaved
    mixed = Data(edge_index=torch.as_tensor(ei[:, rng.permutation(ei.shape[1])]).contiguous())
    mixed.batch, mixed.num_graphs = torch.repeat_interleave(torch.arange(4), torch.as_tensor(np.diff(ptr))), 4
    got = as_np(motif_match(to_dev(mixed, dev), pb))
    for x, y in zip(got, base):
        assert np.array_equal(x, y)
    # a graph alone
    alone = run(batch_of([graphs[2]]), pb, dev)
    for i in range(4):
        assert np.array_equal(alone[i][0], base[i][2])


def case_empty_shapes(dev):
    none = np.zeros((2, 0), dtype=np.int64)
    pb = batch_of([PATH3, DOT])
    res = run(raw_batch(none, [0], [0]), pb, dev)                            # B = 0
    assert res[0].shape == (0, 2) and res[4].tolist() == [-1, -1] and res[5].tolist() == [0]
    res = run(batch_of([HEXAGON]), raw_batch(none, [0], [0]), dev)           # P = 0
    assert res[0].shape == (1, 0) and res[1].shape == (1, 0, 8) and res[3].tolist() == [-1]
    res = run(raw_batch(none, [0, 0, 0], [0, 0, 0]), pb, dev)                # N = 0, B = 2
    assert res[0].tolist() == [[0, 0]] * 2 and (res[1] == -1).all() and res[3].tolist() == [0, 0] and res[4].tolist() == [2, 0]
    res = run(raw_batch(none, [0, 4, 4, 9], [0, 0, 0, 0]), pb, dev)          # E = 0
    assert res[0].tolist() == [[0, 4], [0, 0], [0, 5]] and res[1][2, 1, 0] == 0


def case_rejected_patterns(dev):
    tg = to_dev(batch_of([HEXAGON]), dev)
    nine = (9, both_directions([(i, i + 1) for i in range(8)]))
    for bad in ([nine], [TRIANGLE, TWO_TRIANGLES], [TRIANGLE, (0, np.zeros((2, 0), dtype=np.int64))]):
        before = _lib.query("cal_launch_count") if dev else 0
        with pytest.raises(_lib.CalError, match="connected and have 1 to"):
            motif_match(tg, batch_of(bad))
        assert not dev or _lib.query("cal_launch_count") == before
        with pytest.raises(ValueError):
            MO.motif_match_oracle(np.zeros((2, 0)), [0, 1], [0, 0], *graphs_batch(bad))
    with pytest.raises(_lib.CalError, match="CAL_MOTIF_MAX_PATTERNS"):
        motif_match(tg, batch_of([EDGE] * 65))
    with pytest.raises(ValueError):
        motif_match(tg, batch_of([EDGE]), budget=-1)


def _census_batch():
    ds = spmotif.generate_dataset(2, node_num=5, seed=5)
    return Batch.from_data_list([g for ctx in ("tree", "ba") for s in NAMES for g in ds[ctx][s]])


def case_census_on_a_mask(dev):
    b = _census_batch()
    B = b.num_graphs
    y = b.y.view(-1)
    gt = spmotif.ground_truth(b)[1]
    protos = spmotif.motif_batch()
    res = motif_census(to_dev(b, dev), edge_mask=gt.to(dev) if dev else gt, prototypes=protos)
    iso, con = res["isomorphic"].cpu(), res["contains"].cpu()
    assert iso[torch.arange(B), y].all() and int(iso.sum()) == B             # the planted motif, and no other prototype
    assert torch.equal(con, torch.tensor(NON_INDUCED)[y] > 0)
    assert torch.equal(res["occurrences"].cpu(), torch.tensor(NON_INDUCED)[y] // torch.tensor(AUT))
    assert not res["skipped"].any() and int(res["truncated"].sum()) == 0
    sizes = torch.tensor([spmotif._MOTIFS[s][0] for s in NAMES])
    edges = torch.tensor([len(spmotif._MOTIFS[s][1]) for s in NAMES])
    assert torch.equal(res["nodes"].cpu(), sizes[y]) and torch.equal(res["edges"].cpu(), edges[y])
    # a mask that keeps the motif and more: every edge with a ground-truth endpoint
    ngt = spmotif.ground_truth(b)[0]
    wide = ngt[b.edge_index[0]] | ngt[b.edge_index[1]]
    res = motif_census(to_dev(b, dev), edge_mask=wide.to(dev) if dev else wide, prototypes=protos)
    con, where = res["contains"].cpu(), res["match_nodes"].cpu()
    assert con[torch.arange(B), y].all() and not res["isomorphic"].cpu()[torch.arange(B), y].all()
    pairs = {(int(u), int(v)) for u, v in b.edge_index.t().tolist()}
    for g in range(B):
        for p, s in enumerate(NAMES):
            ids = where[g, p].tolist()
            k, pedges = spmotif._MOTIFS[s]
            if not con[g, p]:
                assert ids == [-1] * 8
                continue
            assert ids[k:] == [-1] * (8 - k) and len(set(ids[:k])) == k
            assert all(int(b.ptr[g]) <= v < int(b.ptr[g + 1]) for v in ids[:k])       # data's numbering
            assert all((ids[a], ids[c]) in pairs or (ids[c], ids[a]) in pairs for a, c in pedges)
    none = motif_census(to_dev(b, dev), edge_mask=torch.zeros_like(gt).to(dev) if dev else torch.zeros_like(gt), prototypes=protos)
    assert not none["contains"].any() and (none["match_nodes"] == -1).all() and int(none["nodes"].sum()) == 0


CASES = [case_motif_tables, case_hexagon_and_triangles, case_star, case_budget_edges, case_labels, case_eight_node_path,
         case_columns_and_layout, case_empty_shapes, case_rejected_patterns, case_census_on_a_mask]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.__name__[5:])
def test_host_twin(case):
    case(None)


def test_host_twin_word_boundaries(boundary_batch):
    case_word_boundaries(None, boundary_batch)


# ---- the restatement against brute force ---------------------------------------------------------------------------------------
def test_restatement_equals_brute_force():
    def nbs(g):
        return MO.simple_graph(g[1], 0, g[0], 0, g[1].shape[1])[0]
    motifs = [nbs(mot(s)) for s in NAMES]
    for induced in (False, True):
        table = [[MO.brute_force(t, p, induced=induced)[0] for p in motifs] for t in motifs]
        want = [row[:] for row in NON_INDUCED]
        if induced:
            want[2][1] = want[3][1] = 0
        assert table == want
    assert [MO.brute_force(p, p, induced=True)[0] for p in motifs] == AUT
    rng = np.random.default_rng(2)
    pats = [nbs(g) for g in (PATH3, TRIANGLE, SQUARE, EDGE, DOT, mot("house"))]
    for trial in range(12):
        n = int(rng.integers(1, 8))
        cols = rng.integers(0, n, (2, int(rng.integers(0, 3 * n))))
        t = MO.simple_graph(cols, 0, n, 0, cols.shape[1])[0]
        tl, labelled = rng.integers(0, 2, n), trial % 3 == 0
        for p in pats:
            pl = rng.integers(0, 2, len(p))
            for induced in (False, True):
                kw = dict(tlab=tl, plab=pl) if labelled else {}
                c, _, f, _ = MO.search(t, p, induced=induced, **kw)
                assert (c, f) == MO.brute_force(t, p, induced=induced, **kw)


def test_abi_symbol_and_limits():
    protos = _lib.parse_header()
    for path in (_lib.LIB_PATH, _lib.HOST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        assert "cal_motif_match" in {l.split()[-1] for l in out.splitlines() if " T " in l}, path
    assert "cal_motif_match" in _lib.HOST_SYMBOLS and len(protos["cal_motif_match"][1]) == 23
    text = open(_lib.HEADER).read()
    for name, v in (("PATTERN", motif.MAX_PATTERN), ("NODES", motif.MAX_NODES), ("PATTERNS", motif.MAX_PATTERNS)):
        assert "#define CAL_MOTIF_MAX_%s %d\n" % (name, v) in text
    assert (MO.MAX_PATTERN, MO.MAX_NODES) == (motif.MAX_PATTERN, motif.MAX_NODES)
    import cal_amd
    assert cal_amd.motif_match is motif_match and cal_amd.MotifPatterns is MotifPatterns


# ---- the drivers ----------------------------------------------------------------------------------------------------------------
def test_eval_explanation_motifs_is_the_tally_of_its_batches():
    import random
    m = _cpu_model("CausalGCN")
    m.train()
    gs = spmotif.train_mix(12, node_num=7, seed=9)
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    py0, t0 = random.getstate(), torch.get_rng_state()
    ev = eval_explanation_motifs(m, DataLoader(gs, batch_size=8, shuffle=False), "cpu", k="gt")
    parts = []
    for i in (0, 8):
        b = Batch.from_data_list(gs[i:i + 8])
        ngt, egt = spmotif.ground_truth(b)
        parts.append(m.explanation_motifs(b, k="gt", edge_gt=egt, node_gt=ngt))
    assert m.training and random.getstate() == py0 and torch.equal(torch.get_rng_state(), t0)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd0[k]), k
    assert ev["skipped"] == 0 and ev["truncated"] == 0                       # (a condition of these inputs at the default budget)
    y = torch.cat([p["y"] for p in parts])
    rows = torch.arange(12)
    con, iso, pla = (torch.cat([p[key] for p in parts]) for key in ("contains", "isomorphic", "planted"))
    assert ev["graphs"] == 12
    assert ev["contain_rate"] == int(con[rows, y].sum()) / 12 and ev["iso_rate"] == int(iso[rows, y].sum()) / 12
    assert ev["planted_rate"] == int(pla[rows, y].sum()) / 12
    assert ev["contains"] == (con.sum(0).double() / 12).tolist() and ev["isomorphic"] == (iso.sum(0).double() / 12).tolist()
    for key in ("contain_rate", "iso_rate", "planted_rate", "wl_not_iso"):
        assert 0.0 <= ev[key] <= 1.0
    assert ev["iso_rate"] <= ev["contain_rate"] and ev["planted_rate"] <= ev["contain_rate"]
    exact = torch.cat([wl_refine(p["subgraph"], iters=3).hash[:, -1:] == wl_refine(spmotif.motif_batch(), iters=3).hash[None, :, -1]
                       for p in parts])
    assert ev["wl_not_iso"] == int((exact & ~iso)[rows, y].sum()) / 12
    for p in parts:                                                          # k = "gt": as many undirected edges as the motif
        want = torch.tensor([len(spmotif._MOTIFS[s][1]) for s in NAMES])[p["y"]]
        assert torch.equal(p["edges"], want) and p["yhat"].shape == p["y"].shape
        assert (p["planted"] <= p["contains"]).all() and (p["isomorphic"] <= p["contains"]).all()
    with pytest.raises(TypeError):
        eval_explanation_motifs(m, [], "cpu", prototypes=MotifPatterns(spmotif.motif_batch()))
    assert eval_explanation_motifs(m, [], "cpu")["graphs"] == 0

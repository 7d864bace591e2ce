"""Batch splice and structure interventions on the CPU: the host twin of cal_graph_splice_count / cal_graph_splice_write against
the plain-torch restatement (every integer output, the copied rows and the totals bit for bit), the exported symbols, the
argument errors of the Python layer, structure_intervention() of a CPU-resident model against the fp64 oracle, and the state
it leaves untouched."""
import argparse
import random
import subprocess

import pytest
import torch

from cal_amd import _lib
from cal_amd.data import Batch
from cal_amd.explain import _Layout, _scores, explain, extract_subgraph
from cal_amd.splice import BRIDGE, _structure_forward, eval_structure_intervention, splice_batches, structure_intervention
from oracle import cal_oracle as O
from tests.splice_oracle import HEADS, KEYS, check_splice, check_structure, splice_cases, structure_oracle

CASES = splice_cases()
SYMBOLS = ("cal_graph_splice_ws", "cal_graph_splice_count", "cal_graph_splice_write")


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_twin_equals_restatement(name):
    a, b, ga, gb, bridge = CASES[name]
    res = splice_batches(a, b, ga, gb, bridge=bridge)
    check_splice(res, a, b, ga, gb, bridge)


def test_abi_symbols_are_exported_by_both_libraries():
    protos = _lib.parse_header()
    for path in (_lib.LIB_PATH, _lib.HOST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
        assert set(SYMBOLS) <= exported, path
    assert set(SYMBOLS) <= set(protos) and set(SYMBOLS) <= set(_lib.HOST_SYMBOLS)
    assert len(protos["cal_graph_splice_count"][1]) == 23 and len(protos["cal_graph_splice_write"][1]) == 32
    assert _lib.query("cal_graph_splice_ws", 10, 20, 3, host=True) >= 40 * 3 + 8 * 30
    assert BRIDGE == -(1 << 63)


def test_the_pieces_of_a_result():
    a, b, _, _, _ = CASES["identity"]
    res = splice_batches(a, b, bridge="first")
    assert res.num_graphs == 9 and res.bridges_unwritten == 0 and res.empty_graphs == 0
    assert torch.equal(res.ptr[1:] - res.ptr[:-1], (a.ptr[1:] - a.ptr[:-1]) + (b.ptr[1:] - b.ptr[:-1]))
    assert torch.equal(res.edge_ptr[1:] - res.edge_ptr[:-1], (a.edge_ptr[1:] - a.edge_ptr[:-1]) + (b.edge_ptr[1:] - b.edge_ptr[:-1]) + 2)
    assert int((res.edge_src == BRIDGE).sum()) == 18 and torch.equal(res.y, a.y)
    # a batch spliced with nothing is the batch; nothing spliced with it is it as well
    none = torch.full((9,), -1)
    for left, right, ga, gb in ((a, b, None, none), (b, a, none, None)):
        res = splice_batches(left, right, ga, gb)
        assert torch.equal(res.edge_index, a.edge_index) and torch.equal(res.ptr, a.ptr) and torch.equal(res.edge_ptr, a.edge_ptr)
        assert torch.equal(res.x, a.x) and torch.equal(res.batch, a.batch)
        assert (res.max_nodes, res.max_edges) == (a.max_nodes, a.max_edges)
    assert res.y is None                                   # no part of the first batch
    # no pair at all
    res = splice_batches(a, b, torch.zeros(0, dtype=torch.long), torch.zeros(0, dtype=torch.long))
    assert res.num_graphs == 0 and res.edge_index.shape == (2, 0) and res.x.shape == (0, 5) and res.ptr.tolist() == [0]
    assert res.batch.numel() == 0 and (res.max_nodes, res.max_edges, res.empty_graphs) == (0, 0, 0)
    # both parts absent in the middle: an empty result graph, counted
    res = splice_batches(a, b, torch.tensor([0, -1, 1]), torch.tensor([0, -1, 1]))
    assert res.empty_graphs == 1 and int(res.ptr[1]) == int(res.ptr[2])


def check_splice_values(res, a, b, gb):
    from tests.splice_oracle import _bridge_ids, splice_oracle
    ba, bb = _bridge_ids(a, b, None, gb, "first")
    r = splice_oracle(a, b, None, gb, ba, bb)
    for key in ("edge_index", "ptr", "edge_ptr", "batch", "node_src", "x"):
        assert torch.equal(getattr(res, key), r[key]), key
    return r


def test_ungrouped_and_foreign_inputs():
    a, b, _, gb, _ = CASES["permutation"]
    perm = torch.randperm(a.edge_index.size(1), generator=torch.Generator().manual_seed(5))

    class Foreign:
        pass
    f = Foreign()
    f.x, f.feat, f.edge_index, f.batch, f.num_graphs, f.y = a.x, None, a.edge_index[:, perm], a.batch, a.num_graphs, a.y
    order = torch.argsort(a.batch[f.edge_index[0]], stable=True)
    res = splice_batches(f, b, None, gb, bridge="first")
    g = Batch()
    g.__dict__.update(a.__dict__)
    g.edge_index = f.edge_index[:, order]                  # the same columns, grouped: what the operator saw
    r = check_splice_values(res, g, b, gb)
    from_a = r["edge_src"] >= 0
    assert torch.equal(res.edge_src[from_a], order[r["edge_src"][from_a]])           # edge_src names the caller's own columns
    assert torch.equal(res.edge_src[~from_a], r["edge_src"][~from_a])


def test_argument_errors():
    a, b, _, _, _ = CASES["identity"]
    with pytest.raises(ValueError):
        splice_batches(a, b, torch.arange(9), torch.arange(8))
    with pytest.raises(TypeError):
        splice_batches(a, b, torch.arange(9).float(), None)
    with pytest.raises(ValueError):
        splice_batches(a, b, bridge="last")
    with pytest.raises(ValueError):
        splice_batches(a, b, bridge=(torch.zeros(9, dtype=torch.long),))
    with pytest.raises(ValueError):
        splice_batches(a, b, bridge=(torch.zeros(9, dtype=torch.long), torch.zeros(8, dtype=torch.long)))
    with pytest.raises(ValueError):
        splice_batches(a, CASES["feat3"][1])                # feature widths differ
    with pytest.raises(ValueError):
        splice_batches(a, CASES["feat0"][1])                # one side without features
    with pytest.raises(TypeError):
        c = Batch()
        c.__dict__.update(b.__dict__)
        c.x = b.x.double()
        splice_batches(a, c)
    for kw in (dict(ratio=0.5, k=1), dict(), dict(ratio=0.5, use="both"), dict(ratio=0.5, undirected="sum"), dict(k="gt"),
               dict(ratio=0.5, partners=-1), dict(ratio=0.5, partners="some"), dict(ratio=0.5, bridge="last")):
        with pytest.raises(ValueError):
            structure_intervention(None, a, **kw)


def _args(**kw):
    d = dict(layers=2, hidden=32, with_random=True, without_node_attention=False, without_edge_attention=False,
             fc_num="222", cat_or_add="add")
    d.update(kw)
    return argparse.Namespace(**d)


def _cpu_model(name, feat, seed=3):
    from cal_amd import model as M
    torch.manual_seed(seed)
    sd = O.init_state(name, feat, 4, hidden=32, layers=2, heads=4)
    m = getattr(M, name)(feat, 4, _args())
    m.load_state_dict(sd, strict=name != "CausalGIN")
    return m, sd


ROWS = torch.stack([torch.randperm(9, generator=torch.Generator().manual_seed(s)) for s in (1, 2)])


@pytest.mark.parametrize("name", ["CausalGCN", "CausalGAT", "CausalGIN"])
@pytest.mark.parametrize("use,bridge", [("nodes", None), ("nodes", "first"), ("edges", None)])
def test_cpu_structure_intervention_matches_the_oracle(name, use, bridge):
    """The partition is the model's own (the ranking is pinned bit for bit in test_explain); the splices, the forwards and the
    metrics are restated through the fp64 oracle.  fp32 operator-level forward vs fp64: 1e-5 on probabilities, the bound
    test_subgraph applies to fidelity; hit counts only on entries whose oracle top-two gap exceeds ten times that."""
    tol = 1e-5
    m, sd = _cpu_model(name, 5)
    b = CASES["identity"][0]
    ex = explain(m, b, ratio=0.4)
    if use == "nodes":
        nm = ex.node_mask
    else:
        nm = torch.zeros(b.batch.numel(), dtype=torch.bool)
        nm[extract_subgraph(b, edge_mask=ex.edge_mask, relabel=True).node_map] = True
    res = m.structure_intervention(b, ratio=0.4, use=use, partners=ROWS, bridge=bridge)
    ref = structure_oracle(name, sd, b, nm, ROWS, bridge, layers=2, heads=4)
    if use == "edges":
        ref["kept"], ref["total"] = int(ex.edge_mask.sum()), ex.edge_mask.numel()
    check_structure(res, [ref], tol)
    assert set(res) == {"%s_%s" % (k, h) for k in KEYS for h in HEADS} | {"sparsity", "graphs", "pairs"}
    assert res["pairs"] == int((ROWS != torch.arange(9)).sum())


def test_cpu_identities_partners_and_eval():
    from cal_amd import spmotif
    from cal_amd.data import DataLoader
    m, _ = _cpu_model("CausalGCN", 10)
    gs = spmotif.train_mix(24, node_num=7, seed=4)
    b = Batch.from_data_list(gs)
    # everything causal / nothing causal: the identity splice is the batch itself
    with torch.no_grad():
        m.eval()
        lay = _Layout(b)
        sc = _scores(m, b)
        for kw in (dict(ratio=1.0, k=None), dict(ratio=None, k=0)):
            full, ident, swaps, _, _, _, sp = _structure_forward(m, b, lay, sc, kw["ratio"], kw["k"], "nodes", None, torch.zeros(0, 24, dtype=torch.long), None)
            assert torch.equal(sp.edge_index, b.edge_index) and torch.equal(sp.ptr, b.ptr)
            assert torch.equal(sp.feat if sp.x is None else sp.x, b.feat if b.x is None else b.x) and (sp.x is None) == (b.x is None)
            assert torch.equal(full, ident) and swaps.shape[0] == 0
    one = structure_intervention(m, b, ratio=1.0, partners=0)
    assert one["pairs"] == 0 and one["sparsity"] == 0.0 and one["acc_swap_o"] != one["acc_swap_o"]
    for h in HEADS:
        assert one["acc_self_" + h] == one["acc_full_" + h]
    # "all": the B - 1 cyclic shifts, every ordered pair once
    allp = structure_intervention(m, b, ratio=0.3, partners="all")
    assert allp["pairs"] == 24 * 23
    shifts = (torch.arange(24).view(1, -1) + torch.arange(1, 24).view(-1, 1)) % 24
    assert allp == structure_intervention(m, b, ratio=0.3, partners=shifts)
    # an int: permutations from the generator, reproducible
    r1 = structure_intervention(m, b, ratio=0.3, partners=2, generator=torch.Generator().manual_seed(7))
    g = torch.Generator().manual_seed(7)
    rows = torch.stack([torch.randperm(24, generator=g) for _ in range(2)])
    assert r1 == structure_intervention(m, b, ratio=0.3, partners=rows)
    # over a loader: sums over the mini-batches
    rows8 = torch.stack([torch.randperm(8, generator=g) for _ in range(2)])
    res = eval_structure_intervention(m, DataLoader(gs, batch_size=8, shuffle=False), "cpu", ratios=(0.25, 0.5), partners=rows8)
    assert sorted(res) == [0.25, 0.5]
    for r in res:
        parts = [structure_intervention(m, Batch.from_data_list(gs[i:i + 8]), ratio=r, partners=rows8) for i in (0, 8, 16)]
        assert res[r]["graphs"] == 24 and res[r]["pairs"] == sum(p["pairs"] for p in parts)
        for h in HEADS:
            assert abs(res[r]["acc_self_" + h] - sum(p["acc_self_" + h] for p in parts) / 3) < 1e-9
            want = sum(p["p_shift_" + h] * p["pairs"] for p in parts) / res[r]["pairs"]
            assert abs(res[r]["p_shift_" + h] - want) < 1e-9
    # a spliced graph without a node is an error that names the count
    with pytest.raises(ValueError, match="1 spliced graphs have no node"):
        lone = Batch.from_data_list(gs[:3])
        causal = extract_subgraph(lone, node_mask=lone.batch != 1, relabel=True)
        trivial = extract_subgraph(lone, node_mask=torch.zeros(lone.batch.numel(), dtype=torch.bool), relabel=True)
        from cal_amd.splice import _spliced_logp
        _spliced_logp(m, causal, trivial, None, None)


def test_cpu_structure_intervention_leaves_state_untouched():
    from cal_amd import model as M
    torch.manual_seed(0)
    m = M.CausalGAT(5, 4, _args())
    m.train()
    b = CASES["identity"][0]
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    x0, ei0 = b.x.clone(), b.edge_index.clone()
    gen = torch.Generator().manual_seed(3)
    g0 = gen.get_state()
    for generator in (gen, None):
        py0, t0 = random.getstate(), torch.get_rng_state()
        res = structure_intervention(m, b, ratio=0.3, partners=2, generator=generator, bridge="first")
        assert m.training and res["graphs"] == b.num_graphs
        assert random.getstate() == py0 and torch.equal(torch.get_rng_state(), t0)
    assert not torch.equal(gen.get_state(), g0)            # the given generator is what advanced
    for key, v in m.state_dict().items():
        assert torch.equal(v, sd0[key]), key
    assert torch.equal(b.x, x0) and torch.equal(b.edge_index, ei0)
    m.eval()
    structure_intervention(m, b, k=2, partners=1)
    assert not m.training


def test_every_builder_makes_one_query_and_two_calls(monkeypatch):
    """splice_batches, occlude_batch and coalition_batch go through one driver: per call one workspace query, the count, the
    write, nothing else; without a result graph they return the empty Batch."""
    from cal_amd.coalition import coalition_batch
    from cal_amd.occlude import occlude_batch
    a, b, _, _, _ = CASES["identity"]
    seen = []
    call, query = _lib.call, _lib.query
    monkeypatch.setattr(_lib, "call", lambda name, *args, **kw: (seen.append(name), call(name, *args, **kw))[1])
    monkeypatch.setattr(_lib, "query", lambda name, *args, **kw: (seen.append(name), query(name, *args, **kw))[1])
    E, N = int(a.edge_index.size(1)), int(a.batch.numel())
    for R in (3, 0):
        rg, none = torch.arange(R), torch.zeros(0, dtype=torch.long)
        runs = [("cal_graph_splice", lambda: splice_batches(a, b, rg, rg, bridge="first"))]
        for use, M in (("edges", E), ("nodes", N)):
            runs.append(("cal_occlude", lambda use=use: occlude_batch(a, rg, a.ptr[:R] if R else none, use=use)))
            runs.append(("cal_coalition", lambda use=use, M=M: coalition_batch(a, rg, torch.full((R,), 1), torch.arange(M) % 3, use=use)))
        for stem, run in runs:
            del seen[:]
            res = run()
            assert seen == [stem + "_ws", stem + "_count", stem + "_write"], stem
            assert res.num_graphs == R and res.ptr.numel() == R + 1 and res.edge_ptr.numel() == R + 1
            if R == 0:
                assert res.edge_index.shape == (2, 0) and res.x.shape == (0, 5) and res.feat is None and res.batch.numel() == 0
                assert res.ptr.tolist() == [0] and res.edge_ptr.tolist() == [0] and res.y.numel() == 0
                assert res.node_src.numel() == 0 and res.edge_src.numel() == 0 and res.no_self_loops == a.no_self_loops
                assert (res.max_nodes, res.max_edges, res.empty_graphs) == (0, 0, 0)
                assert getattr(res, "bridges_unwritten", 0) == 0

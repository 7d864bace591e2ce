"""The count / write kernel pair the occlusion, coalition and subset builders share (cal_amd/csrc/restrict.hpp) on the MI355X,
at the shapes that reach what the case lists do not: the scan over more than one replica per thread, a 5000-node graph between
3-node ones (the <1024> count kernel, a map row of many chunks, element loops of thousands of columns) and feature rows at an odd
offset (the scalar row copy next to the vector one) -- each builder against its own plain restatement, bit for bit.  Then the
two identities that tie the subset builder to the other two, on the device."""
import pytest
import torch

from cal_amd import synth
from cal_amd.coalition import coalition_batch
from cal_amd.counterfactual import pack_bits, subset_batch, unpack_bits
from cal_amd.data import Batch, Data
from cal_amd.explain import edge_twins
from cal_amd.occlude import occlude_batch
from tests.coalition_oracle import check_coalition, coalition_cases
from tests.counterfactual_oracle import check_subset, subset_cases, subset_oracle
from tests.occlude_oracle import check_occlude, occlude_cases

pytestmark = pytest.mark.gpu
DEV = "cuda"
BUILDERS = ["occlude", "coalition", "subset"]


def _dev(b):
    """A device copy of a CPU batch (the case lists are shared between tests)."""
    d = Batch()
    for k, v in b.__dict__.items():
        d.__dict__[k] = v.to(DEV) if torch.is_tensor(v) else v
    d._plan = None
    return d


def _m(t):
    return t.to(DEV) if torch.is_tensor(t) else t


def _subset(c, bd=None):
    """subset_batch of case ``c`` (tests/counterfactual_oracle.py) on the device, checked against the restatement."""
    res = subset_batch(bd if bd is not None else _dev(c["b"]), _m(c["rg"]), _m(c["bits"]), rep_row=_m(c["rrow"]),
                       rep_flip=_m(c["rflip"]), use=c["use"], twin=_m(c["twin"]))
    check_subset(res, c, subset_oracle(c))
    return res


def _words(b, use):
    """words of a bitset row that covers the longest element segment of ``b``"""
    off = b.edge_ptr if use == "edges" else b.ptr
    return -(-int((off[1:] - off[:-1]).max()) // 32)


def _rand_bits(K, W, g):
    return torch.randint(-2 ** 31, 2 ** 31, (K, W), generator=g, dtype=torch.long).to(torch.int32)


def _tiny(n, feat, g, hi=7):
    ds = []
    for _ in range(n):
        k = int(torch.randint(3, hi, (1,), generator=g))
        src = torch.arange(k)
        ei = torch.stack([torch.cat([src, (src + 1) % k]), torch.cat([(src + 1) % k, src])])      # a ring, both directions
        ds.append(Data(x=torch.randn(k, feat, generator=g), edge_index=ei, y=torch.randint(0, 4, (1,), generator=g)))
    return ds


# ---- the scan ---------------------------------------------------------------------------------------------------------------------
def subset_scan_case(b, rg, use, g):
    W = _words(b, use)
    return dict(b=b, bits=_rand_bits(5, W, g), rg=rg, rrow=torch.randint(-1, 6, (3000,), generator=g),
                rflip=torch.randint(-1, 14, (3000,), generator=g), twin=edge_twins(b)[0] if use == "edges" else None, use=use)


@pytest.mark.parametrize("use", ["edges", "nodes"])
@pytest.mark.parametrize("builder", BUILDERS)
def test_hip_scan_beyond_one_run_per_thread(builder, use):
    """3000 replicas of 3-6-node ring graphs, a third with graph id -1 (many short and many empty replicas): every thread of
    the scanning workgroup owns a run of replicas."""
    g = torch.Generator().manual_seed(4)
    b = Batch.from_data_list(_tiny(500, 4, g))
    rg = torch.randint(-250, 500, (3000,), generator=g).clamp(min=-1)
    if builder == "occlude":
        off = b.edge_ptr if use == "edges" else b.ptr
        gc = rg.clamp(min=0)
        re = off[gc] + torch.randint(0, 1 << 20, (3000,), generator=g) % (off[gc + 1] - off[gc])
        twin = edge_twins(b)[0] if use == "edges" else None
        res = occlude_batch(_dev(b), rg.to(DEV), re.to(DEV), use=use, twin=_m(twin))
        empty = check_occlude(res, b, rg, re, use, twin)["totals"][4]
    elif builder == "coalition":
        M = int(b.edge_index.size(1)) if use == "edges" else int(b.batch.numel())
        key = torch.randint(-1, 7, (3, M), generator=g, dtype=torch.int32)
        rrow = torch.randint(-1, 4, (3000,), generator=g)
        rth = torch.randint(0, 8, (3000,), generator=g)
        res = coalition_batch(_dev(b), rg.to(DEV), rth.to(DEV), key.to(DEV), rep_row=rrow.to(DEV), use=use)
        empty = check_coalition(res, b, rg, rrow, rth, key, use, False)["totals"][4]
    else:
        empty = _subset(subset_scan_case(b, rg, use, g)).empty_graphs
    assert empty > 800


# ---- a large graph ----------------------------------------------------------------------------------------------------------------
def large_batch(g):
    """A 5000-node BA graph between four 3-node rings; two of its columns leave its node range.  -> (batch, its first column)"""
    big = synth.ba_graphs(1, n=5000, seed=1)
    F = int(big[0].x.size(1)) if big[0].x is not None else int(big[0].feat.size(1))
    small = _tiny(4, F, g, hi=4)
    for d in small:
        d.x, d.feat = (d.x, None) if big[0].x is not None else (None, d.x)
    b = Batch.from_data_list(small[:2] + [big[0]] + small[2:])
    b.edge_index = b.edge_index.clone()
    lo = int(b.edge_ptr[2])
    b.edge_index[0, lo + 1500] = 0
    b.edge_index[1, lo + 7777] = int(b.ptr[3])
    return b, lo


def subset_large_case(b, use, g):
    """The large graph in the middle, then thrice more: its last element flipped, a flip beyond most of its rows' words' use,
    the control row.  W covers the longest segment (edges: some 600 words)."""
    m = int(b.edge_ptr[3] - b.edge_ptr[2]) if use == "edges" else 5000
    return dict(b=b, bits=_rand_bits(2, _words(b, use), g), rg=torch.tensor([0, 1, 2, 3, 4, 2, 2, 2]),
                rrow=torch.tensor([0, 1, 0, 1, 0, 1, -1, 2]), rflip=torch.tensor([1, -1, 40, 2, 0, m - 1, 4999, -1]),
                twin=edge_twins(b)[0] if use == "edges" else None, use=use)


@pytest.mark.parametrize("use", ["edges", "nodes"])
@pytest.mark.parametrize("builder", BUILDERS)
def test_hip_large_graph_next_to_small_ones(builder, use):
    """Replicas of a 5000-node graph between replicas of 3-node graphs: element loops of thousands of columns in the count and
    in the write, and in node mode a map row far beyond anything that would fit LDS.  The large graph also has columns that
    leave its node range."""
    g = torch.Generator().manual_seed(5)
    b, lo = large_batch(g)
    bd = _dev(b)
    if builder == "occlude":
        twin = edge_twins(b)[0] if use == "edges" else None
        rg = torch.arange(5)                                                  # one replica of the large graph in the middle
        if use == "edges":
            re = torch.tensor([int(b.edge_ptr[0]) + 1, int(b.edge_ptr[1]), lo + 4321, int(b.edge_ptr[3]), int(b.edge_ptr[5]) - 1])
        else:
            re = torch.tensor([int(b.ptr[0]), int(b.ptr[1]) + 1, int(b.ptr[2]) + 17, int(b.ptr[3]), int(b.ptr[5]) - 1])
        res = occlude_batch(bd, rg.to(DEV), re.to(DEV), use=use, twin=_m(twin))
        check_occlude(res, b, rg, re, use, twin)
        assert res.max_nodes == 5000 - (use == "nodes") and res.max_edges > 7000
        # the large graph's column that leaves its range / its last node as the element, and its control replica
        rg = torch.tensor([2, 0, 2])
        re = torch.tensor([lo + 1500 if use == "edges" else int(b.ptr[3]) - 1, -1, -1])
        res = occlude_batch(bd, rg.to(DEV), re.to(DEV), use=use, twin=_m(twin))
        check_occlude(res, b, rg, re, use, twin)
        assert res.max_nodes == 5000
    elif builder == "coalition":
        M = int(b.edge_index.size(1)) if use == "edges" else int(b.batch.numel())
        key = torch.randint(0, 8, (2, M), generator=g, dtype=torch.int32)
        for invert in (False, True):
            rg = torch.tensor([0, 1, 2, 3, 4, 2, 2, 2])                        # the large graph in the middle, then thrice more
            rrow = torch.tensor([0, 1, 0, 1, 0, 1, -1, 0])
            rth = torch.tensor([4, 4, 5, 1, 9, 2, 0, 0])                       # ..., the control replica, nothing / everything
            res = coalition_batch(bd, rg.to(DEV), rth.to(DEV), key.to(DEV), rep_row=rrow.to(DEV), use=use, invert=invert)
            check_coalition(res, b, rg, rrow, rth, key, use, invert)
            assert res.max_nodes == 5000 and res.max_edges > 7000
    else:
        res = _subset(subset_large_case(b, use, g), bd)
        assert res.max_nodes == 5000 and res.max_edges > 7000


# ---- rows at odd offsets ------------------------------------------------------------------------------------------------------------
def _odd_rows(b0, F, drop_feat=True):
    """``b0`` with a random [N, F] x -> (the CPU batch, a device copy whose x starts one float into its storage)"""
    b = Batch()
    b.__dict__.update(b0.__dict__)
    b.x = torch.randn(b0.batch.numel(), F, generator=torch.Generator().manual_seed(31))
    if drop_feat:
        b.feat = None
    bd = _dev(b)
    flat = torch.empty(b.x.numel() + 1, device=DEV)
    flat[1:] = b.x.to(DEV).view(-1)
    bd.x = flat[1:].view(-1, F)
    assert bd.x.data_ptr() % 16 == 4 and bd.x.is_contiguous()
    return b, bd


@pytest.mark.parametrize("F", [5, 4])
@pytest.mark.parametrize("builder", BUILDERS)
def test_hip_rows_at_odd_offsets(builder, F):
    """A feature matrix that starts one float into its storage: F = 5 takes the scalar copy as always, F = 4 takes it because the
    rows are not 16-byte aligned (next to the aligned call, which takes the vector copy)."""
    if builder == "occlude":
        b0, rg, re, use, twin = occlude_cases()["repeated_edges"]
        b, bd = _odd_rows(b0, F, drop_feat=False)
        check_occlude(occlude_batch(bd, rg.to(DEV), re.to(DEV), use=use, twin=twin.to(DEV)), b, rg, re, use, twin)
        check_occlude(occlude_batch(_dev(b), rg.to(DEV), re.to(DEV), use=use, twin=twin.to(DEV)), b, rg, re, use, twin)
    elif builder == "coalition":
        b0, rg, rrow, rth, key, use, invert = coalition_cases()["spmotif_nodes"]
        b, bd = _odd_rows(b0, F)
        args = (rg.to(DEV), rth.to(DEV), key.to(DEV))
        check_coalition(coalition_batch(bd, *args, rep_row=rrow.to(DEV), use=use), b, rg, rrow, rth, key, use, False)
        check_coalition(coalition_batch(_dev(b), *args, rep_row=rrow.to(DEV), use=use), b, rg, rrow, rth, key, use, False)
    else:
        c0 = subset_cases()["spmotif_nodes"]
        b, bd = _odd_rows(c0["b"], F)
        c = dict(c0, b=b)
        _subset(c, bd)
        _subset(c)


# ---- the subset builder is the other two ------------------------------------------------------------------------------------------
def _same(u, v):
    for key in ("edge_index", "ptr", "edge_ptr", "batch", "node_src", "edge_src", "y"):
        assert getattr(u, key).is_cuda and torch.equal(getattr(u, key), getattr(v, key)), key
    fu, fv = (u.feat if u.x is None else u.x), (v.feat if v.x is None else v.x)
    assert torch.equal(fu, fv) and (u.x is None) == (v.x is None)
    assert (u.max_nodes, u.max_edges, u.empty_graphs, u.num_graphs) == (v.max_nodes, v.max_edges, v.empty_graphs, v.num_graphs)


@pytest.mark.parametrize("use,with_twin", [("edges", False), ("edges", True), ("nodes", False)])
def test_hip_no_bits_and_a_flip_is_occlude_batch(use, with_twin):
    b = subset_cases()["spmotif_edges"]["b"]
    off = b.edge_ptr if use == "edges" else b.ptr
    M = int(off[-1])
    re = torch.cat([torch.arange(0, M, 3), torch.tensor([-1])])           # ... and a control replica
    rg = (torch.searchsorted(off, re.clamp(min=0), right=True) - 1)
    twin = _m(edge_twins(b)[0]) if with_twin else None
    bd = _dev(b)
    got = subset_batch(bd, rg.to(DEV), None, rep_flip=torch.where(re >= 0, re - off[rg], re).to(DEV), use=use, twin=twin)
    _same(got, occlude_batch(bd, rg.to(DEV), re.to(DEV), use=use, twin=twin))


@pytest.mark.parametrize("use", ["edges", "nodes"])
@pytest.mark.parametrize("invert", [False, True])
def test_hip_bits_packed_from_a_key_is_coalition_batch(use, invert):
    b = subset_cases()["spmotif_edges"]["b"]
    seg, mx = (b.edge_ptr, b.max_edges) if use == "edges" else (b.ptr, b.max_nodes)
    M, B = int(seg[-1]), b.num_graphs
    g = torch.Generator().manual_seed(3)
    key = torch.randint(-1, 9, (3, M), generator=g, dtype=torch.int32)
    rg, rrow, rth = torch.randint(0, B, (40,), generator=g), torch.randint(0, 3, (40,), generator=g), torch.randint(0, 9, (40,), generator=g)
    # one bitset row per replica: the elements of its graph with key < thresh (inverted: >=)
    rows = []
    for r in range(40):
        stay = (key[rrow[r]] >= rth[r]) if invert else (key[rrow[r]] < rth[r])
        rows.append(pack_bits(stay, seg, mx)[rg[r]])
    bits = torch.stack(rows)
    assert torch.equal(unpack_bits(pack_bits(stay, seg, mx), seg, M), stay)
    bd = _dev(b)
    got = subset_batch(bd, rg.to(DEV), bits.to(DEV), rep_row=torch.arange(40, device=DEV), use=use)
    _same(got, coalition_batch(bd, rg.to(DEV), rth.to(DEV), key.to(DEV), rep_row=rrow.to(DEV), use=use, invert=invert))

"""Plain restatements of the occlusion operators: the replica builder (cal_occlude_count / cal_occlude_write) in torch, one
replica at a time; the ten rank-agreement counts (cal_rank_agreement) in numpy, all pairs of a segment at once; the three
figures made of them; and the occlusion scores through the fp64 oracle's eval forward.  Everything on the CPU."""
import math

import numpy as np
import torch

from tests.subgraph_oracle import oracle_log_probs

HEADS = ("c", "o", "co")


def _feat(b):
    return b.x if getattr(b, "x", None) is not None else getattr(b, "feat", None)


def occlude_oracle(b, rep_graph, rep_elem, use="edges", twin=None):
    """-> dict(ptr, edge_ptr, batch, x, edge_index, node_src, edge_src, totals [5]) for a CPU source with grouped columns."""
    x, ei, B = _feat(b), b.edge_index, int(b.num_graphs)
    ptr, eptr, batch, nsrc, esrc, cols_out, rows = [0], [0], [], [], [], [], []
    empty = mn = me = 0
    for r, (g, e) in enumerate(zip([int(v) for v in rep_graph], [int(v) for v in rep_elem])):
        n0 = ptr[-1]
        nodes, cols, new = torch.zeros(0, dtype=torch.long), torch.zeros(0, dtype=torch.long), torch.zeros(2, 0, dtype=torch.long)
        if 0 <= g < B:
            lo, hi = int(b.ptr[g]), int(b.ptr[g + 1])
            elo, ehi = int(b.edge_ptr[g]), int(b.edge_ptr[g + 1])
            nodes, cols = torch.arange(lo, hi), torch.arange(elo, ehi)
            ends = ei[:, cols]
            ok = ((ends >= lo) & (ends < hi)).all(0)                  # a column that leaves its graph is dropped
            shift = torch.zeros_like(ends)
            if use == "edges":
                if elo <= e < ehi:
                    ok &= cols != e
                    if twin is not None and int(twin[e]) >= 0:
                        ok &= cols != int(twin[e])
            elif lo <= e < hi:
                nodes = nodes[nodes != e]
                ok &= (ends != e).all(0)
                shift = (ends > e).long()
            cols, new = cols[ok], (ends - lo + n0 - shift)[:, ok]
        n, m = nodes.numel(), cols.numel()
        nsrc.append(nodes)
        esrc.append(cols)
        cols_out.append(new)
        batch.append(torch.full((n,), r, dtype=torch.long))
        if x is not None:
            rows.append(x[nodes])
        ptr.append(n0 + n)
        eptr.append(eptr[-1] + m)
        empty += n == 0
        mn, me = max(mn, n), max(me, m)
    cat = lambda ts: torch.cat(ts) if ts else torch.zeros(0, dtype=torch.long)
    out_ei = torch.cat(cols_out, 1).contiguous() if cols_out else torch.zeros(2, 0, dtype=torch.long)
    xo = None
    if x is not None:
        xo = torch.cat(rows) if rows else x[:0]
    return dict(ptr=torch.tensor(ptr), edge_ptr=torch.tensor(eptr), batch=cat(batch), x=xo, edge_index=out_ei, node_src=cat(nsrc),
                edge_src=cat(esrc), totals=[ptr[-1], eptr[-1], mn, me, empty])


def check_occlude(res, b, rep_graph, rep_elem, use, twin):
    """``res`` (an occlude_batch result, any device) of the CPU source ``b``: equals the restatement bit for bit; structural
    properties on their own; node_src / edge_src reproduce the rows and the columns from the source."""
    r = occlude_oracle(b, rep_graph, rep_elem, use, twin)
    ei, ptr, eptr = res.edge_index.cpu(), res.ptr.cpu(), res.edge_ptr.cpu()
    assert torch.equal(ei, r["edge_index"]) and res.edge_index.is_contiguous() and ei.shape == (2, r["totals"][1])
    assert torch.equal(ptr, r["ptr"]) and torch.equal(eptr, r["edge_ptr"])
    assert torch.equal(res.batch.cpu(), r["batch"])
    assert torch.equal(res.node_src.cpu(), r["node_src"]) and torch.equal(res.edge_src.cpu(), r["edge_src"])
    rx = _feat(res)
    if r["x"] is None:
        assert rx is None
    else:
        assert rx.dtype == torch.float32 and torch.equal(rx.cpu(), r["x"]) and (res.x is None) == (b.x is None)
    n2, e2 = int(res.batch.numel()), int(ei.size(1))
    assert [n2, e2, res.max_nodes, res.max_edges, res.empty_graphs] == r["totals"]
    R = len(r["ptr"]) - 1
    assert res.num_graphs == R and res.tile_ptr is None and res.no_self_loops == bool(b.no_self_loops)
    rg = [int(v) for v in rep_graph]
    if b.y is None or any(not 0 <= g < int(b.num_graphs) for g in rg):
        assert res.y is None
    else:
        assert torch.equal(res.y.cpu(), b.y.view(-1)[torch.tensor(rg, dtype=torch.long)])
    # independent of the restatement
    assert int(ptr[0]) == 0 and int(ptr[-1]) == n2 and int(eptr[0]) == 0 and int(eptr[-1]) == e2
    assert bool((ptr[1:] >= ptr[:-1]).all()) and bool((eptr[1:] >= eptr[:-1]).all())
    gid_e = torch.repeat_interleave(torch.arange(R), eptr[1:] - eptr[:-1])
    assert bool(((ei >= ptr[gid_e]) & (ei < ptr[gid_e + 1])).all())
    ns, es = res.node_src.cpu(), res.edge_src.cpu()
    if rx is not None:
        assert torch.equal(rx.cpu(), _feat(b)[ns])
    assert torch.equal(ns[ei], b.edge_index[:, es])                       # the endpoints' sources are the source column's
    return r


# ---- the case list both test files walk (host twin on the CPU, HIP on the GPU) ---------------------------------------------
def hand_batch(graphs, F=3, seed=0):
    """A batch from ``[(nodes, [(u, v), ...]), ...]`` with local endpoints; nothing is checked or cleaned."""
    from cal_amd.data import Batch
    g = torch.Generator().manual_seed(seed)
    ptr, eptr, cols = [0], [0], []
    for n, es in graphs:
        lo = ptr[-1]
        cols += [(lo + u, lo + v) for u, v in es]
        ptr.append(lo + n)
        eptr.append(eptr[-1] + len(es))
    b = Batch()
    B = len(graphs)
    b.x = torch.randn(ptr[-1], F, generator=g) if F else None
    b.edge_index = torch.tensor(cols, dtype=torch.long).t().contiguous() if cols else torch.zeros(2, 0, dtype=torch.long)
    b.ptr, b.edge_ptr, b.num_graphs = torch.tensor(ptr), torch.tensor(eptr), B
    b.batch = torch.repeat_interleave(torch.arange(B), b.ptr[1:] - b.ptr[:-1])
    b.max_nodes = max(n for n, _ in graphs)
    b.max_edges = max(len(es) for _, es in graphs)
    b.y, b.no_self_loops = torch.arange(B) % 4, False
    return b


def _gid(off):
    return torch.repeat_interleave(torch.arange(off.numel() - 1), off[1:] - off[:-1])


def _all_elements(b, use):
    """Every element of ``b`` once with its own graph, then a control replica (-1) per graph."""
    off = b.edge_ptr if use == "edges" else b.ptr
    B = int(b.num_graphs)
    return torch.cat([_gid(off), torch.arange(B)]), torch.cat([torch.arange(int(off[-1])), torch.full((B,), -1)])


def occlude_cases():
    """name -> (batch, rep_graph, rep_elem, use, twin or None), CPU tensors."""
    from cal_amd import spmotif
    from cal_amd.data import Batch
    from cal_amd.explain import edge_twins
    from tests.helpers import random_graph_batch
    g = torch.Generator().manual_seed(0)
    out = {}
    ring = [(0, 1), (1, 2), (2, 0), (1, 0), (2, 1), (0, 2)]
    # a 1-node graph with no edge; a graph with a self loop, duplicate columns (the twin of the j-th is the j-th) and a column
    # with no twin; a ring
    mix = hand_batch([(1, []), (4, [(0, 0), (0, 1), (1, 0), (0, 1), (1, 0), (2, 3), (1, 2), (2, 1)]), (3, ring)])
    tw = edge_twins(mix)[0]
    assert tw.tolist() == [0, 2, 1, 4, 3, -1, 7, 6, 11, 12, 13, 8, 9, 10]
    rg, re = _all_elements(mix, "edges")
    # an element outside its graph (a control replica), graph ids outside the batch
    rg = torch.cat([rg, torch.tensor([1, 2, 0, -1, 99, 3])])
    re = torch.cat([re, torch.tensor([9, 0, 3, 1, 2, 0])])
    out["mix_edges"] = (mix, rg, re, "edges", None)
    out["mix_edges_twin"] = (mix, rg, re, "edges", tw)
    rg, re = _all_elements(mix, "nodes")                    # the first, a middle and the last node; a 1-node graph: empty
    rg = torch.cat([rg, torch.tensor([1, 2, -1, 99, 0])])
    re = torch.cat([re, torch.tensor([0, 3, 1, 2, 5])])
    out["mix_nodes"] = (mix, rg, re, "nodes", None)
    none = torch.zeros(0, dtype=torch.long)
    out["none_edges"] = (mix, none, none, "edges", tw)
    out["none_nodes"] = (mix, none, none, "nodes", None)
    # a source column that leaves its graph's range (and one with a negative endpoint)
    lv = hand_batch([(3, [(0, 1), (1, 0), (2, 3)]), (3, [(0, 2), (6, -3), (1, -4)])], F=2, seed=1)
    assert lv.edge_index.tolist() == [[0, 1, 2, 3, 9, 4], [1, 0, 3, 5, 0, -1]]
    lv.no_self_loops = True
    for use in ("edges", "nodes"):
        rg, re = _all_elements(lv, use)
        out["leaving_" + use] = (lv, rg, re, use, edge_twins(lv)[0] if use == "edges" else None)
    # one graph repeated many times, next to others
    a = random_graph_batch(num_graphs=9, n_lo=3, n_hi=30, feat=5, seed=1)
    ta = edge_twins(a)[0]
    lo, hi = int(a.edge_ptr[4]), int(a.edge_ptr[5])
    re = torch.cat([torch.randint(lo, hi, (40,), generator=g), torch.randint(0, int(a.edge_ptr[-1]), (20,), generator=g)])
    rg = torch.cat([torch.full((40,), 4), _gid(a.edge_ptr)[re[40:]]])
    out["repeated_edges"] = (a, rg, re, "edges", ta)
    lo, hi = int(a.ptr[4]), int(a.ptr[5])
    re = torch.cat([torch.randint(lo, hi, (40,), generator=g), torch.randint(0, int(a.ptr[-1]), (20,), generator=g)])
    rg = torch.cat([torch.full((40,), 4), a.batch[re[40:]]])
    out["repeated_nodes"] = (a, rg, re, "nodes", None)
    for F in (0, 3, 4, 16):
        c = Batch()
        c.__dict__.update(a.__dict__)
        c.x = torch.randn(a.batch.numel(), F, generator=torch.Generator().manual_seed(10 + F)) if F else None
        rg, re = _all_elements(c, "nodes" if F == 3 else "edges")
        out["feat%d" % F] = (c, rg, re, "nodes" if F == 3 else "edges", None if F == 3 else ta)
    sp = Batch.from_data_list(spmotif.train_mix(8, node_num=7, seed=3))
    for use in ("edges", "nodes"):
        rg, re = _all_elements(sp, use)
        out["spmotif_" + use] = (sp, rg, re, use, edge_twins(sp)[0] if use == "edges" else None)
    return out


# ---- rank agreement -----------------------------------------------------------------------------------------------------------
def agreement_counts_np(a, b, seg_ptr, max_seg, sel=None, ratio=None, k=None):
    """The ten counts of every segment, int64 [B, 10], by comparing all pairs."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    seg = [int(v) for v in seg_ptr]
    out = np.zeros((len(seg) - 1, 10), dtype=np.int64)
    for g in range(len(seg) - 1):
        lo, hi = seg[g], seg[g + 1]
        if hi - lo > max_seg:
            out[g, 0] = -1
            continue
        take = ~(np.isnan(a[lo:hi]) | np.isnan(b[lo:hi]))
        if sel is not None:
            take &= np.asarray(sel[lo:hi], dtype=bool)
        x, y = a[lo:hi][take], b[lo:hi][take]
        n = x.size
        kg = min(int(k), n) if k is not None else min(n, int(math.ceil(float(ratio) * n)))
        sx = (x[None, :] > x[:, None]).astype(np.int8) - (x[None, :] < x[:, None]).astype(np.int8)     # sign(x_j - x_i)
        sy = (y[None, :] > y[:, None]).astype(np.int8) - (y[None, :] < y[:, None]).astype(np.int8)
        prod = sx * sy
        r2, top = [], []
        for v, s in ((x, sx), (y, sy)):
            r2.append(2 * (s < 0).sum(1).astype(np.int64) + (s == 0).sum(1) + 1)
            order = np.lexsort((np.arange(n), -v))                        # value descending, then index
            t = np.zeros(n, dtype=bool)
            t[order[:kg]] = True
            top.append(t)
        out[g] = [n, (prod > 0).sum() // 2, (prod < 0).sum() // 2, ((sx == 0).sum() - n) // 2, ((sy == 0).sum() - n) // 2,
                  (r2[0] * r2[0]).sum(), (r2[1] * r2[1]).sum(), (r2[0] * r2[1]).sum(), kg, (top[0] & top[1]).sum()]
    return out


def agreement_metrics_np(counts):
    """fp64 [B, 3]: Spearman's rho, Kendall's tau-b, the top-k Jaccard overlap; NaN where undefined."""
    out = np.full((len(counts), 3), np.nan)
    for g, (n, C, D, Ta, Tb, Saa, Sbb, Sab, kg, inter) in enumerate(np.asarray(counts).tolist()):
        if n < 2:
            continue
        mean = n + 1.0                                                    # of the doubled mid-ranks
        va, vb, cov = Saa / n - mean * mean, Sbb / n - mean * mean, Sab / n - mean * mean
        if va > 0 and vb > 0:
            out[g, 0] = cov / math.sqrt(va * vb)
        n0 = n * (n - 1) // 2
        if (n0 - Ta) * (n0 - Tb) > 0:
            out[g, 1] = (C - D) / math.sqrt((n0 - Ta) * (n0 - Tb))
        if 2 * kg - inter > 0:
            out[g, 2] = inter / (2 * kg - inter)
    return out


def agreement_inputs():
    """-> (a, b, seg_ptr, sel): segments of lengths 0, 1, 2, 63, 64, 65, 2048, 2049 and 5000 of few distinct values (many ties),
    then all ties in a, all ties in both, a segment with NaN entries and one whose sel selects nothing."""
    g = torch.Generator().manual_seed(7)
    lens = [0, 1, 2, 63, 64, 65, 2048, 2049, 5000, 50, 50, 40, 30]
    seg = torch.tensor([0] + lens).cumsum(0)
    M = int(seg[-1])
    a = torch.randint(0, 97, (M,), generator=g).float() / 7 - 3
    b = (a * 0.5 + torch.randint(0, 41, (M,), generator=g).float() / 5 - 4).contiguous()
    a[int(seg[5])] = 0.0
    a[int(seg[5]) + 1] = -0.0                                              # equal as floats
    sel = torch.rand(M, generator=g) < 0.8
    a[seg[9]:seg[10]] = 1.5                                               # all ties in a
    a[seg[10]:seg[11]] = -2.0                                             # all ties in both
    b[seg[10]:seg[11]] = 0.25
    a[seg[11]:seg[12]][::3] = float("nan")                                # NaN entries, in either vector
    b[seg[11]:seg[12]][1::4] = float("nan")
    sel[seg[12]:seg[13]] = False                                          # a sel that selects nothing
    return a, b, seg, sel


# (max_seg, with sel, ratio / k): every segment (the two above the LDS capacity in tiles); 5000 too long for the tiled launch;
# 2049 and 5000 too long for a one-tile launch at the capacity, with k = 0 and ratio = 1.0; a launch of 128-thread groups
AGREE_SPECS = [(5000, False, dict(ratio=0.3)), (5000, True, dict(k=5)), (2049, True, dict(ratio=0.3)), (2048, True, dict(k=0)),
               (2048, False, dict(ratio=1.0)), (65, False, dict(k=3))]
_WANT = {}


def agreement_want(i):
    """The numpy counts of spec i, computed once for the CPU and the GPU test."""
    if i not in _WANT:
        a, b, seg, sel = agreement_inputs()
        mx, use_sel, kw = AGREE_SPECS[i]
        _WANT[i] = agreement_counts_np(a.numpy(), b.numpy(), seg, mx, sel.numpy() if use_sel else None, **kw)
    return _WANT[i]


def check_agreement(dev):
    """cal_amd.occlude.rank_agreement on ``dev`` at every spec: the numpy counts bit for bit, the three figures to 1e-12."""
    from cal_amd.occlude import rank_agreement
    a, b, seg, sel = agreement_inputs()
    for i, (mx, use_sel, kw) in enumerate(AGREE_SPECS):
        want = agreement_want(i)
        counts, met = rank_agreement(a.to(dev), b.to(dev), seg.to(dev), mx, sel=sel.to(dev) if use_sel else None, **kw)
        assert counts.dtype == torch.long and met.dtype == torch.float64 and counts.device.type == torch.device(dev).type
        assert np.array_equal(counts.cpu().numpy(), want), (mx, use_sel, kw)
        wm = agreement_metrics_np(want)
        assert np.array_equal(np.isnan(met.cpu().numpy()), np.isnan(wm))
        assert np.allclose(np.nan_to_num(met.cpu().numpy()), np.nan_to_num(wm), rtol=0, atol=1e-12)
        long = [g for g in range(13) if int(seg[g + 1] - seg[g]) > mx]          # a segment longer than max_seg: n = -1
        assert [g for g in range(13) if want[g, 0] == -1] == long and not want[long, 1:].any()
        assert bool(met[long].isnan().all())
    assert not agreement_want(3)[:, 8:].any()                            # k = 0: nothing selected
    assert not agreement_want(1)[12].any()                               # a sel that selects nothing: n = 0
    assert agreement_want(0)[10].tolist()[:5] == [50, 0, 0, 1225, 1225] and agreement_want(0)[9, 3] == 1225
    return a, b, seg


def faith_from_scores(causal, occ, seg, max_seg, sel, top, **kw):
    """What a faithfulness report is made of, recomputed from score tensors by the numpy counts: (metrics [B, 3], [sum and count
    of the occlusion score inside ``top``, sum and count outside it])."""
    counts = agreement_counts_np(causal.cpu().numpy(), occ.cpu().numpy(), seg.cpu(), max_seg, None if sel is None else sel.cpu().numpy(),
                                 **kw)
    met = agreement_metrics_np(counts)
    took = ~occ.cpu().isnan() if sel is None else ~occ.cpu().isnan() & sel.cpu()
    o, t = occ.cpu().double(), top.cpu()
    return met, [o[took & t].sum().item(), int((took & t).sum()), o[took & ~t].sum().item(), int((took & ~t).sum())]


def check_faith(res, parts):
    """``res`` (a faithfulness report) against ``parts``, the faith_from_scores results of its mini-batches."""
    met = np.concatenate([p[0] for p in parts])
    tails = np.array([p[1] for p in parts]).sum(0)
    for j, key in enumerate(("rho", "tau", "jaccard")):
        ok = ~np.isnan(met[:, j])
        assert res[key + "_undefined"] == int((~ok).sum())
        if ok.any():
            assert abs(res[key] - met[ok, j].mean()) < 1e-12, key
        else:
            assert res[key] != res[key]
    assert res["graphs"] == len(met) and res["elements"] == int(tails[1] + tails[3])
    for key, s, c in (("occ_top", tails[0], tails[1]), ("occ_rest", tails[2], tails[3])):
        if c:
            assert abs(res[key] - s / c) < 1e-12, key
        else:
            assert res[key] != res[key]


# ---- the scores through the fp64 oracle ---------------------------------------------------------------------------------------
def occlusion_oracle(name, sd, b, yhat, use="edges", twin=None, head="o", elements=None, **kw):
    """fp64 [E] / [N]: ``p_full_g(yhat_g) - p_without_element(yhat_g)`` of every element of the CPU batch ``b`` through the fp64
    oracle on the restated replicas, NaN where no replica runs.  ``yhat`` [B] is handed in; ``twin`` (int32 [E]): one undirected
    edge is one element, both columns removed, both scored."""
    h = HEADS.index(head)
    sd64 = {k: v.double().cpu() for k, v in sd.items()}
    x, ei, B = _feat(b).cpu(), b.edge_index.cpu(), int(b.num_graphs)
    yhat = yhat.cpu()
    full = oracle_log_probs(name, sd64, x, ei, b.batch.cpu(), B, **kw)[h]
    p_full = full.gather(-1, yhat.view(-1, 1)).view(-1).exp()
    off = b.edge_ptr if use == "edges" else b.ptr
    M, gid = int(off[-1]), _gid(off.cpu())
    nodes = (b.ptr[1:] - b.ptr[:-1]).cpu()
    ids = [e for e in range(M) if int(nodes[gid[e]]) > (0 if use == "edges" else 1)]
    if twin is not None:
        ids = [e for e in ids if not 0 <= int(twin[e]) < e]
    if elements is not None:
        ids = [e for e in ids if bool(elements[e]) or (twin is not None and int(twin[e]) >= 0 and bool(elements[int(twin[e])]))]
    score = torch.full((M,), float("nan"), dtype=torch.float64)
    if not ids:
        return score
    ids = torch.tensor(ids)
    rg = gid[ids]
    r = occlude_oracle(b, rg, ids, use, twin)
    assert r["totals"][4] == 0
    lp = oracle_log_probs(name, sd64, r["x"], r["edge_index"], r["batch"], ids.numel(), **kw)[h]
    sc = p_full[rg] - lp.gather(-1, yhat[rg].view(-1, 1)).view(-1).exp()
    score[ids] = sc
    if twin is not None:
        t = twin[ids].long()
        score[torch.where(t >= 0, t, ids)] = sc
    return score

"""Plain restatements of the coalition operators: the replica builder (cal_coalition_count / cal_coalition_write) in torch, one
replica at a time; the case list both test files walk; the Shapley scores and the perturbation curves through the fp64 oracle's
eval forward on the restated replicas.  Everything on the CPU."""
import math

import torch

from tests.occlude_oracle import HEADS, _feat, _gid, hand_batch
from tests.subgraph_oracle import oracle_log_probs


def coalition_oracle(b, rep_graph, rep_row, rep_thresh, key, use="edges", invert=False):
    """-> dict(ptr, edge_ptr, batch, x, edge_index, node_src, edge_src, totals [5]) for a CPU source with grouped columns;
    ``key`` an integer tensor [K, M]."""
    x, ei, B = _feat(b), b.edge_index, int(b.num_graphs)
    K = int(key.size(0))
    ptr, eptr, batch, nsrc, esrc, cols_out, rows = [0], [0], [], [], [], [], []
    empty = mn = me = 0
    for r, (g, k, th) in enumerate(zip(*[[int(v) for v in t] for t in (rep_graph, rep_row, rep_thresh)])):
        n0 = ptr[-1]
        nodes, cols, new = torch.zeros(0, dtype=torch.long), torch.zeros(0, dtype=torch.long), torch.zeros(2, 0, dtype=torch.long)
        if 0 <= g < B:
            lo, hi = int(b.ptr[g]), int(b.ptr[g + 1])
            elo, ehi = int(b.edge_ptr[g]), int(b.edge_ptr[g + 1])
            nodes, cols = torch.arange(lo, hi), torch.arange(elo, ehi)
            ends = ei[:, cols]
            ok = ((ends >= lo) & (ends < hi)).all(0)                  # a column that leaves its graph is dropped
            local = ends - lo
            if 0 <= k < K:                                            # else the control replica: everything stays
                row = key[k].long()
                stay = (row >= th) if invert else (row < th)          # [M]
                if use == "edges":
                    ok &= stay[cols]
                elif hi > lo:
                    keep = stay[nodes]
                    new_id = torch.cumsum(keep.long(), 0) - keep.long()   # the staying nodes renumbered densely in their order
                    safe = local.clamp(0, hi - lo - 1)
                    ok &= keep[safe[0]] & keep[safe[1]]                   # a column stays iff both endpoints stay
                    local = new_id[safe]
                    nodes = nodes[keep]
            cols, new = cols[ok], (local + n0)[:, ok]
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


def check_coalition(res, b, rep_graph, rep_row, rep_thresh, key, use, invert):
    """``res`` (a coalition_batch result, any device) of the CPU source ``b``: equals the restatement bit for bit; structural
    properties on their own; node_src / edge_src reproduce the rows and the columns from the source."""
    r = coalition_oracle(b, rep_graph, rep_row, rep_thresh, key, use, invert)
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
    assert bool((ns[1:] > ns[:-1])[res.batch.cpu()[1:] == res.batch.cpu()[:-1]].all())     # kept nodes keep their order
    return r


# ---- the case list both test files walk (host twin on the CPU, HIP on the GPU) ---------------------------------------------
def _ring(n):
    return [(i, (i + 1) % n) for i in range(n)] + [((i + 1) % n, i) for i in range(n)]


def _keys(b, use, seed):
    """Three key rows: a permutation of every graph's elements; tied keys; keys that are no permutation, negative ones among
    them (elements that are always present without ``invert``)."""
    g = torch.Generator().manual_seed(seed)
    off = b.edge_ptr if use == "edges" else b.ptr
    M = int(off[-1])
    perm = torch.zeros(M, dtype=torch.int32)
    for lo, hi in zip(off[:-1].tolist(), off[1:].tolist()):
        perm[lo:hi] = torch.randperm(hi - lo, generator=g).to(torch.int32)
    tied = (torch.arange(M) - off[_gid(off)]).to(torch.int32) // 2
    wild = torch.randint(-2, 6, (M,), generator=g, dtype=torch.int32)
    return torch.stack([perm, tied, wild])


def _grid(b, use, rows=(0, 1, 2, -1, 3)):
    """Every graph at every key row of ``rows`` and the thresholds -3, 0, 1, n - 1, n, n + 5; then graph ids outside the batch."""
    off = b.edge_ptr if use == "edges" else b.ptr
    rg, rrow, rth = [], [], []
    for g in range(int(b.num_graphs)):
        n = int(off[g + 1] - off[g])
        for k in rows:
            for th in (-3, 0, 1, n - 1, n, n + 5):
                rg.append(g), rrow.append(k), rth.append(th)
    rg += [-1, 99, int(b.num_graphs)]
    rrow += [0, 1, -1]
    rth += [2, 2, 2]
    return torch.tensor(rg), torch.tensor(rrow), torch.tensor(rth)


def coalition_cases():
    """name -> (batch, rep_graph, rep_row, rep_thresh, key [K, M], use, invert), CPU tensors."""
    from cal_amd import spmotif
    from cal_amd.data import Batch
    from tests.occlude_oracle import occlude_cases
    out = {}
    # rings of 3 - 6 nodes; a 1-node graph with no edge; a graph with a self loop and duplicate columns
    rings = hand_batch([(n, _ring(n)) for n in (3, 4, 5, 6)] + [(1, []), (4, [(0, 0), (0, 1), (1, 0), (0, 1), (2, 3), (3, 2)])])
    for use in ("edges", "nodes"):
        key = _keys(rings, use, 1)
        for invert in (False, True):
            out["rings_%s%s" % (use, "_invert" if invert else "")] = (rings,) + _grid(rings, use) + (key, use, invert)
        none = torch.zeros(0, dtype=torch.long)
        out["none_" + use] = (rings, none, none, none, key, use, False)
        out["one_row_" + use] = (rings,) + _grid(rings, use, rows=(0,)) + (key[1:2], use, False)
    # a source column that leaves its graph's range (and one with a negative endpoint)
    lv = occlude_cases()["leaving_edges"][0]
    for use in ("edges", "nodes"):
        out["leaving_" + use] = (lv,) + _grid(lv, use) + (_keys(lv, use, 2), use, use == "nodes")
    # feat instead of x, no features, F = 4 and 16 (the vector row copy on the GPU), F = 5
    sp = Batch.from_data_list(spmotif.train_mix(6, node_num=7, seed=3))
    for F in (0, 4, 5, 16):
        c = Batch()
        c.__dict__.update(sp.__dict__)
        c.x, c.feat = None, None
        if F:
            c.feat = torch.randn(sp.batch.numel(), F, generator=torch.Generator().manual_seed(10 + F))
        use = "nodes" if F in (0, 5, 16) else "edges"
        out["feat%d" % F] = (c,) + _grid(c, use, rows=(0, 2, -1)) + (_keys(c, use, 3 + F), use, F == 16)
    for use in ("edges", "nodes"):
        out["spmotif_" + use] = (sp,) + _grid(sp, use, rows=(0, 1)) + (_keys(sp, use, 4), use, False)
    return out


# ---- keys the way the drivers make them ---------------------------------------------------------------------------------------
def representatives(twin, M):
    """bool [M]: one column per undirected edge (the lower column of a pair, an unpaired column, a self loop)."""
    return torch.ones(M, dtype=torch.bool) if twin is None else ~((twin >= 0) & (twin < torch.arange(M)))


def random_orders(b, S, use="edges", twin=None, elements=None, seed=0):
    """int32 [S, M]: S random orders of the players of the CPU batch ``b`` (grouped columns) as ``shapley(perms=...)`` takes them:
    per graph the players' positions 0 .. n_g - 1 (both columns of an undirected edge the same), -1 for any other element."""
    g = torch.Generator().manual_seed(seed)
    off = (b.edge_ptr if use == "edges" else b.ptr).tolist()
    M = off[-1]
    rep = representatives(twin, M)
    want = torch.ones(M, dtype=torch.bool) if elements is None else elements.clone()
    if twin is not None:
        want = want | (want[twin.clamp(min=0).long()] & (twin >= 0))
    keys = torch.full((S, M), -1, dtype=torch.int32)
    for s in range(S):
        for lo, hi in zip(off[:-1], off[1:]):
            pl = (lo + (rep & want)[lo:hi].nonzero().view(-1)).tolist()
            for pos, j in enumerate(torch.randperm(len(pl), generator=g).tolist()):
                keys[s, pl[j]] = pos
                if twin is not None and int(twin[pl[j]]) >= 0:
                    keys[s, int(twin[pl[j]])] = pos
    return keys


def rank_keys(score, b, use="edges", twin=None):
    """int32 [M]: every element's position inside its graph under ``score`` (descending, then index ascending; with ``twin`` the
    position of its undirected edge, whose two columns must carry one score)."""
    off = (b.edge_ptr if use == "edges" else b.ptr).tolist()
    M = off[-1]
    rep = representatives(twin, M)
    key = torch.full((M,), -1, dtype=torch.int32)
    for lo, hi in zip(off[:-1], off[1:]):
        ids = (lo + rep[lo:hi].nonzero().view(-1)).tolist()
        ids.sort(key=lambda e: (-float(score[e]), e))
        for pos, e in enumerate(ids):
            key[e] = pos
            if twin is not None and int(twin[e]) >= 0:
                assert float(score[int(twin[e])]) == float(score[e])
                key[int(twin[e])] = pos
    return key


# ---- the drivers through the fp64 oracle --------------------------------------------------------------------------------------
def _probs(name, sd64, h, r, R, yhat_r, **kw):
    lp = oracle_log_probs(name, sd64, r["x"], r["edge_index"], r["batch"], R, **kw)[h]
    return lp.gather(-1, yhat_r.view(-1, 1)).view(-1).exp()


def shapley_oracle(name, sd, b, yhat, keys, use="edges", head="o", **kw):
    """-> ``(score fp64 [M], p_full [B], p_empty [B], replicas)``: the Shapley estimate of the orders ``keys`` (int32 [S, M] as
    ``random_orders`` gives them; an element with a negative key is no player: always present, NaN) of the CPU batch ``b``
    through the fp64 oracle on the restated replicas.  ``yhat`` [B] is handed in.  A replica without a node is not run: 1 / C."""
    h = HEADS.index(head)
    sd64 = {k: v.double().cpu() for k, v in sd.items()}
    x, B = _feat(b).cpu(), int(b.num_graphs)
    yhat, keys = yhat.cpu(), keys.cpu()
    full = oracle_log_probs(name, sd64, x, b.edge_index.cpu(), b.batch.cpu(), B, **kw)[h]
    C = full.size(-1)
    p_full = full.gather(-1, yhat.view(-1, 1)).view(-1).exp()
    off = (b.edge_ptr if use == "edges" else b.ptr).tolist()
    S, M = keys.shape
    n = [int(keys[0, lo:hi].max()) + 1 if hi > lo else 0 for lo, hi in zip(off[:-1], off[1:])]
    skip = [use == "nodes" and hi > lo and bool((keys[0, lo:hi] >= 0).all()) for lo, hi in zip(off[:-1], off[1:])]
    rg, rrow, rth = [], [], []
    for s in range(S):
        for g in range(B):
            for t in range(1 if skip[g] else 0, n[g]):
                rg.append(g), rrow.append(s), rth.append(t)
    v = [[[1.0 / C if skip[g] else None] + [None] * (n[g] - 1) + [float(p_full[g])] if n[g] else [float(p_full[g])] for g in range(B)]
         for _ in range(S)]
    if rg:
        r = coalition_oracle(b, rg, rrow, rth, keys, use, False)
        assert r["totals"][4] == 0
        p = _probs(name, sd64, h, r, len(rg), yhat[torch.tensor(rg)], **kw).tolist()
        for g, s, t, val in zip(rg, rrow, rth, p):
            v[s][g][t] = val
    gid = _gid(torch.tensor(off)).tolist()
    score = torch.full((M,), float("nan"), dtype=torch.float64)
    for e in range(M):
        if int(keys[0, e]) >= 0:
            g = gid[e]
            score[e] = math.fsum(v[s][g][int(keys[s, e]) + 1] - v[s][g][int(keys[s, e])] for s in range(S)) / S
    p_empty = torch.tensor([math.fsum(v[s][g][0] for s in range(S)) / S for g in range(B)], dtype=torch.float64)
    return score, p_full, p_empty, len(rg)


def curve_oracle(name, sd, b, yhat, key, ratios, use="edges", head="o", **kw):
    """-> ``(insertion fp64 [B, T], deletion fp64 [B, T], p_full [B])`` of the CPU batch ``b`` under the ranking ``key`` (int32
    [M] as ``rank_keys`` gives it) through the fp64 oracle on the restated replicas.  A replica without a node: 1 / C."""
    h = HEADS.index(head)
    sd64 = {k: v.double().cpu() for k, v in sd.items()}
    x, B = _feat(b).cpu(), int(b.num_graphs)
    yhat, key = yhat.cpu(), key.cpu().view(1, -1)
    full = oracle_log_probs(name, sd64, x, b.edge_index.cpu(), b.batch.cpu(), B, **kw)[h]
    C = full.size(-1)
    p_full = full.gather(-1, yhat.view(-1, 1)).view(-1).exp()
    off = (b.edge_ptr if use == "edges" else b.ptr).tolist()
    n = [int(key[0, lo:hi].max()) + 1 if hi > lo else 0 for lo, hi in zip(off[:-1], off[1:])]
    out = []
    for invert in (False, True):
        tab = torch.full((B, len(ratios)), 1.0 / C, dtype=torch.float64)
        rg, rth, where = [], [], []
        for t, ratio in enumerate(ratios):
            for g in range(B):
                k = min(n[g], int(math.ceil(float(ratio) * n[g])))
                if use == "nodes" and (n[g] - k if invert else k) == 0:
                    continue
                rg.append(g), rth.append(k), where.append((g, t))
        if rg:
            r = coalition_oracle(b, rg, [0] * len(rg), rth, key, use, invert)
            assert r["totals"][4] == 0
            p = _probs(name, sd64, h, r, len(rg), yhat[torch.tensor(rg)], **kw)
            for (g, t), val in zip(where, p.tolist()):
                tab[g, t] = val
        out.append(tab)
    return out[0], out[1], p_full

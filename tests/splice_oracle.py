"""Plain-torch restatement of the batch splice contract (cal_graph_splice_count / cal_graph_splice_write) and of the
structure-intervention report through the fp64 oracle's eval forward.  Everything on the CPU: one pair at a time, arange,
boolean indexing and cat only."""
import torch

from tests.subgraph_oracle import extract_oracle, oracle_log_probs

BRIDGE = -(1 << 63)


def _feat(b):
    return b.x if getattr(b, "x", None) is not None else getattr(b, "feat", None)


def _part(b, g):
    """Node range, the valid columns (global ids) of graph ``g`` of ``b``; an id outside the batch: nothing."""
    B = int(b.num_graphs)
    if not 0 <= g < B:
        return 0, 0, torch.zeros(0, dtype=torch.long)
    lo, hi = int(b.ptr[g]), int(b.ptr[g + 1])
    cols = torch.arange(int(b.edge_ptr[g]), int(b.edge_ptr[g + 1]))
    ends = b.edge_index[:, cols]
    ok = ((ends >= lo) & (ends < hi)).all(0)                      # a column that leaves its graph is dropped
    return lo, hi, cols[ok]


def splice_oracle(a, b, ga=None, gb=None, bridge_a=None, bridge_b=None):
    """-> dict(ptr, edge_ptr, batch, x, edge_index, node_src, edge_src, totals [6]) for CPU sources with grouped columns."""
    ga = list(range(int(a.num_graphs))) if ga is None else [int(v) for v in ga]
    gb = list(range(int(b.num_graphs))) if gb is None else [int(v) for v in gb]
    assert len(ga) == len(gb)
    xa, xb = _feat(a), _feat(b)
    ptr, eptr, batch, nsrc, esrc, cols_out, rows = [0], [0], [], [], [], [], []
    empty = unput = mn = me = 0
    for p, (g, h) in enumerate(zip(ga, gb)):
        alo, ahi, ca = _part(a, g)
        blo, bhi, cb = _part(b, h)
        n0, an = ptr[-1], ahi - alo
        na, nb = torch.arange(alo, ahi), torch.arange(blo, bhi)
        nsrc += [na, -1 - nb]
        if xa is not None:
            rows += [xa[na], xb[nb]]
        n = an + (bhi - blo)
        batch.append(torch.full((n,), p, dtype=torch.long))
        cols_out += [a.edge_index[:, ca] - alo + n0, b.edge_index[:, cb] - blo + n0 + an]
        esrc += [ca, -1 - cb]
        m = ca.numel() + cb.numel()
        ba = int(bridge_a[p]) if bridge_a is not None else -1
        bb = int(bridge_b[p]) if bridge_b is not None else -1
        if ba >= 0 and bb >= 0 and alo <= ba < ahi and blo <= bb < bhi:
            u, v = n0 + ba - alo, n0 + an + bb - blo
            cols_out.append(torch.tensor([[u, v], [v, u]]))
            esrc.append(torch.tensor([BRIDGE, BRIDGE]))
            m += 2
        elif ba >= 0 or bb >= 0:
            unput += 1
        ptr.append(n0 + n)
        eptr.append(eptr[-1] + m)
        empty += n == 0
        mn, me = max(mn, n), max(me, m)
    cat = lambda ts, d=0: torch.cat(ts, d) if ts else torch.zeros(0, dtype=torch.long)
    ei = torch.cat(cols_out, 1).contiguous() if cols_out else torch.zeros(2, 0, dtype=torch.long)
    x = None
    if xa is not None:
        x = torch.cat(rows) if rows else xa[:0]
    return dict(ptr=torch.tensor(ptr), edge_ptr=torch.tensor(eptr), batch=cat(batch), x=x, edge_index=ei, node_src=cat(nsrc),
                edge_src=cat(esrc), totals=[ptr[-1], eptr[-1], mn, me, empty, unput])


def _bridge_ids(a, b, ga, gb, bridge):
    """The bridge argument of splice_batches as two id tensors (``"first"``: the first node of each part)."""
    if bridge is None:
        return None, None
    if isinstance(bridge, str):
        assert bridge == "first"
        ga = list(range(int(a.num_graphs))) if ga is None else [int(v) for v in ga]
        gb = list(range(int(b.num_graphs))) if gb is None else [int(v) for v in gb]
        first = lambda s, g: int(s.ptr[g]) if 0 <= g < int(s.num_graphs) else -1
        return torch.tensor([first(a, g) for g in ga]), torch.tensor([first(b, g) for g in gb])
    return bridge


def check_splice(res, a, b, ga=None, gb=None, bridge=None):
    """``res`` (a splice_batches result, any device) of the CPU sources ``a``, ``b``: equals the restatement bit for bit; the
    structural properties on their own; node_src / edge_src reproduce the rows and the rewritten endpoints from the sources."""
    ba, bb = _bridge_ids(a, b, ga, gb, bridge)
    r = splice_oracle(a, b, ga, gb, ba, bb)
    ei, ptr, eptr = res.edge_index.cpu(), res.ptr.cpu(), res.edge_ptr.cpu()
    assert torch.equal(ei, r["edge_index"]) and res.edge_index.is_contiguous() and ei.shape == (2, r["totals"][1])
    assert torch.equal(ptr, r["ptr"]) and torch.equal(eptr, r["edge_ptr"])
    assert torch.equal(res.batch.cpu(), r["batch"])
    assert torch.equal(res.node_src.cpu(), r["node_src"]) and torch.equal(res.edge_src.cpu(), r["edge_src"])
    rx = _feat(res)
    if r["x"] is None:
        assert rx is None
    else:
        assert rx.dtype == torch.float32 and torch.equal(rx.cpu(), r["x"]) and (res.x is None) == (a.x is None)
    n2, e2 = int(res.batch.numel()), int(ei.size(1))
    assert [n2, e2, res.max_nodes, res.max_edges, res.empty_graphs, res.bridges_unwritten] == r["totals"]
    P = len(r["ptr"]) - 1
    assert res.num_graphs == P and res.tile_ptr is None
    assert res.no_self_loops == (bool(a.no_self_loops) and bool(b.no_self_loops))
    gal = list(range(int(a.num_graphs))) if ga is None else [int(v) for v in ga]
    if a.y is None or any(not 0 <= g < int(a.num_graphs) for g in gal):
        assert res.y is None
    else:
        assert torch.equal(res.y.cpu(), a.y.view(-1)[torch.tensor(gal, dtype=torch.long)])
    # independent of the restatement
    assert int(ptr[0]) == 0 and int(ptr[-1]) == n2 and int(eptr[0]) == 0 and int(eptr[-1]) == e2
    assert bool((ptr[1:] >= ptr[:-1]).all()) and bool((eptr[1:] >= eptr[:-1]).all())
    gid_e = torch.repeat_interleave(torch.arange(P), eptr[1:] - eptr[:-1])
    assert bool(((ei >= ptr[gid_e]) & (ei < ptr[gid_e + 1])).all())
    assert torch.equal(res.batch.cpu(), torch.repeat_interleave(torch.arange(P), ptr[1:] - ptr[:-1]))
    # the source maps
    ns, es = res.node_src.cpu(), res.edge_src.cpu()
    xa, xb = _feat(a), _feat(b)
    if xa is not None:
        from_a = ns >= 0
        assert torch.equal(rx.cpu()[from_a], xa[ns[from_a]]) and torch.equal(rx.cpu()[~from_a], xb[-1 - ns[~from_a]])
    is_br = es == BRIDGE
    ca, cb = (es >= 0), (es < 0) & ~is_br
    assert torch.equal(ns[ei[:, ca]], a.edge_index[:, es[ca]])               # a's columns: the endpoints' sources are a's ids
    assert torch.equal(-1 - ns[ei[:, cb]], b.edge_index[:, -1 - es[cb]])
    if bool(is_br.any()):
        cols, gp = ei[:, is_br], gid_e[is_br]
        assert cols.size(1) % 2 == 0 and torch.equal(cols[:, 0::2], cols[:, 1::2].flip(0))
        assert torch.equal(ns[cols[0, 0::2]], ba[gp[0::2]]) and torch.equal(-1 - ns[cols[1, 0::2]], bb[gp[0::2]])
    return r


# ---- the case list both test files walk (host twin on the CPU, HIP on the GPU) ---------------------------------------------
def _with_feat(b, F, seed):
    """``b`` with fresh features of F columns (F = 0: none)."""
    from cal_amd.data import Batch
    c = Batch()
    c.__dict__.update(b.__dict__)
    c.x = torch.randn(b.batch.numel(), F, generator=torch.Generator().manual_seed(seed)) if F else None
    c.feat = None
    return c


def splice_cases():
    """name -> (a, b, pairs_a, pairs_b, bridge), CPU batches; pairs ``None`` = the default."""
    from cal_amd import spmotif
    from cal_amd.data import Batch, Data
    from tests.helpers import random_graph_batch
    g = torch.Generator().manual_seed(0)
    a = random_graph_batch(num_graphs=9, n_lo=3, n_hi=30, feat=5, seed=1)
    b = random_graph_batch(num_graphs=9, n_lo=3, n_hi=30, feat=5, seed=2)
    b4 = random_graph_batch(num_graphs=4, n_lo=1, n_hi=9, feat=5, seed=3)
    out = {}
    out["identity"] = (a, b, None, None, None)
    out["permutation"] = (a, b, None, torch.randperm(9, generator=g), None)
    out["repeats"] = (a, b, torch.randint(0, 9, (14,), generator=g), torch.randint(0, 9, (14,), generator=g), None)
    out["sizes_differ"] = (a, b4, None, torch.arange(9) % 4, None)
    out["few_of_many"] = (b4, a, torch.tensor([3, 3]), torch.tensor([8, 0]), None)
    absent = (torch.tensor([0, -1, 2, -1, 4, 99, 1]), torch.tensor([1, 3, -1, -1, -7, 2, 9]))
    out["absent_parts"] = (a, b, absent[0], absent[1], None)
    ds = [Data(x=torch.randn(4, 3, generator=g), edge_index=torch.tensor([[0, 1, 2, 3], [1, 0, 3, 2]]), y=torch.tensor([0])),
          Data(x=torch.randn(5, 3, generator=g), edge_index=torch.zeros(2, 0, dtype=torch.long), y=torch.tensor([1])),
          Data(x=torch.randn(3, 3, generator=g), edge_index=torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]]), y=torch.tensor([2]))]
    be = Batch.from_data_list(ds)
    out["edgeless_source"] = (be, be, torch.tensor([1, 0, 1, 2]), torch.tensor([1, 1, 2, 0]), "first")
    for F in (0, 3, 4, 16):
        out["feat%d" % F] = (_with_feat(a, F, 10 + F), _with_feat(b, F, 20 + F), None, torch.randperm(9, generator=g), None)
    out["bridge_first"] = (a, b, None, torch.randperm(9, generator=g), "first")
    out["bridge_first_absent"] = (a, b, absent[0], absent[1], "first")
    la, lb = a.ptr[1:] - a.ptr[:-1], b.ptr[1:] - b.ptr[:-1]
    ia = a.ptr[:-1] + torch.randint(0, 1 << 20, (9,), generator=g) % la
    ib = b.ptr[:-1] + torch.randint(0, 1 << 20, (9,), generator=g) % lb
    out["bridge_explicit"] = (a, b, None, None, (ia, ib))
    wa, wb = ia.clone(), ib.clone()
    wa[1] = a.ptr[3]                                  # a node of another graph
    wb[2] = b.batch.numel() + 5                       # no node at all
    wa[4], wb[5] = -1, -1                             # half a bridge
    wa[6] = wb[6] = -1                                # none
    out["bridge_invalid"] = (a, b, None, None, (wa, wb))
    ba7 = torch.tensor([int(a.ptr[0]), 3, int(a.ptr[2]), -1, int(a.ptr[4]), 0, int(a.ptr[1])])
    bb7 = torch.tensor([int(b.ptr[1]), int(b.ptr[3]), 0, -1, 2, int(b.ptr[2]), -1])
    out["bridge_absent_part"] = (a, b, absent[0], absent[1], (ba7, bb7))
    # a source column that leaves its graph's range (and one with a negative endpoint)
    lv = Batch()
    lv.x, lv.edge_index, lv.batch = torch.randn(6, 2, generator=g), torch.tensor([[0, 1, 2, 3, 9, 4], [1, 0, 3, 5, 0, -1]]), \
        torch.tensor([0, 0, 0, 1, 1, 1])
    lv.ptr, lv.edge_ptr, lv.num_graphs, lv.max_nodes, lv.max_edges = torch.tensor([0, 3, 6]), torch.tensor([0, 3, 6]), 2, 3, 3
    lv.y, lv.no_self_loops = torch.tensor([0, 1]), True
    out["leaving_column"] = (lv, lv, torch.tensor([0, 1, 1]), torch.tensor([1, 0, 1]), "first")
    sa = Batch.from_data_list(spmotif.train_mix(32, node_num=7, seed=3))
    sb = Batch.from_data_list(spmotif.train_mix(32, node_num=7, seed=4))
    out["spmotif"] = (sa, sb, None, torch.randperm(32, generator=g), "first")
    return out


# ---- the report through the fp64 oracle ---------------------------------------------------------------------------------------
class _Part:
    """An extract_oracle result as a splice source."""

    def __init__(self, r, B):
        self.x, self.feat, self.edge_index, self.ptr, self.edge_ptr, self.num_graphs = r["x"], None, r["edge_index"], r["ptr"], \
            r["edge_ptr"], B


def structure_oracle(name, sd, b, node_mask, rows, bridge=None, **kw):
    """The sums of cal_amd.splice.structure_intervention for the causal node mask ``node_mask`` (bool [N], in b's order) and the
    partner permutations ``rows`` [m, B], through the fp64 oracle on the restatement's batches.  -> dict(num [3, 6], differ,
    pairs, graphs, margin [3, 2 + m, B] (top-two log-probability gap on the whole batch, the identity splice, every swap),
    pair [m, B] (j != g), differ [m, B])."""
    sd64 = {k: v.double().cpu() for k, v in sd.items()}
    x = _feat(b).cpu()
    ei, B, y = b.edge_index.cpu(), int(b.num_graphs), b.y.view(-1).cpu()
    rows = rows.cpu()
    nm = node_mask.cpu().bool()
    parts = [_Part(extract_oracle(ei, b.ptr, b.edge_ptr, x.size(0), node_keep=nm, complement=c, relabel=True, x=x), B)
             for c in (False, True)]
    lps = [oracle_log_probs(name, sd64, x, ei, b.batch.cpu(), B, **kw)]
    for perm in [torch.arange(B)] + list(rows):
        ba, bb = _bridge_ids(parts[0], parts[1], None, perm, bridge)
        r = splice_oracle(parts[0], parts[1], None, perm, ba, bb)
        assert r["totals"][4] == 0
        lps.append(oracle_log_probs(name, sd64, r["x"], r["edge_index"], r["batch"], B, **kw))
    lp = torch.stack(lps, 1)                                           # [3, 2 + m, B, C]
    top2 = lp.topk(2, -1).values
    pred = lp.argmax(-1)                                               # [3, 2 + m, B]
    yhat = pred[:, 0]
    pair = rows != torch.arange(B).view(1, B)
    yj = y[rows]
    differ = pair & (yj != y)
    p = lp.gather(-1, yhat.view(3, 1, B, 1).expand(3, lp.size(1), B, 1)).squeeze(-1).exp()
    num = torch.stack([(yhat == y).sum(-1).double(), (pred[:, 1] == y).sum(-1).double(),
                       ((pred[:, 2:] == y) & pair).sum((1, 2)).double(), ((pred[:, 2:] == yj) & differ).sum((1, 2)).double(),
                       ((pred[:, 2:] == yhat.unsqueeze(1)) & pair).sum((1, 2)).double(),
                       ((p[:, :1] - p[:, 2:]) * pair).sum((1, 2))], 1)              # [3, 6]
    return dict(num=num, n_differ=int(differ.sum()), pairs=int(pair.sum()), graphs=B, margin=top2[..., 0] - top2[..., 1],
                pair=pair, differ=differ, kept=int(nm.sum()), total=nm.numel())


HEADS = ("c", "o", "co")
KEYS = ("acc_full", "acc_self", "acc_swap", "follow", "agree", "p_shift")


def check_structure(res, parts, tol, cap=0.05):
    """``res`` (a structure_intervention / eval_structure_intervention report) against the structure_oracle results ``parts`` of
    its mini-batches: the probability metric within ``tol``; hit counts may differ only by (head, pair) entries whose oracle
    top-two gap is within 10 tol, at most ``cap`` of all entries; the whole graph's argmax must be unambiguous."""
    num = sum(q["num"] for q in parts)
    n, pairs, n_differ = (sum(q[k] for q in parts) for k in ("graphs", "pairs", "n_differ"))
    unsure = torch.cat([q["margin"] <= 10 * tol for q in parts], -1)              # [3, 2 + m, B_total]
    pair, differ = torch.cat([q["pair"] for q in parts], -1), torch.cat([q["differ"] for q in parts], -1)
    print("structure check: tol %g, near-ties %d of %d" % (tol, int(unsure.sum()), unsure.numel()))
    assert not bool(unsure[:, 0].any()), "the whole graph's argmax must be unambiguous in the oracle (pick another seed)"
    assert unsure.double().mean().item() <= cap
    assert res["graphs"] == n and res["pairs"] == pairs
    den = (n, n, pairs, n_differ, pairs, pairs)
    for h, head in enumerate(HEADS):
        slack = (0, int(unsure[h, 1].sum()), int((unsure[h, 2:] & pair).sum()), int((unsure[h, 2:] & differ).sum()),
                 int((unsure[h, 2:] & pair).sum()))
        for j, key in enumerate(KEYS):
            got, want = res["%s_%s" % (key, head)], (num[h, j].item() / den[j] if den[j] else float("nan"))
            print("  %s_%s: %.9f vs %.9f" % (key, head, got, want))
            if want != want:
                assert got != got, (key, head)
            elif key == "p_shift":
                assert abs(got - want) <= tol, (key, head, got, want)
            else:
                assert abs(got - want) * den[j] <= slack[j] + 1e-6, (key, head, got, want, slack[j])
    kept, total = sum(q["kept"] for q in parts), sum(q["total"] for q in parts)
    assert abs(res["sparsity"] - (1.0 - kept / total)) < 1e-12

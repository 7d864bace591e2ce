"""Plain restatements of the counterfactual operators: the subset replica rule (cal_subset_count / cal_subset_write) and the beam
step (cal_beam_step) over Python lists and Python ints -- no torch inside the rules --, each with seedable defects; the case
lists both test files walk; a brute-force minimum flip search, a greedy loop over occlude_batch and a prefix loop over
coalition_batch for the drivers.  Everything on the CPU."""
import itertools
import math

import torch

from tests.occlude_oracle import _feat, hand_batch

SUBSET_DEFECTS = ("twin not toggled", "off by one at a word edge", "absent bit read as present", "mode-1 endpoints not rewritten")
BEAM_DEFECTS = ("duplicate kept from the later parent", "tie-break by rep_flip dropped")


# ---- the subset rule in Python ints -------------------------------------------------------------------------------------------
def _clamp_seg(p, g, M):
    lo = min(max(p[g], 0), M)
    hi = min(max(p[g + 1], lo), M)
    return lo, hi - lo


def _bit(row, W, j, defect=None):
    """bit j of a row of W words (``None``: everything present)"""
    if row is None:
        return True
    if j >= 32 * W:
        return defect == "absent bit read as present"
    w = j >> 5
    if defect == "off by one at a word edge" and j & 31 == 0 and j > 0:
        w -= 1
    return bool((row[w] >> (j & 31)) & 1)


def _flips(f, lo, m, twin, defect=None):
    """the local indices a flip toggles"""
    if not 0 <= f < m:
        return ()
    out = [f]
    if twin is not None and defect != "twin not toggled":
        t = twin[lo + f] - lo
        if 0 <= t < m and t != f:
            out.append(t)
    return tuple(out)


def subset_rule(ei, E, N, ptr, eptr, B, bits, K, W, rep_graph, rep_row, rep_flip, twin, mode, max_nodes, defect=None):
    """Lists of Python ints in, lists of Python ints out: ``ei`` = (sources, targets), ``bits`` K rows of W words in [0, 2^32).
    -> dict(ptr, edge_ptr, batch, node_src, edge_src, edge_index (two lists), totals [5])."""
    o_ptr, o_eptr, batch, nsrc, esrc, ou, ov = [0], [0], [], [], [], [], []
    mn = me = empty = 0
    for r, (g, k, f) in enumerate(zip(rep_graph, rep_row, rep_flip)):
        n0 = o_ptr[-1]
        nodes, cols = [], []
        if 0 <= g < B:
            nlo, nn = _clamp_seg(ptr, g, N)
            elo, em = _clamp_seg(eptr, g, E)
            if mode == 1 and nn > max_nodes:
                nlo = nn = elo = em = 0
            row = bits[k] if 0 <= k < K else None
            fl = _flips(f, elo, em, twin, defect) if mode == 0 else _flips(f, nlo, nn, None)
            stays = lambda j: _bit(row, W, j, defect) != (j in fl)
            if mode == 0:
                nodes = list(range(nlo, nlo + nn))
                new = {s: s - nlo for s in nodes}
            else:
                nodes = [nlo + l for l in range(nn) if stays(l)]
                new = {s: i for i, s in enumerate(nodes)}
                if defect == "mode-1 endpoints not rewritten":
                    new = {s: s - nlo for s in nodes}
            for e in range(elo, elo + em):
                u, v = ei[0][e], ei[1][e]
                if not (nlo <= u < nlo + nn and nlo <= v < nlo + nn):
                    continue                                              # a column that leaves its graph is dropped
                if stays(e - elo) if mode == 0 else (u in new and v in new):
                    cols.append(e)
                    ou.append(n0 + new[u])
                    ov.append(n0 + new[v])
        nsrc += nodes
        esrc += cols
        batch += [r] * len(nodes)
        o_ptr.append(n0 + len(nodes))
        o_eptr.append(o_eptr[-1] + len(cols))
        mn, me, empty = max(mn, len(nodes)), max(me, len(cols)), empty + (not nodes)
    return dict(ptr=o_ptr, edge_ptr=o_eptr, batch=batch, node_src=nsrc, edge_src=esrc, edge_index=(ou, ov),
                totals=[o_ptr[-1], o_eptr[-1], mn, me, empty])


def _u32(t):
    """an int32 tensor's words as Python ints in [0, 2^32)"""
    return [[int(v) & 0xFFFFFFFF for v in row] for row in t.tolist()]


def subset_oracle(c, defect=None):
    """The restatement of case ``c`` (a dict of ``subset_cases``) -> the rule's dict as tensors, plus ``x``."""
    b, bits, use = c["b"], c["bits"], c["use"]
    mode = 0 if use == "edges" else 1
    E, N, B = int(b.edge_index.size(1)), int(b.batch.numel()), int(b.num_graphs)
    K, W = (0, 0) if bits is None else (int(bits.size(0)), int(bits.size(1)))
    mx = max([0] + (b.ptr[1:] - b.ptr[:-1]).tolist())
    r = subset_rule(b.edge_index.tolist(), E, N, b.ptr.tolist(), b.edge_ptr.tolist(), B, [] if bits is None else _u32(bits), K, W,
                    c["rg"].tolist(), c["rrow"].tolist(), c["rflip"].tolist(), None if c["twin"] is None else c["twin"].tolist(),
                    mode, mx, defect)
    out = {k: torch.tensor(v, dtype=torch.long) for k, v in r.items() if k not in ("edge_index", "totals")}
    out["edge_index"] = torch.tensor(r["edge_index"], dtype=torch.long).view(2, -1)
    out["totals"] = r["totals"]
    x = _feat(b)
    out["x"] = None if x is None else x[out["node_src"]]
    return out


_WANT = {}


def subset_want(name):
    """The restatement of case ``name``, computed once for the CPU and the GPU test."""
    if name not in _WANT:
        _WANT[name] = subset_oracle(subset_cases()[name])
    return _WANT[name]


def check_subset(res, c, r):
    """``res`` (a subset_batch result, any device) of case ``c`` equals the restatement ``r`` bit for bit; structural properties
    on their own."""
    b = c["b"]
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
    rg = c["rg"].tolist()
    if b.y is None or any(not 0 <= g < int(b.num_graphs) for g in rg):
        assert res.y is None
    else:
        assert torch.equal(res.y.cpu(), b.y.view(-1)[c["rg"]])
    # independent of the restatement
    assert int(ptr[0]) == 0 and int(ptr[-1]) == n2 and int(eptr[0]) == 0 and int(eptr[-1]) == e2
    gid_e = torch.repeat_interleave(torch.arange(R), eptr[1:] - eptr[:-1])
    assert bool(((ei >= ptr[gid_e]) & (ei < ptr[gid_e + 1])).all())
    ns, es = res.node_src.cpu(), res.edge_src.cpu()
    assert torch.equal(ns[ei], b.edge_index[:, es])                       # the endpoints' sources are the source column's


def same_subset(r1, r2):
    return all(torch.equal(r1[k], r2[k]) for k in ("ptr", "edge_ptr", "batch", "node_src", "edge_src", "edge_index")) \
        and r1["totals"] == r2["totals"]


# ---- the subset case list -----------------------------------------------------------------------------------------------------
def _rand_bits(K, W, g):
    return torch.randint(-2 ** 31, 2 ** 31, (K, W), generator=g, dtype=torch.long).to(torch.int32)


def _seg_graphs(use, g):
    """Graphs whose element segments have 0, 1, 31, 32, 33, 64 and 65 elements (the word edges): columns over five nodes, self loops
    and duplicates among them (``use="edges"``), or nodes with a few columns each."""
    out = []
    for m in (0, 1, 31, 32, 33, 64, 65):
        if use == "edges":
            out.append((5, [tuple(torch.randint(0, 5, (2,), generator=g).tolist()) for _ in range(m)]))
        else:
            out.append((m, [tuple(torch.randint(0, m, (2,), generator=g).tolist()) for _ in range(2 * m)] if m else []))
    return out


def _grid(b, use, K, g, extra=()):
    """Per graph: its rows (a sample of [0, K), the control row -1 and the row K) x the flips -1, 0, 1, m - 1, m, m + 5 and two
    random ones; then graph ids outside the batch."""
    off = (b.edge_ptr if use == "edges" else b.ptr).tolist()
    rg, rrow, rflip = [], [], []
    for gi in range(int(b.num_graphs)):
        m = off[gi + 1] - off[gi]
        rows = sorted(set(torch.randint(0, max(K, 1), (3,), generator=g).tolist())) + [-1, K]
        for k in rows:
            for f in [-1, 0, 1, m - 1, m, m + 5] + torch.randint(0, max(m, 1), (2,), generator=g).tolist():
                rg.append(gi), rrow.append(k), rflip.append(f)
    B = int(b.num_graphs)
    rg += [-1, B + 7, B] + list(extra)
    rrow += [0, 1, -1] + [0] * len(extra)
    rflip += [0, 0, 0] + [0] * len(extra)
    return torch.tensor(rg), torch.tensor(rrow), torch.tensor(rflip)


def _case(b, bits, grid, twin, use):
    return dict(b=b, bits=bits, rg=grid[0], rrow=grid[1], rflip=grid[2], twin=twin, use=use)


_CASES = {}


def subset_cases():
    """name -> dict(b, bits int32 [K, W] or None, rg, rrow, rflip, twin or None, use), CPU tensors."""
    if _CASES:
        return _CASES
    from cal_amd import spmotif, synth
    from cal_amd.data import Batch
    from cal_amd.explain import edge_twins
    from tests.occlude_oracle import occlude_cases
    out = _CASES
    g = torch.Generator().manual_seed(11)
    # the word edges, with W exactly enough for the longest segment (3), one word short for it (2) and short for most (1)
    for use in ("edges", "nodes"):
        b = hand_batch(_seg_graphs(use, g) + [(1, []), (3, [])], F=3, seed=2)        # ... a one-node graph, a graph without edges
        tw = edge_twins(b)[0] if use == "edges" else None
        for W in (3, 2, 1):
            bits = _rand_bits(6, W, g)
            out["words_%s_W%d" % (use, W)] = _case(b, bits, _grid(b, use, 6, g), tw, use)
        out["words_%s_W0" % use] = _case(b, torch.zeros(2, 0, dtype=torch.int32), _grid(b, use, 2, g), tw, use)
        out["words_%s_K0" % use] = _case(b, None, _grid(b, use, 0, g), tw, use)
        none = torch.zeros(0, dtype=torch.long)
        out["none_" + use] = _case(b, _rand_bits(2, 3, g), (none, none, none), tw, use)
    # a flip onto a cleared bit sets it again: row 0 is empty, row 1 full; every element of every graph flipped once in each
    b = hand_batch([(4, [(0, 1), (1, 0), (1, 2), (2, 1), (2, 3), (3, 2), (0, 0)]), (3, [(0, 1), (1, 2), (2, 0)])], F=3, seed=3)
    for use in ("edges", "nodes"):
        off = (b.edge_ptr if use == "edges" else b.ptr).tolist()
        rg = [gi for gi in range(2) for _ in range(off[gi + 1] - off[gi]) for _ in range(2)]
        rflip = [j for gi in range(2) for j in range(off[gi + 1] - off[gi]) for _ in range(2)]
        rrow = [0, 1] * (len(rg) // 2)
        bits = torch.tensor([[0], [-1]], dtype=torch.int32)
        out["set_again_" + use] = _case(b, bits, (torch.tensor(rg), torch.tensor(rrow), torch.tensor(rflip)),
                                        edge_twins(b)[0] if use == "edges" else None, use)
    # a self loop (its own twin), a column without a twin, a twin outside the segment, and no twin map at all
    ring = [(0, 1), (1, 2), (2, 0), (1, 0), (2, 1), (0, 2)]
    mix = hand_batch([(1, []), (4, [(0, 0), (0, 1), (1, 0), (0, 1), (1, 0), (2, 3), (1, 2), (2, 1)]), (3, ring)])
    tw = edge_twins(mix)[0].clone()
    lo = int(mix.edge_ptr[1])
    tw[lo + 1] = int(mix.edge_ptr[2])                                     # the first column of the NEXT graph: outside the segment
    for name, t in (("twin_outside", tw), ("twin_none", None), ("twin", edge_twins(mix)[0])):
        out[name] = _case(mix, _rand_bits(4, 1, g), _grid(mix, "edges", 4, g), t, "edges")
    # a source column that leaves its graph's node range (and one with a negative endpoint)
    lv = occlude_cases()["leaving_edges"][0]
    for use in ("edges", "nodes"):
        out["leaving_" + use] = _case(lv, _rand_bits(3, 1, g), _grid(lv, use, 3, g), edge_twins(lv)[0] if use == "edges" else None, use)
    # F = 0 (no rows), 3 (the scalar row copy), 4 (the vector row copy); feat instead of x
    sp = Batch.from_data_list(spmotif.train_mix(6, node_num=5, seed=3))          # (at most 37 nodes a graph)
    tws = edge_twins(sp)[0]
    for F in (0, 3, 4):
        for use in ("edges", "nodes"):
            c = Batch()
            c.__dict__.update(sp.__dict__)
            c.x, c.feat = None, None
            if F:
                c.feat = torch.randn(sp.batch.numel(), F, generator=torch.Generator().manual_seed(10 + F))
            W = -(-(sp.max_edges if use == "edges" else sp.max_nodes) // 32)
            out["feat%d_%s" % (F, use)] = _case(c, _rand_bits(5, W, g), _grid(c, use, 5, g), tws if use == "edges" else None, use)
    for use in ("edges", "nodes"):
        W = -(-(sp.max_edges if use == "edges" else sp.max_nodes) // 32)
        out["spmotif_" + use] = _case(sp, _rand_bits(8, W, g), _grid(sp, use, 8, g), tws if use == "edges" else None, use)
    # R beyond one scan run per thread: 700 replicas, a third of them of no graph
    for use in ("edges", "nodes"):
        W = -(-(sp.max_edges if use == "edges" else sp.max_nodes) // 32)
        rg = torch.randint(-3, 6, (700,), generator=g).clamp(min=-1)
        out["scan_" + use] = _case(sp, _rand_bits(16, W, g), (rg, torch.randint(-1, 17, (700,), generator=g),
                                                               torch.randint(-1, 40, (700,), generator=g)),
                                   tws if use == "edges" else None, use)
    # a 5000-node graph between 3-node ones, with columns that leave its node range; W enough (edges: 2048 bits of ~20 000: short)
    big = synth.ba_graphs(1, n=5000, seed=1)[0]
    F = int(_feat(big).size(1))
    small = []
    for _ in range(4):
        d = type(big)(edge_index=torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]]), y=torch.zeros(1, dtype=torch.long))
        d.x, d.feat = (torch.randn(3, F, generator=g), None) if big.x is not None else (None, torch.randn(3, F, generator=g))
        small.append(d)
    bb = Batch.from_data_list(small[:2] + [big] + small[2:])
    bb.edge_index = bb.edge_index.clone()
    lo = int(bb.edge_ptr[2])
    bb.edge_index[0, lo + 1500] = 0
    bb.edge_index[1, lo + 7777] = int(bb.ptr[3])
    twb = edge_twins(bb)[0]
    for use, W in (("edges", 64), ("nodes", 157)):
        m = int(bb.edge_ptr[3] - bb.edge_ptr[2]) if use == "edges" else 5000
        grid = (torch.tensor([0, 1, 2, 3, 4, 2, 2, 2]), torch.tensor([0, 1, 0, 1, 0, 1, -1, 2]),
                torch.tensor([1, -1, 40, 2, 0, m - 1, 4999, -1]))
        out["large_" + use] = _case(bb, _rand_bits(2, W, g), grid, twb if use == "edges" else None, use)
    return out


# ---- the beam step in Python ints ---------------------------------------------------------------------------------------------
def score_key(u):
    """rules.hpp score_key on the bit pattern ``u`` of a float32"""
    if (u & 0x7F800000) == 0x7F800000 and (u & 0x007FFFFF):
        return 1                                                          # NaN: below every number
    if (u & 0x7FFFFFFF) == 0:
        u = 0                                                             # -0 ranks as +0
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def beam_rule(bits, B, beam, W, n_state, cand_ptr, rep_row, rep_flip, pbits, flipped, seg_ptr, M, twin, max_cand, done, cf_bits,
              cf_p, cf_cand, defect=None):
    """Lists of Python ints in (``pbits``, ``cf_p``: the bit patterns of the floats; ``bits`` B beam rows of W words) -> dict of
    lists: bits_out, p_out, n_out, status, done, cf_bits, cf_p, cf_cand (the last four updated copies)."""
    R = len(rep_row)
    bits_out = [[0] * W for _ in range(B * beam)]
    p_out, n_out, status = [0] * (B * beam), [0] * B, [0] * B
    done, cf_bits, cf_p, cf_cand = list(done), [list(r) for r in cf_bits], list(cf_p), list(cf_cand)
    for g in range(B):
        clo, cn = _clamp_seg(cand_ptr, g, R)
        if done[g] or cn == 0:
            continue
        if cn > max_cand:
            status[g] = 2
            continue
        lo, m = _clamp_seg(seg_ptr, g, M)
        live = min(max(n_state[g], 0), beam)
        top = min(m, 32 * W)
        full = [((1 << max(0, min(32, top - 32 * w))) - 1) for w in range(W)]

        def child(i):
            s = rep_row[i] - g * beam
            row = list(bits[g * beam + s]) if 0 <= s < live else list(full)
            for j in _flips(rep_flip[i], lo, m, twin):
                if j < 32 * W:
                    row[j >> 5] ^= 1 << (j & 31)
            return tuple(row)

        def order(i):
            key = (0 if flipped[i] else 1, score_key(pbits[i]), rep_row[i])
            return key + ((i,) if defect == "tie-break by rep_flip dropped" else (rep_flip[i], i))

        ord_ = sorted(range(clo, clo + cn), key=order)
        if flipped[ord_[0]]:
            done[g], cf_bits[g], cf_p[g], cf_cand[g] = 1, list(child(ord_[0])), pbits[ord_[0]], ord_[0]
            continue
        picked = {}                                                       # child -> the candidate that stands for it
        for i in ord_:
            ch = child(i)
            if ch in picked:
                if defect == "duplicate kept from the later parent":
                    picked[ch] = i
                continue
            if len(picked) == beam:
                if defect == "duplicate kept from the later parent":
                    continue
                break
            picked[ch] = i
        for s, (ch, i) in enumerate(picked.items()):
            bits_out[g * beam + s], p_out[g * beam + s] = list(ch), pbits[i]
        n_out[g] = len(picked)
    return dict(bits_out=bits_out, p_out=p_out, n_out=n_out, status=status, done=done, cf_bits=cf_bits, cf_p=cf_p, cf_cand=cf_cand)


_P_VALUES = [0.0, -0.0, 0.25, 0.25, 0.5, 0.75, 1.0, float("nan"), 1e-30, -1.0, 0.1]      # few values: forced ties


def _beam_case(seed, beam, max_cand, counts, m_hi=9, W=None, flip_rate=0.03):
    """Random inputs of one beam step: graph g has ``counts[g]`` candidates (``None``: a few), segments of up to ``m_hi`` elements
    paired (2j, 2j + 1) by the twin map with a self twin and a twin outside the segment among them."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi: int(torch.randint(lo, hi, (1,), generator=g))
    B = len(counts)
    ms = [ri(0, m_hi + 1) for _ in range(B)]
    ms[0] = m_hi
    seg = [0]
    for m in ms:
        seg.append(seg[-1] + m)
    M = seg[-1]
    W = max(1, -(-m_hi // 32)) if W is None else W
    twin = []
    for gi, m in enumerate(ms):
        for j in range(m):
            t = j ^ 1
            twin.append(seg[gi] + t if t < m else -1)
    if ms[0] >= 4:
        twin[2] = 2                                                       # its own twin
        twin[3] = -1
    if B > 1 and ms[0] >= 6 and ms[1] >= 1:
        twin[5] = seg[1]                                                  # a twin outside the segment
        twin[4] = -1
    mode = seed % 2 if seed % 3 else 0
    n_state = [ri(0, beam + 1) for _ in range(B)]
    bits = [[ri(0, 1 << 32) & ((1 << max(0, min(32, ms[r // beam] - 32 * w))) - 1) for w in range(W)] for r in range(B * beam)]
    for gi in range(B):                                                   # two states one element apart: children from two parents
        if n_state[gi] >= 2 and ms[gi] >= 2:
            base = bits[gi * beam][0] | 3
            bits[gi * beam][0], bits[gi * beam + 1][0] = base & ~1, base & ~2
            bits[gi * beam + 1][1:] = bits[gi * beam][1:]
    cand_ptr, rrow, rflip, p, fl = [0], [], [], [], []
    for gi, c in enumerate(counts):
        c = ri(1, 12) if c is None else c
        for _ in range(c):
            rrow.append(gi * beam + ri(-1, beam + 1))
            rflip.append(ri(-1, ms[gi] + 2))
            p.append(_P_VALUES[ri(0, len(_P_VALUES))])
            fl.append(int(torch.rand(1, generator=g).item() < flip_rate))
        cand_ptr.append(cand_ptr[-1] + c)
    done = [int(torch.rand(1, generator=g).item() < 0.15 and counts[gi] is None) for gi in range(B)]
    return dict(bits=torch.tensor(bits, dtype=torch.long).view(B * beam, W), B=B, beam=beam, W=W, n_state=torch.tensor(n_state),
                cand_ptr=torch.tensor(cand_ptr), rep_row=torch.tensor(rrow, dtype=torch.long),
                rep_flip=torch.tensor(rflip, dtype=torch.long), p=torch.tensor(p, dtype=torch.float32),
                flipped=torch.tensor(fl, dtype=torch.uint8), seg_ptr=torch.tensor(seg), M=M,
                twin=torch.tensor(twin, dtype=torch.int32), mode=mode, max_cand=max_cand,
                done=torch.tensor(done, dtype=torch.uint8))


def beam_cases():
    """name -> the inputs of one cal_beam_step (``_beam_case``), CPU tensors: beams of 1, 4 and 16; ties in p (equal bit patterns,
    -0.0 next to 0.0, NaN); duplicate children; exactly ``max_cand`` candidates and one more; two words, and one word short."""
    out = {}
    for beam in (1, 4, 16):
        for seed in range(3):
            out["beam%d_seed%d" % (beam, seed)] = _beam_case(100 * beam + seed, beam, 40, [None] * 10 + [40, 41, 0])
        out["beam%d_many" % beam] = _beam_case(7 + beam, beam, 40, [40] * 6, m_hi=6, flip_rate=0.0)
    out["two_words"] = _beam_case(5, 4, 300, [300, 301, None, 299], m_hi=40, flip_rate=0.002)
    out["word_short"] = _beam_case(6, 4, 64, [None] * 8, m_hi=40, W=1)
    out["cap"] = _beam_case(8, 16, 2048, [2048, 2049, None], m_hi=64, flip_rate=0.0)
    return out


def _pbits(t):
    return [int(v) & 0xFFFFFFFF for v in t.view(torch.int32).tolist()]


def beam_oracle(c, defect=None):
    """The restatement of beam case ``c`` -> dict of lists (floats as bit patterns)."""
    B, beam, W = c["B"], c["beam"], c["W"]
    bits = [[int(v) for v in row] for row in c["bits"].tolist()]
    cf_bits = [[0] * W for _ in range(B)]
    return beam_rule(bits, B, beam, W, c["n_state"].tolist(), c["cand_ptr"].tolist(), c["rep_row"].tolist(), c["rep_flip"].tolist(),
                     _pbits(c["p"]), c["flipped"].tolist(), c["seg_ptr"].tolist(), c["M"],
                     c["twin"].tolist() if c["mode"] == 0 else None, c["max_cand"], c["done"].tolist(), cf_bits,
                     [0x7FC00000] * B, [-1] * B, defect)


def _i32(t):
    """words in [0, 2^32) as an int32 tensor of the same bit patterns"""
    return torch.where(t >= 2 ** 31, t - 2 ** 32, t).to(torch.int32)


def run_beam(c, dev):
    """``cal_amd.counterfactual.beam_step`` of beam case ``c`` on ``dev`` -> the dict ``beam_oracle`` gives."""
    from cal_amd.counterfactual import beam_step
    B, W = c["B"], c["W"]
    done = c["done"].clone().to(dev)
    cf_bits = torch.zeros(B, W, dtype=torch.int32, device=dev)
    cf_p = torch.tensor([0x7FC00000] * B, dtype=torch.int32).view(torch.float32).to(dev)
    cf_cand = torch.full((B,), -1, dtype=torch.long, device=dev)
    t = lambda k: c[k].to(dev)
    bits_out, p_out, n_out, status = beam_step(_i32(c["bits"]).to(dev), t("n_state"), t("cand_ptr"), t("rep_row"), t("rep_flip"),
                                               t("p"), t("flipped"), t("seg_ptr"), c["M"], done, cf_bits, cf_p, cf_cand,
                                               beam=c["beam"], twin=t("twin"), use="edges" if c["mode"] == 0 else "nodes",
                                               max_cand=c["max_cand"])
    return dict(bits_out=_u32(bits_out.cpu()), p_out=_pbits(p_out.cpu()), n_out=n_out.tolist(), status=status.tolist(),
                done=done.tolist(), cf_bits=_u32(cf_bits.cpu()), cf_p=_pbits(cf_p.cpu()), cf_cand=cf_cand.tolist())


# ---- the drivers --------------------------------------------------------------------------------------------------------------
def cut_graphs(n, max_und, seed, node_num=5):
    """``n`` SPMotif graphs cut to at most ``max_und`` undirected edges: the first ``max_und`` pairs of twin columns in column
    order and the nodes they touch, renumbered."""
    from cal_amd import spmotif
    from cal_amd.data import Data
    out = []
    for d in spmotif.train_mix(n, node_num=node_num, seed=seed):
        ei = d.edge_index
        und, seen = [], set()
        for u, v in ei.t().tolist():
            if u != v and (min(u, v), max(u, v)) not in seen:
                seen.add((min(u, v), max(u, v)))
                und.append((u, v))
        und = und[-max_und:]                                              # the last pairs: the motif's end of the graph
        nodes = sorted({a for e in und for a in e})
        new = {s: i for i, s in enumerate(nodes)}
        cols = sorted([(new[u], new[v]) for u, v in und] + [(new[v], new[u]) for u, v in und])
        x = d.x if d.x is not None else d.feat
        c = Data(edge_index=torch.tensor(cols, dtype=torch.long).t().contiguous(), y=d.y)
        c.x, c.feat = (x[nodes], None) if d.x is not None else (None, x[nodes])
        out.append(c)
    return out


def balance_head(model, b, head="o"):
    """Shift the head's last bias so that the classes' mean log-probabilities over ``b`` agree: a model whose predictions sit
    near its decision boundaries, as a search for prediction flips needs (a random initialisation calls every graph the same
    class from far away)."""
    from cal_amd.explain import _eval_mode, _log_probs
    h = ("c", "o", "co").index(head)
    with _eval_mode(model):
        lp = _log_probs(model, b)[h]
    with torch.no_grad():
        getattr(model, "fc2_" + head).bias -= lp.mean(0).to(getattr(model, "fc2_" + head).bias.dtype)
    return model


def probs_of_subsets(model, d, subsets, head="o", dev=None):
    """Head ``head``'s probabilities [S, C] of the graph ``d`` (a ``Data``; run on ``dev``) without the undirected edges of
    every subset (tuples of indices into the graph's undirected edges in column order of their lower column): the graphs are
    built here column by column, no replica builder involved."""
    from cal_amd.data import Batch, Data
    from cal_amd.explain import _eval_mode, _Layout, _log_probs, _untiled
    ei = d.edge_index.cpu()
    pairs = sorted({(min(u, v), max(u, v)) for u, v in ei.t().tolist()}, key=lambda e: min(
        j for j, (u, v) in enumerate(ei.t().tolist()) if (min(u, v), max(u, v)) == e))
    gs = []
    for sub in subsets:
        gone = {pairs[j] for j in sub}
        keep = [j for j, (u, v) in enumerate(ei.t().tolist()) if (min(u, v), max(u, v)) not in gone]
        c = Data(edge_index=d.edge_index[:, keep], y=d.y)
        c.x, c.feat = d.x, d.feat
        c.num_nodes = int((d.x if d.x is not None else d.feat).size(0))
        gs.append(c)
    b = Batch.from_data_list(gs)
    b = b.to((d.x if d.x is not None else d.feat).device if dev is None else dev)
    with _eval_mode(model):
        lp = _log_probs(model, _untiled(b, _Layout(b)))[("c", "o", "co").index(head)]
    return lp.exp(), len(pairs)


def brute_min_flip(model, d, yhat, head="o", chunk=400, dev=None):
    """The brute-force minimum flip search over ALL subsets of the undirected edges of ``d``, smallest first.
    -> (the minimum size or -1, the decisive margin: the smallest |p(ŷ) - p(runner-up)| over every subset of at most that size,
    the number of undirected edges)."""
    n = probs_of_subsets(model, d, [()], head, dev)[1]
    margin = float("inf")
    for k in range(1, n + 1):
        subs = list(itertools.combinations(range(n), k))
        hit = False
        for i in range(0, len(subs), chunk):
            p = probs_of_subsets(model, d, subs[i:i + chunk], head, dev)[0].double().cpu()
            py = p[:, yhat]
            other = p.clone()
            other[:, yhat] = -1.0
            margin = min(margin, float((py - other.max(1).values).abs().min()))
            hit = hit or bool((p.argmax(1) != yhat).any())
        if hit:
            return k, margin, n
    return -1, margin, n


def greedy_occlude(model, b, twin, lim, head="o"):
    """The greedy search written with ``occlude_batch`` on the shrinking batch ``b`` (undirected edges; ``twin`` its map): every
    round removes, per graph still searched, the undirected edge whose removal leaves the smallest ``p(ŷ)`` -- a flipping one
    first; ties by the lower column -- until the argmax leaves ŷ or ``lim[g]`` edges are gone.
    -> (removed bool [E] over b's columns, size [B], gap: per graph the smallest difference between the best and the second
    best p of a round)."""
    from cal_amd.explain import _eval_mode, _Layout, _log_probs, _untiled, edge_twins
    from cal_amd.occlude import occlude_batch
    from tests.counterfactual_oracle import score_key as sk
    h = ("c", "o", "co").index(head)
    B, dev = int(b.num_graphs), b.edge_index.device
    with _eval_mode(model):
        full = _log_probs(model, _untiled(b, _Layout(b)))[h]
        yhat = full.argmax(-1)
        cur, orig = b, torch.arange(int(b.edge_index.size(1)), device=dev)
        removed = torch.zeros_like(orig, dtype=torch.bool)
        size, gap, active = [-1] * B, [float("inf")] * B, [lim[g] > 0 for g in range(B)]
        for t in range(max(lim) if lim else 0):
            tw = edge_twins(cur)[0]
            E = int(cur.edge_index.size(1))
            gid = cur.batch[cur.edge_index[0]]
            rep = ~((tw >= 0) & (tw < torch.arange(E, device=dev)))
            sel = [e for e in rep.nonzero().view(-1).tolist() if active[int(gid[e])] and t < lim[int(gid[e])]]
            if not sel:
                break
            ids = torch.tensor(sel, device=dev)
            rb = occlude_batch(cur, gid[ids], ids, twin=tw)
            lp = _log_probs(model, rb)[h]
            py = lp.gather(-1, yhat[gid[ids]].view(-1, 1)).view(-1).exp().float()
            fl = lp.argmax(-1) != yhat[gid[ids]]
            pick = torch.full((B,), -1, dtype=torch.long, device=dev)
            keys = [(0 if f else 1, sk(int(u) & 0xFFFFFFFF), e) for f, u, e in zip(fl.tolist(), py.view(torch.int32).tolist(), sel)]
            for g in range(B):
                mine = sorted((k, j) for j, k in enumerate(keys) if int(gid[sel[j]]) == g)
                if not mine:
                    continue
                (k0, j0) = mine[0]
                if len(mine) > 1:
                    gap[g] = min(gap[g], abs(float(py[mine[1][1]]) - float(py[j0])))
                pick[g] = sel[j0]
                gone = [sel[j0]] + ([int(tw[sel[j0]])] if int(tw[sel[j0]]) >= 0 else [])
                removed[orig[torch.tensor(gone, device=dev)]] = True
                if k0[0] == 0:
                    size[g], active[g] = t + 1, False
            cur = occlude_batch(cur, torch.arange(B, device=dev), pick, twin=tw)
            orig = orig[cur.edge_src]
        for g in range(B):
            if size[g] < 0:
                removed[(b.batch[b.edge_index[0]] == g)] = False
    return removed, size, gap


def prefix_flip(model, b, key, lim, use="edges", head="o"):
    """The smallest k <= lim[g] such that graph g without the elements of rank < k under ``key`` (int32 [M]) leaves ŷ, by one
    ``coalition_batch`` of the whole batch per k; -1: none."""
    from cal_amd.coalition import coalition_batch
    from cal_amd.explain import _eval_mode, _Layout, _log_probs, _untiled
    h = ("c", "o", "co").index(head)
    B, dev = int(b.num_graphs), b.edge_index.device
    size = [-1] * B
    with _eval_mode(model):
        yhat = _log_probs(model, _untiled(b, _Layout(b)))[h].argmax(-1)
        for k in range(1, max(lim) + 1 if lim else 1):
            rb = coalition_batch(b, torch.arange(B, device=dev), torch.full((B,), k, device=dev), key, use=use, invert=True)
            fl = (_log_probs(model, rb)[h].argmax(-1) != yhat).tolist()
            for g in range(B):
                if fl[g] and size[g] < 0 and k <= lim[g]:
                    size[g] = k
    return size


def binom_ok(n, k, beam):
    """A beam of ``beam`` states holds every subset of every size below k (so the search sees all of size k), and is at least
    the number of subsets of size k."""
    return all(math.comb(n, j) <= beam for j in range(1, k + 1))

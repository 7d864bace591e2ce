"""Plain restatements of the noise operators: splitmix64 on Python ints, the replica builder (cal_noise_count / cal_noise_write)
one replica and one candidate at a time, the capped one-hot degree (cal_degree_onehot), the twin map, the case list both test
files walk, and the integer side of noise_curve() / stability().  Everything on the CPU."""
import math

import torch

from tests.occlude_oracle import _feat, hand_batch

MASK = (1 << 64) - 1
C_DEL = 0xA0761D6478BD642F                 # CAL_NOISE_C_DEL
C_ADD = 0xE7037ED1A0B428DB                 # CAL_NOISE_C_ADD
MAX63 = (1 << 63) - 1


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def H(s, i):
    return splitmix64((splitmix64(s & MASK) + i) & MASK)


def twin_map(b):
    """cal_edge_twin's rule in plain Python: inside a graph the j-th column (u, v), u != v, pairs with the j-th column (v, u); a
    self loop is its own twin; a column that leaves its graph pairs with nothing.  -> list [E]."""
    ei, E = b.edge_index.tolist(), int(b.edge_index.size(1))
    twin = [-1] * E
    for g in range(int(b.num_graphs)):
        lo, hi = int(b.ptr[g]), int(b.ptr[g + 1])
        occ = {}
        for e in range(int(b.edge_ptr[g]), int(b.edge_ptr[g + 1])):
            u, v = ei[0][e], ei[1][e]
            if not (lo <= u < hi and lo <= v < hi):
                continue
            if u == v:
                twin[e] = e
            else:
                occ.setdefault((u, v), []).append(e)
        for (u, v), cols in occ.items():
            for j, e in enumerate(cols):
                back = occ.get((v, u), [])
                if j < len(back):
                    twin[e] = back[j]
    return twin


def _per_replica(v, R):
    return [float(x) for x in v.tolist()] if torch.is_tensor(v) else [float(v)] * R


def noise_args(b, rep_graph, add, delete, seed, undirected):
    """The operator's per-replica arguments as noise_batch derives them -> (twin or None, rep_seed, rep_del, rep_add) lists."""
    rg = [int(g) for g in rep_graph]
    R, B = len(rg), int(b.num_graphs)
    twin = twin_map(b) if undirected else None
    ei = b.edge_index.tolist()
    U = []
    for g in range(B):
        n = 0
        for e in range(int(b.edge_ptr[g]), int(b.edge_ptr[g + 1])):
            rep = not (twin is not None and 0 <= twin[e] < e)
            n += rep and ei[0][e] != ei[1][e]
        U.append(n)
    radd = [int(math.floor(U[g] * a)) if 0 <= g < B else 0 for g, a in zip(rg, _per_replica(add, R))]
    rdel = [min(max(int(math.floor(d * 2.0 ** 63)), 0), MAX63) for d in _per_replica(delete, R)]
    rseed = [int(s) for s in seed.tolist()] if torch.is_tensor(seed) else [seed + r for r in range(R)]
    return twin, rseed, rdel, radd


def noise_oracle(b, rep_graph, add=0.0, delete=0.0, seed=0, undirected=True, tries=8):
    """-> dict(ptr, edge_ptr, batch, x, edge_index, node_src, edge_src, added, totals [7], dups, cross, walked, deleted, players)
    for a CPU source with grouped columns.  ``dups``: per replica the candidates refused only because an earlier candidate was
    the same pair; ``cross``: per replica ``{256: .., 1024: ..}``, those of them whose earlier candidate lies in an earlier chunk
    of that many candidates; ``walked``: per replica the candidates looked at before the count was reached; ``deleted`` /
    ``players``: per replica the players that went and the players there were."""
    x, ei, B = _feat(b), b.edge_index.tolist(), int(b.num_graphs)
    rg = list(range(B)) if rep_graph is None else [int(g) for g in rep_graph]
    twin, rseed, rdel, radd = noise_args(b, rg, add, delete, seed, undirected)
    ptr, eptr, batch, nsrc, esrc, cu, cv = [0], [0], [], [], [], [], []
    added, dups, cross, walked, deleted, players = [], [], [], [], [], []
    empty = mn = me = fell = 0
    for r, g in enumerate(rg):
        n0 = ptr[-1]
        n = m = got = dup = gone = pl = seen_c = 0
        far = {256: 0, 1024: 0}
        if 0 <= g < B:
            lo, hi = int(b.ptr[g]), int(b.ptr[g + 1])
            elo, ehi = int(b.edge_ptr[g]), int(b.edge_ptr[g + 1])
            n = hi - lo
            source = set()
            for e in range(elo, ehi):
                u, v = ei[0][e], ei[1][e]
                if not (lo <= u < hi and lo <= v < hi):
                    continue                                              # a column that leaves its graph is dropped
                stays = True
                if u != v:
                    source.add((u - lo, v - lo))
                    rep = twin[e] if twin is not None and elo <= twin[e] < e else e
                    stays = not ((H(rseed[r] ^ C_DEL, rep - elo) >> 1) < rdel[r])
                    pl += rep == e
                    gone += rep == e and not stays
                if stays:
                    cu.append(n0 + u - lo), cv.append(n0 + v - lo), esrc.append(e)
                    m += 1
            a = max(radd[r], 0)
            seen = {}
            if n > 1:
                for c in range(tries * a):
                    if got == a:
                        break
                    seen_c = c + 1
                    h = H(rseed[r] ^ C_ADD, c)
                    u, v = (h >> 32) % n, (h & 0xFFFFFFFF) % n
                    if u == v or (u, v) in source or (undirected and (v, u) in source):
                        continue
                    pair = (min(u, v), max(u, v)) if undirected else (u, v)
                    if pair in seen:
                        dup += 1
                        for w in far:
                            far[w] += seen[pair] // w < c // w
                        continue
                    seen[pair] = c
                    got += 1
                    for s, t in ((u, v), (v, u)) if undirected else ((u, v),):
                        cu.append(n0 + s), cv.append(n0 + t), esrc.append(-1)
                        m += 1
            nsrc += list(range(lo, hi))
            batch += [r] * n
        fell += got < max(radd[r], 0)
        added.append(got), dups.append(dup), cross.append(far), walked.append(seen_c), deleted.append(gone), players.append(pl)
        ptr.append(n0 + n)
        eptr.append(eptr[-1] + m)
        empty += n == 0
        mn, me = max(mn, n), max(me, m)
    lng = lambda v: torch.tensor(v, dtype=torch.long)
    return dict(ptr=lng(ptr), edge_ptr=lng(eptr), batch=lng(batch), x=None if x is None else x[lng(nsrc)],
                edge_index=torch.stack([lng(cu), lng(cv)]), node_src=lng(nsrc), edge_src=lng(esrc), added=lng(added),
                totals=[ptr[-1], eptr[-1], mn, me, empty, sum(added), fell], dups=dups, cross=cross, walked=walked, deleted=deleted,
                players=players)


def check_noise(res, b, rep_graph, add=0.0, delete=0.0, seed=0, undirected=True, tries=8):
    """``res`` (a noise_batch result, any device) of the CPU source ``b``: equals the restatement bit for bit; the structural
    properties of the insertions on their own."""
    r = noise_oracle(b, rep_graph, add, delete, seed, undirected, tries)
    ei, ptr, eptr = res.edge_index.cpu(), res.ptr.cpu(), res.edge_ptr.cpu()
    assert torch.equal(ptr, r["ptr"]) and torch.equal(eptr, r["edge_ptr"])
    assert torch.equal(ei, r["edge_index"]) and res.edge_index.is_contiguous() and ei.shape == (2, r["totals"][1])
    assert torch.equal(res.batch.cpu(), r["batch"])
    assert torch.equal(res.node_src.cpu(), r["node_src"]) and torch.equal(res.edge_src.cpu(), r["edge_src"])
    assert torch.equal(res.added.cpu(), r["added"]) and res.added.device == res.edge_index.device
    rx = _feat(res)
    if r["x"] is None:
        assert rx is None
    else:
        assert rx.dtype == torch.float32 and torch.equal(rx.cpu(), r["x"]) and (res.x is None) == (b.x is None)
    n2, e2 = int(res.batch.numel()), int(ei.size(1))
    assert [n2, e2, res.max_nodes, res.max_edges, res.empty_graphs, res.n_added, res.short] == r["totals"]
    R = len(r["ptr"]) - 1
    assert res.num_graphs == R and res.tile_ptr is None and res.no_self_loops == bool(b.no_self_loops)
    rg = list(range(int(b.num_graphs))) if rep_graph is None else [int(v) for v in rep_graph]
    if b.y is None or any(not 0 <= g < int(b.num_graphs) for g in rg):
        assert res.y is None
    else:
        assert torch.equal(res.y.cpu(), b.y.view(-1)[torch.tensor(rg, dtype=torch.long)])
    # independent of the restatement: survivors are the source's columns, in order; insertions are distinct pairs of distinct
    # nodes, not adjacent in the source, after the survivors, symmetric in undirected mode
    es, ns = res.edge_src.cpu(), res.node_src.cpu()
    surv = es >= 0
    assert torch.equal(ns[ei[:, surv]], b.edge_index[:, es[surv]])
    src_ei = b.edge_index.tolist()
    for q in range(R):
        lo, hi = int(eptr[q]), int(eptr[q + 1])
        s = surv[lo:hi].tolist()
        k = sum(s)
        assert all(s[:k]) and not any(s[k:])
        assert es[lo:lo + k].tolist() == sorted(es[lo:lo + k].tolist())
        w = 2 if undirected else 1
        assert hi - lo - k == w * int(res.added[q])
        if hi - lo == k:
            continue
        g, n0 = rg[q], int(ptr[q])
        base = int(b.ptr[g])
        have = {(src_ei[0][e] - base, src_ei[1][e] - base) for e in range(int(b.edge_ptr[g]), int(b.edge_ptr[g + 1]))}
        new = [(int(ei[0, j]) - n0, int(ei[1, j]) - n0) for j in range(lo + k, hi)]
        assert all(u != v and 0 <= u < int(ptr[q + 1]) - n0 and 0 <= v < int(ptr[q + 1]) - n0 for u, v in new)
        assert not (set(new) & have) and len(set(new)) == len(new)
        if undirected:
            assert all(new[2 * j] == new[2 * j + 1][::-1] for j in range(len(new) // 2))
            assert not ({(v, u) for u, v in new} & have)
    return r


# ---- the case list both test files walk (host twin on the CPU, HIP on the GPU) ---------------------------------------------
def ring(n):
    return [(i, (i + 1) % n) for i in range(n)] + [((i + 1) % n, i) for i in range(n)]


def _complete(n):
    return [(u, v) for u in range(n) for v in range(n) if u != v]


def noise_cases():
    """name -> (batch, rep_graph, add, delete, seed, undirected, tries), CPU tensors."""
    out = {}
    lng = lambda v: torch.tensor(v, dtype=torch.long)
    # graphs 0-3: rings of 3 - 6 nodes (the 3-ring is complete: every candidate is refused); 4: no column; 5: one node; 6: two
    # nodes; 7: K5; 8: duplicate columns, unpaired columns, self loops and a column that leaves the graph
    odd = (5, [(0, 0), (0, 1), (1, 0), (0, 1), (2, 3), (3, 2), (3, 2), (1, 4), (4, 4), (2, 7), (4, 2), (2, 4)])
    graphs = [(n, ring(n)) for n in (3, 4, 5, 6)] + [(4, []), (1, []), (2, [(0, 1), (1, 0)]), (5, _complete(5)), odd]
    for F in (3, 4, 5, 0):
        hb = hand_batch(graphs, F=F, seed=F)
        B = hb.num_graphs
        every = list(range(B))
        # every graph at add = 1 (K5: short, nothing added) and some deletion; ids outside the batch; one graph under many seeds
        rg = lng(every + [-1, B] + [3] * 6 + every)
        R = rg.numel()
        add = torch.cat([torch.ones(B + 2), torch.tensor([0.0, 0.5, 0.5, 1.0, 2.0, 2.0]), torch.full((B,), 0.5)]).double()
        dele = torch.cat([torch.full((B + 2,), 0.3), torch.tensor([0.0, 0.0, 0.5, 0.5, 1.0, 0.2]), torch.zeros(B)]).double()
        seed = torch.arange(R) * 7919 + 11 * F
        for und in (True, False):
            out["hand_F%d_%s" % (F, "und" if und else "dir")] = (hb, rg, add, dele, seed, und, 8)
    hb = hand_batch(graphs, F=3, seed=1)
    # the 6-ring at a = 12 against 9 free pairs (short), the 4-ring at a = 2, the 5-ring at a = 5 (all its free pairs), K5
    rg = lng([3, 1, 2, 7, 3, 1, 2])
    add = torch.tensor([2.0, 0.5, 1.0, 1.0, 2.0, 0.5, 1.0]).double()
    out["short_und"] = (hb, rg, add, 0.0, 5, True, 8)
    out["short_dir"] = (hb, rg, add, 0.0, 5, False, 8)
    out["tries1"] = (hb, lng(list(range(9))), 1.0, 0.25, 3, True, 1)
    out["tries3_floats"] = (hb, lng(list(range(9)) * 2), 0.75, 0.5, -4, True, 3)
    out["delete_all"] = (hb, lng(list(range(9))), 0.0, 1.0, 9, True, 8)
    out["none"] = (hb, lng([]), 0.3, 0.3, 0, True, 8)
    out["default_ids"] = (hb, None, 0.4, 0.1, 123456789012345678901234567890, True, 8)
    # a 40-ring at add = 1: 320 candidates, but all 40 insertions are found among the first 256
    r40 = hand_batch([(3, ring(3)), (40, ring(40)), (4, ring(4))], F=4, seed=2)
    out["ring40_und"] = (r40, lng([0, 1, 2, 1]), 1.0, 0.1, 17, True, 8)
    out["ring40_dir"] = (r40, lng([0, 1, 2, 1]), 1.0, 0.1, 17, False, 8)
    # a 60-ring at add = 5: a = 300 (directed: 600) of 1710 (3420) free pairs with 120 source columns, so the LDS path walks
    # several chunks of 256 candidates and a later chunk repeats pairs that an earlier one accepted
    r60 = hand_batch([(60, ring(60)), (4, ring(4))], F=4, seed=6)
    out["ring60_und"] = (r60, lng([0, 1, 0]), torch.tensor([5.0, 0.5, 5.0]).double(), 0.1, 23, True, 8)
    out["ring60_dir"] = (r60, lng([0, 1, 0]), torch.tensor([5.0, 0.5, 5.0]).double(), 0.1, 23, False, 8)
    return out


def wide_lds_case():
    """A 60-ring at add = 18 (a = 1080 of 1710 free pairs) beside a 2600-node ring: the batch's average graph has more than 2048
    columns, so the workgroups are 1024 threads wide, and the 60-ring (120 columns: the LDS path) needs more than one chunk of
    1024 candidates."""
    b = hand_batch([(60, ring(60)), (2600, ring(2600))], F=4, seed=7)
    return b, torch.tensor([0, 1, 0]), torch.tensor([18.0, 0.05, 18.0]).double(), 0.1, 29, True, 8


def big_ring_case():
    """A 1100-node ring (2200 columns: above the LDS cap) at add = 1 (8800 candidates) beside 3-node graphs."""
    b = hand_batch([(3, ring(3)), (1100, ring(1100)), (3, ring(3))], F=4, seed=3)
    return b, torch.tensor([0, 1, 2, 1]), torch.tensor([1.0, 1.0, 1.0, 0.25]).double(), 0.05, 21, True, 8


def many_tiny_case():
    """3000 replicas of rings of 3 - 6 nodes, a third of them with graph id -1."""
    g = torch.Generator().manual_seed(4)
    sizes = torch.randint(3, 7, (500,), generator=g).tolist()
    b = hand_batch([(n, ring(n)) for n in sizes], F=4, seed=4)
    rg = torch.randint(-250, 500, (3000,), generator=g).clamp(min=-1)
    return b, rg, 0.5, 0.2, 77, True, 8


def check_the_case_list_meets_duplicates(cases):
    """The de-duplication cannot go untested: the 4-ring, the 5-ring and the 40-ring each refuse a candidate only because an
    earlier one was the same pair, and the 40-ring still reaches its full count."""
    b, rg, add, dele, seed, und, tries = cases["short_und"]
    r = noise_oracle(b, rg, add, dele, seed, und, tries)
    assert r["dups"][1] > 0 and r["dups"][6] > 0, r["dups"]               # the 4-ring, the 5-ring (its second replica)
    assert r["added"].tolist()[0] == 9 and r["added"].tolist()[3] == 0 and r["totals"][6] >= 2      # the 6-ring, K5: short
    b, rg, add, dele, seed, und, tries = cases["ring40_und"]
    r = noise_oracle(b, rg, add, dele, seed, und, tries)
    assert r["dups"][1] > 0 and r["added"].tolist()[1] == 40 and r["added"].tolist()[0] == 0
    # the LDS path beyond its first chunk: a duplicate whose earlier candidate lies in an earlier chunk is refused only if the
    # accepted pairs of that chunk are found in the set
    for name in ("ring60_und", "ring60_dir"):
        b, rg, add, dele, seed, und, tries = cases[name]
        assert int(b.edge_ptr[1]) <= 2048
        r = noise_oracle(b, rg, add, dele, seed, und, tries)
        for q in (0, 2):
            assert r["walked"][q] > 256 and r["cross"][q][256] > 0 and r["added"].tolist()[q] == (300 if und else 600), (name, q)
    b, rg, add, dele, seed, und, tries = wide_lds_case()
    assert int(b.edge_index.size(1)) // int(b.num_graphs) > 2048 and int(b.edge_ptr[1]) <= 2048
    r = noise_oracle(b, rg, add, dele, seed, und, tries)
    for q in (0, 2):
        assert r["walked"][q] > 1024 and r["cross"][q][1024] > 0 and r["added"].tolist()[q] == 1080, q


def degree_oracle(edge_index, N, F):
    out = torch.zeros(N, F)
    deg = [0] * N
    for u, v in zip(*edge_index.tolist()):
        if 0 <= u < N and u != v:
            deg[u] += 1
    for i in range(N):
        out[i, min(deg[i], F - 1)] = 1.0
    return out


# ---- the integer side of the drivers ------------------------------------------------------------------------------------------
def representatives(twin, M):
    t = torch.tensor(twin, dtype=torch.long) if not torch.is_tensor(twin) else twin.long()
    return ~((t >= 0) & (t < torch.arange(M)))


def replica_oracle(b, trials, add, delete, seed, undirected):
    """The replicas noise_curve() / stability() build of the CPU batch ``b``: replica t B + g is graph g under seed + t B + g."""
    B = int(b.num_graphs)
    rg = torch.arange(B).repeat(trials)
    return rg, noise_oracle(b, rg, add, delete, seed, undirected, 8)

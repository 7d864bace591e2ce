"""Plain-torch restatement of the subgraph extraction contract (cal_subgraph_extract) and of the fidelity metrics through the
fp64 oracle's eval forward.  Everything on the CPU; boolean indexing and cumsum only."""
import torch

from oracle import cal_oracle as O


def extract_oracle(edge_index, ptr, edge_ptr, N, edge_keep=None, node_keep=None, complement=False, relabel=False, x=None):
    """-> dict(edge_index, ptr, edge_ptr, batch, x, node_map, edge_map, totals) for edge columns grouped by graph."""
    edge_index, ptr, edge_ptr = edge_index.cpu(), ptr.cpu(), edge_ptr.cpu()
    B = ptr.numel() - 1
    gid_e = torch.repeat_interleave(torch.arange(B), edge_ptr[1:] - edge_ptr[:-1])
    gid_n = torch.repeat_interleave(torch.arange(B), ptr[1:] - ptr[:-1])
    src, dst = edge_index[0], edge_index[1]
    lo, hi = ptr[gid_e], ptr[gid_e + 1]
    keep = (src >= lo) & (src < hi) & (dst >= lo) & (dst < hi)            # an edge that leaves its graph is dropped
    if edge_keep is not None:
        keep &= edge_keep.cpu().bool() ^ bool(complement)
    nf = None
    if node_keep is not None:
        nf = node_keep.cpu().bool() ^ bool(complement)
        keep &= nf[src.clamp(0, max(N - 1, 0))] & nf[dst.clamp(0, max(N - 1, 0))]
    if relabel:
        nodes = nf
        if nodes is None:
            nodes = torch.zeros(N, dtype=torch.bool)
            nodes[src[keep]] = True
            nodes[dst[keep]] = True
    else:
        nodes = torch.ones(N, dtype=torch.bool)
    node_map = nodes.nonzero().view(-1)
    edge_map = keep.nonzero().view(-1)
    ei = edge_index[:, edge_map]
    if relabel:
        newid = torch.cumsum(nodes.long(), 0) - 1
        ei = newid[ei]
    batch = gid_n[node_map]
    ncnt = torch.bincount(batch, minlength=B)[:B] if B else torch.zeros(0, dtype=torch.long)
    ecnt = torch.bincount(gid_e[edge_map], minlength=B)[:B] if B else torch.zeros(0, dtype=torch.long)
    zero = torch.zeros(1, dtype=torch.long)
    totals = [int(node_map.numel()), int(edge_map.numel()), int(ncnt.max()) if B else 0, int(ecnt.max()) if B else 0]
    return dict(edge_index=ei.contiguous(), ptr=torch.cat([zero, ncnt.cumsum(0)]), edge_ptr=torch.cat([zero, ecnt.cumsum(0)]),
                batch=batch, x=None if x is None else (x.cpu()[node_map] if relabel else x.cpu()), node_map=node_map,
                edge_map=edge_map, totals=totals)


def oracle_log_probs(name, sd64, x, edge_index, batch, num_graphs, **kw):
    """fp64 eval forward with the identity permutation -> [3, B, C] (heads c, o, co)."""
    return torch.stack(O.causal_forward(name, sd64, x.double(), edge_index, batch, num_graphs=num_graphs, **kw))


def fidelity_oracle(name, sd, b, edge_mask=None, node_mask=None, **kw):
    """Fidelity of the selection (edge_mask / node_mask, bool, in b's order) through the fp64 oracle: the metric dict of
    cal_amd.explain.fidelity plus ``margin`` [3, 3, B]: the top-two log-probability gap of every head on the full / kept /
    removed batch (for excluding near-ties from hit counts) and ``hits`` [3, 3, B] bool."""
    sd64 = {k: v.double().cpu() for k, v in sd.items()}
    x = (b.x if b.x is not None else b.feat).cpu()
    ei, bvec, B = b.edge_index.cpu(), b.batch.cpu(), int(b.num_graphs)
    y = b.y.view(-1).cpu()
    N = x.size(0)
    subs = [ei]
    for comp in (False, True):
        r = extract_oracle(ei, b.ptr, b.edge_ptr, N, edge_keep=edge_mask, node_keep=node_mask, complement=comp)
        subs.append(r["edge_index"])
    lps = [oracle_log_probs(name, sd64, x, e, bvec, B, **kw) for e in subs]           # full, keep, drop
    yhat = lps[0].argmax(-1, keepdim=True)
    p = [lp.gather(-1, yhat).exp().squeeze(-1) for lp in lps]                        # [3, B] each
    hits = torch.stack([lp.argmax(-1) == y for lp in lps], 1)                        # [head, variant, B]
    top2 = torch.stack([lp.topk(2, -1).values for lp in lps], 1)                     # [head, variant, B, 2]
    res = {}
    for h, head in enumerate(("c", "o", "co")):
        res["acc_full_" + head] = hits[h, 0].double().mean().item()
        res["acc_keep_" + head] = hits[h, 1].double().mean().item()
        res["acc_drop_" + head] = hits[h, 2].double().mean().item()
        res["fid_plus_" + head] = (p[0][h] - p[2][h]).mean().item()
        res["fid_minus_" + head] = (p[0][h] - p[1][h]).mean().item()
    ms = [m.cpu().bool() for m in (edge_mask, node_mask) if m is not None]
    res["sparsity"] = 1.0 - sum(int(m.sum()) for m in ms) / sum(m.numel() for m in ms)
    res["graphs"] = B
    res["hits"] = hits
    res["margin"] = top2[..., 0] - top2[..., 1]
    return res


# ---- the case list both test files walk (host twin on the CPU, HIP on the GPU) ---------------------------------------------
def case_batches():
    """name -> (Batch on the CPU, edge_mask or None, node_mask or None)."""
    from cal_amd import spmotif
    from cal_amd.data import Batch, Data
    from tests.helpers import random_graph_batch, ref_batch
    g = torch.Generator().manual_seed(0)
    out = {}
    b = random_graph_batch(num_graphs=9, n_lo=3, n_hi=30, feat=5, seed=1)
    E, N = b.edge_index.size(1), b.batch.numel()
    em, nm = torch.rand(E, generator=g) < 0.4, torch.rand(N, generator=g) < 0.6
    out["edge"] = (b, em, None)
    out["node"] = (b, None, nm)
    out["both"] = (b, em, nm)
    out["all_kept"] = (b, torch.ones(E, dtype=torch.bool), torch.ones(N, dtype=torch.bool))
    out["all_dropped"] = (b, torch.zeros(E, dtype=torch.bool), torch.zeros(N, dtype=torch.bool))
    b1 = random_graph_batch(num_graphs=1, n_lo=40, n_hi=40, feat=3, seed=2)
    out["one_graph"] = (b1, torch.rand(b1.edge_index.size(1), generator=g) < 0.5, torch.rand(40, generator=g) < 0.5)
    # a graph without edges in the middle of the batch
    ds = [Data(x=torch.randn(4, 3, generator=g), edge_index=torch.tensor([[0, 1, 2, 3], [1, 0, 3, 2]]), y=torch.tensor([0])),
          Data(x=torch.randn(5, 3, generator=g), edge_index=torch.zeros(2, 0, dtype=torch.long), y=torch.tensor([1])),
          Data(x=torch.randn(3, 3, generator=g), edge_index=torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]]), y=torch.tensor([2]))]
    be = Batch.from_data_list(ds)
    out["edgeless_middle"] = (be, torch.tensor([1, 1, 0, 0, 0, 1, 1, 0], dtype=torch.bool), torch.rand(12, generator=g) < 0.7)
    br = ref_batch(range(8))
    out["golden"] = (br, torch.rand(br.edge_index.size(1), generator=g) < 0.3, torch.rand(br.batch.numel(), generator=g) < 0.5)
    bs = Batch.from_data_list(spmotif.train_mix(32, node_num=7, seed=3))
    out["spmotif"] = (bs, torch.rand(bs.edge_index.size(1), generator=g) < 0.5, torch.rand(bs.batch.numel(), generator=g) < 0.5)
    return out


def check_extraction(sub, b, em, nm, complement, relabel):
    """``sub`` (an extract_subgraph result, any device) equals the restatement bit for bit; structural properties."""
    x = b.x if b.x is not None else b.feat
    N = b.batch.numel()
    r = extract_oracle(b.edge_index, b.ptr, b.edge_ptr, N, em, nm, complement, relabel, x)
    assert torch.equal(sub.edge_index.cpu(), r["edge_index"]) and sub.edge_index.is_contiguous()
    assert torch.equal(sub.ptr.cpu(), r["ptr"]) and torch.equal(sub.edge_ptr.cpu(), r["edge_ptr"])
    assert torch.equal(sub.batch.cpu(), r["batch"])
    assert torch.equal(sub.node_map.cpu(), r["node_map"]) and torch.equal(sub.edge_map.cpu(), r["edge_map"])
    sx = sub.x if sub.x is not None else sub.feat
    assert torch.equal(sx.cpu(), r["x"])
    assert (sub.x is None) == (b.x is None)
    n2, e2 = int(sub.batch.numel()), int(sub.edge_index.size(1))
    assert [n2, e2, sub.max_nodes, sub.max_edges] == r["totals"]
    assert sub.num_graphs == b.num_graphs and sub.no_self_loops == b.no_self_loops and sub.tile_ptr is None
    assert sub.y is b.y or torch.equal(sub.y.cpu(), b.y.cpu())
    # independent of the restatement
    ptr, eptr, ei = sub.ptr.cpu(), sub.edge_ptr.cpu(), sub.edge_index.cpu()
    assert int(ptr[0]) == 0 and int(ptr[-1]) == n2 and int(eptr[0]) == 0 and int(eptr[-1]) == e2
    assert bool((ptr[1:] >= ptr[:-1]).all()) and bool((eptr[1:] >= eptr[:-1]).all())
    for gph in range(sub.num_graphs):
        cols = ei[:, int(eptr[gph]):int(eptr[gph + 1])]
        assert bool(((cols >= ptr[gph]) & (cols < ptr[gph + 1])).all())
    nmap, emap = sub.node_map.cpu(), sub.edge_map.cpu()
    assert bool((nmap[1:] > nmap[:-1]).all()) and bool((emap[1:] > emap[:-1]).all())
    if not relabel:
        assert n2 == N and torch.equal(nmap, torch.arange(N))
        assert torch.equal(ei, b.edge_index.cpu()[:, emap])
    else:
        assert torch.equal(nmap[ei], b.edge_index.cpu()[:, emap])
    return r


def check_fidelity(res, ref, tol, cap=0.05):
    """``res`` (cal_amd.explain.fidelity) against ``ref`` (fidelity_oracle): probability metrics within ``tol``; hit counts
    may differ only by graphs whose oracle top-two log-probability gap is within 10 tol (at most ``cap`` of all)."""
    B = ref["graphs"]
    unsure = ref["margin"] <= 10 * tol                                   # [head, variant, B]
    print("fidelity check: tol %g, near-ties %d of %d" % (tol, int(unsure.sum()), unsure.numel()))
    assert not bool(unsure[:, 0].any()), "the full graph's argmax must be unambiguous in the oracle (pick another seed)"
    assert unsure.double().mean().item() <= cap
    for h, head in enumerate(("c", "o", "co")):
        for key in ("fid_plus_", "fid_minus_"):
            err = abs(res[key + head] - ref[key + head])
            print("  %s%s: %.9f vs %.9f (|diff| %.3g)" % (key, head, res[key + head], ref[key + head], err))
            assert err <= tol, (key + head, err)
        for v, key in enumerate(("acc_full_", "acc_keep_", "acc_drop_")):
            diff = abs(res[key + head] - ref[key + head]) * B
            assert diff <= int(unsure[h, v].sum()) + 1e-9, (key + head, diff)
    assert abs(res["sparsity"] - ref["sparsity"]) < 1e-12 and res["graphs"] == B

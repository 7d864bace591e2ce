"""Time the explanation path on the GPU: the HIP per-graph ranking (cal_explain_rank) alone, a torch-composed ranking of
the same scores (stable sort by score, stable sort by graph id, masks), and eval_explanation against eval_acc_causal over
the same loader; and the fidelity leg: the HIP subgraph extraction (cal_subgraph_extract, with its one read-back) against the
plain-torch composition of the same extraction (nonzero / cumsum / index_select) on the same device, and one whole fidelity()
call.  Device events around synchronised regions, after warm-up; one JSON line per shape.  ``--undirected`` prints one more
line instead: explain() and eval_fidelity() at the SPMotif headline batch, directed against undirected ("mean"), and the
twin map and the pair ranking alone, all in this one process.

    python scripts/bench_explain.py [--shapes headline,nodenum15,config5] [--iters 50]
    python scripts/bench_explain.py --undirected [--iters 50]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cal_amd import model as M, spmotif, synth          # noqa: E402
from cal_amd.data import Batch, DataLoader               # noqa: E402
from cal_amd.explain import (_Layout, _scores, eval_explanation, eval_fidelity, explain, extract_subgraph, fidelity,   # noqa: E402
                             rank_segments)
from cal_amd.train_causal import eval_acc_causal         # noqa: E402

SHAPES = {
    "headline": dict(graphs=lambda n: spmotif.train_mix(n, node_num=7, seed=1), B=128),
    "nodenum15": dict(graphs=lambda n: spmotif.train_mix(n, node_num=15, seed=1), B=128),
    "config5": dict(graphs=lambda n: synth.ba_graphs(n, n=5000, seed=1), B=32),
}


def _time(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def torch_rank(score, gid, eptr, k):
    """Torch-composed baseline: stable sort by score descending, then stable sort by graph id -> per-graph ranks, masks."""
    o1 = torch.argsort(score, descending=True, stable=True)
    o2 = torch.argsort(gid[o1], stable=True)
    order = o1[o2]
    rank = torch.empty_like(order)
    rank[order] = torch.arange(order.numel(), device=score.device) - eptr[gid[order]]
    return rank < k, rank


def torch_extract(ei, ptr, eptr, batch, x, keep, relabel):
    """Torch-composed extraction of an edge mask (edge columns grouped by graph): the kept columns in order, per-graph
    offsets and bounds and, with relabel, the touched nodes renumbered by a cumsum and their rows gathered."""
    B, N = ptr.numel() - 1, batch.numel()
    emap = keep.nonzero().view(-1)
    new = ei.index_select(1, emap)
    ecnt = torch.bincount(batch[new[0]], minlength=B)
    zero = torch.zeros(1, dtype=torch.long, device=ei.device)
    eptr2 = torch.cat([zero, ecnt.cumsum(0)])
    if relabel:
        nodes = torch.zeros(N, dtype=torch.bool, device=ei.device)
        nodes[new.view(-1)] = True
        nmap = nodes.nonzero().view(-1)
        new = (nodes.long().cumsum(0) - 1)[new]
        batch, x = batch.index_select(0, nmap), x.index_select(0, nmap)
        ncnt = torch.bincount(batch, minlength=B)
        ptr = torch.cat([zero, ncnt.cumsum(0)])
    else:
        ncnt = ptr[1:] - ptr[:-1]
    mn, me = torch.stack([ncnt.max(), ecnt.max()]).tolist()            # the bounds as host ints, like the HIP path's read-back
    return new, ptr, eptr2, batch, x, emap, mn, me


def undirected_line(m, dev, iters):
    """explain / eval_fidelity at the headline batch, directed against undirected, in one process."""
    sh = SHAPES["headline"]
    B = sh["B"]
    b = Batch.from_data_list(sh["graphs"](B)).to(dev)
    node_gt, edge_gt = spmotif.ground_truth(b)
    edge = _scores(m, b)[0].clone()

    def twins():
        return _Layout(b).twins(b.edge_index)

    lay = _Layout(b)
    lay.twins(b.edge_index)
    out = dict(shape="headline", graphs=B, edges=int(b.edge_index.size(1)), max_edges=lay.max_edges,
               unpaired=int(lay.twins(b.edge_index)[1][0]))
    kw = dict(k="gt", edge_gt=edge_gt, node_gt=node_gt)
    out["explain_directed_ms"] = round(_time(lambda: explain(m, b, **kw), iters), 4)
    out["explain_undirected_ms"] = round(_time(lambda: explain(m, b, undirected="mean", **kw), iters), 4)
    out["edge_twin_ms"] = round(_time(twins, iters), 4)
    out["rank_edges_ms"] = round(_time(lambda: lay.rank_edges(edge, k="gt", gt=edge_gt, metrics=True), iters), 4)
    out["rank_edge_pairs_ms"] = round(_time(lambda: lay.rank_edge_pairs(edge, b.edge_index, "mean", k="gt", gt=edge_gt,
                                                                        metrics=True), iters), 4)
    n = max(3, iters // 5)
    out["eval_fidelity_directed_ms"] = round(_time(lambda: eval_fidelity(m, [b], dev), n, warmup=2), 4)
    out["eval_fidelity_undirected_ms"] = round(_time(lambda: eval_fidelity(m, [b], dev, undirected="mean"), n, warmup=2), 4)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,nodenum15,config5")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--undirected", action="store_true", help="the directed-against-undirected line at the headline batch")
    a = ap.parse_args()
    dev = "cuda"
    args = argparse.Namespace(layers=3, hidden=128, with_random=True, without_node_attention=False,
                              without_edge_attention=False, fc_num="222", cat_or_add="add", c=0.5, o=1.0, co=0.5,
                              eval_random=False)
    if a.undirected:
        torch.manual_seed(0)
        undirected_line(M.CausalGCN(10, 4, args).to(dev).eval(), dev, a.iters)
        return
    for name in a.shapes.split(","):
        sh = SHAPES[name]
        B = sh["B"]
        torch.manual_seed(0)
        m = M.CausalGCN(10, 4, args).to(dev).eval()
        gs = sh["graphs"](B * a.batches)
        b = Batch.from_data_list(gs[:B]).to(dev)
        edge, node = _scores(m, b)
        edge, node = edge.clone(), node.clone()
        lay = _Layout(b)
        node_gt, edge_gt = spmotif.ground_truth(b) if name != "config5" else (None, None)
        kw = dict(k="gt", gt=edge_gt, metrics=True) if edge_gt is not None else dict(k=16)
        t_rank = _time(lambda: rank_segments(edge, lay.edge_ptr, lay.max_edges, **kw), a.iters)
        t_rank_nodes = _time(lambda: rank_segments(node, lay.ptr, lay.max_nodes, k=16), a.iters)
        gid = b.batch[b.edge_index[0]]
        t_torch = _time(lambda: torch_rank(edge, gid, lay.edge_ptr, 16), a.iters)
        hm, hr, _ = rank_segments(edge, lay.edge_ptr, lay.max_edges, k=16)
        tm, tr = torch_rank(edge, gid, lay.edge_ptr, 16)
        same = bool(torch.equal(hr.long(), tr) and torch.equal(hm, tm))
        out = dict(shape=name, graphs=B, edges=int(b.edge_index.size(1)), nodes=int(b.batch.numel()),
                   max_edges=lay.max_edges, rank_edges_ms=round(t_rank, 4), rank_nodes_ms=round(t_rank_nodes, 4),
                   torch_rank_edges_ms=round(t_torch, 4), hip_equals_torch=same)
        # fidelity leg: extraction of the top 30 % of every graph's edges, HIP against the torch composition, and fidelity()
        keep = rank_segments(edge, lay.edge_ptr, lay.max_edges, ratio=0.3)[0]
        xf = b.x if b.x is not None else b.feat
        for relabel in (False, True):
            tag = "relabel" if relabel else "keep_ids"
            t_hip = _time(lambda: extract_subgraph(b, edge_mask=keep, relabel=relabel), a.iters)
            t_tor = _time(lambda: torch_extract(b.edge_index, lay.ptr, lay.edge_ptr, b.batch, xf, keep, relabel), a.iters)
            sub = extract_subgraph(b, edge_mask=keep, relabel=relabel)
            ref = torch_extract(b.edge_index, lay.ptr, lay.edge_ptr, b.batch, xf, keep, relabel)
            same_x = torch.equal(sub.x if sub.x is not None else sub.feat, ref[4])
            out["extract_%s_ms" % tag] = round(t_hip, 4)
            out["torch_extract_%s_ms" % tag] = round(t_tor, 4)
            out["extract_%s_equals_torch" % tag] = bool(torch.equal(sub.edge_index, ref[0]) and torch.equal(sub.edge_ptr, ref[2])
                                                        and torch.equal(sub.ptr, ref[1]) and same_x
                                                        and (sub.max_nodes, sub.max_edges) == (ref[6], ref[7]))
        out["fidelity_ms"] = round(_time(lambda: fidelity(m, b, ratio=0.3), max(3, a.iters // 5), warmup=2), 4)
        if name != "config5":
            loader = DataLoader(gs, batch_size=B, shuffle=False)
            t_ee = _time(lambda: eval_explanation(m, loader, dev), max(3, a.iters // 10), warmup=2)
            t_acc = _time(lambda: eval_acc_causal(m, loader, dev, args), max(3, a.iters // 10), warmup=2)
            out.update(batches=a.batches, eval_explanation_ms=round(t_ee, 3), eval_acc_causal_ms=round(t_acc, 3))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

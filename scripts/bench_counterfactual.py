"""ms per call of the counterfactual operators on one GPU, each beside its yardstick in the same process:

* ``subset_batch`` (two launches, one read-back) at the headline batch (SPMotif ``node_num`` 7, B 128, undirected players) for
  one round of a beam of 4 -- every state "graph minus one undirected edge" expanded by every remaining edge -- against the only
  other way to build the same replicas, ``coalition_batch`` with one int32 key row over the whole batch per replica (R x E
  keys; ``--max-key-gb`` caps R for that comparison).  The two are asserted equal before anything is timed, and timed alternately.
* the same ``subset_batch`` call through libcalhost (``--host-threads`` OpenMP threads).
* ``cal_beam_step`` on that round's candidates: the entry point alone (outputs allocated once) and the Python wrapper.
* ``counterfactual(beam=4, max_remove=3)`` end to end, per round and in total, against its forwards' share.
* with ``--train-steps``: a briefly trained CausalGCN on SPMotif (bias 0.9): the mean flip size of the search against the
  attention ranking and a random ranking (``eval_counterfactual`` with ``spmotif.ground_truth``).

    python scripts/bench_counterfactual.py [--iters 10] [--repeats 5] [--train-steps 300]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def sync():
    if torch.cuda.is_initialized():
        torch.cuda.synchronize()


def timed(fn, iters):
    sync()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    sync()
    return (time.perf_counter() - t0) / iters * 1e3


def alternate(fns, iters, repeats, warm=3):
    """Median ms per call of every function, the functions timed in turns (so drift hits all of them alike)."""
    for fn in fns:
        for _ in range(warm):
            fn()
    runs = [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            runs[i].append(timed(fn, iters))
    return [statistics.median(r) for r in runs], [max(r) - min(r) for r in runs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--graphs", type=int, default=128, help="batch size (128: the headline batch)")
    ap.add_argument("--beam", type=int, default=4)
    ap.add_argument("--max-key-gb", type=float, default=16.0, help="cap on the R x E int32 keys of the coalition_batch yardstick")
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--train-steps", type=int, default=300, help="0: skip the trained-model finding")
    ap.add_argument("--device", default="cuda", help="cpu rehearses the script through libcalhost; its times say nothing")
    a = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", str(a.host_threads))
    from cal_amd import _lib, model as M, spmotif
    from cal_amd.coalition import coalition_batch
    from cal_amd.counterfactual import beam_step, counterfactual, eval_counterfactual, lds_cap, pack_bits, subset_batch
    from cal_amd.data import Batch, DataLoader
    from cal_amd.explain import _Layout, _log_probs
    from cal_amd.plan import _p, _stream
    from cal_amd.replica import _grouped, _Players
    dev, beam = a.device, a.beam
    args = argparse.Namespace(layers=3, hidden=128, with_random=True, without_node_attention=False,
                              without_edge_attention=False, fc_num="222", cat_or_add="add", c=0.5, o=1.0, co=0.5)
    torch.manual_seed(0)
    m = M.CausalGCN(10, 4, args).to(dev).eval()
    b = Batch.from_data_list(spmotif.train_mix(a.graphs, node_num=7, seed=1)).to(dev)
    lay = _Layout(b)
    src = _grouped(b, lay)
    B, E = int(b.num_graphs), int(b.edge_index.size(1))
    out = {"batch": {"graphs": B, "nodes": int(b.batch.numel()), "columns": E}}

    # the second round of a beam of `beam`: state s of graph g is g without its s-th undirected edge; every state is expanded by
    # every undirected edge still in it
    P = _Players(b, lay, src, "edges", "mean")
    gid, loc = P.gid, torch.arange(E, device=dev) - P.seg[P.gid]
    n = P.count(P.rep)
    pos = torch.cumsum(P.rep.long(), 0) - 1 - (torch.cumsum(n, 0) - n)[gid]              # a representative's index among its graph's
    rows = []
    for s in range(beam):
        gone = P.rep & (pos == s)
        gone = gone | (gone[P.twin.clamp(min=0).long()] & (P.twin >= 0))
        rows.append(pack_bits(~gone, P.seg, P.max_seg))
    bits = torch.stack(rows, 1).reshape(B * beam, -1).contiguous()
    cand = (P.rep.view(E, 1) & (pos.view(E, 1) != torch.arange(beam, device=dev).view(1, beam))).view(-1).nonzero().view(-1)
    e, s = cand // beam, cand % beam
    rg, rflip = gid[e], loc[e]
    rrow = rg * beam + s
    R = int(rg.numel())
    cnt = torch.zeros(B, dtype=torch.long, device=dev).index_add_(0, rg, torch.ones_like(rg))
    cand_ptr = torch.cat([torch.zeros(1, dtype=torch.long, device=dev), torch.cumsum(cnt, 0)])
    print("one round of beam %d: %d replicas of %d graphs (%d undirected edges); bits %s" % (beam, R, B, int(n.sum()), tuple(bits.shape)),
          flush=True)

    # 1. subset_batch against coalition_batch with a key row per replica
    Rk = min(R, int(a.max_key_gb * 2 ** 30 / (4 * E)))
    key = torch.zeros(Rk, E, dtype=torch.int32, device=dev)                              # 0: stays; 1: gone (threshold 1)
    rr = torch.arange(Rk, device=dev)
    state_gone = ~torch.stack([((bits[rrow[:Rk], w].long().view(-1, 1) >> torch.arange(32, device=dev)) & 1).bool()
                               for w in range(bits.size(1))], 1).reshape(Rk, -1)          # [Rk, 32 W] local
    elo = P.seg[rg[:Rk]]
    m_g = (P.seg[1:] - P.seg[:-1])[rg[:Rk]]
    j = torch.arange(state_gone.size(1), device=dev).view(1, -1)
    rows_, cols_ = (state_gone & (j < m_g.view(-1, 1))).nonzero(as_tuple=True)
    key[rows_, elo[rows_] + cols_] = 1
    key[rr, elo + rflip[:Rk]] = 1
    tw = P.twin[(elo + rflip[:Rk])].long()
    key[rr[tw >= 0], tw[tw >= 0]] = 1
    one_th = torch.ones(Rk, dtype=torch.long, device=dev)
    sub = lambda k=Rk: subset_batch(src, rg[:k], bits, rep_row=rrow[:k], rep_flip=rflip[:k], twin=P.twin)
    coal = lambda: coalition_batch(src, rg[:Rk], one_th, key, rep_row=rr)
    one, two = sub(), coal()
    for k in ("edge_index", "ptr", "edge_ptr", "batch", "node_src", "edge_src", "feat" if one.x is None else "x"):
        assert torch.equal(getattr(one, k), getattr(two, k)), k
    (t1, t2), (s1, s2) = alternate([sub, coal], a.iters, a.repeats)
    out["builder"] = {"replicas": Rk, "of": R, "nodes": int(one.batch.numel()), "columns": int(one.edge_index.size(1)),
                      "key_bytes": 4 * Rk * E, "bits_bytes": 4 * bits.numel() + 24 * Rk, "subset_batch_ms": t1,
                      "coalition_batch_ms": t2, "spread_ms": [s1, s2]}
    print("builder  R %6d of %6d  N' %8d  E' %9d  subset_batch %8.3f ms (spread %.3f; %.1f MB of bits and replica lists)  "
          "coalition_batch %8.3f ms (spread %.3f; %.1f MB of keys)" % (Rk, R, one.batch.numel(), one.edge_index.size(1), t1, s1,
                                                                       out["builder"]["bits_bytes"] / 1e6, t2, s2, 4 * Rk * E / 1e6), flush=True)
    del key, two, state_gone
    if R != Rk:
        (t1,), (s1,) = alternate([lambda: sub(R)], a.iters, a.repeats)
        out["builder_all"] = {"replicas": R, "subset_batch_ms": t1, "spread_ms": s1}
        print("builder  all %d replicas: subset_batch %8.3f ms (spread %.3f)" % (R, t1, s1), flush=True)

    # 2. the same call through libcalhost
    cpu = lambda t: t.cpu()
    hb = Batch.from_data_list(spmotif.train_mix(a.graphs, node_num=7, seed=1))
    hsrc = _grouped(hb, _Layout(hb))
    hargs = (cpu(rg), cpu(bits))
    hkw = dict(rep_row=cpu(rrow), rep_flip=cpu(rflip), twin=cpu(P.twin))
    assert torch.equal(subset_batch(hsrc, *hargs, **hkw).edge_index, sub(R).edge_index.cpu())
    (t1,), (s1,) = alternate([lambda: subset_batch(hsrc, *hargs, **hkw)], max(a.iters // 5, 2), max(a.repeats // 2, 3), warm=1)
    out["builder_host"] = {"replicas": R, "threads": int(os.environ["OMP_NUM_THREADS"]), "subset_batch_ms": t1, "spread_ms": s1}
    print("builder  libcalhost, %s threads, all %d replicas: subset_batch %8.3f ms (spread %.3f)" % (os.environ["OMP_NUM_THREADS"], R, t1, s1),
          flush=True)

    # 3. the beam step on that round's candidates
    g = torch.Generator().manual_seed(2)
    p = torch.rand(R, generator=g).to(dev)
    fl = torch.zeros(R, dtype=torch.uint8, device=dev)
    n_state = torch.full((B,), beam, dtype=torch.long, device=dev)
    W = int(bits.size(1))
    cap = lds_cap(dev == "cpu")
    assert int(cnt.max()) <= cap

    def wrapper():
        done = torch.zeros(B, dtype=torch.uint8, device=dev)
        return beam_step(bits, n_state, cand_ptr, rrow, rflip, p, fl, P.seg, E, done, torch.zeros(B, W, dtype=torch.int32, device=dev),
                         torch.zeros(B, device=dev), torch.full((B,), -1, dtype=torch.long, device=dev), beam=beam, twin=P.twin,
                         max_cand=cap)
    nxt = wrapper()
    assert int(nxt[2].min()) == beam and int(nxt[3].max()) == 0
    done = torch.zeros(B, dtype=torch.uint8, device=dev)
    bo, po, no, st = torch.zeros_like(bits), torch.zeros(B * beam, device=dev), torch.zeros(B, dtype=torch.long, device=dev), \
        torch.zeros(B, dtype=torch.int32, device=dev)
    cfb, cfp, cfc = torch.zeros(B, W, dtype=torch.int32, device=dev), torch.zeros(B, device=dev), torch.zeros(B, dtype=torch.long, device=dev)
    host = dev == "cpu"
    seg = P.seg.contiguous()

    def entry():
        _lib.call("cal_beam_step", _p(bits), B, beam, W, _p(n_state), _p(cand_ptr), _p(rrow), _p(rflip), _p(p), _p(fl), R, _p(seg), E,
                  _p(P.twin), 0, cap, _p(done), _p(bo), _p(po), _p(no), _p(cfb), _p(cfp), _p(cfc), _p(st), None if host else _stream(),
                  host=host)
    (t1, t2), (s1, s2) = alternate([entry, wrapper], a.iters * 20, a.repeats)
    out["beam_step"] = {"graphs": B, "candidates": R, "largest": int(cnt.max()), "entry_ms": t1, "wrapper_ms": t2, "spread_ms": [s1, s2]}
    print("beam step  %d graphs, %d candidates (at most %d a graph)  cal_beam_step %7.4f ms (spread %.4f)  beam_step() %7.4f ms "
          "(spread %.4f)" % (B, R, int(cnt.max()), t1, s1, t2, s2), flush=True)

    # 4. counterfactual end to end (an untrained model: hardly a graph flips, so every round runs on the whole batch)
    kw = dict(undirected="mean", beam=beam, max_remove=3)
    cf = counterfactual(m, b, **kw)
    (t1,), (s1,) = alternate([lambda: counterfactual(m, b, **kw)], max(a.iters // 5, 2), a.repeats, warm=1)
    out["counterfactual"] = {"rounds": cf.rounds, "replicas": cf.replicas, "forwards": cf.forwards, "found": int(cf.found.sum()),
                             "total_ms": t1, "per_round_ms": t1 / max(cf.rounds, 1), "spread_ms": s1}
    print("counterfactual beam %d, %d rounds  replicas %7d  forwards %4d  found %d  total %9.3f ms (spread %.3f)  per round %9.3f ms"
          % (beam, cf.rounds, cf.replicas, cf.forwards, int(cf.found.sum()), t1, s1, t1 / max(cf.rounds, 1)), flush=True)
    rep512 = sub(512)

    def fwd():
        with torch.no_grad():
            _log_probs(m, rep512)
    (t1,), (s1,) = alternate([fwd], a.iters * 2, a.repeats)
    out["counterfactual"]["forward_512_ms"] = t1
    print("   one eval forward of 512 replicas %7.3f ms (spread %.3f): the %d forwards alone are about %.1f ms"
          % (t1, s1, cf.forwards, t1 * cf.forwards), flush=True)

    # 5. the finding: a briefly trained CausalGCN on SPMotif, bias 0.9
    if dev != "cpu" and a.train_steps:
        from cal_amd.trainer import CausalTrainer
        torch.manual_seed(0)
        mt = M.CausalGCN(10, 4, args).to(dev)
        train = spmotif.train_mix(a.graphs * 8, bias=0.9, node_num=7, seed=2)
        test = spmotif.train_mix(a.graphs, bias=0.9, node_num=7, seed=3)
        tr = CausalTrainer(mt, args, lr=1e-3, use_graph=False)
        step = 0
        while step < a.train_steps:
            for bt in DataLoader(train, batch_size=a.graphs, shuffle=True):
                tr.step(bt.to(dev))
                step += 1
                if step >= a.train_steps:
                    break
        mt.eval()
        t = time.perf_counter()
        res = eval_counterfactual(mt, DataLoader(test, batch_size=a.graphs, shuffle=False), dev, undirected="mean", beam=beam,
                                  edge_gt="spmotif")
        sync()
        res["ms"] = (time.perf_counter() - t) * 1e3
        res["train_steps"] = a.train_steps
        out["trained"] = res
        print("after %d steps, %d test graphs: search flips %.3f of them with %.2f undirected edges on average; the attention ranking "
              "%.3f with %.2f; a random ranking %.3f with %.2f; %.3f of the removed edges lie in the motif, %.3f of the sets entirely "
              "(%d replicas, %d forwards, %.0f ms)"
              % (a.train_steps, res["graphs"], res["flip_rate"], res["size_mean"], res["attention_flip_rate"], res["attention_size_mean"],
                 res["random_flip_rate"], res["random_size_mean"], res["removed_in_motif"], res["inside_motif_rate"], res["replicas"],
                 res["forwards"], res["ms"]), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

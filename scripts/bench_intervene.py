"""ms per call of ``intervene`` (bank=None style: the batch's pooled rows against a bank of trivial rows), read-back included,
beside the torch broadcast composition of the same result on the same device in the same process.

Headline batch: SPMotif ``node_num`` 7, B 128, H 128, add; banks of 128 rows (the batch's own) and 2 048 rows.

    python scripts/bench_intervene.py [--iters 50]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_composition(m, xo, xc, y):
    """The same five results by broadcasting: materialises [B, M, H] (and the B M x H x H GEMM behind fc1)."""
    x = xc[None, :, :] + xo[:, None, :]                                  # add
    B, M, H = x.shape
    h = torch.relu(m.fc1_co(m.fc1_bn_co(x.view(B * M, H))))
    lp = torch.log_softmax(m.fc2_co(m.fc2_bn_co(h)), -1).view(B, M, -1)
    p = lp.exp()
    pr = p.gather(2, y[:, None, None].expand(-1, M, 1)).squeeze(2)
    pmin, jmin = pr.min(1)
    return p.mean(1), (lp.argmax(-1) == y[:, None]).sum(1), pmin, jmin


def timed(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    from cal_amd import model as M, spmotif
    from cal_amd.data import Batch
    from cal_amd.intervene import intervene, intervention_readout, pooled_representations
    dev = "cuda"
    args = argparse.Namespace(layers=3, hidden=128, with_random=True, without_node_attention=False, without_edge_attention=False,
                              fc_num="222", cat_or_add="add", c=0.5, o=1.0, co=0.5)
    torch.manual_seed(0)
    m = M.CausalGCN(10, 4, args).to(dev).eval()
    b = Batch.from_data_list(spmotif.train_mix(128, node_num=7, seed=1)).to(dev)
    y = b.y.view(-1)
    xc, xo = pooled_representations(m, b)
    big = torch.cat([xc] * 16)[torch.randperm(2048, device=dev)].contiguous()      # 2 048 trivial rows
    out = {}
    for name, bank in (("bank128", None), ("bank2048", big)):
        rows = xc if bank is None else bank
        r = intervene(m, b, bank=bank)
        with torch.no_grad():
            ref = torch_composition(m, xo, rows, y)
        out[name + "_max_abs_p_do_diff"] = float((r.p_do - ref[0]).abs().max())

        def full():                                                      # forward + readout + read-back
            res = intervene(m, b, bank=bank)
            return res.p_do.cpu(), res.hits.cpu(), res.p_min.cpu(), res.j_min.cpu()

        def op():                                                        # the operator alone + read-back
            res = intervention_readout(m, xo, rows, y)
            return res.p_do.cpu(), res.hits.cpu(), res.p_min.cpu(), res.j_min.cpu()

        def comp():
            with torch.no_grad():
                return [t.cpu() for t in torch_composition(m, xo, rows, y)]

        out[name + "_intervene_ms"] = timed(full, a.iters)
        out[name + "_operator_ms"] = timed(op, a.iters)
        out[name + "_torch_ms"] = timed(comp, a.iters)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

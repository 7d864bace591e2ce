"""Phase clocks of the products of the per-graph GCNConv backward (engine_gconv_bwd_body.hpp), for either build-time order of
dX' and dW (-DCAL_GCB_ORDER=0|1).  Build with CAL_HIPCC_EXTRA="-DCAL_BLK_CLOCKS -DCAL_GCB_ORDER=.." and run from the repo root:

    python scripts/blk_clocks_order.py

Runs the headline step truncated behind every launch site named k_gconv_bwd or k_att_bwd_graph (the folded ATT entry) and
prints, per site, the marks of the body.  Every translation unit that holds an entry has clock buffers of its own (engine.hip:
cal_debug_blk_clocks / _x; gconv_bwd_seq.hip: cal_debug_blk_clocks_seq; gconv_bwd_att.hip: cal_debug_blk_clocks_att): the unit
whose entry clocks are the latest is the one that ran the site's launch.

    mark4   order 0: the dX' accumulators of wave 0 are done          order 1: the dX' accumulator of wave 4 (row tile 1) is done
    mark5   order 0: wave 0's dX' tiles and striped atomics have left  order 1: wave 4's tile and atomics have left
    mark6   order 0: wave 4's dW slab tiles have left                  order 1: wave 4's slab tile has left (last into stage B)
    exit    lane 0 of wave 0 (order 0: behind mark5; order 1: behind its own slab tile's ISSUE, not its arrival)

Every mark waits for the memory counters of its own wave only -- in order 1 that makes wave 4 wait at mark5 for the very
atomics the order lets drain under stage B, so mark5 -> mark6 of that build is stage B in isolation and the launch is longer than
it is without clocks.  LEAN instantiations run order 0 and carry its marks in either build."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cal_amd import _lib, model as M, spmotif          # noqa: E402
from cal_amd.data import Batch                         # noqa: E402
from cal_amd.engine import StepEngine                  # noqa: E402
import argparse                                        # noqa: E402

args = argparse.Namespace(layers=3, hidden=128, with_random=True, without_node_attention=False,
                          without_edge_attention=False, fc_num="222", cat_or_add="add", c=0.5, o=1.0, co=0.5)
torch.manual_seed(0)
m = M.CausalGCN(10, 4, args).cuda().train()
eng = StepEngine(m)
b = Batch.from_data_list(spmotif.train_mix(128, seed=5)).to("cuda")
perm = torch.randperm(128, device="cuda")
h = _lib.lib()
for fn in ("cal_debug_blk_clocks", "cal_debug_blk_clocks_x"):
    getattr(h, fn).argtypes = [ctypes.c_void_p]
    getattr(h, fn).restype = ctypes.c_int
for fn in ("cal_debug_blk_clocks_att", "cal_debug_blk_clocks_seq"):
    getattr(h, fn).argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    getattr(h, fn).restype = ctypes.c_int
eng.train_step(b, perm, adam=False)
torch.cuda.synchronize()
names, k = [], 1
while True:
    nm = h.cal_engine_stage_name(k)
    nm = nm.decode() if isinstance(nm, bytes) else nm
    if not nm:
        break
    names.append(nm)
    k += 1
NWG = int(os.environ.get("BLK_N", "256"))                  # 128 graphs x 2 slices
for site, nm in enumerate(names, 1):
    if nm not in ("k_gconv_bwd", "k_att_bwd_graph"):
        continue
    h.cal_engine_debug_stop(site)
    for _ in range(5):
        eng.train_step(b, perm, adam=False)
    torch.cuda.synchronize()
    o, x = (ctypes.c_longlong * 8192)(), (ctypes.c_longlong * 8192)()
    src = "engine.hip"
    assert h.cal_debug_blk_clocks(o) == 0 and h.cal_debug_blk_clocks_x(x) == 0
    t = np.concatenate([np.array(list(o), dtype=np.int64).reshape(2048, 4), np.array(list(x), dtype=np.int64).reshape(2048, 4)], 1)[:NWG] / 100.0
    for acc, unit in ((h.cal_debug_blk_clocks_att, "gconv_bwd_att.hip"), (h.cal_debug_blk_clocks_seq, "gconv_bwd_seq.hip")):
        assert acc(o, x) == 0
        ta = np.concatenate([np.array(list(o), dtype=np.int64).reshape(2048, 4), np.array(list(x), dtype=np.int64).reshape(2048, 4)], 1)[:NWG] / 100.0
        if ta[:, 0].max() > t[:, 0].max():                # this unit's entry ran the latest instrumented launch
            t, src = ta, unit
    t = t[t[:, 3] > 0]
    t = t[t[:, 0] > t[:, 0].max() - 100.0]                 # the workgroups of the latest launch
    t0 = t[:, 0].min()
    d = t[:, 3] - t[:, 0]
    print("site %d %s (%s): %d workgroups, starts spread %.2f us, entry->exit min/med/max %.2f/%.2f/%.2f us"
          % (site, nm, src, len(t), t[:, 0].max() - t0, d.min(), np.median(d), d.max()))
    ok = (t[:, 4] > t[:, 0]) & (t[:, 5] > t[:, 0]) & (t[:, 6] > t[:, 0])
    if not ok.all():
        print("   no marks 4-6 from this launch (a LEAN instantiation)")
        continue
    end = np.maximum(t[:, 3], t[:, 6])
    for name, ya, yb in (("entry->mark4", t[:, 0], t[:, 4]), ("mark4->mark5", t[:, 4], t[:, 5]), ("mark5->mark6", t[:, 5], t[:, 6]),
                         ("mark4->mark6", t[:, 4], t[:, 6]), ("mark6->exit", t[:, 6], t[:, 3]), ("entry->last of exit, mark6", t[:, 0], end)):
        v = yb - ya
        print("   %-28s min/med/max %6.2f/%6.2f/%6.2f us" % (name, v.min(), np.median(v), v.max()))
    print("   launch: first entry -> last end %.2f us" % (end.max() - t0))
h.cal_engine_debug_stop(0)

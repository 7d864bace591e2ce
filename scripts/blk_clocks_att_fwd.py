"""Phase clocks of the folded attention forward k_gconv_fwd_att (gconv_fwd_att.hip: engine_gconv.hpp + engine_attfwd_fold.hpp).
Build with CAL_HIPCC_EXTRA="-DCAL_BLK_CLOCKS" (add -DCAL_AFF_ACQUIRE for the consumer form with the agent-scope acquire) and run
from the repo root:

    python scripts/blk_clocks_att_fwd.py

Runs the headline step truncated behind the launch site k_gconv_fwd_att and prints the marks of its 256 workgroups (the kernel
writes gconv_fwd_att.hip's copy of the clock buffers, read through cal_debug_blk_clocks_fwd_att):

    entry   top of the kernel                       mark2   extents known            mark3   operands staged (first product starts)
    mark4   wave 0's second product is done         mark5   partial dots stored, drained, barrier passed (the flag store follows)
    mark6   partner's flag seen, barrier passed     mark7   column statistics issued    exit    (slice 0: behind the edge phase)

mark5 -> mark6 is the hand-off: the flag's way to the partner, and the partner's own delay."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cal_amd import _lib, model as M, spmotif          # noqa: E402
from cal_amd.data import Batch                         # noqa: E402
from cal_amd.engine import StepEngine                  # noqa: E402

args = argparse.Namespace(layers=3, hidden=128, with_random=True, without_node_attention=False,
                          without_edge_attention=False, fc_num="222", cat_or_add="add", c=0.5, o=1.0, co=0.5)
torch.manual_seed(0)
m = M.CausalGCN(10, 4, args).cuda().train()
eng = StepEngine(m)
b = Batch.from_data_list(spmotif.train_mix(128, seed=5)).to("cuda")
perm = torch.randperm(128, device="cuda")
h = _lib.lib()
h.cal_debug_blk_clocks_fwd_att.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
h.cal_debug_blk_clocks_fwd_att.restype = ctypes.c_int
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
site = names.index("k_gconv_fwd_att") + 1
h.cal_engine_debug_stop(site)
for rep in range(3):
    for _ in range(5):
        eng.train_step(b, perm, adam=False)
    torch.cuda.synchronize()
    o, x = (ctypes.c_longlong * 8192)(), (ctypes.c_longlong * 8192)()
    assert h.cal_debug_blk_clocks_fwd_att(o, x) == 0
    t = np.concatenate([np.array(list(o), dtype=np.int64).reshape(2048, 4), np.array(list(x), dtype=np.int64).reshape(2048, 4)], 1)[:256] / 100.0
    t0 = t[:, 0].min()
    print("run %d: 256 workgroups, starts spread %.2f us, launch first entry -> last exit %.2f us" % (rep, t[:, 0].max() - t0, t[:, 3].max() - t0))
    for sl, tag in ((slice(0, 128), "slice 0"), (slice(128, 256), "slice 1")):
        u = t[sl]
        for name, ya, yb in (("entry->mark3 (staged)", 0, 2), ("mark3->mark4 (products)", 2, 4), ("mark4->mark5 (published)", 4, 5),
                             ("mark5->mark6 (partner seen)", 5, 6), ("mark6->mark7 (statistics)", 6, 7), ("mark7->exit", 7, 3), ("entry->exit", 0, 3)):
            v = u[:, yb] - u[:, ya]
            print("   %s  %-28s min/med/max %6.2f/%6.2f/%6.2f us" % (tag, name, v.min(), np.median(v), v.max()))
h.cal_engine_debug_stop(0)

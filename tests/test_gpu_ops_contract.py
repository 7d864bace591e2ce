"""The operator-level kernels of csrc/gcn.hip, csrc/attn.hip and csrc/plan.hip on the MI355X, launcher by launcher through the
exported entry points with raw pointers, on the case table of tests/ops_contract_cases.py (56 instantiations of the ten dispatched
kernels, every sweep and part count, every aligned16 term once the only false one) against the float64 restatement and the
derived bounds of tests/ops_contract_ref.py (its module docstring has every derivation; tests/test_ops_contract_ref.py ties it
to the oracle, to autograd and to the host twin, and shows that the bounds notice fourteen seeded defects).

Every case: outputs and workspaces NaN-filled (integers -7) before the launch; a canary block behind every operand, output and
workspace, and in front of the ones that start one element past their allocation; self-loop columns of w, norm_e and datt NaN;
every launcher twice on fresh outputs, identical bits asked for (one writer per element, fixed order); intermediates that a
launcher hands back (dis, gn_e, gself, ddeg, pq, att_n) judged stage by stage against fp64 on the kernel's own stored values.
The relative error x of the device's fp32 exp in the two softmax bounds is measured by test_gpu_sparse_contract's helper
(against fp64 exp over the range of the case's arguments, at least 2 u).

The worst err / bound seen on MI355X is recorded in each test's docstring: a record, the threshold is the derived bound, 1.
"""
import time

import numpy as np
import pytest
import torch

from tests import ops_contract_cases as C
from tests.helpers import Buf, pool_intact
from tests.test_gpu_sparse_contract import _device_exp_error

pytestmark = pytest.mark.gpu


class GpuBackend:
    """libcalhip.so on device pointers, on torch's current stream"""

    def __init__(self):
        self.pool = []

    def buf(self, n, dtype=torch.float32, fill=None, data=None, off=0):
        return Buf(self.pool, n, dtype, fill, data, off)

    def call(self, name, *args):
        from cal_amd import _lib
        from cal_amd.plan import _stream
        _lib.call(name, *args, _stream())

    def query(self, name, *args):
        from cal_amd import _lib
        return _lib.query(name, *args)

    def intact(self):
        torch.cuda.synchronize()
        return pool_intact(self.pool)

    def cpu(self, b):
        return b.t.cpu()


def _exp_error(gap):
    return _device_exp_error(-float(np.ceil(gap + 1.0)))


def _run_launcher(launcher):
    worst, bad, t0 = {}, [], time.time()
    cs = C.cases_of(launcher)
    assert cs
    for c in cs:
        i = C.inputs_of(c)
        got, fails = C.run(c, i, GpuBackend())
        rat, f2 = C.judge(c, i, got, _exp_error)
        bad += ["%s: %s" % (c["name"], f) for f in fails + f2]
        for k, v in rat.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("%-16s %3d cases in %.1f s, worst err/bound %s" % (launcher, len(cs), time.time() - t0, {k: "%.3g" % v for k, v in worst.items()}))
    assert not bad, "\n".join(bad)
    assert all(v <= 1.0 for v in worst.values()), worst


def test_gcn_norm_fwd():
    """k_gcn_deg, k_gcn_norm_e.  Worst on MI355X (err / bound, bound 1): dis 0.15, norm_e 0.45."""
    _run_launcher("norm_fwd")


def test_spmm_fwd():
    """k_spmm<VEC, G>, eight instantiations, both views.  Worst on MI355X: out 0.38."""
    _run_launcher("spmm")


def test_relu_bwd_colsum():
    """k_relu_bwd_colsum<VEC>, k_colsum_finish in every mode.  Worst on MI355X: dz exact, dbias 0.041."""
    _run_launcher("relu_bwd_colsum")


def test_gcn_norm_bwd():
    """k_sddmm<VEC, G>, k_gcn_norm_bwd_node, k_gcn_norm_bwd_edge, stage by stage.  Worst on MI355X: gn_e 0.54, gself 0.52, ddeg 0.29, dw 0.36."""
    _run_launcher("norm_bwd")


def test_edge_att_fwd():
    """k_edge_proj<VEC, G>, k_edge_softmax2.  Worst on MI355X: pq 0.53, att 0.25 (the measured error of the device exp stayed under its floor of 2 u)."""
    _run_launcher("edge_att_fwd")


def test_edge_att_bwd():
    """k_edge_softmax2_bwd, k_edge_att_bwd_node, k_edge_att_bwd_x<VEC>, k_edge_att_bwd_finish, end to end, accumulate 0 and 1.
    Worst on MI355X: dx 0.38, dW 0.020, db 0.0083."""
    _run_launcher("edge_att_bwd")


def test_node_att_split_fwd():
    """k_node_att_split<VEC, G>.  Worst on MI355X: att_n 0.15, xc 0.999, xo 0.996 (one multiply against a bound of one rounding:
    an entry rounded by almost half an ulp sits at 1 / SLACK)."""
    _run_launcher("node_att_fwd")


def test_node_att_split_bwd():
    """k_node_att_split_bwd<VEC, G>, k_wcolsum1<VEC>, k_node_att_bwd_finish, end to end.  Worst on MI355X: dx 0.41, dWn 0.0069,
    dbn 0.0030."""
    _run_launcher("node_att_bwd")


def test_add_pool_fwd():
    """k_add_pool<VEC>, k_pool_finish at S = 1, 2, 3, 64.  Worst on MI355X: out 0.998 (a graph of two rows: one rounding against a bound of one)."""
    _run_launcher("add_pool_fwd")


def test_add_pool_bwd():
    """k_add_pool_bwd<VEC, G>: exact."""
    _run_launcher("add_pool_bwd")


@pytest.mark.parametrize("name", list(C.PLAN_CASES))
def test_plan_build(name):
    """cal_plan_build: every output exactly the stable counting sort, nothing written behind nnz, status, `work` inside its
    canaries; two launches give the same six arrays (the unordered tn / te scratch inside `work` is not compared)"""
    ei, n = C.PLAN_CASES[name]()
    be = GpuBackend()
    a, b = C.launch_plan(ei, n, be), C.launch_plan(ei, n, be)
    assert be.intact()
    got, again = ({k: be.cpu(v).numpy() for k, v in o.items()} for o in (a, b))
    fails = C.judge_plan(ei, n, got)
    assert not fails, fails
    assert all(np.array_equal(got[k], again[k]) for k in got)


@pytest.mark.parametrize("name", list(C.GRAPH_PTR_CASES))
def test_graph_ptr(name):
    batch, B, valid = C.GRAPH_PTR_CASES[name]
    be = GpuBackend()
    o = C.launch_graph_ptr(batch, B, be)
    assert be.intact()
    fails = C.judge_graph_ptr(batch, B, valid, {k: be.cpu(v).numpy() for k, v in o.items()})
    assert not fails, fails

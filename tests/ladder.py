"""The degree-ladder batch of the kernel-by-kernel contract tests (tests/test_gpu_sparse_contract.py,
tests/test_gpu_gat_contract.py): N = 301 nodes in three block-diagonal graphs, ~4.5 k edges.  Graph 0 has 256 nodes, node v has
exactly ladder[v] slots over distinct neighbours in the view under test -- every count 0..72, then 127..129 and 191..193, the
rest 1..6; graph 1 has 5 nodes and no edge; graph 2 is a 40-node random graph with one directed edge; five input self loops
(their edge ids carry no slot).  numpy only: the CPU tests use it too."""
import functools

import numpy as np

from tests import sparse_contract_ref as ref

LADDER = list(range(73)) + [127, 128, 129, 191, 192, 193]
N0, N1, N2 = 256, 5, 40
N = N0 + N1 + N2


@functools.lru_cache(maxsize=None)
def ladder_batch(key):
    """the batch whose view by edge_index[key] carries the ladder; -> dict of numpy arrays"""
    rng = np.random.default_rng(1000 + key)
    deg0 = np.array(LADDER + list(rng.integers(1, 7, N0 - len(LADDER))))
    rng.shuffle(deg0)
    own, other = [], []
    for v in range(N0):
        nb = rng.choice(N0 - 1, int(deg0[v]), replace=False)
        nb = nb + (nb >= v)                                     # distinct neighbours, never v itself
        own += [v] * int(deg0[v]); other += nb.tolist()
    a = np.triu(rng.random((N2, N2)) < 0.15, 1)
    a = a | a.T
    s, d = np.nonzero(a)
    off = N0 + N1
    own += (s + off).tolist(); other += (d + off).tolist()
    i, j = next((i, j) for i in range(N2) for j in range(i + 1, N2) if not a[i, j])
    own.append(off + i); other.append(off + j)                  # the directed edge: no reverse
    deg = np.concatenate([deg0, np.zeros(N1, np.int64), a.sum(1)])
    deg[off + i] += 1
    for v in (3, 3, 100, off + 9, off + 30):                    # input self loops: their edge ids have no slot
        own.append(v); other.append(v)
    perm = rng.permutation(len(own))
    ei = np.zeros((2, len(own)), np.int64)
    ei[key], ei[1 - key] = np.asarray(own)[perm], np.asarray(other)[perm]
    ptr, nbr, eid = ref.csr_view(ei, N, key)
    batch = np.repeat(np.arange(3), [N0, N1, N2]).astype(np.int64)
    slotted = np.zeros(ei.shape[1], bool)
    slotted[eid] = True
    return {"ei": ei, "E": ei.shape[1], "ptr": ptr, "nbr": nbr, "eid": eid, "deg": deg, "deg0": deg0, "batch": batch,
            "slotted": slotted, "key": key}

"""The toolkit the three batch builders share (cal_amd/csrc/rebatch.hpp), where their own suites do not reach: the 256-thread
count kernels walking several chunks of nodes and columns (the suites' graphs above 468 columns all take the 1024-thread
kernels, and no coalition case has more than one chunk), and the completion tickets with calls in flight on two streams.
Every result is compared bit for bit with the host twin's on the CPU copy of the same inputs.

    python -m pytest tests/test_gpu_rebatch.py -m gpu
"""
import pytest
import torch

from cal_amd.coalition import coalition_batch
from cal_amd.data import Batch, Data
from cal_amd.occlude import occlude_batch
from cal_amd.splice import splice_batches

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


def _ring(k, feat, g):
    src = torch.arange(k)
    ei = torch.stack([torch.cat([src, (src + 1) % k]), torch.cat([(src + 1) % k, src])])          # a ring, both directions
    return Data(x=torch.randn(k, feat, generator=g), edge_index=ei, y=torch.randint(0, 4, (1,), generator=g))


def _dev(b):
    d = Batch()
    for k, v in b.__dict__.items():
        d.__dict__[k] = v.to(DEV) if torch.is_tensor(v) else v
    d._plan = None
    return d


def _same(u, v):
    assert u.edge_index.is_cuda and not v.edge_index.is_cuda
    for key in ("edge_index", "ptr", "edge_ptr", "batch", "node_src", "edge_src", "x", "y"):
        a, b = getattr(u, key), getattr(v, key)
        assert (a is None) == (b is None) and (a is None or torch.equal(a.cpu(), b)), key
    for key in ("num_graphs", "max_nodes", "max_edges", "empty_graphs", "no_self_loops"):
        assert getattr(u, key) == getattr(v, key), key
    assert getattr(u, "bridges_unwritten", None) == getattr(v, "bridges_unwritten", None)


def _on(dev, args, kw):
    return [a.to(dev) if torch.is_tensor(a) else a for a in args], {k: v.to(dev) if torch.is_tensor(v) else v for k, v in kw.items()}


def _both(fn, batches, args, kw):
    """fn on the device and on the CPU copy of the same inputs."""
    da, dk = _on(DEV, args, kw)
    return fn(*[_dev(b) for b in batches], *da, **dk), fn(*batches, *args, **kw)


# ---- 1. several chunks on the 256-thread kernels --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chunked():
    """A 600-node ring (1200 columns) between ten 3-node rings: 114 columns per graph on average, so the count kernels run with
    256 threads and walk 3 chunks of nodes and 5 of columns at the large graph (graph 5: nodes 15 .. 614, columns 30 .. 1229)."""
    g = torch.Generator().manual_seed(13)
    b = Batch.from_data_list([_ring(3, 4, g) for _ in range(5)] + [_ring(600, 4, g)] + [_ring(3, 4, g) for _ in range(5)])
    assert int(b.edge_index.size(1)) // b.num_graphs <= 2048 and int(b.edge_ptr[6] - b.edge_ptr[5]) == 1200
    return b, g


def test_splice_walks_chunks(chunked):
    b, _ = chunked
    ga = torch.tensor([5, 0, 5, -1, 3, 5])
    gb = torch.tensor([1, 5, 5, 5, -1, 11])
    _same(*_both(splice_batches, [b, b], [ga, gb], {"bridge": "first"}))


@pytest.mark.parametrize("use", ["edges", "nodes"])
def test_occlude_walks_chunks(chunked, use):
    b, _ = chunked
    rg = torch.tensor([4, 5, 5, 5, 5, 6, -1, 5])
    lo = 30 if use == "edges" else 15                     # the large graph's first column / node
    re = torch.tensor([0, lo, lo + 255, lo + 256, lo + 599, -1, 0, -1])   # chunk edges, the last node, two controls
    _same(*_both(occlude_batch, [b], [rg, re], {"use": use}))


@pytest.mark.parametrize("use", ["edges", "nodes"])
def test_coalition_walks_chunks(chunked, use):
    b, g = chunked
    M = int(b.edge_index.size(1)) if use == "edges" else int(b.batch.numel())
    key = torch.randint(0, 8, (2, M), generator=g, dtype=torch.int32)
    rg = torch.tensor([5, 0, 5, 5, 7, 5, 5])
    rrow = torch.tensor([0, 1, 1, -1, 0, 0, 1])
    rth = torch.tensor([4, 4, 2, 0, 9, 0, 8])              # ..., the control replica, ..., nothing, everything
    for invert in (False, True):
        _same(*_both(coalition_batch, [b], [rg, rth, key], {"rep_row": rrow, "use": use, "invert": invert}))


# ---- 2. tickets with calls in flight on two streams -----------------------------------------------------------------------------
def test_tickets_on_two_streams():
    """8 calls of each builder, alternating between two streams, 300 replicas of 3-6-node rings each: every call takes the next
    ticket slot of its operator while the other stream's call may still be running."""
    g = torch.Generator().manual_seed(4)
    b = Batch.from_data_list([_ring(int(torch.randint(3, 7, (1,), generator=g)), 4, g) for _ in range(500)])
    E, N = int(b.edge_index.size(1)), int(b.batch.numel())
    calls = []
    for i in range(8):
        rg = torch.randint(-50, 500, (300,), generator=g).clamp(min=-1)
        use = ("edges", "nodes")[i % 2]
        calls.append((splice_batches, [b, b], [rg, torch.randint(-1, 500, (300,), generator=g)], {"bridge": "first"}))
        first = (b.edge_ptr if use == "edges" else b.ptr)[rg.clamp(min=0)]
        calls.append((occlude_batch, [b], [rg, first + torch.randint(-1, 3, (300,), generator=g)], {"use": use}))
        key = torch.randint(-1, 7, (3, E if use == "edges" else N), generator=g, dtype=torch.int32)
        calls.append((coalition_batch, [b], [rg, torch.randint(0, 8, (300,), generator=g), key],
                      {"rep_row": torch.randint(-1, 4, (300,), generator=g), "use": use}))
    bd = _dev(b)
    on_dev = [_on(DEV, args, kw) for _, _, args, kw in calls]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    res = []
    for i, ((fn, batches, _, _), (da, dk)) in enumerate(zip(calls, on_dev)):
        with torch.cuda.stream(streams[i % 2]):
            res.append(fn(*[bd for _ in batches], *da, **dk))
    for s in streams:
        torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for r, (fn, batches, args, kw) in zip(res, calls):
        _same(r, fn(*batches, *args, **kw))

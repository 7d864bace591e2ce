"""gc_store_tile (cal_amd/csrc/engine_mma.hpp) under both store policies, through the test hook cal_probe_store_tile
(csrc/store_probe.hip): one 64-lane workgroup stores a 32 x 32 accumulator whose element (row, col) holds the bits
0x40000000 | row << 8 | col into a buffer pre-filled with a sentinel, with a guard band of one row in front and behind.

Every word of the rows < nrow inside the tile must hold its (row, col) bits, every other word of the buffer -- guard bands
included -- must still be the sentinel, and the write-through policy must leave the same bits as the plain one.  The
write-through store goes through a buffer resource whose extent the caller names: what lies past it is dropped."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = np.int32(-0x21524111)                 # 0xDEADBEEF
NROWS = (0, 1, 3, 4, 5, 31, 32)
LDS = (32, 36, 128, 132)
OFFS = (0, 4, 32, 96)                        # column offset of the tile inside a wider row


def _expected(words, tile_off, nrow, ld, keep=lambda row, col: True):
    exp = np.full(words, SENT, dtype=np.int32)
    for row in range(nrow):
        for col in range(32):
            if keep(row, col):
                exp[tile_off + row * ld + col] = 0x40000000 | row << 8 | col
    return exp


def _store(policy, nrow, ld, off, nbytes=None):
    """-> (buffer after the store as int32 on the host, words, tile_off)"""
    from cal_amd import _lib
    from cal_amd.plan import _p, _stream
    words = ld + off + 32 * ld + ld          # guard row, the tile's 32 rows behind its column offset, guard row
    tile_off = ld + off
    if nbytes is None:
        nbytes = ((nrow - 1) * ld + 32) * 4 if nrow > 0 else 0
    buf = torch.full((words,), int(SENT), dtype=torch.int32, device=DEV)
    _lib.call("cal_probe_store_tile", policy, _p(buf), words, tile_off, nrow, ld, nbytes, _stream())
    return buf, words, tile_off


@pytest.mark.parametrize("ld", LDS)
def test_tile_store_writes_its_rows_and_nothing_else_under_both_policies(ld):
    runs = []
    for nrow, off in itertools.product(NROWS, OFFS):
        plain, words, tile_off = _store(0, nrow, ld, off)
        wt, _, _ = _store(1, nrow, ld, off)
        runs.append((nrow, off, words, tile_off, plain, wt))
    torch.cuda.synchronize()
    for nrow, off, words, tile_off, plain, wt in runs:
        exp = _expected(words, tile_off, nrow, ld)
        got_p, got_w = plain.cpu().numpy(), wt.cpu().numpy()
        bad = np.nonzero(got_p != exp)[0]
        assert bad.size == 0, "plain: nrow %d ld %d off %d: first wrong word %d" % (nrow, ld, off, bad[0])
        bad = np.nonzero(got_w != got_p)[0]
        assert bad.size == 0, "write-through != plain: nrow %d ld %d off %d: first word %d" % (nrow, ld, off, bad[0])


@pytest.mark.parametrize("ld,off", [(36, 4), (128, 96)])
def test_write_through_store_drops_what_lies_past_its_extent(ld, off):
    """A full tile whose extent ends behind row 19 (and, second cut, in the middle of row 20, on a 16-byte boundary): the rows
    past the extent are not written, the rows before it are intact, the guard bands untouched."""
    cuts = [(20 * ld * 4, lambda row, col: row < 20),
            ((20 * ld + 16) * 4, lambda row, col: row < 20 or (row == 20 and col < 16)),
            (0, lambda row, col: False)]
    for nbytes, keep in cuts:
        buf, words, tile_off = _store(1, 32, ld, off, nbytes)
        exp = _expected(words, tile_off, 32, ld, keep)
        bad = np.nonzero(buf.cpu().numpy() != exp)[0]
        assert bad.size == 0, "extent %d: first wrong word %d (tile at %d, ld %d)" % (nbytes, bad[0], tile_off, ld)


def test_probe_refuses_a_tile_that_leaves_its_buffer():
    from cal_amd import _lib
    from cal_amd.plan import _p, _stream
    buf = torch.full((64 * 32,), int(SENT), dtype=torch.int32, device=DEV)
    h = _lib.lib()
    for policy in (0, 1):
        assert h.cal_probe_store_tile(policy, _p(buf), 64 * 32, 40 * 32, 32, 32, 0, _stream()) == 2      # rows past the end
        assert h.cal_probe_store_tile(policy, _p(buf), 64 * 32, 2, 1, 32, 0, _stream()) == 2             # not 16-byte aligned
        assert h.cal_probe_store_tile(policy, _p(buf), 64 * 32, 0, 32, 32, 64 * 32 * 4 + 16, _stream()) == 2   # extent past the end
    torch.cuda.synchronize()
    assert bool((buf == int(SENT)).all())

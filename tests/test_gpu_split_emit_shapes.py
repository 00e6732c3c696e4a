"""Shapes that steer the split pipeline's emit and mixed kernels down their other paths.

split_emit_kernel takes 16 codes per thread and a chunk of 4096 points per workgroup,
stages the first kEmitMres = 512 mixed answers of a chunk in LDS (the rest it reads from
global memory) and writes a chunk's pairs through a window of kEmitWin = 2048; a chunk's
mixed points go through pip_mixed_kernel 256 at a time, the tiles past the first through
pip_mixed_more_kernel.  Each test shows on the host, with the pixel index's own lookup
(mgpu_test_raster_host), that its points take the path in question, then compares the
ordered pairs with the oracle exactly, on the NYC res-9 table.
"""
import os
import sys

import numpy as np
import pytest
import torch

import mosaic_amd as M
import oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from geom_util import nyc_points  # noqa: E402
from test_raster_host import raster_lookup  # noqa: E402

pytestmark = pytest.mark.gpu

CHUNK = 4096      # kChunk: points per emit workgroup
ITEMS = 16        # kClsItems: codes per emit thread
STAGED = 512      # kEmitMres: mixed answers of a chunk staged in LDS
TILE = 256        # kGTile: mixed points per mixed tile
WINDOW = 2048     # kEmitWin: pairs staged at a time
MIXED = 2         # mgpu_test_raster_host's kind of a point the pixel index leaves to the mixed tiles


def oracle_join(c, x, y):
    return O.pip_join(c.index_system, 9, x, y, c.cell, c.polygon_id, c.is_core, c.wkb_offsets, c.wkb)


def split_join(xt, yt, d):
    r = M.pip_join(xt, yt, d, 9)
    assert r.stats["pipeline"] == 1  # the split pipeline (classify / mixed / emit)
    return r.numpy()


def per_chunk(v):
    return np.add.reduceat(v.astype(np.int64), np.arange(0, len(v), CHUNK))


def assert_pairs_equal(got, want):
    assert len(got[0]) == len(want[0]), "%d pairs, the oracle has %d" % (len(got[0]), len(want[0]))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("aligned", [True, False])
def test_partial_last_chunk_and_thread(gpu, nyc_chips_r9, aligned):
    """3 chunks and 5 points: the last chunk is partial and its one thread has fewer than
    16 codes.  With x one element into its buffer (8 bytes off a 16-byte boundary) the
    codes come from classify_wave_kernel instead of classify_pair_kernel."""
    n = 3 * CHUNK + 5
    x, y = nyc_points(n, 71)
    assert n % CHUNK and (n % CHUNK) % ITEMS and n % CHUNK < ITEMS
    kind, _, mask, _ = raster_lookup(nyc_chips_r9, 9, x, y)
    assert (kind[3 * CHUNK:] == 1).any(), "the partial thread has a pair to emit"
    assert (kind[:3 * CHUNK] == MIXED).any() and (kind[:3 * CHUNK] == 1).any()
    bx = torch.from_numpy(np.concatenate([[0.0], x])).to(gpu)
    by = torch.from_numpy(np.concatenate([[0.0], y])).to(gpu)
    assert bx.data_ptr() % 16 == 0 and by.data_ptr() % 16 == 0
    if aligned:
        xt, yt = bx[1:].clone(), by[1:].clone()
        assert xt.data_ptr() % 16 == 0 and yt.data_ptr() % 16 == 0
    else:
        xt, yt = bx[1:], by[1:]
        assert xt.data_ptr() % 16 == 8
    assert_pairs_equal(split_join(xt, yt, nyc_chips_r9.upload()), oracle_join(nyc_chips_r9, x, y))


def test_mixed_points_past_the_staged_count(gpu, nyc_zones, nyc_chips_r9):
    """Two chunks of points a few metres from zone boundaries: more mixed points per chunk
    than the emit stages in LDS (the rest it reads from global memory), and more than one
    mixed tile per chunk (pip_mixed_more_kernel)."""
    import bench_workloads as W
    x, y = W.boundary_points(nyc_zones, 2 * CHUNK, 72, 3e-5)
    kind, _, _, _ = raster_lookup(nyc_chips_r9, 9, x, y)
    nm = per_chunk(kind == MIXED)
    assert len(nm) == 2
    assert nm.max() > STAGED, "a chunk with mixed points beyond the staged count (%s)" % nm
    assert nm.max() > TILE, "a chunk with a second mixed tile (%s)" % nm
    got = split_join(torch.from_numpy(x).to(gpu), torch.from_numpy(y).to(gpu), nyc_chips_r9.upload())
    assert_pairs_equal(got, oracle_join(nyc_chips_r9, x, y))


def test_more_pairs_than_one_window(gpu, nyc_chips_r9):
    """Two chunks of points that all lie inside a zone: each chunk has more pairs than one
    kEmitWin window, so the emit's window loop runs more than once per workgroup."""
    x, y = nyc_points(40_000, 73)
    op, _ = oracle_join(nyc_chips_r9, x, y)
    inside = np.zeros(len(x), bool)
    inside[op] = True
    sel = np.nonzero(inside)[0][:2 * CHUNK]
    assert len(sel) == 2 * CHUNK
    x, y = np.ascontiguousarray(x[sel]), np.ascontiguousarray(y[sel])
    kind, _, mask, _ = raster_lookup(nyc_chips_r9, 9, x, y)
    pure_pairs = np.where(kind == 1, np.array([bin(int(m)).count("1") for m in mask]), 0)
    pc = per_chunk(pure_pairs)
    assert len(pc) == 2 and pc.min() > WINDOW, "pairs per chunk from pure pixels alone: %s" % pc
    want = oracle_join(nyc_chips_r9, x, y)
    assert np.bincount(want[0], minlength=len(x)).min() >= 1
    got = split_join(torch.from_numpy(x).to(gpu), torch.from_numpy(y).to(gpu), nyc_chips_r9.upload())
    assert_pairs_equal(got, want)

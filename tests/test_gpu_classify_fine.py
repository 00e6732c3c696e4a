"""The classify kernels' finer byte-coded block table (chip_table.h raster_fine).

When an H3 table with a block table, row bands and a second level is adopted, a kernel
derives one byte per block of 4x4 (or 8x4, 4x8) pixels from the pixel classes: the class all
of the block's pixels share when it is below 255, else 0xFF.  classify_pair_kernel and
classify_wave_kernel hold those bytes in LDS instead of the 8x8 block table; a byte below
0xFF is the point's class, 0xFF sends the lane through the pixel and sub-pixel lookups as
before.  Context option cfy_fine = 0 keeps the 8x8 table on the same handle.

The builder tests recompute the bytes in numpy from the pixel classes the hook copies out
(mgpu_test_fine_table): the NYC res-9 table, a small table whose raster is no multiple of 4
either way (partial edge blocks) and a table of 324 squares with more than 254 classes,
where classes of 255 and above fill whole blocks and must read 0xFF.  The join tests compare
ordered pairs with the oracle exactly, with the option on and off: boundary points over two
chunks and a partial one; points on the pixel-grid lines that bound 4- and 8-pixel blocks
and one ulp to either side, points on the box's maximum edges (the clamped last pixel, the
partial edge block) and outside points among them -- aligned (classify_pair_kernel), 8
bytes off (classify_wave_kernel) and through a validity bitmap; pip_join_count, which
shares the classify launch; and a table without a second level, which gets no derived table.
"""
import os
import sys

import numpy as np
import pytest
import torch

import mosaic_amd as M
import oracle as O
from mosaic_amd import arrow as A

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_raster_host import raster_lookup  # noqa: E402

pytestmark = pytest.mark.gpu

CHUNK = 4096              # kChunk: points per classify wave
N_ODD = 2 * CHUNK + 131   # two chunks and a partial one whose last pair item holds one point
LOOKUP = 0xFF             # kFineLookup
MIXED = 2                 # mgpu_test_raster_host's kind of a point left to the mixed tiles


def oracle_join(c, x, y):
    return O.pip_join(c.index_system, 9, x, y, c.cell, c.polygon_id, c.is_core, c.wkb_offsets, c.wkb)


def derive(classes, sx, sy):
    """The fine table of `classes` [ny, nx] in numpy: blocks clipped at the raster's edges
    (edge padding repeats a block's own pixels, so it changes no block's verdict)."""
    ny, nx = classes.shape
    by, bx = -(-ny // (1 << sy)), -(-nx // (1 << sx))
    pad = np.pad(classes, ((0, (by << sy) - ny), (0, (bx << sx) - nx)), mode="edge")
    blocks = pad.reshape(by, 1 << sy, bx, 1 << sx)
    first = blocks[:, 0, :, 0]
    same = (blocks == first[:, None, :, None]).all(axis=(1, 3))
    return np.where(same & (first < LOOKUP), first, LOOKUP).astype(np.uint8), same, first


def assert_built(ft):
    """The hook's table equals the numpy one; returns (bytes, uniform, first class)."""
    assert ft["fine"] is not None and (ft["sx"], ft["sy"]) in ((2, 2), (3, 2), (2, 3))
    want, same, first = derive(ft["classes"], ft["sx"], ft["sy"])
    assert ft["fine"].shape == want.shape
    assert np.array_equal(ft["fine"], want), "%d blocks differ" % (ft["fine"] != want).sum()
    return want, same, first


def pixel_of(ft, x, y):
    """raster.h raster_index's pixel of points inside the box."""
    ny, nx = ft["classes"].shape
    ix = np.minimum(((x - ft["x0"]) * ft["inv_dx"]).astype(np.uint32), nx - 1)
    iy = np.minimum(((y - ft["y0"]) * ft["inv_dy"]).astype(np.uint32), ny - 1)
    return ix.astype(np.int64), iy.astype(np.int64)


def joins(gpu, d, xt, yt):
    """The split join with the fine table and without it -> the two results."""
    out = []
    for fine in (1, 0):
        with d.ctx.options(cfy_fine=fine):
            r = M.pip_join(xt, yt, d, 9)
        assert r.stats["pipeline"] == 1  # the split pipeline (classify / mixed / emit)
        out.append(r)
    return out


def assert_pairs_equal(got, want):
    assert len(got[0]) == len(want[0]), "%d pairs, expected %d" % (len(got[0]), len(want[0]))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def assert_both_equal_oracle(gpu, d, x, y, want):
    on, off = joins(gpu, d, torch.from_numpy(x).to(gpu), torch.from_numpy(y).to(gpu))
    assert_pairs_equal(on.numpy(), off.numpy())
    assert_pairs_equal(on.numpy(), want)
    assert on.stats["n_candidates"] == off.stats["n_candidates"]  # the same mixed lists


@pytest.fixture(scope="module")
def nyc_dev(gpu, nyc_chips_r9):
    return nyc_chips_r9.upload()


@pytest.fixture(scope="module")
def nyc_fine(nyc_dev):
    return nyc_dev.fine_table()


@pytest.fixture(scope="module")
def boundary(nyc_zones, nyc_chips_r9):
    """N_ODD points a few metres from zone boundaries, and the oracle's pairs."""
    import bench_workloads as W
    x, y = W.boundary_points(nyc_zones, N_ODD, 1101, 3e-5)
    return x, y, oracle_join(nyc_chips_r9, x, y)


def ulps(v):
    """v, the double below it and the double above it."""
    return np.concatenate([v, np.nextafter(v, -np.inf), np.nextafter(v, np.inf)])


def grid_line(o, inv, k):
    """The smallest doubles whose pixel coordinate, computed as raster_index computes it,
    is k (an integer array): o + k / inv, moved the few ulps the rounding asks for."""
    pix = lambda v: np.floor((v - o) * inv)  # noqa: E731
    v = o + k / inv
    for _ in range(64):
        up, down = pix(v) < k, pix(np.nextafter(v, -np.inf)) >= k
        if not (up | down).any():
            return v
        v = np.where(up, np.nextafter(v, np.inf), np.where(down, np.nextafter(v, -np.inf), v))
    raise AssertionError("no pixel boundary within 64 ulps")


@pytest.fixture(scope="module")
def seams(nyc_zones, nyc_chips_r9, nyc_fine, boundary):
    """N_ODD points: on the pixel-grid lines at multiples of 4 and 8 pixels where the fine
    table's neighbouring blocks differ, and one ulp to either side; on the box's maximum
    edges, one ulp inside and one ulp outside them; boundary points; an outside point in
    every 7th place.  -> x, y, the oracle's pairs, and the index ranges of the kinds."""
    ft = nyc_fine
    fine, _, _ = derive(ft["classes"], ft["sx"], ft["sy"])
    ny, nx = ft["classes"].shape
    rng = np.random.default_rng(1102)
    xs, ys = [], []
    # vertical lines between horizontally neighbouring blocks with different bytes
    by, bx = np.nonzero(fine[:, 1:] != fine[:, :-1])
    pick = rng.choice(len(by), 400, replace=False)
    kx = (bx[pick] + 1) << ft["sx"]
    line = ulps(grid_line(ft["x0"], ft["inv_dx"], kx))
    row = ((by[pick] << ft["sy"]) + rng.uniform(0.05, (1 << ft["sy"]) - 0.05, 400)).clip(0, ny - 0.05)
    xs.append(line)
    ys.append(np.tile(ft["y0"] + row / ft["inv_dy"], 3))
    n_v = len(line)
    # horizontal lines between vertically neighbouring blocks with different bytes
    by, bx = np.nonzero(fine[1:, :] != fine[:-1, :])
    pick = rng.choice(len(by), 400, replace=False)
    ky = (by[pick] + 1) << ft["sy"]
    line = ulps(grid_line(ft["y0"], ft["inv_dy"], ky))
    col = ((bx[pick] << ft["sx"]) + rng.uniform(0.05, (1 << ft["sx"]) - 0.05, 400)).clip(0, nx - 0.05)
    xs.append(np.tile(ft["x0"] + col / ft["inv_dx"], 3))
    ys.append(line)
    n_h = len(line)
    # crossings of lines at multiples of 8 pixels (corners of four 8x8 blocks), all nine ulp combinations
    cx = grid_line(ft["x0"], ft["inv_dx"], 8 * rng.integers(1, nx // 8, 60))
    cy = grid_line(ft["y0"], ft["inv_dy"], 8 * rng.integers(1, ny // 8, 60))
    for dx in (-np.inf, None, np.inf):
        for dy in (-np.inf, None, np.inf):
            xs.append(cx if dx is None else np.nextafter(cx, dx))
            ys.append(cy if dy is None else np.nextafter(cy, dy))
    n_c = 9 * 60
    # the box's maximum edges: on them, one ulp inside, one ulp outside; the corner
    x_lo, y_lo, x_hi, y_hi = ft["bbox"]
    ex, ey = rng.uniform(x_lo, x_hi, 100), rng.uniform(y_lo, y_hi, 100)
    xs += [ulps(np.full(100, x_hi)), np.tile(ex, 3), ulps(np.array([x_hi]))]
    ys += [np.tile(ey, 3), ulps(np.full(100, y_hi)), ulps(np.array([y_hi]))]
    n_e = 603
    sx_, sy_ = np.concatenate(xs), np.concatenate(ys)
    bxp, byp, _ = boundary
    fill = N_ODD - len(sx_)
    assert fill > 0
    x, y = np.concatenate([sx_, bxp[:fill]]), np.concatenate([sy_, byp[:fill]])
    # shuffle, so that a wave's lanes hold every kind, then an outside point in every 7th place
    order = rng.permutation(N_ODD)
    x, y, kind_of = x[order], y[order], order
    k = np.arange(3, N_ODD, 7)
    x[k], y[k] = rng.uniform(-76.5, -75.5, len(k)), rng.uniform(38.5, 39.5, len(k))
    kind_of = np.where(np.isin(np.arange(N_ODD), k), -1, kind_of)
    ranges = {"v": (0, n_v), "h": (n_v, n_v + n_h), "c": (n_v + n_h, n_v + n_h + n_c),
              "e": (n_v + n_h + n_c, n_v + n_h + n_c + n_e)}
    return x, y, oracle_join(nyc_chips_r9, x, y), kind_of, ranges


def test_builder_nyc(nyc_fine):
    want, same, first = assert_built(nyc_fine)
    # a table worth staging: most blocks answer, some do not
    assert 0.3 < (want != LOOKUP).mean() < 0.99
    assert (nyc_fine["sx"], nyc_fine["sy"]) != (3, 3)


def small_zones(nyc_zones):
    return nyc_zones.select(range(60, 66))


def test_builder_partial_edge_blocks(gpu, nyc_zones):
    """Six zones: the raster's width and height are no multiples of 4, so the last block
    column and row are clipped."""
    chips = M.tessellate(small_zones(nyc_zones), M.H3IndexSystem(), 9)
    d = chips.upload()
    ft = d.fine_table()
    ny, nx = ft["classes"].shape
    assert nx % 4 and ny % 4, (nx, ny)
    want, _, _ = assert_built(ft)
    assert want.shape == (-(-ny // (1 << ft["sy"])), -(-nx // (1 << ft["sx"])))
    # the join over it, points on its maximum edges included
    x_lo, y_lo, x_hi, y_hi = ft["bbox"]
    rng = np.random.default_rng(1103)
    x, y = rng.uniform(x_lo, x_hi, CHUNK + 77), rng.uniform(y_lo, y_hi, CHUNK + 77)
    x[:50], y[50:100] = x_hi, y_hi
    assert_both_equal_oracle(gpu, d, x, y, oracle_join(chips, x, y))
    d.close()


@pytest.fixture(scope="module")
def squares():
    """18 x 18 squares of 0.012 degrees (about seven res-9 cell edges), 0.003 apart: more
    than 254 one-match classes, and blocks of 4x4 pixels well inside every square."""
    polys = []
    for j in range(18):
        for i in range(18):
            x0, y0 = -74.2 + 0.015 * i, 40.5 + 0.015 * j
            polys.append((1000 + 18 * j + i, [[[(x0, y0), (x0 + 0.012, y0), (x0 + 0.012, y0 + 0.012), (x0, y0 + 0.012),
                                               (x0, y0)]]]))
    P = M.Polygons.from_lists(polys)
    return P, M.tessellate(P, M.H3IndexSystem(), 9)


def test_more_than_254_classes(gpu, squares):
    """Blocks filled by a class of 255 or above hold 0xFF (one byte cannot name them); their
    points take the pixel lookup and the join still equals the oracle."""
    P, chips = squares
    d = chips.upload()
    ft = d.fine_table()
    want, same, first = assert_built(ft)
    high = same & (first >= LOOKUP) & (first < 0x8000)
    low = same & (first > 0) & (first < LOOKUP)
    assert d.info()["raster_ncls"] > 255 and high.sum() > 50 and low.sum() > 50
    assert (ft["fine"][high] == LOOKUP).all() and (ft["fine"][low] == first[low]).all()
    # points in the middle of such blocks, of both kinds, then uniform points
    rng = np.random.default_rng(1104)
    hy, hx = np.nonzero(high)
    ly, lx = np.nonzero(low)
    by = np.concatenate([hy[:1000], ly[:1000]])
    bx = np.concatenate([hx[:1000], lx[:1000]])
    px = ((bx << ft["sx"]) + rng.uniform(0.1, 0.9, len(bx)) * (1 << ft["sx"])) / ft["inv_dx"] + ft["x0"]
    py = ((by << ft["sy"]) + rng.uniform(0.1, 0.9, len(by)) * (1 << ft["sy"])) / ft["inv_dy"] + ft["y0"]
    x_lo, y_lo, x_hi, y_hi = ft["bbox"]
    n = N_ODD - len(px)
    x = np.concatenate([px, rng.uniform(x_lo, x_hi, n)]).clip(x_lo, x_hi)
    y = np.concatenate([py, rng.uniform(y_lo, y_hi, n)]).clip(y_lo, y_hi)
    order = rng.permutation(N_ODD)
    x, y = x[order], y[order]
    op, oq = oracle_join(chips, x, y)
    assert len(op) > N_ODD // 3
    assert_both_equal_oracle(gpu, d, x, y, (op, oq))
    d.close()


def test_boundary_points(gpu, nyc_chips_r9, nyc_dev, nyc_fine, boundary):
    """Two chunks and a partial one of points a few metres from zone boundaries."""
    x, y, want = boundary
    kind, _, _, _ = raster_lookup(nyc_chips_r9, 9, x, y)
    assert (kind == 1).sum() > CHUNK // 2 and (kind == MIXED).sum() > CHUNK // 2
    # both kinds of block under them: bytes that answer and bytes that send the lane on
    ix, iy = pixel_of(nyc_fine, x, y)
    b = nyc_fine["fine"][iy >> nyc_fine["sy"], ix >> nyc_fine["sx"]]
    assert (b == LOOKUP).sum() > CHUNK and (b != LOOKUP).sum() > 100
    assert_both_equal_oracle(gpu, nyc_dev, x, y, want)


def test_seams_edges_and_outside_points(gpu, nyc_dev, nyc_fine, seams):
    x, y, want, kind_of, ranges = seams
    ft = nyc_fine
    ny, nx = ft["classes"].shape
    inside = kind_of >= 0
    ix, iy = pixel_of(ft, np.where(inside, x, ft["x0"]), np.where(inside, y, ft["y0"]))

    def of(name, part):
        """The surviving points of part 0 (on the line), 1 (below), 2 (above) of a kind."""
        lo, hi = ranges[name]
        m = (hi - lo) // 3
        return np.nonzero((kind_of >= lo + part * m) & (kind_of < lo + (part + 1) * m))[0]
    # on a vertical line and above it: the first pixel column of a block; below: the last of the one before
    step = 1 << ft["sx"]
    assert len(of("v", 0)) > 200 and (ix[of("v", 0)] % step == 0).all() and (ix[of("v", 2)] % step == 0).all()
    assert (ix[of("v", 1)] % step == step - 1).all()
    step = 1 << ft["sy"]
    assert len(of("h", 0)) > 200 and (iy[of("h", 0)] % step == 0).all() and (iy[of("h", 2)] % step == 0).all()
    assert (iy[of("h", 1)] % step == step - 1).all()
    lo, hi = ranges["c"]
    c = np.nonzero((kind_of >= lo) & (kind_of < hi))[0]
    assert set(np.unique(ix[c] % 8)) == {0, 7} and set(np.unique(iy[c] % 8)) == {0, 7}
    # the maximum edges: the clamped last pixel column and row, and points one ulp outside
    lo, hi = ranges["e"]
    e = np.nonzero((kind_of >= lo) & (kind_of < hi))[0]
    assert (ix[e] == nx - 1).sum() > 100 and (iy[e] == ny - 1).sum() > 100
    assert (x[e] > ft["bbox"][2]).sum() > 20 and (y[e] > ft["bbox"][3]).sum() > 20
    assert (~inside).sum() > N_ODD // 8
    assert len(want[0]) > N_ODD // 4
    assert_both_equal_oracle(gpu, nyc_dev, x, y, want)


def test_unaligned_arrays_take_the_wave_kernel(gpu, nyc_dev, seams):
    """The same points one element into their buffers: 8 bytes off 16-byte alignment."""
    x, y, want = seams[:3]
    bx = torch.from_numpy(np.concatenate([[0.0], x])).to(gpu)
    by = torch.from_numpy(np.concatenate([[0.0], y])).to(gpu)
    xt, yt = bx[1:], by[1:]
    assert xt.data_ptr() % 16 == 8 and yt.data_ptr() % 16 == 8
    on, off = joins(gpu, nyc_dev, xt, yt)
    assert_pairs_equal(on.numpy(), want)
    assert_pairs_equal(off.numpy(), want)


@pytest.mark.parametrize("offset", [0, 1])
def test_validity_bitmap(gpu, nyc_dev, seams, offset):
    """The same points through a validity bitmap (offset 0: classify_pair_kernel; 1: the
    columns start one row in, classify_wave_kernel).  A null row gives no pair; a pair's
    point id is its row in the whole column."""
    x, y, want = seams[:3]
    n = N_ODD - offset
    present = np.random.default_rng(1105).random(N_ODD) >= 0.3
    xt, yt = torch.from_numpy(x).to(gpu), torch.from_numpy(y).to(gpu)
    xc = A.float64_column(xt, present, offset=offset, length=n)
    yc = A.float64_column(yt, present, offset=offset, length=n)
    keep = present[want[0]] & (want[0] >= offset)
    wp, wq = want[0][keep], want[1][keep]
    assert 0 < len(wp) < len(want[0])
    for fine in (1, 0):
        with nyc_dev.ctx.options(cfy_fine=fine):
            r = A.pip_join_arrow(xc, yc, nyc_dev, 9)
        assert r.stats["pipeline"] == 1
        assert_pairs_equal(r.numpy(), (wp, wq))


def test_count_shares_the_classify_launch(gpu, nyc_dev, boundary):
    x, y, (op, oq) = boundary
    ids = nyc_dev.polygons()
    want = np.bincount(np.searchsorted(ids, oq), minlength=len(ids))
    xt, yt = torch.from_numpy(x).to(gpu), torch.from_numpy(y).to(gpu)
    for fine in (1, 0):
        with nyc_dev.ctx.options(cfy_fine=fine):
            r = M.pip_join_count(xt, yt, nyc_dev, 9)
        assert np.array_equal(r.polygon_id.cpu().numpy(), ids)
        assert np.array_equal(r.count.cpu().numpy(), want)


def test_table_without_second_level_gets_no_fine_table(gpu, nyc_chips_r9, boundary):
    """raster_sub = 0: no sub-pixel level and no row bands -- nothing is derived, and the
    join runs the kernels' if-ladder form as before."""
    x, y, want = boundary
    ctx = M.GpuContext(gpu)
    ctx.set_option("raster_sub", 0)
    d = nyc_chips_r9.upload(ctx)
    ft = d.fine_table()
    assert ft["fine"] is None and ft["classes"] is not None and (ft["sx"], ft["sy"]) == (0, 0)
    assert_both_equal_oracle(gpu, d, x, y, want)
    d.close()
    ctx.close()

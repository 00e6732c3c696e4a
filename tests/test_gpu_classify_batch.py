"""The classify kernels' staged batch lookup (kernels.hip raster_class_batch).

classify_pair_kernel and classify_wave_kernel look up the pixel classes of a batch of four
points per lane stage by stage: the block classes from LDS, then every pixel class, then
every sub-pixel class, a lane that needs no load reading index 0 of the table.  The shapes
below put idle and gathering lanes into the same instruction in every combination: a
chunk of one repeated point in a uniform block (no lane gathers), a chunk of points a few
metres from zone boundaries (nearly every lane gathers pixel and sub-pixel classes or is
mixed), the two interleaved point by point (a lane's pair holds one of each) and by blocks
of 128 (whole pair items alternate), each with points outside the table's box mixed in;
a size whose last chunk is partial and whose last pair item holds one point, 16-byte
aligned (classify_pair_kernel) and 8 bytes off (classify_wave_kernel); the same through a
validity bitmap with nulls on boundary points in each of a lane's four batch positions;
and a table uploaded without a second level, which takes the kernels' if-ladder path.
Each test shows on the host, with the pixel index's own lookup (mgpu_test_raster_host),
what its points are, then compares the ordered pairs with the oracle exactly, on the NYC
res-9 table.
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
import nulls_util as U  # noqa: E402
from geom_util import nyc_points  # noqa: E402
from test_raster_host import raster_lookup  # noqa: E402

pytestmark = pytest.mark.gpu

CHUNK = 4096   # kChunk: points per classify wave
ITEM = 128     # points of one pair item of a wave (two per lane)
MIXED = 2      # mgpu_test_raster_host's kind of a point left to the mixed tiles
N_ODD = 2 * CHUNK + 131  # the last chunk partial, the last pair item with one point
FAR = 0.01     # degrees (about 1 km) to the nearest zone vertex: "far from any boundary"


def oracle_join(c, x, y):
    return O.pip_join(c.index_system, 9, x, y, c.cell, c.polygon_id, c.is_core, c.wkb_offsets, c.wkb)


def split_join(xt, yt, d):
    r = M.pip_join(xt, yt, d, 9)
    assert r.stats["pipeline"] == 1  # the split pipeline (classify / mixed / emit)
    return r


def assert_pairs_equal(got, want):
    assert len(got[0]) == len(want[0]), "%d pairs, the oracle has %d" % (len(got[0]), len(want[0]))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def gpu_join_equals_oracle(gpu, chips, d, x, y):
    got = split_join(torch.from_numpy(x).to(gpu), torch.from_numpy(y).to(gpu), d).numpy()
    assert_pairs_equal(got, oracle_join(chips, x, y))


@pytest.fixture(scope="module")
def nyc_dev(gpu, nyc_chips_r9):
    return nyc_chips_r9.upload()


OUTSIDE = 3 * CHUNK  # points kept outside the table's box


def lookup_kinds(chips, *xy):
    """The host kinds of several point sets in one call (mgpu_test_raster_host builds the
    table each time it is called: about a second)."""
    kind, _, mask, _ = raster_lookup(chips, 9, np.concatenate([x for x, _ in xy]), np.concatenate([y for _, y in xy]))
    cut = np.cumsum([len(x) for x, _ in xy])[:-1]
    return np.split(kind, cut), np.split(mask, cut)


@pytest.fixture(scope="module")
def sets(nyc_zones, nyc_chips_r9):
    """The kinds of points, computed once: `far` = one empty and one pure point whose whole
    neighbourhood has their answer, `bx, by, bk` = three chunks of boundary points with
    their host kinds, `out` = points west and south of the zones, outside the table's box
    (kNoPixel in the kernels; the host lookup calls them empty)."""
    import bench_workloads as W
    c = nyc_chips_r9
    x, y = nyc_points(100, 501)
    bx, by = W.boundary_points(nyc_zones, 3 * CHUNK, 502, 3e-5)
    rng = np.random.default_rng(503)
    out = rng.uniform(-76.5, -75.5, OUTSIDE), rng.uniform(38.5, 39.5, OUTSIDE)
    (kind, bk, ok), _ = lookup_kinds(c, (x, y), (bx, by), out)
    assert (ok == 0).all()
    assert (bk == 1).sum() > CHUNK // 4 and (bk == MIXED).sum() > CHUNK // 4, np.bincount(bk, minlength=3)
    v = np.asarray(nyc_zones.xy, np.float64).reshape(-1, 2)
    dist = np.array([np.sqrt(((v - (px, py)) ** 2).sum(1).min()) for px, py in zip(x, y)])
    far, rings = {}, []
    a = np.linspace(0, 2 * np.pi, 64, endpoint=False)
    for k in (0, 1):
        i = np.nonzero(kind == k)[0]
        i = i[np.argmax(dist[i])]
        assert dist[i] > (FAR if k == 0 else FAR / 4), (k, dist[i])
        far[k] = (x[i], y[i])
        rings += [(x[i] + r * np.cos(a), y[i] + r * np.sin(a)) for r in (dist[i] / 8, dist[i] / 2)]
    # their neighbourhoods answer alike: no boundary within half the distance
    rk, rm = lookup_kinds(c, *rings)
    assert all((q == 0).all() for q in rk[:2]) and all((q == 1).all() for q in rk[2:]) and all((m != 0).all() for m in rm[2:])
    return far, bx, by, bk, out


def repeated(pt, n):
    return np.full(n, pt[0]), np.full(n, pt[1])


def with_outside(sets, x, y, every):
    """x, y with every `every`-th point (from the third on) replaced by an outside point."""
    x, y = x.copy(), y.copy()
    k = np.arange(2, len(x), every)
    x[k], y[k] = sets[4][0][:len(k)], sets[4][1][:len(k)]
    return x, y


_INTERLEAVED = {}


def interleaved(sets, chips, n):
    """n points: boundary points and the repeated pure point alternating point by point in
    the first chunk (the boundary point first in one batch of two items, second in the
    next), by blocks of 128 afterwards, an outside point every 11th place.  Computed once
    per size."""
    if n not in _INTERLEAVED:
        far, bx, by = sets[:3]
        assert n <= len(bx)
        ux, uy = repeated(far[1], n)
        i = np.arange(n)
        take_b = np.where(i < CHUNK, (i & 1) == ((i // (2 * ITEM)) & 1), ((i // ITEM) & 1) == 0)
        x, y = np.where(take_b, bx[:n], ux), np.where(take_b, by[:n], uy)
        x, y = with_outside(sets, x, y, 11)
        kind, _, _, _ = raster_lookup(chips, 9, x, y)
        _INTERLEAVED[n] = (x, y, kind, take_b)
    return _INTERLEAVED[n]


def test_uniform_block_points(gpu, nyc_chips_r9, nyc_dev, sets):
    """A chunk of one repeated empty point and a chunk of one repeated pure point, both far
    from any boundary (no lane gathers: every lane reads index 0), then the pure point with
    outside points among it."""
    far = sets[0]
    ex, ey = repeated(far[0], CHUNK)
    px, py = repeated(far[1], CHUNK)
    ox, oy = with_outside(sets, px, py, 5)
    x, y = np.concatenate([ex, px, ox]), np.concatenate([ey, py, oy])
    kind, _, _, _ = raster_lookup(nyc_chips_r9, 9, x, y)
    assert (kind[:CHUNK] == 0).all() and (kind[CHUNK:2 * CHUNK] == 1).all()
    assert set(np.unique(kind[2 * CHUNK:])) == {0, 1}
    gpu_join_equals_oracle(gpu, nyc_chips_r9, nyc_dev, x, y)


def test_boundary_points(gpu, nyc_chips_r9, nyc_dev, sets):
    """A chunk of points a few metres from zone boundaries (nearly every lane refined or
    mixed), then one with outside points among them."""
    _, bx, by, bk, _ = sets
    assert (bk[:CHUNK] == 1).any() and (bk[:CHUNK] == MIXED).any()
    assert ((bk[:CHUNK] == 1) | (bk[:CHUNK] == MIXED)).mean() > 0.7
    ox, oy = with_outside(sets, bx[CHUNK:2 * CHUNK], by[CHUNK:2 * CHUNK], 3)
    x, y = np.concatenate([bx[:CHUNK], ox]), np.concatenate([by[:CHUNK], oy])
    gpu_join_equals_oracle(gpu, nyc_chips_r9, nyc_dev, x, y)


def assert_interleaved(kind, take_b):
    """Both kinds in the lanes' pairs of the first chunk and in whole items after it."""
    b, u = kind[take_b], kind[~take_b]
    assert (b == 1).any() and (b == MIXED).any() and (u == 1).mean() > 0.8
    first = take_b[:CHUNK].reshape(-1, 2)
    assert (first[:, 0] ^ first[:, 1]).all()  # one of each in every lane's pair
    items = take_b[CHUNK:2 * CHUNK].reshape(-1, ITEM)
    assert (items.all(1) | (~items).all(1)).all() and items.all(1).any() and (~items).all(1).any()


def test_mixed_within_one_instruction(gpu, nyc_chips_r9, nyc_dev, sets):
    """Idle and gathering lanes in one instruction: boundary and uniform points alternate
    point by point in the first chunk, item by item in the second."""
    x, y, kind, take_b = interleaved(sets, nyc_chips_r9, 2 * CHUNK)
    assert_interleaved(kind, take_b)
    gpu_join_equals_oracle(gpu, nyc_chips_r9, nyc_dev, x, y)


@pytest.mark.parametrize("aligned", [True, False])
def test_partial_chunk_and_alignment(gpu, nyc_chips_r9, nyc_dev, sets, aligned):
    """2 chunks and 131 points of the interleaved set: the last chunk is partial and the
    last pair item holds one point.  16-byte aligned it goes through classify_pair_kernel,
    one element into its buffer (8 bytes off) through classify_wave_kernel."""
    x, y, kind, take_b = interleaved(sets, nyc_chips_r9, N_ODD)
    assert_interleaved(kind, take_b)
    assert N_ODD % CHUNK and N_ODD % 2 == 1
    bx = torch.from_numpy(np.concatenate([[0.0], x])).to(gpu)
    by = torch.from_numpy(np.concatenate([[0.0], y])).to(gpu)
    assert bx.data_ptr() % 16 == 0 and by.data_ptr() % 16 == 0
    if aligned:
        xt, yt = bx[1:].clone(), by[1:].clone()
        assert xt.data_ptr() % 16 == 0 and yt.data_ptr() % 16 == 0
    else:
        xt, yt = bx[1:], by[1:]
        assert xt.data_ptr() % 16 == 8 and yt.data_ptr() % 16 == 8
    assert_pairs_equal(split_join(xt, yt, nyc_dev).numpy(), oracle_join(nyc_chips_r9, x, y))


@pytest.mark.parametrize("offs", [(2, 2), (3, 3)])
def test_validity_bitmap(gpu, nyc_chips_r9, nyc_dev, sets, offs):
    """The same points through mgpu_pip_join_arrow with a validity bitmap at a non-zero
    offset (even: classify_pair_kernel, odd: classify_wave_kernel), nulls on boundary
    points in each of a lane's four batch positions of either kernel.  Null rows give no
    pair and take no mixed slot: the candidates counted are those of the join without a
    bitmap that has an outside point in every null row's place."""
    far = sets[0]
    x, y, kind, take_b = interleaved(sets, nyc_chips_r9, N_ODD)
    i = np.arange(N_ODD)
    null = take_b & (i % 3 == 0) & ((kind == 1) | (kind == MIXED))
    # a lane's batch positions: the pair kernel's (item parity, point of the pair), the
    # wave kernel's four items of 64
    pos_pair = ((i // ITEM) & 1) * 2 + (i & 1)
    pos_wave = (i // 64) & 3
    for pos in (pos_pair, pos_wave):
        for k in range(4):
            for kd in (1, MIXED):
                assert (null & (pos == k) & (kind == kd)).any(), (k, kd)
    # (every null row keeps its coordinates: a kernel that looked at one would add its pair
    # or its mixed slot)
    rows = U.null_rows(x, y, ~null, None, keep_rows=np.nonzero(null)[0])
    assert np.array_equal(rows.kept, np.nonzero(null)[0]) and len(rows.sel) == N_ODD - null.sum()
    op, oq = oracle_join(nyc_chips_r9, x[rows.sel], y[rows.sel])
    assert len(oracle_join(nyc_chips_r9, x[rows.kept], y[rows.kept])[0]) > 0
    fx, fy = repeated(far[1], U.HEAD + U.TAIL)
    case = U.embed(rows, offs[0], offs[1], fx, fy)
    xc, yc = U.columns(case, gpu)
    assert U.classify_kernel(xc, yc) == ("pair" if offs[0] % 2 == 0 else "wave")
    r = A.pip_join_arrow(xc, yc, nyc_dev, 9)
    assert r.stats["pipeline"] == 1
    gp, gq = r.numpy()
    assert len(gp) == len(op), (len(gp), len(op))
    assert np.array_equal(gp, rows.sel[op] + offs[0]) and np.array_equal(gq, oq)
    # (the same rows with an outside point in every null row's place: the valid points keep
    # their chunks and mixed tiles, so the candidates are counted tile for tile alike)
    ox, oy = x.copy(), y.copy()
    ox[null], oy[null] = sets[4][0][:null.sum()], sets[4][1][:null.sum()]
    no_nulls = split_join(torch.from_numpy(ox).to(gpu), torch.from_numpy(oy).to(gpu), nyc_dev)
    assert len(no_nulls.numpy()[0]) == len(op) and no_nulls.stats["n_candidates"] > 0
    assert r.stats["n_candidates"] == no_nulls.stats["n_candidates"]


def test_table_without_second_level(gpu, nyc_chips_r9, sets):
    """The table uploaded with raster_sub = 0 has no sub-pixel level and no row bands: the
    kernels keep raster_class_blk's if ladder for it."""
    x, y, kind, take_b = interleaved(sets, nyc_chips_r9, N_ODD)
    ctx = M.GpuContext(gpu)
    ctx.set_option("raster_sub", 0)
    d = nyc_chips_r9.upload(ctx)
    gpu_join_equals_oracle(gpu, nyc_chips_r9, d, x, y)
    ctx.close()

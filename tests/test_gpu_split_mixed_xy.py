"""The split pipeline's mixed lists around the mixed tile's edge, its one clear and one
read-back per join, and the padded chunk scan.

A chunk's listed (mixed) points go through pip_mixed_kernel kGTile = 256 at a time, the
list positions past the first tile through pip_mixed_more_kernel; the classify kernels
rank them (two points per lane in classify_pair_kernel, one in classify_wave_kernel) and
zero the chunk's candidate count.  Each input is built on the host from points the pixel
index's own lookup (mgpu_test_raster_host) calls mixed and points it does not, laid out so
that the chunks have the mixed counts and positions in question -- asserted before the
join -- and the ordered pairs are compared with the oracle exactly, on the NYC res-9 table.
"""
import os
import sys

import numpy as np
import pytest
import torch

import mosaic_amd as M
import oracle as O
from mosaic_amd import _native as N
from mosaic_amd import arrow as A

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from geom_util import nyc_points  # noqa: E402
from test_raster_host import raster_lookup  # noqa: E402

pytestmark = pytest.mark.gpu

CHUNK = 4096      # kChunk: points per classify wave / emit workgroup
TILE = 256        # kGTile: mixed points per mixed tile
SCAN_BLOCK = 1024  # kScanBlock: threads of tile_scan_kernel
SCAN_LDS = 24576  # kScanLds: chunk counts tile_scan_kernel stages in LDS
MIXED = 2         # mgpu_test_raster_host's kind of a point left to the mixed tiles


def oracle_join(c, x, y):
    return O.pip_join(c.index_system, 9, x, y, c.cell, c.polygon_id, c.is_core, c.wkb_offsets, c.wkb)


def assert_pairs_equal(got, want):
    assert len(got[0]) == len(want[0]), "%d pairs, the oracle has %d" % (len(got[0]), len(want[0]))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def per_chunk(v):
    return np.add.reduceat(v.astype(np.int64), np.arange(0, len(v), CHUNK))


@pytest.fixture(scope="module")
def pools(nyc_zones, nyc_chips_r9):
    """(mixed x, y), (other x, y): points the pixel index leaves to the mixed tiles (a few
    metres from zone boundaries) and points it answers itself."""
    import bench_workloads as W
    bx, by = W.boundary_points(nyc_zones, 24_000, 81, 3e-5)
    kb = raster_lookup(nyc_chips_r9, 9, bx, by)[0]
    ux, uy = nyc_points(40_000, 82)
    ku = raster_lookup(nyc_chips_r9, 9, ux, uy)[0]
    mixed = (bx[kb == MIXED], by[kb == MIXED], kb[kb == MIXED])
    other = (ux[ku != MIXED], uy[ku != MIXED], ku[ku != MIXED])
    assert len(mixed[0]) >= 2 * CHUNK + 1000 and len(other[0]) >= 6 * CHUNK, (len(mixed[0]), len(other[0]))
    assert (other[2] == 1).sum() > 1000, "pure pixels with pairs among the others"
    return mixed, other


@pytest.fixture(scope="module")
def nyc_dev(gpu, nyc_chips_r9):
    return nyc_chips_r9.upload()


def lay_out(pools, is_mixed):
    """Points with a mixed one exactly where is_mixed says, the rest answered by the pixel
    index -> x, y and each point's kind as the host lookup gave it (pools)."""
    (mx, my, mk), (ox, oy, ok) = pools
    nm, no = int(is_mixed.sum()), int((~is_mixed).sum())
    assert nm <= len(mx) and no <= len(ox)
    x = np.empty(len(is_mixed))
    y = np.empty(len(is_mixed))
    kind = np.empty(len(is_mixed), np.int8)
    x[is_mixed], y[is_mixed], kind[is_mixed] = mx[:nm], my[:nm], mk[:nm]
    x[~is_mixed], y[~is_mixed], kind[~is_mixed] = ox[:no], oy[:no], ok[:no]
    return x, y, kind


def on_device(x, y, gpu, aligned=True):
    """x, y on the GPU 16-byte aligned (classify_pair_kernel) or 8 bytes off that
    (classify_wave_kernel)."""
    bx = torch.from_numpy(np.concatenate([[0.0], x])).to(gpu)
    by = torch.from_numpy(np.concatenate([[0.0], y])).to(gpu)
    assert bx.data_ptr() % 16 == 0 and by.data_ptr() % 16 == 0
    if aligned:
        xt, yt = bx[1:].clone(), by[1:].clone()
        assert xt.data_ptr() % 16 == 0 and yt.data_ptr() % 16 == 0
    else:
        xt, yt = bx[1:], by[1:]
        assert xt.data_ptr() % 16 == 8 and yt.data_ptr() % 16 == 8
    return xt, yt


def split_join(xt, yt, d, **kw):
    r = M.pip_join(xt, yt, d, 9, **kw)
    assert r.stats["pipeline"] == N.MGPU_PIPELINE_SPLIT
    return r


EDGE_COUNTS = (0, 1, 255, 256, 257, CHUNK)


@pytest.fixture(scope="module")
def tile_edge_case(pools, nyc_chips_r9):
    """One chunk per mixed count around the tile edge.  The listed points include a chunk's
    first and last point, both points of a lane's pair item (2 lane, 2 lane + 1), and pair
    items with only the first or only the second point listed."""
    rng = np.random.default_rng(83)
    is_mixed = np.zeros(len(EDGE_COUNTS) * CHUNK, bool)
    for c, m in enumerate(EDGE_COUNTS):
        fixed = [CHUNK - 1, 0, 1, 2, 5, 128 + 2 * 63, 128 + 2 * 63 + 1][:m]
        rest = np.setdiff1d(np.arange(CHUNK), fixed)
        pos = np.concatenate([fixed, rng.choice(rest, m - len(fixed), replace=False)]).astype(np.int64)
        is_mixed[c * CHUNK + pos] = True
    x, y, kind = lay_out(pools, is_mixed)
    listed = kind == MIXED
    assert tuple(per_chunk(listed)) == EDGE_COUNTS
    ev, od = listed[0::2], listed[1::2]
    assert (ev & od).any() and (ev & ~od).any() and (~ev & od).any()
    for c in (2, 3, 4):
        assert listed[c * CHUNK] and listed[c * CHUNK + CHUNK - 1]
    return x, y, oracle_join(nyc_chips_r9, x, y)


@pytest.mark.parametrize("aligned", [True, False])
def test_mixed_counts_around_the_tile_edge(gpu, nyc_dev, tile_edge_case, aligned):
    """Chunks with 0, 1, 255, 256, 257 and 4096 mixed points: a first mixed tile one short
    of full, full, and overfull (list positions 256 on go through pip_mixed_more_kernel),
    through both classify kernels."""
    x, y, want = tile_edge_case
    xt, yt = on_device(x, y, gpu, aligned)
    assert_pairs_equal(split_join(xt, yt, nyc_dev).numpy(), want)


@pytest.mark.parametrize("n", [3 * CHUNK + 1, 2 * CHUNK + 77])
def test_short_tails(gpu, nyc_chips_r9, nyc_dev, pools, n):
    """An odd n whose last point is mixed: it is alone in its pair item, the branch of
    classify_pair_kernel that loads one point (p + 1 < n fails)."""
    assert n % 2 == 1
    rng = np.random.default_rng(84)
    is_mixed = rng.random(n) < 0.05
    is_mixed[n - 1] = True
    x, y, kind = lay_out(pools, is_mixed)
    assert kind[n - 1] == MIXED and (kind[:n - 1] == MIXED).sum() > 100
    xt, yt = on_device(x, y, gpu, aligned=True)
    assert_pairs_equal(split_join(xt, yt, nyc_dev).numpy(), oracle_join(nyc_chips_r9, x, y))


@pytest.mark.parametrize("aligned", [True, False])
def test_null_mixed_points_take_no_slot(gpu, nyc_chips_r9, nyc_dev, pools, aligned):
    """Would-be mixed points nulled by the validity bitmap, coordinates kept: chunk 0 has 300
    of them of which 60 are null, so its 240 listed points fit the first mixed tile only if
    the nulls take no slot and the ranks behind them close up; chunk 1 has 257 listed."""
    rng = np.random.default_rng(85)
    is_mixed = np.zeros(2 * CHUNK, bool)
    is_mixed[rng.choice(CHUNK, 300, replace=False)] = True
    is_mixed[CHUNK + rng.choice(CHUNK, 290, replace=False)] = True
    x, y, kind = lay_out(pools, is_mixed)
    assert np.array_equal(kind == MIXED, is_mixed)
    present = np.ones(2 * CHUNK, bool)
    m0, m1 = np.nonzero(is_mixed[:CHUNK])[0], CHUNK + np.nonzero(is_mixed[CHUNK:])[0]
    present[m0[::5]] = False       # 60 of chunk 0's 300, from its first listed point on
    present[m1[::8][:33]] = False     # 33 of chunk 1's 290
    other = np.nonzero(~is_mixed)[0]
    present[other[::7]] = False
    assert tuple(per_chunk(is_mixed & present)) == (240, 257)
    nulled = np.nonzero(is_mixed & ~present)[0]
    assert len(oracle_join(nyc_chips_r9, x[nulled], y[nulled])[0]) > 0, "the nulled mixed points would have pairs"
    sel = np.nonzero(present)[0]
    op, oq = oracle_join(nyc_chips_r9, x[sel], y[sel])
    off = 0 if aligned else 1
    xt = torch.from_numpy(np.concatenate([np.zeros(off), x])).to(gpu)
    yt = torch.from_numpy(np.concatenate([np.zeros(off), y])).to(gpu)
    pres = np.concatenate([np.ones(off, bool), present])
    xc = A.float64_column(xt, pres, offset=off, length=len(x))
    yc = A.float64_column(yt, None, offset=off, length=len(x))
    assert (xt.data_ptr() + 8 * off) % 16 == (0 if aligned else 8)
    r = A.pip_join_arrow(xc, yc, nyc_dev, 9)
    assert r.stats["pipeline"] == N.MGPU_PIPELINE_SPLIT
    gp, gq = r.numpy()
    assert len(gp) == len(op)
    assert np.array_equal(gp, sel[op] + off) and np.array_equal(gq, oq)


STAT_KEYS = ("n_points", "n_pairs", "n_candidates", "n_near_ties")


def test_back_to_back_joins_on_one_context(gpu, nyc_chips_r9, nyc_dev, pools):
    """Joins of very different sizes one after another on one context: each join's counters
    and near-tie queue are cleared by its own first launch and its candidates counted from
    zero by its classify kernel, so every join's stats equal the same join's on a fresh
    context; then pip_join_count and the asynchronous pair on the same context."""
    mx, my, mk = pools[0]
    x3, y3 = nyc_points(3 * CHUNK, 86)
    inputs = [(mx[:2 * CHUNK], my[:2 * CHUNK]), (x3[:5], y3[:5]), (x3[:0], y3[:0]), (x3, y3)]
    assert (mk[:2 * CHUNK] == MIXED).all()
    wants = [oracle_join(nyc_chips_r9, x, y) if len(x) else (np.zeros(0, np.int64), np.zeros(0, np.int32))
             for x, y in inputs]
    # (every context's table is a device copy of the one uploaded blob)
    blob = nyc_dev.device_blob()
    ctx = M.GpuContext(gpu)
    d = M.chips.DeviceChips.from_device_blob(ctx, *blob, table=nyc_chips_r9)
    for (x, y), want in zip(inputs, wants):
        xt, yt = torch.from_numpy(x).to(gpu), torch.from_numpy(y).to(gpu)
        r = M.pip_join(xt, yt, d, 9)
        assert_pairs_equal(r.numpy(), want)
        fd = M.chips.DeviceChips.from_device_blob(M.GpuContext(gpu), *blob, table=nyc_chips_r9)
        f = M.pip_join(xt, yt, fd, 9)
        assert_pairs_equal(f.numpy(), want)
        assert {k: r.stats[k] for k in STAT_KEYS} == {k: f.stats[k] for k in STAT_KEYS}
        assert r.stats["n_pairs"] == len(want[0]) and r.stats["n_points"] == len(x)
    assert f.stats["n_candidates"] > 0
    # the count entry after a join, on the same context
    x, y = inputs[0]
    xt, yt = torch.from_numpy(x).to(gpu), torch.from_numpy(y).to(gpu)
    c = M.pip_join_count(xt, yt, d, 9)
    ids = c.polygon_id.cpu().numpy()
    want_counts = np.array([(wants[0][1] == i).sum() for i in ids], np.int64)
    assert np.array_equal(c.count.cpu().numpy(), want_counts)
    assert c.stats["n_pairs"] == len(wants[0][0])
    # ... and the asynchronous pair
    x, y = inputs[3]
    xt, yt = torch.from_numpy(x).to(gpu), torch.from_numpy(y).to(gpu)
    j = M.pip_join_async(xt, yt, d, 9)
    r = j.finish()
    assert_pairs_equal(r.numpy(), wants[3])
    assert int(j.count.item()) == len(wants[3][0])
    assert {k: r.stats[k] for k in STAT_KEYS} == {k: f.stats[k] for k in STAT_KEYS}


# ---------------------------------------------------------------- the chunk scan

SPARSE_BOX = (-76.0, -72.0, 39.0, 42.5)  # lon / lat around the zones: most points lie outside every zone
SCAN_CHUNKS = (1, 2, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1)


@pytest.fixture(scope="module")
def sparse_case(nyc_chips_r9):
    """1025 chunks of sparse points and their oracle pairs, computed once: the shorter
    inputs are its prefixes (the pairs are ordered by point)."""
    rng = np.random.default_rng(87)
    n = max(SCAN_CHUNKS) * CHUNK
    x = rng.uniform(SPARSE_BOX[0], SPARSE_BOX[1], n)
    y = rng.uniform(SPARSE_BOX[2], SPARSE_BOX[3], n)
    op, oq = oracle_join(nyc_chips_r9, x, y)
    assert 1000 < len(op) < n // 20
    return x, y, op, oq


@pytest.mark.parametrize("chunks", SCAN_CHUNKS)
def test_scan_chunk_counts(gpu, nyc_dev, sparse_case, chunks):
    """tile_scan_kernel's runs per thread: one chunk, two, one run short of a count per
    thread, exactly one per thread, and the first size with runs of two."""
    x, y, op, oq = sparse_case
    n = chunks * CHUNK - (3 if chunks > 1 else 0)  # (the last chunk partial where there are several)
    k = int(np.searchsorted(op, n))
    r = split_join(torch.from_numpy(x[:n]).to(gpu), torch.from_numpy(y[:n]).to(gpu), nyc_dev)
    assert_pairs_equal(r.numpy(), (op[:k], oq[:k]))


def test_scan_past_its_lds_counts(gpu, nyc_chips_r9, nyc_dev):
    """One chunk more than tile_scan_kernel stages in LDS (its global-memory path): points
    generated on the device, the split pipeline's pairs compared on the device with the
    fused pipeline's (no oracle at this size)."""
    n = SCAN_LDS * CHUNK + 1
    g = torch.Generator(device=gpu)
    g.manual_seed(88)
    x = torch.rand(n, dtype=torch.float64, device=gpu, generator=g) * (SPARSE_BOX[1] - SPARSE_BOX[0]) + SPARSE_BOX[0]
    y = torch.rand(n, dtype=torch.float64, device=gpu, generator=g) * (SPARSE_BOX[3] - SPARSE_BOX[2]) + SPARSE_BOX[2]
    ctx = M.GpuContext(gpu)
    d = M.chips.DeviceChips.from_device_blob(ctx, *nyc_dev.device_blob(), table=nyc_chips_r9)
    cap = n // 16
    s = split_join(x, y, d, capacity=cap)
    assert (n + CHUNK - 1) // CHUNK == SCAN_LDS + 1 and 100_000 < len(s) < cap
    with ctx.options(pipeline=N.MGPU_PIPELINE_FUSED):
        f = M.pip_join(x, y, d, 9, capacity=cap)
    assert f.stats["pipeline"] == N.MGPU_PIPELINE_FUSED
    assert len(f) == len(s)
    assert torch.equal(f.point_id, s.point_id) and torch.equal(f.polygon_id, s.polygon_id)
    ctx.close()

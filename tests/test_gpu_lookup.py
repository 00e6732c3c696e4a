"""mgpu_pip_join_lookup on the GPU: per input point, the polygon id of the first pair
pip_join emits for it (the lowest matching id; null_id without a pair) and its number of
pairs, exactly equal to what the oracle's ordered pairs give -- in the split, fused and
binned pipelines, around the units' sizes, for overlapping polygons (runs of records that
cross a wave and the slot / overflow-pool boundary), negative and sparse ids, BNG through
the fused and the split code path, mixed-pixel points of both outcomes, near-ties settled
by the host before the lookup kernel, caller tensors and errors that leave them untouched.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import mosaic_amd as M
import oracle as O
from mosaic_amd import _native as N

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from geom_util import nyc_points  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PIPELINES = [0, 1, 2]
SENTINEL = 0x5A5A5A5  # what the outputs hold before a call (no id or count of any table here)
INT32_MIN = -2 ** 31


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def oracle_join(c, x, y, res=9, isys=0):
    return O.pip_join(isys, res, x, y, c.cell, c.polygon_id, c.is_core, c.wkb_offsets, c.wkb)


def truth(op, oq, n, null_id=-1):
    """(first polygon, matches) per point from the oracle's pairs, which ascend by point and
    then polygon."""
    matches = np.bincount(op, minlength=n).astype(np.int32)
    first = np.full(n, null_id, np.int64)
    if len(op):
        head = np.concatenate([[True], op[1:] != op[:-1]])
        first[op[head]] = oq[head]
    return first.astype(np.int32), matches


def run(gpu, d, x, y, res, isys=None, pipeline=None, opts=None, **kw):
    opts = dict(opts or {})
    if pipeline is not None:
        opts["pipeline"] = pipeline
    with M.default_context(gpu).options(**opts):
        return M.pip_join_lookup(T(x, gpu), T(y, gpu), d, res, index_system=isys, **kw)


def check(r, first, matches, pipeline=None):
    assert r.polygon_id.dtype == torch.int32 and r.matches.dtype == torch.int32
    assert r.polygon_id.numel() == len(first) and r.matches.numel() == len(first)
    assert np.array_equal(r.matches.cpu().numpy(), matches)
    assert np.array_equal(r.polygon_id.cpu().numpy(), first)
    assert r.stats["n_pairs"] == int(matches.sum(dtype=np.int64))
    if pipeline is not None:
        assert r.stats["pipeline"] == pipeline


# ---------------------------------------------------------------- 1: NYC, every pipeline

@pytest.fixture(scope="module")
def nyc(gpu, nyc_chips_r9):
    x, y = nyc_points(300_000, 5)
    op, oq = oracle_join(nyc_chips_r9, x, y)
    return nyc_chips_r9, nyc_chips_r9.upload(), x, y, op, oq


@pytest.mark.parametrize("null_id", [-1, INT32_MIN])
@pytest.mark.parametrize("pipeline", PIPELINES)
def test_lookup_nyc(gpu, nyc, pipeline, null_id):
    c, d, x, y, op, oq = nyc
    first, matches = truth(op, oq, len(x), null_id)
    none = (matches == 0).mean()
    assert 0.1 < none < 0.9, none  # both branches
    check(run(gpu, d, x, y, 9, pipeline=pipeline, null_id=null_id), first, matches, pipeline)


# ---------------------------------------------------------------- 2: sizes around the units

def unit_sizes():
    t = int(N.lib().mgpu_join_tile_points())
    return sorted({0, 1, 63, 64, 65, 4095, 4096, 4097, 2 * 4096 + 1, t - 1, t, t + 1})


@pytest.mark.parametrize("pipeline", PIPELINES)
def test_lookup_sizes_around_the_units(gpu, nyc, pipeline):
    """A wave is 64 points, a fused tile mgpu_join_tile_points(), a chunk 4096.  The outputs
    are views into sentinel-filled buffers: every element of [0, n) changes, nothing beyond
    it (nor before it) does."""
    c, d, x, y, op, oq = nyc
    for n, pad in [(n, pad) for n in unit_sizes() for pad in (8, 3)]:  # (16-byte aligned views, and not)
        k = np.searchsorted(op, n)  # (the pairs of the first n points)
        first, matches = truth(op[:k], oq[:k], n)
        bp = torch.full((n + 2 * pad,), SENTINEL, dtype=torch.int32, device=gpu)
        bm = torch.full((n + 2 * pad,), SENTINEL, dtype=torch.int32, device=gpu)
        out = (bp[pad:pad + n], bm[pad:pad + n])
        assert n == 0 or out[0].data_ptr() % 16 == (0 if pad == 8 else 12)
        r = run(gpu, d, x[:n], y[:n], 9, pipeline=pipeline, out=out)
        if n:
            assert r.stats["pipeline"] == pipeline, n
        hp, hm = bp.cpu().numpy(), bm.cpu().numpy()
        for h in (hp, hm):
            assert (h[:pad] == SENTINEL).all() and (h[pad + n:] == SENTINEL).all(), (n, pad)
            assert (h[pad:pad + n] != SENTINEL).all(), (n, pad)
        assert np.array_equal(hm[pad:pad + n], matches), (n, pad)
        assert np.array_equal(hp[pad:pad + n], first), (n, pad)
        assert r.stats["n_pairs"] == matches.sum(), (n, pad)


# ---------------------------------------------------------------- 3: overlaps, lowest id wins

@pytest.fixture(scope="module")
def five_squares(gpu):
    sq = [(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0), (0.0, 0.0)]
    polys = [(pid, [[[(x * (1 + 0.01 * pid), y * (1 + 0.01 * pid)) for x, y in sq]]]) for pid in (5, 3, 9, 1, 7)]
    c = M.tessellate(M.Polygons.from_lists(polys), M.H3IndexSystem(), 5)
    rng = np.random.default_rng(8)
    # (past the squares' far corners, where they peel off one by one: every count 0..5)
    x = rng.uniform(0.05, 1.12, 50_000)
    y = rng.uniform(0.05, 1.12, 50_000)
    op, oq = oracle_join(c, x, y, res=5)
    return c, c.upload(), x, y, op, oq


@pytest.mark.parametrize("pipeline", [None, 0, 1, 2])
def test_lookup_five_overlapping_polygons(gpu, five_squares, pipeline):
    """(pipeline: the planner's choice, then each asked for -- taken where the table allows it)"""
    c, d, x, y, op, oq = five_squares
    first, matches = truth(op, oq, len(x))
    for k in range(1, 6):
        assert (matches == k).sum() > 0, k
    assert (first[matches == 5] == 1).all() and set(first[matches > 0]) == {1, 3, 5, 7, 9}
    check(run(gpu, d, x, y, 5, pipeline=pipeline), first, matches)


@pytest.mark.parametrize("isys", ["h3", "bng"])
def test_lookup_more_than_32_chips_per_cell(gpu, isys):
    """40 nested squares: the fused pipeline with its fix kernels; every tile holds more
    records than its slot, so the records lie in the overflow pool, the pool sized from n is
    short and the entry reruns the join once; a point's run of up to 40 records crosses the
    lanes of a wave and the 64-record batches."""
    if isys == "h3":
        base, sc, res, I = (-74.0, 40.7), 0.02, 7, M.H3IndexSystem()
    else:
        base, sc, res, I = (530000.0, 180000.0), 3000.0, 3, M.BNGIndexSystem()
    sq = [(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0), (0.0, 0.0)]
    polys = [(pid, [[[(base[0] + sc * u * (1 + 0.01 * pid), base[1] + sc * v * (1 + 0.013 * pid))
                      for u, v in sq]]]) for pid in range(40, 0, -1)]
    c = M.tessellate(M.Polygons.from_lists(polys), I, res)
    rng = np.random.default_rng(33)
    x = base[0] + sc * rng.uniform(-0.1, 1.6, 60_000)
    y = base[1] + sc * rng.uniform(-0.1, 1.6, 60_000)
    op, oq = oracle_join(c, x, y, res=res, isys=0 if isys == "h3" else 1)
    first, matches = truth(op, oq, len(x))
    assert (matches >= 30).sum() > 0 and len(op) > 10 * len(x)
    d = c.upload()
    check(run(gpu, d, x, y, res, isys=I), first, matches, 0)  # (more than 32 chips per cell: fused)


# ---------------------------------------------------------------- 4: negative and sparse ids

@pytest.mark.parametrize("pipeline", PIPELINES)
def test_lookup_negative_sparse_ids(gpu, nyc_chips_r9, pipeline):
    c0 = nyc_chips_r9
    pid = -c0.polygon_id.astype(np.int64) * 1000
    pid[c0.polygon_id == c0.polygon_id.max()] = INT32_MIN
    c = M.ChipTable(c0.cell, pid.astype(np.int32), c0.is_core, c0.wkb_offsets, c0.wkb)
    x, y = nyc_points(100_000, 17)
    op, oq = oracle_join(c, x, y)
    assert (oq < 0).all() and (oq == INT32_MIN).any() and not (c.polygon_id == 0).any()
    first, matches = truth(op, oq, len(x), null_id=0)
    check(run(gpu, c.upload(), x, y, 9, pipeline=pipeline, null_id=0), first, matches, pipeline)


# ---------------------------------------------------------------- 5: BNG

def test_lookup_london_districts_bng(gpu):
    """A C4-like table at res 4 through the fused pipeline and, with bng_split, through the
    split pipeline's BNG codes (first chip << 8 | mask)."""
    import bench_workloads as W
    I = M.BNGIndexSystem()
    c = M.tessellate(W.london_districts(), I, 4)
    x, y = W.london_points(200_000, 44)
    op, oq = oracle_join(c, x, y, res=4, isys=1)
    assert len(op) > 0.95 * len(x)
    first, matches = truth(op, oq, len(x))
    d = c.upload()
    for split in (0, 1):
        check(run(gpu, d, x, y, 4, isys=I, opts={"bng_split": split}), first, matches, 1 if split else 0)


# ---------------------------------------------------------------- 6: mixed points, both outcomes

def test_lookup_mixed_points_with_and_without_a_match(gpu, nyc_zones, nyc_chips_r9):
    """Points a few metres (sigma 3e-5 degrees) either side of zone boundaries: the pixel
    index leaves them to the mixed tiles, and those on the water side match nothing: a
    mixed position must end as (null_id, 0) for them and as the mixed tile's answer for the
    others, each taken from the chunk's list at the right place."""
    import bench_workloads as W
    from test_raster_host import raster_lookup
    bx, by = W.boundary_points(nyc_zones, 24_000, 81, 3e-5)
    ux, uy = nyc_points(20_000, 83)
    x, y = np.concatenate([bx, ux]), np.concatenate([by, uy])
    mixed = raster_lookup(nyc_chips_r9, 9, x, y)[0] == 2  # (the host lookup's kind of a mixed point)
    op, oq = oracle_join(nyc_chips_r9, x, y)
    first, matches = truth(op, oq, len(x), null_id=-7)
    assert (mixed & (matches == 0)).sum() >= 1000 and (mixed & (matches > 0)).sum() >= 1000
    check(run(gpu, nyc_chips_r9.upload(), x, y, 9, pipeline=1, null_id=-7), first, matches, 1)


# ---------------------------------------------------------------- 7: out= and matches=False

def test_lookup_out_and_no_matches(gpu, nyc):
    c, d, x, y, op, oq = nyc
    n = 50_000
    k = np.searchsorted(op, n)
    first, matches = truth(op[:k], oq[:k], n)
    xt, yt = T(x[:n], gpu), T(y[:n], gpu)
    new = lambda dtype=torch.int32, m=n, dev=gpu: torch.full((m,), SENTINEL, dtype=dtype, device=dev)
    op_t, om_t = new(), new()
    r = M.pip_join_lookup(xt, yt, d, 9, out=(op_t, om_t))
    assert r.polygon_id is op_t and r.matches is om_t
    check(r, first, matches)
    op_t = new()
    r = M.pip_join_lookup(xt, yt, d, 9, matches=False, out=(op_t, None))
    assert r.matches is None and r.polygon_id is op_t
    assert np.array_equal(op_t.cpu().numpy(), first) and r.stats["n_pairs"] == matches.sum()
    r = M.pip_join_lookup(xt, yt, d, 9, matches=False)
    assert r.matches is None and np.array_equal(r.polygon_id.cpu().numpy(), first)
    bad = [(new(torch.int64), new()), (new(), new(torch.int64)), (new(m=n - 1), new()), (new(), new(m=n + 1)),
           (new(dev="cpu"), new()), (new(m=2 * n)[::2], new()), (None, new()), (new(), None)]
    for out in bad:
        with pytest.raises(M.IllegalArgumentException):
            M.pip_join_lookup(xt, yt, d, 9, out=out)
    with pytest.raises(M.IllegalArgumentException):
        M.pip_join_lookup(xt, yt, d, 9, matches=False, out=(new(), new()))
    # the C entry: out_polygon NULL with n > 0
    st = N.MgpuStats()
    got = N.lib().mgpu_pip_join_lookup(d.ctx.handle, d.handle, N.MGPU_H3, 9, xt.data_ptr(), yt.data_ptr(), n, -1, None,
                                       None, None, ctypes.byref(st))
    assert got == N.MGPU_E_INVALID_ARG


# ---------------------------------------------------------------- 8: errors leave the output untouched

def test_lookup_errors_leave_the_output_untouched(gpu, nyc):
    import bench_workloads as W
    c, d, x, y, op, oq = nyc
    n = 20_000
    new = lambda: torch.full((n,), SENTINEL, dtype=torch.int32, device=gpu)
    xb = x[:n].copy()
    xb[n // 2] = np.nan
    for pipeline in PIPELINES:
        out = (new(), new())
        with pytest.raises(M.IllegalArgumentException):  # (what pip_join raises for H3)
            run(gpu, d, xb, y[:n], 9, pipeline=pipeline, out=out)
        assert bool((out[0] == SENTINEL).all()) and bool((out[1] == SENTINEL).all())
    with pytest.raises(M.IllegalArgumentException):
        M.pip_join(T(xb, gpu), T(y[:n], gpu), d, 9)
    I = M.BNGIndexSystem()
    cb = M.tessellate(W.london_districts(), I, 3)
    bx, by = W.london_points(n, 9)
    bx[7] = np.nan
    out = (new(), new())
    with pytest.raises(M.IllegalStateException, match="NaN"):
        run(gpu, cb.upload(), bx, by, 3, isys=I, out=out)
    assert bool((out[0] == SENTINEL).all()) and bool((out[1] == SENTINEL).all())
    with pytest.raises(M.IllegalStateException, match="NaN"):
        M.pip_join(T(bx, gpu), T(by, gpu), cb, 3, index_system=I)


# ---------------------------------------------------------------- 9: the records are kept

@pytest.mark.parametrize("pipeline", PIPELINES)
def test_lookup_keeps_the_join_records(gpu, nyc, pipeline):
    c, d, x, y, op, oq = nyc
    n = 100_000
    xt, yt = T(x[:n], gpu), T(y[:n], gpu)
    with M.default_context(gpu).options(pipeline=pipeline):
        want = M.pip_join(xt, yt, d, 9)
        r = M.pip_join_lookup(xt, yt, d, 9)
        assert r.stats["pipeline"] == pipeline
        cap = r.stats["n_pairs"]
        fp = torch.empty(cap, dtype=torch.int64, device=gpu)
        fq = torch.empty(cap, dtype=torch.int32, device=gpu)
        cnt = ctypes.c_int64()
        N.check(N.lib().mgpu_pip_join_fetch(d.ctx.handle, cap, ctypes.byref(cnt), fp.data_ptr(), fq.data_ptr(), None))
    assert cnt.value == cap == len(want)
    assert torch.equal(fp, want.point_id) and torch.equal(fq, want.polygon_id)


# ---------------------------------------------------------------- 10: near-ties

def test_lookup_near_ties_of_the_edge_fixture(gpu):
    """The tie band's fixture (tests/golden/h3_edge_points.npz: points on / within 1e-14
    degrees of H3 cell corners and edges, 12 per cell): those of its first 20,000 res-9
    points that lie within 20 degrees of the first and on its icosahedron face (one face: a
    table across faces is the join's matter, not the lookup's), over a table of two
    overlapping boxes around each of their cells.  The near-tie queue and the host libm pass
    run before the lookup kernel, and the column equals the reference oracle's."""
    f = np.load(os.path.join(GOLDEN, "h3_edge_points.npz"))
    m = np.nonzero(f["res"] == 9)[0][:20_000]
    lon, lat = f["lon"][m], f["lat"][m]
    face = lambda i: O.h3_geo_to_hex2d(np.radians(lat[i]), np.radians(lon[i]), 9)[0]
    near = np.nonzero((np.abs(lon - lon[0]) < 20.0) & (np.abs(lat - lat[0]) < 20.0))[0]
    assert len(near) % 12 == 0 and (near[::12] % 12 == 0).all()  # (whole cells of 12 points)
    keep = [k for k in near[::12] if all(face(i) == face(0) for i in range(k, k + 12))]
    sel = np.concatenate([np.arange(k, k + 12) for k in keep])
    x, y = lon[sel], lat[sel]
    assert 300 < len(x) <= 20_000
    box = lambda pid, cx, cy, h: (pid, [[[(cx - h, cy - h), (cx + h, cy - h), (cx + h, cy + h), (cx - h, cy + h),
                                          (cx - h, cy - h)]]])
    polys = []
    for k in range(0, len(x), 12):
        cx, cy = x[k:k + 12].mean(), y[k:k + 12].mean()
        polys += [box(k + 2, cx, cy, 0.006), box(k + 1, cx + 0.002, cy, 0.004)]
    c = M.tessellate(M.Polygons.from_lists(polys), M.H3IndexSystem(), 9)
    op, oq = oracle_join(c, x, y)
    first, matches = truth(op, oq, len(x))
    assert (matches == 1).sum() > 100 and (matches == 2).sum() > 100
    r = run(gpu, c.upload(), x, y, 9)
    assert r.stats["n_near_ties"] > 0
    check(r, first, matches)


def corner_points(c):
    """Points exactly on chip vertices and edge midpoints (H3 cell corners among them)."""
    import struct
    xs, ys = [], []
    for r in range(0, len(c), 3):
        blob = bytes(c.wkb[c.wkb_offsets[r]:c.wkb_offsets[r + 1]])
        if not blob or blob[4] != 3:
            continue
        (npts,) = struct.unpack(">I", blob[9:13])
        pts = [struct.unpack(">dd", blob[13 + 16 * i:29 + 16 * i]) for i in range(npts)]
        for i in range(npts - 1):
            xs += [pts[i][0], 0.5 * (pts[i][0] + pts[i + 1][0])]
            ys += [pts[i][1], 0.5 * (pts[i][1] + pts[i + 1][1])]
    return np.array(xs), np.array(ys)


@pytest.fixture(scope="module")
def nyc_corners(nyc_chips_r9):
    ax, ay = corner_points(nyc_chips_r9)
    ux, uy = nyc_points(20_000, 91)
    x, y = np.concatenate([ax, ux]), np.concatenate([ay, uy])
    o = np.random.default_rng(92).permutation(len(x))
    x, y = x[o], y[o]
    op, oq = oracle_join(nyc_chips_r9, x, y)
    return x, y, op, oq


@pytest.mark.parametrize("pipeline", PIPELINES)
def test_lookup_near_ties_settle_first(gpu, nyc, nyc_corners, pipeline):
    """NYC's own cell corners through every pipeline: the host's libm pass moves some cells,
    the column follows the override rerun."""
    x, y, op, oq = nyc_corners
    first, matches = truth(op, oq, len(x))
    r = run(gpu, nyc[1], x, y, 9, pipeline=pipeline)
    assert r.stats["n_near_ties"] > 0 and r.stats["libm_overrides"] > 0
    check(r, first, matches, pipeline)

"""Validity bitmaps and sliced columns through every entry that takes one, on the GPU.

A Spark columnar batch hands over sliced Arrow arrays with nulls.  The
bitmap is read as bit (offset + row) by the cell kernels, the fused join, both classify
kernels of the split pipeline, the bitmap merge and the two geometry decoders; the tests
below reach each of them with nulls, at even and odd offsets, at sizes around every unit
(byte, wave, tile, chunk), with null slots that hold NaN / inf / 1e300 / in-polygon points
and with in-polygon points (bits set) before and after the slice (tests/nulls_util.py).

References: the oracle's join of the rows valid in both columns (positions mapped back as
sel[op] + offset), the oracle's cells of the valid rows' centroids, numpy's packbits.
"""
import os
import struct
import sys
import types

import numpy as np
import pytest
import torch

import mosaic_amd as M
import nulls_util as U
import oracle as O
from geom_util import nyc_points
from mosaic_amd import arrow as A
from test_gpu_parity import adversarial_points, oracle_join

pytestmark = pytest.mark.gpu
BNG = M.BNGIndexSystem()


# ---------------------------------------------------------------- shared inputs and references

@pytest.fixture(scope="module")
def nyc_dev(gpu, nyc_chips_r9):
    return nyc_chips_r9.upload()


@pytest.fixture(scope="module")
def nyc_inside(nyc_chips_r9):
    """NYC points that lie in a zone, by the oracle (about a third of the uniform ones)."""
    x, y = nyc_points(60_000, 301)
    op, _ = oracle_join(nyc_chips_r9, x, y)
    k = np.unique(op)
    assert len(k) >= 13_000
    return x[k], y[k]


def reference(rows, chips, res=9, isys=0):
    """The oracle's pairs of the valid rows (rows.op positions within rows.sel, rows.oq) and
    the number of pairs the null rows that kept their coordinates would add
    (rows.kept_pairs: the guard against a vacuous case)."""
    none = (np.zeros(0, np.int64), np.zeros(0, np.int32))
    rows.op, rows.oq = oracle_join(chips, rows.x[rows.sel], rows.y[rows.sel], res, isys) if len(rows.sel) else none
    rows.kept_pairs = len(oracle_join(chips, rows.x[rows.kept], rows.y[rows.kept], res, isys)[0]) if len(rows.kept) else 0
    return rows


_ROWS = {}


def nyc_rows(chips, n, xpat, ypat, seed=310):
    """n uniform NYC points with the two columns' patterns (None: no bitmap) and their
    reference, computed once per parameter set."""
    key = (n, xpat, ypat, seed)
    if key not in _ROWS:
        x, y = nyc_points(n, seed)
        xp = None if xpat is None else U.present_pattern(xpat, n, seed + 1)
        yp = None if ypat is None else U.present_pattern(ypat, n, seed + 2)
        _ROWS[key] = reference(U.null_rows(x, y, xp, yp), chips)
    return _ROWS[key]


def arrow_join(rows, offs, d, res, fill, isys=None, null_counts=(None, None), **kw):
    case = U.embed(rows, offs[0], offs[1], *fill)
    xc, yc = U.columns(case, d.ctx.device, *null_counts)
    return A.pip_join_arrow(xc, yc, d, res, index_system=isys, **kw), xc, yc


def assert_pairs(got, rows, x_off):
    gp, gq = (t.cpu().numpy() for t in got) if isinstance(got, tuple) else got.numpy()
    assert len(gp) == len(rows.op), (len(gp), len(rows.op))
    assert np.array_equal(gp, rows.sel[rows.op] + x_off) and np.array_equal(gq, rows.oq)


# ---------------------------------------------------------------- the join: bitmap patterns

# (x pattern, y pattern, (x offset, y offset), points): every pattern on one column at an
# offset pair that takes classify_pair_kernel (both even) and at one that takes
# classify_wave_kernel, every offset pair used, and both columns with different patterns
PATTERN_CASES = [
    ("random30", None, (0, 0), 100_000), (None, "random30", (123, 123), 100_000),
    (None, "even_null", (2, 2), 20_000), ("even_null", None, (6, 13), 20_000),
    ("odd_null", None, (8, 8), 20_000), (None, "odd_null", (64, 1), 20_000),
    (None, "runs64", (0, 0), 20_000), ("runs64", None, (123, 123), 20_000),
    ("runs4096", None, (2, 2), 20_000), (None, "runs4096", (6, 13), 20_000),
    (None, "all_null", (8, 8), 20_000), ("all_null", None, (64, 1), 20_000),
    ("all_valid", None, (2, 2), 20_000), (None, "all_valid", (123, 123), 20_000),
    ("random30", "runs64", (6, 13), 100_000), ("odd_null", "random30", (2, 2), 100_000),
    ("runs4096", "even_null", (64, 1), 100_000), ("random30", "all_valid", (8, 8), 100_000),
]


def declared_kernel(offs):
    """Device allocations are at least 16-byte aligned, so the slice's first x and y are
    both 16-byte aligned exactly when both offsets are even (checked per case from the
    pointers, below)."""
    return "pair" if offs[0] % 2 == 0 and offs[1] % 2 == 0 else "wave"


def assert_pattern_coverage(cases):
    for pat in U.PATTERNS:
        met = {declared_kernel(o) for xp, yp, o, _ in cases if pat in (xp, yp)}
        assert met == {"pair", "wave"}, (pat, met)
    with_nulls = [c for c in cases if {c[0], c[1]} - {None, "all_valid"}]
    assert {declared_kernel(c[2]) for c in with_nulls} == {"pair", "wave"}
    both = [c for c in cases if c[0] and c[1]]
    assert any(c[2][0] != c[2][1] for c in both) and {declared_kernel(c[2]) for c in both} == {"pair", "wave"}
    assert {c[2] for c in cases} >= {(0, 0), (2, 2), (8, 8), (123, 123), (6, 13), (64, 1)}


assert_pattern_coverage(PATTERN_CASES)


@pytest.mark.parametrize("xpat,ypat,offs,n", PATTERN_CASES,
                         ids=["%s-%s-%d_%d" % (c[0] or "none", c[1] or "none", c[2][0], c[2][1]) for c in PATTERN_CASES])
def test_arrow_join_bitmap_patterns(gpu, nyc_chips_r9, nyc_dev, nyc_inside, xpat, ypat, offs, n):
    rows = nyc_rows(nyc_chips_r9, n, xpat, ypat)
    nulls = n - len(rows.sel)
    if {xpat, ypat} - {None, "all_valid"}:
        # the guard: the null slots that kept their coordinates would have produced pairs
        assert nulls > 0 and rows.kept_pairs >= (1000 if n >= 100_000 else 1), rows.kept_pairs
    else:
        assert nulls == 0
    # all_valid: null_count -1 ("not computed"), or the bitmap would not be read at all
    ncs = tuple(-1 if p == "all_valid" else None for p in (xpat, ypat))
    r, xc, yc = arrow_join(rows, offs, nyc_dev, 9, nyc_inside, null_counts=ncs)
    # the kernel the alignment rule selects, from the pointers: the table above covers both
    assert U.classify_kernel(xc, yc) == declared_kernel(offs)
    assert r.stats["pipeline"] == 1  # the split pipeline: the classify kernels ran
    assert_pairs(r, rows, offs[0])


# ---------------------------------------------------------------- the join: sizes around every unit

SIZES = [1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097, 12289]
SIZE_CASES = [(n, off) for i, n in enumerate(SIZES) for off in (8 + 2 * (i % 4), 9 + 2 * ((i + 2) % 4))]
assert {(off + n) % 8 for n, off in SIZE_CASES} == set(range(8))  # the slice's last bit on every position of a byte


@pytest.mark.parametrize("n,off", SIZE_CASES)
def test_arrow_join_sizes_around_units(gpu, nyc_chips_r9, nyc_dev, nyc_inside, n, off):
    """Every row lies in a zone here, so each valid row gives a pair and each null row
    would: odd rows null, the bitmap on x (even sizes' index) or on y."""
    ix, iy = nyc_inside
    x, y = ix[300:300 + n], iy[300:300 + n]
    p = U.present_pattern("odd_null", n)
    on_x = SIZES.index(n) % 2 == 0
    rows = reference(U.null_rows(x, y, p if on_x else None, None if on_x else p), nyc_chips_r9)
    assert len(rows.op) >= len(rows.sel) == (n + 1) // 2
    assert rows.kept_pairs >= len(rows.kept) and (n < 8 or len(rows.kept) >= 1)
    r, xc, yc = arrow_join(rows, (off, off), nyc_dev, 9, nyc_inside)
    assert U.classify_kernel(xc, yc) == declared_kernel((off, off))
    assert_pairs(r, rows, off)


# ---------------------------------------------------------------- the join: fused, binned request

@pytest.mark.parametrize("pipeline", [0, 2])
@pytest.mark.parametrize("offs", [(6, 13), (2, 2)])
def test_arrow_join_fused_and_binned_request(gpu, nyc_chips_r9, nyc_dev, nyc_inside, pipeline, offs):
    """The fused join with a merged bitmap; a request for the binned pipeline is declined
    with a bitmap (plan_bins), not served without it: the fused join runs."""
    rows = nyc_rows(nyc_chips_r9, 100_000, "random30", "runs64")
    assert rows.kept_pairs >= 1000
    with nyc_dev.ctx.options(pipeline=pipeline):
        r, _, _ = arrow_join(rows, offs, nyc_dev, 9, nyc_inside)
    assert r.stats["pipeline"] == 0
    assert_pairs(r, rows, offs[0])


@pytest.fixture(scope="module")
def nested(gpu):
    """40 nested, overlapping squares (test_pip_join_more_than_32_chips_per_cell): every
    cell holds 40 chips, so the fused join runs and every tile goes through its fix
    kernel -- here with nulls in both columns."""
    base, sc, res = (-74.0, 40.7), 0.02, 7
    sq = [(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0), (0.0, 0.0)]
    polys = [(pid, [[[(base[0] + sc * u * (1 + 0.01 * pid), base[1] + sc * v * (1 + 0.013 * pid))
                      for u, v in sq]]]) for pid in range(40, 0, -1)]
    c = M.tessellate(M.Polygons.from_lists(polys), M.H3IndexSystem(), res)
    rng = np.random.default_rng(331)
    n = 30_000
    x = base[0] + sc * rng.uniform(-0.1, 1.6, n)
    y = base[1] + sc * rng.uniform(-0.1, 1.6, n)
    fill = (base[0] + sc * rng.uniform(0.1, 0.9, 400), base[1] + sc * rng.uniform(0.1, 0.9, 400))
    rows = reference(U.null_rows(x, y, U.present_pattern("random30", n, 332), U.present_pattern("odd_null", n)), c, res=res)
    assert len(rows.op) > 5 * len(rows.sel) and rows.kept_pairs >= 1000
    assert len(oracle_join(c, fill[0], fill[1], res=res)[0]) >= 40 * 400  # the fill points lie in every square
    return types.SimpleNamespace(chips=c, d=c.upload(), res=res, rows=rows, fill=fill)


@pytest.mark.parametrize("offs", [(6, 13), (2, 2)])
def test_arrow_join_fused_fix_path_with_nulls(gpu, nested, offs):
    r, _, _ = arrow_join(nested.rows, offs, nested.d, nested.res, nested.fill, capacity=len(nested.rows.op) + 16)
    assert r.stats["pipeline"] == 0
    assert_pairs(r, nested.rows, offs[0])


# ---------------------------------------------------------------- the join: BNG

@pytest.fixture(scope="module")
def bng_cases():
    """_bng_synthetic(seed=21, n=40) at res 3 and 4; 100k UPRN-like points with random
    nulls in both columns, null payloads NaN, a negative coordinate, inf, 1e300, kept."""
    from test_host import _bng_synthetic
    P = _bng_synthetic(seed=21, n=40)
    out = {}
    for res in (3, 4):
        c = M.tessellate(P, BNG, res)
        rng = np.random.default_rng(340 + res)
        n = 100_000
        x = np.round(rng.uniform(505000, 560000, n), 2)
        y = np.round(rng.uniform(155000, 200000, n), 2)
        fx = np.round(rng.uniform(505000, 560000, 20_000), 2)
        fy = np.round(rng.uniform(155000, 200000, 20_000), 2)
        k = np.unique(oracle_join(c, fx, fy, res=res, isys=1)[0])
        assert len(k) >= U.HEAD + U.TAIL
        rows = U.null_rows(x, y, U.present_pattern("random30", n, 341), U.present_pattern("random30", n, 342),
                           payloads=U.BNG_PAYLOADS)
        out[res] = types.SimpleNamespace(chips=c, rows=reference(rows, c, res=res, isys=1), fill=(fx[k], fy[k]))
    return out


@pytest.mark.parametrize("offs", [(0, 0), (5, 5)])
@pytest.mark.parametrize("res", [3, 4])
def test_arrow_join_bng_nulls(gpu, bng_cases, res, offs):
    """BNG with nulls through the split pipeline with the grid entry as the code (the
    bng_grid_class path of the classify kernels; even offsets take the pair kernel, odd
    the wave kernel) -- the planner takes it for these tables with option bng_split = 1, as
    in test_pip_join_bng_split_grid_codes (the option is off by default) -- then with the
    default options, and through the fused join."""
    b = bng_cases[res]
    assert b.rows.kept_pairs >= 100 and len(b.rows.op) >= 1000
    ctx = M.default_context(gpu)
    d = b.chips.upload(ctx)
    with ctx.options(bng_split=1):
        r, xc, yc = arrow_join(b.rows, offs, d, res, b.fill, isys=BNG)
    assert U.classify_kernel(xc, yc) == declared_kernel(offs)
    assert r.stats["pipeline"] == 1
    assert_pairs(r, b.rows, offs[0])
    r, _, _ = arrow_join(b.rows, offs, d, res, b.fill, isys=BNG)
    assert_pairs(r, b.rows, offs[0])
    with ctx.options(pipeline=0):
        r0, _, _ = arrow_join(b.rows, offs, d, res, b.fill, isys=BNG)
    assert r0.stats["pipeline"] == 0
    assert_pairs(r0, b.rows, offs[0])


# ---------------------------------------------------------------- the join: override pass

@pytest.fixture(scope="module")
def override_case(nyc_chips_r9):
    """The adversarial points (H3 cell corners) spread through 150k uniform points.  The
    movers -- points whose cell differs between the oracle's two libm modes -- are nulled
    every other one, keeping their coordinates; 30 % of the other rows are null too.  The
    nulls alternate between the two columns."""
    c = nyc_chips_r9
    ax, ay = adversarial_points(c)
    rng = np.random.default_rng(351)
    n = 150_000
    x = rng.uniform(-74.25, -73.70, n)
    y = rng.uniform(40.50, 40.91, n)
    at = np.sort(rng.choice(n, len(ax), replace=False))
    x[at], y[at] = ax, ay
    glibc = O.h3_points_to_cells(x, y, 9)
    with O.h3_libm("cr"):
        cr = O.h3_points_to_cells(x, y, 9)
    movers = np.nonzero(glibc != cr)[0]
    assert len(movers) >= 2, "fewer than two points move between the libm modes: nothing to null and keep"
    null = rng.random(n) < 0.3
    null[movers] = False
    null[movers[::2]] = True
    idx = np.nonzero(null)[0]
    xp, yp = np.ones(n, bool), np.ones(n, bool)
    xp[idx[0::2]] = False
    yp[idx[1::2]] = False
    rows = reference(U.null_rows(x, y, xp, yp, keep_rows=movers[::2]), c)
    assert rows.both[movers[1::2]].all() and not rows.both[movers[::2]].any()
    assert np.isin(movers[::2], rows.kept).all()
    return rows


@pytest.mark.parametrize("pipeline", [0, 1])
@pytest.mark.parametrize("offs", [(2, 2), (6, 13)])
def test_arrow_join_override_pass_with_nulls(gpu, nyc_dev, nyc_inside, override_case, pipeline, offs):
    """The override pass (the host's libm moved some near-ties' cells; their tiles / chunks
    are unpaired and rerun) with null rows among the near-tie points: the pairs equal the
    reference's on the valid rows, and no null row was ever queued as a near-tie."""
    rows = override_case
    with nyc_dev.ctx.options(pipeline=pipeline):
        r, _, _ = arrow_join(rows, offs, nyc_dev, 9, nyc_inside)
        ties = nyc_dev.ctx.last_near_ties()
    assert r.stats["pipeline"] == pipeline
    assert r.stats["libm_overrides"] > 0
    assert_pairs(r, rows, offs[0])  # (the reference's: the oracle with glibc's libm)
    assert len(ties) > 0 and ties.min() >= 0 and ties.max() < rows.n
    assert rows.both[ties].all(), "null rows among the near-ties: %s" % ties[~rows.both[ties]][:10]


# ---------------------------------------------------------------- the join: capacity, then fetch

def test_arrow_join_capacity_then_fetch_with_nulls(gpu, nyc_chips_r9, nyc_dev, nyc_inside, nested):
    """Nulls in both columns: the merged bitmap lives in the context's scratch between the
    join that overflows and mgpu_pip_join_fetch.  The split pipeline keeps its answers; the
    fused join whose overflow pool (bounded by the capacity) dropped records is run again
    by the fetch, with that bitmap."""
    rows = nyc_rows(nyc_chips_r9, 100_000, "random30", "runs64")
    for offs in ((6, 13), (2, 2)):
        with pytest.raises(M.CapacityError) as ei:
            arrow_join(rows, offs, nyc_dev, 9, nyc_inside, capacity=100)
        assert ei.value.required == len(rows.op) > 100
        assert_pairs(A.pip_join_fetch(nyc_dev.ctx, ei.value.required), rows, offs[0])
    with nyc_dev.ctx.options(pipeline=0):
        with pytest.raises(M.CapacityError) as ei:
            arrow_join(rows, (6, 13), nyc_dev, 9, nyc_inside, capacity=100)
        assert ei.value.required == len(rows.op)
        assert_pairs(A.pip_join_fetch(nyc_dev.ctx, ei.value.required), rows, 6)
    # more pairs than points in every tile, a pool of 100 records: the fetch reruns the join
    with pytest.raises(M.CapacityError) as ei:
        arrow_join(nested.rows, (6, 13), nested.d, nested.res, nested.fill, capacity=100)
    assert ei.value.required == len(nested.rows.op)
    assert_pairs(A.pip_join_fetch(nested.d.ctx, ei.value.required), nested.rows, 6)


# ---------------------------------------------------------------- the join: null_count, argument errors

def test_arrow_join_null_count_unknown_and_zero(gpu, nyc_chips_r9, nyc_dev, nyc_inside):
    n = 20_000
    # null_count -1 ("not computed") with a bitmap: the bitmap decides
    rows = nyc_rows(nyc_chips_r9, n, "random30", None)
    assert rows.kept_pairs >= 1
    r, xc, _ = arrow_join(rows, (2, 2), nyc_dev, 9, nyc_inside, null_counts=(-1, None))
    assert xc.struct.array.null_count == -1
    assert_pairs(r, rows, 2)
    # null_count 0 with a bitmap of zeros: no nulls, the bitmap is not read (mosaic_arrow.h)
    x, y = nyc_points(n, 361)
    every = reference(U.null_rows(x, y, None, None), nyc_chips_r9)
    every.x_present = np.zeros(n, bool)
    case = U.embed(every, 3, 3, *nyc_inside)
    case.x_present[:] = False
    xc, yc = U.columns(case, gpu, 0, None)
    assert xc.struct.array.null_count == 0 and xc.struct.array.buffers[0] is not None
    assert_pairs(A.pip_join_arrow(xc, yc, nyc_dev, 9), every, 3)
    # a point_id column with nulls; x and y of different lengths
    xt = torch.from_numpy(x).to(gpu)
    yt = torch.from_numpy(y).to(gpu)
    ids = torch.arange(n, dtype=torch.int64, device=gpu)
    pc = A.DeviceColumn(n, [A.bitmap(U.present_pattern("random30", n, 362), gpu), ids], null_count=5)
    with pytest.raises(M.IllegalArgumentException):
        A.pip_join_arrow(A.float64_column(xt), A.float64_column(yt), nyc_dev, 9, point_id_col=pc)
    with pytest.raises(M.IllegalArgumentException):
        A.pip_join_arrow(A.float64_column(xt, length=n - 1), A.float64_column(yt), nyc_dev, 9)


# ---------------------------------------------------------------- geometry columns

GEO_SIZES = (1, 8, 9, 255, 256, 257, 2049)
GEO_OFFSETS = (0, 3, 8, 61)
GEO_ROWS = 61 + 2049 + 45


@pytest.fixture(scope="module")
def geo(gpu):
    """The geometries of test_geom_host._random_geoms(21, ...) in every format, whole
    (no nulls: the tests slice them and attach bitmaps), with the oracle's res-9 cells of
    their JTS centroids; BNG points as WKB with their res-3 cells."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import jts_centroid as JC
    from test_geom_host import _internal_rows, _json, _random_geoms, _wkt, w_geom
    geoms = _random_geoms(21, 2600)
    wkbs = [w_geom(*g, le=(i % 2 == 0)) for i, g in enumerate(geoms)]
    cx, cy = np.array([JC.centroid_wkb(w) for w in wkbs]).T
    cells = O.h3_points_to_cells(cx, cy, 9)
    flat = [i for i, g in enumerate(geoms) if g[0] != "collection"]  # (no InternalGeometry collection)
    assert len(flat) >= GEO_ROWS
    g = types.SimpleNamespace(cells=cells[:GEO_ROWS], internal_cells=cells[flat][:GEO_ROWS], cx=cx, cy=cy, wkbs=wkbs)
    R = range(GEO_ROWS)
    g.cols = {
        "wkb": M.GeometryColumn.from_rows([wkbs[i] for i in R], gpu),
        "hex": M.GeometryColumn.from_rows([wkbs[i].hex() if i % 3 else wkbs[i].hex().upper() for i in R], gpu, fmt="hex"),
        "wkt": M.GeometryColumn.from_rows([_wkt(*geoms[i], z=(i % 5 == 0)) for i in R], gpu, fmt="wkt"),
        "geojson": M.GeometryColumn.from_rows([_json(*geoms[i]) for i in R], gpu, fmt="geojson"),
    }
    g.internal = M.InternalGeometryColumn.from_rows(_internal_rows([geoms[i] for i in flat[:GEO_ROWS]]), gpu)
    rng = np.random.default_rng(371)
    e, nn = rng.uniform(503000, 561000, GEO_ROWS), rng.uniform(155000, 201000, GEO_ROWS)
    g.cols["bng"] = M.GeometryColumn.from_rows([struct.pack("<BIdd", 1, 1, a, b) for a, b in zip(e, nn)], gpu)
    g.bng_cells = O.bng_points_to_cells(e, nn, 3)
    g.present = rng.random(GEO_ROWS) >= 0.3
    return g


def geo_present(geo, off, n):
    """The random 30 % bitmap within the slice, every row outside it present."""
    p = geo.present.copy()
    p[:off] = True
    p[off + n:] = True
    return p


def assert_geometry(cells, valid, p, off, n, want):
    c = cells.cpu().numpy()
    sl = p[off:off + n]
    assert len(c) == n
    assert np.array_equal(c[sl], want[off:off + n][sl]), "cells of valid rows"
    assert (c[~sl] == 0).all(), "cells of null rows"
    v = valid.cpu().numpy()
    nb = (n + 7) // 8
    assert np.array_equal(v[:nb], U.expected_bitmap(p, off, n)), "bitmap (bits at or above n zero)"
    assert len(v) == nb + 1 and v[nb] == 0xAA, "the byte after the bitmap"


GEO_ENTRIES = ["wkb", "hex", "wkt", "geojson", "arrow-wkb-32", "arrow-wkb-64", "arrow-wkt-32", "arrow-wkt-64",
               "internal", "bng"]


@pytest.mark.parametrize("entry", GEO_ENTRIES)
def test_geometry_nulls_offsets_all_entries(gpu, geo, entry):
    """mgpu_geometry_to_cells (WKB, hex, WKT, GeoJSON; BNG res 3 for WKB points) with
    valid_offset = the row offset over a view of the whole offsets array,
    mgpu_geometry_to_cells_arrow (WKB, WKT; int32 and int64 offsets) with ArrowArray.offset,
    mgpu_internal_geometry_to_cells: every size and offset, a caller-owned bitmap."""
    for n in GEO_SIZES:
        for off in GEO_OFFSETS:
            p = geo_present(geo, off, n)
            bm = A.bitmap(p, gpu)
            out = torch.full(((n + 7) // 8 + 1,), 0xAA, dtype=torch.uint8, device=gpu)
            want, isys, res = geo.cells, None, 9
            if entry.startswith("arrow"):
                col = geo.cols[entry.split("-")[1]]
                whole = M.GeometryColumn(col.format, col.data, col.offsets, valid=bm)
                cells, valid = A.grid_pointascellid_arrow(whole, res, large=entry.endswith("64"), offset=off, length=n,
                                                          out_valid=out)
            elif entry == "internal":
                ic = geo.internal
                sliced = M.InternalGeometryColumn(ic.type_id[off:off + n], ic.row_part[off:off + n + 1], ic.part_ring,
                                                  ic.ring_off, ic.xy, valid=bm, valid_offset=off)
                cells, valid = M.grid_pointascellid(sliced, res, out_valid=out)
                want = geo.internal_cells
            else:
                col = geo.cols[entry]
                if entry == "bng":
                    want, isys, res = geo.bng_cells, BNG, 3
                sliced = M.GeometryColumn(col.format, col.data, col.offsets[off:off + n + 1], valid=bm, valid_offset=off)
                cells, valid = M.grid_pointascellid(sliced, res, index_system=isys, out_valid=out)
            assert valid.data_ptr() == out.data_ptr()
            try:
                assert_geometry(cells, valid, p, off, n, want)
            except AssertionError as e:
                raise AssertionError("%s n=%d offset=%d: %s" % (entry, n, off, e))


def test_geometry_null_rows_hold_garbage(gpu):
    """Null rows hold bytes no decoder accepts; the call succeeds and the valid rows' cells
    are right.  With one such row flipped to valid the decoder's exception comes out."""
    x, y = nyc_points(40, 381)
    want = O.h3_points_to_cells(x, y, 9)
    point = lambda i: struct.pack("<BIdd", 1, 1, x[i], y[i])  # noqa: E731
    garbage = {
        "wkb": {3: (point(3)[:-1], M.IllegalArgumentException),                      # truncated
                8: (struct.pack("<BI", 1, 99) + b"\0" * 16, M.MosaicGpuError),          # a type no decoder builds
                9: (struct.pack("<BII", 1, 3, 0), M.IllegalStateException),            # POLYGON EMPTY
                17: (b"\x07\x07", M.IllegalArgumentException),                            # no byte order
                18: (b"", M.IllegalArgumentException)},                                # end < begin, below
        "wkt": {3: ("POINT (1 2", M.MosaicGpuError), 8: ("POLYGON EMPTY", M.MosaicGpuError),
                9: ("POINT (", M.MosaicGpuError), 17: ("LINESTRING (1 2", M.MosaicGpuError),
                18: ("", M.IllegalArgumentException)},
    }
    for fmt, bad in garbage.items():
        rows = [bad[i][0] if i in bad else (point(i) if fmt == "wkb" else "POINT (%r %r)" % (float(x[i]), float(y[i])))
                for i in range(40)]
        col = M.GeometryColumn.from_rows(rows, gpu, fmt=fmt)
        offsets = col.offsets.clone()
        offsets[18] += 5  # row 18 (null, empty): end < begin; row 17 (null) runs into row 19's bytes
        present = np.array([i not in bad for i in range(40)])
        for off, n in ((0, 40), (2, 38)):
            def column(p):
                return M.GeometryColumn(col.format, col.data, offsets[off:off + n + 1], valid=A.bitmap(p, gpu), valid_offset=off)
            cells, valid = M.grid_pointascellid(column(present), 9)
            c = cells.cpu().numpy()
            sl = present[off:off + n]
            assert np.array_equal(c[sl], want[off:off + n][sl]) and (c[~sl] == 0).all()
            assert np.array_equal(valid.cpu().numpy(), U.expected_bitmap(present, off, n))
            for i, (_, exc) in bad.items():
                flipped = present.copy()
                flipped[i] = True
                with pytest.raises(exc):
                    M.grid_pointascellid(column(flipped), 9)
        if fmt == "wkt":  # the Arrow entry, int32 offsets, sliced by ArrowArray.offset
            whole = M.GeometryColumn(col.format, col.data, offsets, valid=A.bitmap(present, gpu))
            cells, valid = A.grid_pointascellid_arrow(whole, 9, large=False, offset=2, length=37)
            c = cells.cpu().numpy()
            sl = present[2:39]
            assert np.array_equal(c[sl], want[2:39][sl]) and (c[~sl] == 0).all()
            assert np.array_equal(valid.cpu().numpy(), U.expected_bitmap(present, 2, 37))


def test_points_from_geometry_nulls(gpu, geo):
    """mgpu_points_from_geometry: NaN for null rows (whatever they hold), the point for the
    rest -- WKB points, so the centroid is the row's own coordinates, bit for bit."""
    x, y = nyc_points(GEO_ROWS, 391)
    col = M.GeometryColumn.from_rows([struct.pack("<BIdd" if i % 2 else ">BIdd", i % 2, 1, a, b)
                                      for i, (a, b) in enumerate(zip(x, y))], gpu)
    for n in (1, 9, 257, 2049):
        for off in (0, 3, 61):
            p = geo_present(geo, off, n)
            sliced = M.GeometryColumn(col.format, col.data, col.offsets[off:off + n + 1], valid=A.bitmap(p, gpu), valid_offset=off)
            gx, gy = (t.cpu().numpy() for t in M.points_from_geometry(sliced))
            sl = p[off:off + n]
            assert np.array_equal(gx[sl], x[off:off + n][sl]) and np.array_equal(gy[sl], y[off:off + n][sl]), (n, off)
            assert np.isnan(gx[~sl]).all() and np.isnan(gy[~sl]).all(), (n, off)

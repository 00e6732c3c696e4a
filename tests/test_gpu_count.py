"""mgpu_pip_join_count on the GPU: per-polygon counts and integer sums equal, exactly, what
np.add.at gives over the oracle's pairs for the same table and points -- in the split,
fused and binned pipelines, with the LDS histograms (the default) and with global atomics
(count_lds_slots = 0), for dense, negative and sparse polygon ids.  Sections 10 to 15 run
the branches that need either a very large batch or unusual inputs: a capped grid
(count_groups) so that a workgroup strides over many chunks or tiles, weights over the
whole int64 range in random and in spatially sorted order, every id -> slot lookup,
unaligned weight columns, and accumulation onto arbitrary contents."""
import ctypes
import struct

import numpy as np
import pytest
import torch

import mosaic_amd as M
import oracle as O
from mosaic_amd import _native as N
from geom_util import nyc_points

pytestmark = pytest.mark.gpu

PIPELINES = [0, 1, 2]
LDS = [None, 0]  # count_lds_slots: the default, or 0 = the global path


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def oracle_join(c, x, y, res=9, isys=0):
    return O.pip_join(isys, res, x, y, c.cell, c.polygon_id, c.is_core, c.wkb_offsets, c.wkb)


def weights(n):
    return np.arange(n, dtype=np.int64) * 3 - 7


def truth(c, op, oq, w=None):
    """(ids, count, sum) from the oracle's pairs; the sums in unsigned arithmetic, so that
    they wrap modulo 2^64 whatever numpy does on signed overflow."""
    ids = np.unique(c.polygon_id)
    slot = np.searchsorted(ids, oq)
    cnt = np.zeros(len(ids), np.int64)
    np.add.at(cnt, slot, 1)
    sm = None
    if w is not None:
        assert w.dtype == np.int64
        sm = np.zeros(len(ids), np.int64)
        np.add.at(sm.view(np.uint64), slot, w.view(np.uint64)[op])
    return ids.astype(np.int32), cnt, sm


def run(gpu, d, x, y, res, isys=None, w=None, pipeline=None, lds=None, wt=None, opts=None, **kw):
    """w: a numpy weight column, or wt: a ready-made device tensor; opts: further context
    options."""
    opts = dict(opts or {})
    if pipeline is not None:
        opts["pipeline"] = pipeline
    if lds is not None:
        opts["count_lds_slots"] = lds
    if wt is None and w is not None:
        wt = torch.from_numpy(w).to(gpu)
    with M.default_context(gpu).options(**opts):
        return M.pip_join_count(T(x, gpu), T(y, gpu), d, res, index_system=isys, weight=wt, **kw)


def check(r, ids, cnt, sm):
    assert r.polygon_id.dtype == torch.int32 and r.count.dtype == torch.int64
    assert np.array_equal(r.polygon_id.cpu().numpy(), ids)
    assert np.array_equal(r.count.cpu().numpy(), cnt)
    assert int(r.count.sum()) == r.stats["n_pairs"] == int(cnt.sum())
    if sm is None:
        assert r.sum is None
    else:
        assert np.array_equal(r.sum.cpu().numpy(), sm)


# ---------------------------------------------------------------- 1, 2: the NYC table

@pytest.fixture(scope="module")
def nyc(gpu, nyc_chips_r9):
    x, y = nyc_points(300_000, 5)
    op, oq = oracle_join(nyc_chips_r9, x, y)
    return nyc_chips_r9, nyc_chips_r9.upload(), x, y, op, oq


@pytest.mark.parametrize("lds", LDS)
@pytest.mark.parametrize("pipeline", PIPELINES)
def test_count_nyc(gpu, nyc, pipeline, lds):
    c, d, x, y, op, oq = nyc
    w = weights(len(x))
    ids, cnt, sm = truth(c, op, oq, w)
    assert cnt.sum() > 0.25 * len(x) and (cnt > 0).sum() > 200
    r = run(gpu, d, x, y, 9, w=w, pipeline=pipeline, lds=lds)
    assert r.stats["pipeline"] == pipeline
    check(r, ids, cnt, sm)
    check(run(gpu, d, x, y, 9, pipeline=pipeline, lds=lds), ids, cnt, None)


@pytest.mark.parametrize("pipeline", PIPELINES)
@pytest.mark.parametrize("n", [0, 1, 63, 4095, 4096, 4097])
def test_count_sizes_around_the_units(gpu, nyc, n, pipeline):
    """kChunk is 4096 points, a wave 64."""
    c, d, x, y, op, oq = nyc
    k = np.searchsorted(op, n)  # (the oracle's pairs ascend by point: those of the first n points)
    w = weights(n)
    ids, cnt, sm = truth(c, op[:k], oq[:k], w)
    for lds in LDS:
        check(run(gpu, d, x[:n], y[:n], 9, w=w, pipeline=pipeline, lds=lds), ids, cnt, sm)


# ---------------------------------------------------------------- 3: negative and sparse ids

@pytest.fixture(scope="module")
def negative_ids(gpu, nyc_chips_r9):
    c0 = nyc_chips_r9
    pid = -c0.polygon_id.astype(np.int64) * 1000
    pid[c0.polygon_id == c0.polygon_id.max()] = -2 ** 31
    c = M.ChipTable(c0.cell, pid.astype(np.int32), c0.is_core, c0.wkb_offsets, c0.wkb)
    x, y = nyc_points(100_000, 17)
    op, oq = oracle_join(c, x, y)
    assert (oq < 0).all() and (oq == -2 ** 31).any()
    return c, c.upload(), x, y, op, oq


@pytest.mark.parametrize("pipeline", PIPELINES)
def test_count_negative_sparse_ids(gpu, negative_ids, pipeline):
    """Ids scaled by -1000 and INT32_MIN: too sparse for the dense table, so the slot
    lookup is the binary search."""
    c, d, x, y, op, oq = negative_ids
    w = weights(len(x))
    ids, cnt, sm = truth(c, op, oq, w)
    assert ids[0] == -2 ** 31 and np.array_equal(d.polygons(), ids)
    for lds in LDS:
        r = run(gpu, d, x, y, 9, w=w, pipeline=pipeline, lds=lds)
        assert r.stats["pipeline"] == pipeline
        check(r, ids, cnt, sm)


@pytest.fixture(scope="module")
def gapped_ids(gpu, nyc_chips_r9):
    c0 = nyc_chips_r9
    c = M.ChipTable(c0.cell, c0.polygon_id * 3 + 5, c0.is_core, c0.wkb_offsets, c0.wkb)
    x, y = nyc_points(100_000, 18)
    op, oq = oracle_join(c, x, y)
    return c, c.upload(), x, y, op, oq


@pytest.mark.parametrize("pipeline", PIPELINES)
def test_count_gapped_ids(gpu, gapped_ids, pipeline):
    """Ids 8, 11, 14, ...: not contiguous (no slot = id - min shortcut) but close enough
    for the dense id -> slot table."""
    c, d, x, y, op, oq = gapped_ids
    w = weights(len(x))
    ids, cnt, sm = truth(c, op, oq, w)
    assert ids[-1] - ids[0] + 1 > len(ids)
    for lds in LDS + [100]:
        r = run(gpu, d, x, y, 9, w=w, pipeline=pipeline, lds=lds)
        assert r.stats["pipeline"] == pipeline
        check(r, ids, cnt, sm)


# ---------------------------------------------------------------- 4: many pairs per point

@pytest.mark.parametrize("isys", ["h3", "bng"])
def test_count_more_than_32_chips_per_cell(gpu, isys):
    """40 nested polygons: every tile goes through the fix kernels and holds more records
    than its slot, so the fused pipeline's pool (sized from n) is short and the join runs
    once more with the size the first run reported."""
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
    assert len(op) > 10 * len(x)
    w = weights(len(x))
    ids, cnt, sm = truth(c, op, oq, w)
    d = c.upload()
    for lds in LDS:
        r = run(gpu, d, x, y, res, isys=I, w=w, lds=lds)
        assert r.stats["pipeline"] == 0  # (more than 32 chips per cell: the planner's fused pipeline)
        check(r, ids, cnt, sm)
        check(run(gpu, d, x, y, res, isys=I, w=w, lds=lds, pipeline=0), ids, cnt, sm)


@pytest.fixture(scope="module")
def five_squares(gpu):
    sq = [(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0), (0.0, 0.0)]
    polys = [(pid, [[[(x * (1 + 0.01 * pid), y * (1 + 0.01 * pid)) for x, y in sq]]]) for pid in (5, 3, 9, 1, 7)]
    c = M.tessellate(M.Polygons.from_lists(polys), M.H3IndexSystem(), 5)
    rng = np.random.default_rng(8)
    x = rng.uniform(0.05, 0.95, 50_000)
    y = rng.uniform(0.05, 0.95, 50_000)
    op, oq = oracle_join(c, x, y, res=5)
    assert len(op) > 4 * len(x)
    return c, c.upload(), x, y, op, oq


def test_count_five_overlapping_polygons(gpu, five_squares):
    c, d, x, y, op, oq = five_squares
    w = weights(len(x))
    ids, cnt, sm = truth(c, op, oq, w)
    for pipeline in (None, 0, 1, 2):
        for lds in LDS:
            check(run(gpu, d, x, y, 5, w=w, pipeline=pipeline, lds=lds), ids, cnt, sm)


# ---------------------------------------------------------------- 5: the near-tie override

def adversarial_points(c):
    """Points exactly on chip vertices and edge midpoints (H3 cell corners)."""
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
def override_input(gpu, nyc):
    c, d = nyc[0], nyc[1]
    ax, ay = adversarial_points(c)
    rng = np.random.default_rng(91)
    n = 200_000
    x = rng.uniform(-74.25, -73.70, n)
    y = rng.uniform(40.50, 40.91, n)
    at = np.sort(rng.choice(n, len(ax), replace=False))
    x[at], y[at] = ax, ay
    op, oq = oracle_join(c, x, y)
    return c, d, x, y, op, oq


@pytest.mark.parametrize("pipeline", PIPELINES)
def test_count_adversarial_override_pass(gpu, override_input, pipeline):
    """The host's libm pass moves some cells: the counts follow the rerun and equal the
    reference (glibc) oracle's."""
    c, d, x, y, op, oq = override_input
    w = weights(len(x))
    ids, cnt, sm = truth(c, op, oq, w)
    r = run(gpu, d, x, y, 9, w=w, pipeline=pipeline)
    assert r.stats["pipeline"] == pipeline
    assert r.stats["libm_overrides"] > 0
    check(r, ids, cnt, sm)


# ---------------------------------------------------------------- 6: a large slot count

@pytest.fixture(scope="module")
def tracts(gpu):
    import bench_workloads as W
    E = (-75.0, 40.0, -74.5, 40.4)
    P = W.tract_polygons(n_cells=3000, extent=E, seed=21)
    c = M.tessellate(P, M.H3IndexSystem(), 10, keep_core_geometries=False)
    x, y = W.extent_points(E, 200_000, 6)
    x, y = np.asarray(x), np.asarray(y)
    op, oq = oracle_join(c, x, y, res=10)
    return c, c.upload(), x, y, op, oq


@pytest.mark.parametrize("lds", LDS + [1000])
@pytest.mark.parametrize("pipeline", [None, 0, 1, 2])
def test_count_3000_tracts(gpu, tracts, pipeline, lds):
    """3000 polygons: LDS histograms by default; with count_lds_slots = 1000 the table has
    more polygons than slots and the workgroups keep an LDS hash table of 4096 entries in
    front of the global atomics (full enough here that some additions miss it); 0: global
    atomics only.  The table has a pixel index of more than kEmitCls = 2048 classes (one
    per polygon at least, the one-match classes in polygon order), so in the split
    pipeline the classes past the LDS class table go through raster_cls."""
    c, d, x, y, op, oq = tracts
    w = weights(len(x))
    ids, cnt, sm = truth(c, op, oq, w)
    assert len(ids) == 3000
    if pipeline == 1:
        assert d.info()["raster_mode"] != 0 and d.info()["raster_ncls"] > 3000
        # (every polygon here has pure pixels, hence a one-match class, and those are numbered
        # in polygon order from 1: the pure points of these polygons carry codes past the table)
        assert (cnt[2048:] > 0).sum() > 900
    r = run(gpu, d, x, y, 10, w=w, pipeline=pipeline, lds=lds)
    if pipeline is not None:
        assert r.stats["pipeline"] == pipeline
    check(r, ids, cnt, sm)


# ---------------------------------------------------------------- 7: BNG

@pytest.mark.parametrize("res", [3, 4])
def test_count_london_districts_bng(gpu, res):
    import bench_workloads as W
    I = M.BNGIndexSystem()
    c = M.tessellate(W.london_districts(), I, res)
    x, y = W.london_points(200_000, 40 + res)
    op, oq = oracle_join(c, x, y, res=res, isys=1)
    assert len(op) > 0.95 * len(x)
    w = weights(len(x))
    ids, cnt, sm = truth(c, op, oq, w)
    d = c.upload()
    for lds in LDS:
        check(run(gpu, d, x, y, res, isys=I, w=w, lds=lds), ids, cnt, sm)


# ---------------------------------------------------------------- 8: accumulate and errors

def test_count_accumulate_two_batches(gpu, nyc):
    c, d, x, y, op, oq = nyc
    n, h = len(x), 123_457
    w = weights(n)
    ids, cnt, sm = truth(c, op, oq, w)
    out = (torch.zeros(len(ids), dtype=torch.int64, device=gpu), torch.zeros(len(ids), dtype=torch.int64, device=gpu))
    r1 = run(gpu, d, x[:h], y[:h], 9, w=w[:h], out=out, accumulate=True)
    r2 = run(gpu, d, x[h:], y[h:], 9, w=w[h:], out=out, accumulate=True)
    assert r1.stats["n_pairs"] + r2.stats["n_pairs"] == cnt.sum()
    assert np.array_equal(out[0].cpu().numpy(), cnt) and np.array_equal(out[1].cpu().numpy(), sm)
    # without accumulate the arrays are overwritten
    r3 = run(gpu, d, x[:h], y[:h], 9, w=w[:h], out=out)
    k = np.searchsorted(op, h)
    _, cnt_h, sm_h = truth(c, op[:k], oq[:k], w)
    assert np.array_equal(r3.count.cpu().numpy(), cnt_h) and np.array_equal(r3.sum.cpu().numpy(), sm_h)


@pytest.mark.parametrize("isys", ["h3", "bng"])
def test_count_nan_raises_and_leaves_outputs(gpu, nyc, isys):
    if isys == "h3":
        c, d, x, y = nyc[:4]
        I, res = M.H3IndexSystem(), 9
    else:
        I, res = M.BNGIndexSystem(), 3
        sq = [[[(530000.0, 180000.0), (533000.0, 180000.0), (533000.0, 183000.0), (530000.0, 183000.0),
                (530000.0, 180000.0)]]]
        c = M.tessellate(M.Polygons.from_lists([(1, sq)]), I, res)
        d = c.upload()
        rng = np.random.default_rng(3)
        x, y = rng.uniform(529000, 534000, 20_000), rng.uniform(179000, 184000, 20_000)
    x, y = x[:20_000].copy(), y[:20_000].copy()
    x[7777] = np.nan
    with pytest.raises(M.MosaicGpuError) as e_join:
        M.pip_join(T(x, gpu), T(y, gpu), d, res, index_system=I)
    P = len(d.polygons())
    out = (torch.full((P,), 41, dtype=torch.int64, device=gpu), torch.full((P,), -43, dtype=torch.int64, device=gpu))
    for acc in (False, True):
        with pytest.raises(M.MosaicGpuError) as e_cnt:
            run(gpu, d, x, y, res, isys=I, w=weights(len(x)), out=out, accumulate=acc)
        assert type(e_cnt.value) is type(e_join.value) and str(e_cnt.value) == str(e_join.value)
        assert (out[0] == 41).all() and (out[1] == -43).all()


def test_count_wrong_n_slots_and_arguments(gpu, nyc):
    c, d, x, y = nyc[:4]
    P = len(d.polygons())
    for bad in (P - 1, P + 1):
        out = (torch.zeros(bad, dtype=torch.int64, device=gpu), None)
        with pytest.raises(M.IllegalArgumentException):
            run(gpu, d, x[:1000], y[:1000], 9, out=out)
    with pytest.raises(M.IllegalArgumentException):  # a weight without a sum
        run(gpu, d, x[:1000], y[:1000], 9, w=weights(1000), out=(torch.zeros(P, dtype=torch.int64, device=gpu), None))
    with pytest.raises(M.IllegalArgumentException):  # one weight per point
        run(gpu, d, x[:1000], y[:1000], 9, w=weights(999))
    with pytest.raises(M.IllegalArgumentException):
        M.default_context(gpu).set_option("count_lds_slots", 4097)


# ---------------------------------------------------------------- 9: fetch after count

@pytest.mark.parametrize("pipeline", [1, 0])
def test_fetch_after_count(gpu, nyc, pipeline):
    """The join's records stay in the context: mgpu_pip_join_fetch after a count call
    writes the pairs mgpu_pip_join would have."""
    c, d, x, y, op, oq = nyc
    n = 100_000
    k = np.searchsorted(op, n)
    r = run(gpu, d, x[:n], y[:n], 9, pipeline=pipeline)
    assert r.stats["pipeline"] == pipeline and r.stats["n_pairs"] == k
    gp = torch.empty(k, dtype=torch.int64, device=gpu)
    gq = torch.empty(k, dtype=torch.int32, device=gpu)
    cnt = ctypes.c_int64()
    s = torch.cuda.current_stream(gpu).cuda_stream
    N.check(N.lib().mgpu_pip_join_fetch(d.ctx.handle, k, ctypes.byref(cnt), gp.data_ptr(), gq.data_ptr(), s))
    assert cnt.value == k
    assert np.array_equal(gp.cpu().numpy(), op[:k]) and np.array_equal(gq.cpu().numpy(), oq[:k])


def test_fetch_after_count_with_pool(gpu):
    """Fused with an overflow pool in use (5 pairs per point): the fetch compares against
    the pool the count call used, not a capacity it never had."""
    sq = [(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0), (0.0, 0.0)]
    polys = [(pid, [[[(x * (1 + 0.01 * pid), y * (1 + 0.01 * pid)) for x, y in sq]]]) for pid in (5, 3, 9, 1, 7)]
    c = M.tessellate(M.Polygons.from_lists(polys), M.H3IndexSystem(), 5)
    rng = np.random.default_rng(8)
    x = rng.uniform(0.05, 0.95, 20_000)
    y = rng.uniform(0.05, 0.95, 20_000)
    op, oq = oracle_join(c, x, y, res=5)
    d = c.upload()
    r = run(gpu, d, x, y, 5, pipeline=0)
    k = len(op)
    assert r.stats["pipeline"] == 0 and r.stats["n_pairs"] == k
    gp = torch.empty(k, dtype=torch.int64, device=gpu)
    gq = torch.empty(k, dtype=torch.int32, device=gpu)
    cnt = ctypes.c_int64()
    s = torch.cuda.current_stream(gpu).cuda_stream
    N.check(N.lib().mgpu_pip_join_fetch(d.ctx.handle, k, ctypes.byref(cnt), gp.data_ptr(), gq.data_ptr(), s))
    assert np.array_equal(gp.cpu().numpy(), op) and np.array_equal(gq.cpu().numpy(), oq)


# ---------------------------------------------------------------- 10: weights over the whole int64 range

I64 = np.iinfo(np.int64)
COLUMNS = ["uniform", "high_word", "low_ones", "min_max", "all_max"]


def weight_column(name, n, seed=77):
    rng = np.random.default_rng(seed)
    if name == "uniform":  # the whole range
        return rng.integers(I64.min, I64.max, n, dtype=np.int64, endpoint=True)
    if name == "high_word":  # k << 32: the low word is zero
        return rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64) * (1 << 32)
    if name == "low_ones":  # every addition of two carries into the high word
        return np.full(n, 0xFFFFFFFF, np.int64)
    if name == "min_max":
        return np.where(np.arange(n) & 1, I64.max, I64.min).astype(np.int64)
    assert name == "all_max"
    return np.full(n, I64.max, np.int64)


def first_polygons(n, op, oq):
    """(matched, first): whether point i has a pair, and the polygon of its first one (the
    oracle's pairs ascend by point)."""
    pts, at = np.unique(op, return_index=True)
    matched = np.zeros(n, bool)
    matched[pts] = True
    first = np.zeros(n, np.int64)
    first[pts] = oq[at]
    return matched, first


def sorted_order(n, op, oq):
    """A permutation of the points as spatially sorted data arrives: the matched points
    ordered by their first polygon, an unmatched point at every seventh position inside
    those runs (the unmatched points that are left follow the runs)."""
    matched, first = first_polygons(n, op, oq)
    m = np.flatnonzero(matched)
    m = m[np.argsort(first[m], kind="stable")]
    u = np.flatnonzero(~matched)
    k = min(len(u), len(m) // 6)
    inner = np.empty(len(m) + k, np.int64)
    is_u = np.zeros(len(inner), bool)
    is_u[7 * np.arange(k) + 6] = True
    inner[is_u] = u[:k]
    inner[~is_u] = m
    perm = np.concatenate([inner, u[k:]])
    assert np.array_equal(np.sort(perm), np.arange(n))
    return perm


def share_in_long_runs(perm, n, op, oq, min_run=128):
    """The share of the matched points that lie, in the order perm, in a run of at least
    min_run matched points with the same first polygon (unmatched points in between do not
    end a run and are not counted into its length)."""
    matched, first = first_polygons(n, op, oq)
    key = first[perm[matched[perm]]]
    cut = np.flatnonzero(np.diff(key) != 0) + 1
    lens = np.diff(np.concatenate([[0], cut, [len(key)]]))
    return lens[lens >= min_run].sum() / len(key)


@pytest.fixture(scope="module")
def nyc_sorted(nyc):
    """(perm, the oracle's point column in the permuted numbering).  A wave of the split
    kernel holds points 8 apart, so a run of 128 equal points gives count_add 16 equal lanes:
    above kCountFewLanes = 8, the butterfly sum."""
    c, d, x, y, op, oq = nyc
    n = len(x)
    perm = sorted_order(n, op, oq)
    assert share_in_long_runs(perm, n, op, oq) >= 0.5
    assert share_in_long_runs(np.arange(n), n, op, oq) == 0  # (the fixture's own order has no such run)
    matched, _ = first_polygons(n, op, oq)
    inside = perm[:7 * (matched.sum() // 6)]
    assert (~matched[inside]).sum() >= len(inside) // 7 - 1  # the unmatched points inside the runs
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    return perm, inv[op]


@pytest.fixture(scope="module")
def nyc_truth(nyc, nyc_sorted):
    """(order, column) -> (x, y, w, ids, count, sum), each computed once.  With x' = x[perm],
    y' = y[perm] and a column w' given in the new order, the counts are unchanged and the
    sums are those of w' over the renumbered pairs."""
    c, d, x, y, op, oq = nyc
    perm, op_sorted = nyc_sorted
    xs, ys = x[perm], y[perm]
    cache = {}

    def get(order, name):
        if (order, name) not in cache:
            w = weight_column(name, len(x))
            ids, cnt, sm = truth(c, op if order == "random" else op_sorted, oq, w)
            if name in ("uniform", "all_max"):  # some true sums lie outside int64: they wrap
                wide = np.zeros(len(ids))
                np.add.at(wide, np.searchsorted(ids, oq), w[op if order == "random" else op_sorted].astype(np.float64))
                assert (np.abs(wide) > 2.0 ** 63 * 1.01).sum() > 20
            cache[order, name] = (x, y, w, ids, cnt, sm) if order == "random" else (xs, ys, w, ids, cnt, sm)
        return cache[order, name]
    return get


@pytest.mark.parametrize("order", ["random", "sorted"])
@pytest.mark.parametrize("lds", LDS)
@pytest.mark.parametrize("pipeline", PIPELINES)
def test_count_full_range_weights(gpu, nyc, nyc_truth, pipeline, lds, order):
    """Sums that wrap, weights at both ends of int64, carries out of a full low word, in the
    fixture's random order (a few equal lanes per wave: the lane-by-lane 64-bit reads) and
    sorted by polygon (many equal lanes: wave_sum_u64)."""
    d = nyc[1]
    for name in COLUMNS:
        x, y, w, ids, cnt, sm = nyc_truth(order, name)
        r = run(gpu, d, x, y, 9, w=w, pipeline=pipeline, lds=lds)
        assert r.stats["pipeline"] == pipeline
        check(r, ids, cnt, sm)


@pytest.fixture(scope="module")
def five_squares_dense(gpu):
    """The five overlapping squares at a place and size where the table gets a dense grid and
    a pixel index (the unit squares at the origin get neither, so every pipeline forced on
    them is the fused one)."""
    sq = [(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0), (0.0, 0.0)]
    polys = [(pid, [[[(-74.0 + 0.2 * u * (1 + 0.01 * pid), 40.7 + 0.2 * v * (1 + 0.01 * pid)) for u, v in sq]]])
             for pid in (5, 3, 9, 1, 7)]
    c = M.tessellate(M.Polygons.from_lists(polys), M.H3IndexSystem(), 7)
    rng = np.random.default_rng(9)
    x = -74.0 + 0.2 * rng.uniform(0.05, 0.95, 50_000)
    y = 40.7 + 0.2 * rng.uniform(0.05, 0.95, 50_000)
    op, oq = oracle_join(c, x, y, res=7)
    assert len(op) >= 5 * len(x) - 5
    return c, c.upload(), x, y, op, oq


@pytest.mark.parametrize("where", ["origin", "dense"])
def test_count_full_range_weights_five_matches_per_point(gpu, five_squares, five_squares_dense, where):
    """Every point matches the same five polygons: all 64 lanes of a wave are equal in every
    round -- of the fused kernel's records and, on the table with a pixel index, of
    count_answer's loop over the match mask in the split and binned kernels."""
    c, d, x, y, op, oq = five_squares if where == "origin" else five_squares_dense
    res = 5 if where == "origin" else 7
    n = len(x)
    perm = sorted_order(n, op, oq)
    assert share_in_long_runs(perm, n, op, oq) > 0.99
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    w = weight_column("uniform", n)
    ids, cnt, sm = truth(c, inv[op], oq, w)
    assert (cnt >= n - 5).all()
    for pipeline in PIPELINES:
        for lds in LDS:
            r = run(gpu, d, x[perm], y[perm], res, w=w, pipeline=pipeline, lds=lds)
            assert r.stats["pipeline"] == (pipeline if where == "dense" else 0)
            check(r, ids, cnt, sm)


# ---------------------------------------------------------------- 11: a capped grid (count_groups)

GROUPS = [1, 3, 65536]


@pytest.mark.parametrize("lds", LDS)
@pytest.mark.parametrize("pipeline", PIPELINES)
@pytest.mark.parametrize("groups", GROUPS)
def test_count_capped_grid(gpu, nyc, nyc_truth, groups, pipeline, lds):
    """The resident grid's stride loops, which a test-sized batch never repeats on a whole
    device: with one workgroup the split kernel's takes all 74 chunks and each of the fused
    kernel's four waves every fourth of the 19 groups of 64 tiles; with three the binned
    kernel's runs are 25, 25 and 24 chunks.  The LDS histogram is carried across all of them
    to the one flush."""
    d = nyc[1]
    x, y, w, ids, cnt, sm = nyc_truth("random", "uniform")
    n = len(x)
    assert -(-n // 4096) == 74 and -(-n // (64 * N.lib().mgpu_join_tile_points())) == 19
    opts = {"count_groups": groups}
    r = run(gpu, d, x, y, 9, w=w, pipeline=pipeline, lds=lds, opts=opts)
    assert r.stats["pipeline"] == pipeline
    check(r, ids, cnt, sm)
    check(run(gpu, d, x, y, 9, pipeline=pipeline, lds=lds, opts=opts), ids, cnt, None)
    assert M.default_context(gpu).get_option("count_groups") == 0


@pytest.mark.parametrize("pipeline", PIPELINES)
def test_count_one_group_sorted_full_range(gpu, nyc, nyc_truth, pipeline):
    """The stride loops and the full-width merged sums together."""
    x, y, w, ids, cnt, sm = nyc_truth("sorted", "uniform")
    r = run(gpu, nyc[1], x, y, 9, w=w, pipeline=pipeline, opts={"count_groups": 1})
    assert r.stats["pipeline"] == pipeline
    check(r, ids, cnt, sm)


@pytest.mark.parametrize("pipeline", PIPELINES)
def test_count_one_group_hash_table(gpu, tracts, pipeline):
    """One workgroup, so one hash table of 4096 entries and 8 probes, meets all 3000 slots:
    additions that find their entry are mixed with ones that give up and go to global
    atomics."""
    c, d, x, y, op, oq = tracts
    w = weight_column("uniform", len(x))
    ids, cnt, sm = truth(c, op, oq, w)
    assert (cnt > 0).sum() > 2900
    opts = {"count_groups": 1}
    r = run(gpu, d, x, y, 10, w=w, pipeline=pipeline, lds=1000, opts=opts)
    assert r.stats["pipeline"] == pipeline
    check(r, ids, cnt, sm)
    check(run(gpu, d, x, y, 10, pipeline=pipeline, lds=1000, opts=opts), ids, cnt, None)


def test_count_groups_option_range(gpu):
    ctx = M.default_context(gpu)
    assert ctx.get_option("count_groups") == 0
    for bad in (-1, 65537):
        with pytest.raises(M.IllegalArgumentException):
            ctx.set_option("count_groups", bad)
    assert ctx.get_option("count_groups") == 0
    with ctx.options(count_groups=65536):
        assert ctx.get_option("count_groups") == 65536
    assert ctx.get_option("count_groups") == 0


# ---------------------------------------------------------------- 12: the id -> slot lookups

def remap_ids(name, pid):
    pid = pid.astype(np.int64)
    if name == "dense_global":  # 8, 11, ..., 9005: a dense table of 8998 entries, too long for LDS
        out = 3 * pid + 5
    elif name == "search_global":  # too sparse for the dense table, more ids than LDS stages
        out = -1000 * pid
        out[pid == 3000] = -2 ** 31
    else:
        assert name == "contiguous_negative"
        out = pid - 5000
    return out.astype(np.int32)


@pytest.fixture(scope="module", params=["dense_global", "search_global", "contiguous_negative"])
def remapped_tracts(request, gpu, tracts):
    c0, _, x, y, op, oq = tracts
    name = request.param
    c = M.ChipTable(c0.cell, remap_ids(name, c0.polygon_id), c0.is_core, c0.wkb_offsets, c0.wkb)
    P, ids = 3000, np.unique(c.polygon_id).astype(np.int64)
    span = ids[-1] - ids[0] + 1
    stage_max, dense = 2048, span <= 16 * P + 1024  # kCountStageMax; poly_slots_dense
    assert len(ids) == P
    if name == "dense_global":
        assert span > P and dense and span > stage_max
    elif name == "search_global":
        assert not dense and P > stage_max and ids[0] == -2 ** 31
    else:
        assert span == P and ids[0] == -4999
    w = weight_column("uniform", len(x))
    return name, c.upload(), x, y, w, truth(c, op, remap_ids(name, oq), w)


@pytest.mark.parametrize("lds", LDS + [1000])
@pytest.mark.parametrize("pipeline", PIPELINES)
def test_count_lookup_variants(gpu, remapped_tracts, pipeline, lds):
    """The 3000 tracts under other ids: the dense table and the binary search read from
    global memory (their lookups are too long to stage in LDS, and the hash table of
    count_lds_slots = 1000 never stages), and contiguous ids with a negative minimum."""
    name, d, x, y, w, (ids, cnt, sm) = remapped_tracts
    assert np.array_equal(d.polygons(), ids) and (np.diff(ids.astype(np.int64)) > 0).all()
    r = run(gpu, d, x, y, 10, w=w, pipeline=pipeline, lds=lds)
    assert r.stats["pipeline"] == pipeline
    check(r, ids, cnt, sm)


# ---------------------------------------------------------------- 13: unaligned weight columns

def weight_tensor(gpu, w, aligned):
    """The column on the device, 16-byte aligned or starting 8 bytes past such an address
    (a contiguous view from element 1)."""
    if aligned:
        wt = torch.from_numpy(w).to(gpu)
    else:
        wt = torch.empty(len(w) + 1, dtype=torch.int64, device=gpu)[1:]
        wt.copy_(torch.from_numpy(w))
    assert wt.is_contiguous() and wt.data_ptr() % 16 == (0 if aligned else 8)
    return wt


@pytest.mark.parametrize("pipeline", PIPELINES)
@pytest.mark.parametrize("n", [1, 7, 8, 9, 4095, 4096, 4097, 12_289])
def test_count_unaligned_weights(gpu, nyc, n, pipeline):
    """The split kernel reads 8 weights per thread: two 16-byte loads when the column is
    aligned and the 8 are whole, scalar loads otherwise."""
    c, d, x, y, op, oq = nyc
    k = np.searchsorted(op, n)
    w = weight_column("uniform", n)
    ids, cnt, sm = truth(c, op[:k], oq[:k], w)
    for aligned in (False, True):
        r = run(gpu, d, x[:n], y[:n], 9, wt=weight_tensor(gpu, w, aligned), pipeline=pipeline)
        assert r.stats["pipeline"] == pipeline
        check(r, ids, cnt, sm)


@pytest.fixture(scope="module")
def london3(gpu):
    import bench_workloads as W
    c = M.tessellate(W.london_districts(), M.BNGIndexSystem(), 3)
    x, y = W.london_points(4097, 43)
    x, y = np.asarray(x), np.asarray(y)
    op, oq = oracle_join(c, x, y, res=3, isys=1)
    assert len(np.unique(op[op < 3])) == 3  # (the smallest case has pairs)
    return c, c.upload(), x, y, op, oq


@pytest.mark.parametrize("n", [3, 4, 5, 4097])
def test_count_unaligned_weights_bng_split(gpu, london3, n):
    """BNG codes are 4 bytes: 4 per 16-byte load, so 4 weights per thread."""
    c, d, x, y, op, oq = london3
    k = np.searchsorted(op, n)
    w = weight_column("uniform", n)
    ids, cnt, sm = truth(c, op[:k], oq[:k], w)
    for aligned in (False, True):
        r = run(gpu, d, x[:n], y[:n], 3, isys=M.BNGIndexSystem(), wt=weight_tensor(gpu, w, aligned), pipeline=1,
                opts={"bng_split": 1})
        assert r.stats["pipeline"] == 1
        check(r, ids, cnt, sm)


# ---------------------------------------------------------------- 14: accumulate onto prior contents

def test_count_accumulate_onto_contents(gpu, nyc, nyc_truth):
    c, d, x, y, op, oq = nyc
    _, _, w, ids, cnt, sm = nyc_truth("random", "uniform")
    n, h, P = len(x), 123_457, len(ids)
    rng = np.random.default_rng(141)
    pre = rng.integers(I64.min, I64.max, (2, P), dtype=np.int64, endpoint=True)
    busy = np.argsort(cnt)[-2:]
    pre[0][busy] = I64.max, -1  # counts that wrap too: past INT64_MAX, and a carry through every bit
    want = [(pre[0].view(np.uint64) + cnt.view(np.uint64)).view(np.int64),
            (pre[1].view(np.uint64) + sm.view(np.uint64)).view(np.int64)]
    assert want[0][busy[0]] < 0 and want[0][busy[1]] == cnt[busy[1]] - 1 > 0
    out = (torch.from_numpy(pre[0].copy()).to(gpu), torch.from_numpy(pre[1].copy()).to(gpu))
    run(gpu, d, x[:h], y[:h], 9, w=w[:h], out=out, accumulate=True)
    run(gpu, d, x[h:], y[h:], 9, w=w[h:], out=out, accumulate=True)
    assert np.array_equal(out[0].cpu().numpy(), want[0]) and np.array_equal(out[1].cpu().numpy(), want[1])
    # the same call without accumulate overwrites both arrays
    r = run(gpu, d, x[h:], y[h:], 9, w=w[h:], out=out)
    k = np.searchsorted(op, h)
    _, cnt_h, sm_h = truth(c, op[k:] - h, oq[k:], w[h:])
    assert r.count.data_ptr() == out[0].data_ptr() and r.sum.data_ptr() == out[1].data_ptr()
    assert np.array_equal(out[0].cpu().numpy(), cnt_h) and np.array_equal(out[1].cpu().numpy(), sm_h)

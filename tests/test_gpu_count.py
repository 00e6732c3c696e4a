"""mgpu_pip_join_count on the GPU: per-polygon counts and integer sums equal, exactly, what
np.add.at gives over the oracle's pairs for the same table and points -- in the split,
fused and binned pipelines, with the LDS histograms (the default) and with global atomics
(count_lds_slots = 0), for dense, negative and sparse polygon ids."""
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
    """(ids, count, sum) from the oracle's pairs."""
    ids = np.unique(c.polygon_id)
    slot = np.searchsorted(ids, oq)
    cnt = np.zeros(len(ids), np.int64)
    np.add.at(cnt, slot, 1)
    sm = None
    if w is not None:
        sm = np.zeros(len(ids), np.int64)
        np.add.at(sm, slot, w[op])
    return ids.astype(np.int32), cnt, sm


def run(gpu, d, x, y, res, isys=None, w=None, pipeline=None, lds=None, **kw):
    opts = {}
    if pipeline is not None:
        opts["pipeline"] = pipeline
    if lds is not None:
        opts["count_lds_slots"] = lds
    wt = None if w is None else torch.from_numpy(w).to(gpu)
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


def test_count_five_overlapping_polygons(gpu):
    sq = [(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0), (0.0, 0.0)]
    polys = [(pid, [[[(x * (1 + 0.01 * pid), y * (1 + 0.01 * pid)) for x, y in sq]]]) for pid in (5, 3, 9, 1, 7)]
    c = M.tessellate(M.Polygons.from_lists(polys), M.H3IndexSystem(), 5)
    rng = np.random.default_rng(8)
    x = rng.uniform(0.05, 0.95, 50_000)
    y = rng.uniform(0.05, 0.95, 50_000)
    op, oq = oracle_join(c, x, y, res=5)
    assert len(op) > 4 * len(x)
    w = weights(len(x))
    ids, cnt, sm = truth(c, op, oq, w)
    d = c.upload()
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
@pytest.mark.parametrize("pipeline", [None, 0, 2])
def test_count_3000_tracts(gpu, tracts, pipeline, lds):
    """3000 polygons: LDS histograms by default; with count_lds_slots = 1000 the table has
    more polygons than slots and the workgroups keep an LDS hash table of 4096 entries in
    front of the global atomics (full enough here that some additions miss it); 0: global
    atomics only."""
    c, d, x, y, op, oq = tracts
    w = weights(len(x))
    ids, cnt, sm = truth(c, op, oq, w)
    assert len(ids) == 3000
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

"""CellAggregate on the GPU (mgpu_cell_agg_*): per-cell counts and integer sums equal,
exactly, np.unique(cells, return_counts=True) and np.add.at on the uint64 view over the
oracle's cells -- through the LDS table and the direct path, across batches, table growth
(keys first), arbitrary int64 keys, validity bitmaps, the fetch's capacity protocol and
add_counted."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mosaic_amd as M
import oracle as O
from mosaic_amd import _native as N
from conftest import GOLDEN
from geom_util import nyc_points

pytestmark = pytest.mark.gpu

H3 = M.H3IndexSystem()
BNG = M.BNGIndexSystem()
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1


def F(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def L(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)


def unaligned(a, dev):
    """`a` as a device view 8 bytes past a 16-byte boundary (a tensor sliced at +1)."""
    t = torch.empty(len(a) + 1, dtype=torch.int64, device=dev)
    t[1:] = torch.from_numpy(a)
    v = t[1:]
    assert v.data_ptr() % 16 == 8
    return v


def truth(cells, w=None):
    """(cells ascending, counts, sums); the sums in unsigned arithmetic, so that they wrap
    modulo 2^64 whatever numpy does on signed overflow."""
    cells = np.asarray(cells, np.int64)
    u, inv, cnt = np.unique(cells, return_inverse=True, return_counts=True)
    sm = None
    if w is not None:
        assert w.dtype == np.int64
        sm = np.zeros(len(u), np.int64)
        np.add.at(sm.view(np.uint64), inv.reshape(-1), w.view(np.uint64))
    return u, cnt.astype(np.int64), sm


def check(r, ref):
    u, cnt, sm = ref
    assert r.cell.dtype == torch.int64 and r.count.dtype == torch.int64
    cell = r.cell.cpu().numpy()
    assert np.all(cell[1:] > cell[:-1])  # ascending as signed int64, distinct
    assert np.array_equal(cell, u)
    assert np.array_equal(r.count.cpu().numpy(), cnt)
    if sm is None:
        assert r.sum is None
    else:
        assert r.sum.dtype == torch.int64 and np.array_equal(r.sum.cpu().numpy(), sm)


def same(a, b):
    assert torch.equal(a.cell, b.cell) and torch.equal(a.count, b.count)
    assert (a.sum is None) == (b.sum is None) and (a.sum is None or torch.equal(a.sum, b.sum))


@pytest.fixture(scope="module")
def nyc():
    x, y = nyc_points(200_000, 1)
    return x, y, {r: O.h3_points_to_cells(x, y, r) for r in (6, 9)}


# ---------------------------------------------------------------- 1: H3, LDS and direct path

@pytest.mark.parametrize("res,lds", [(9, 1), (6, 1), (9, 0)])
def test_h3_nyc(gpu, nyc, res, lds):
    """r9: more distinct cells than one LDS table holds (both paths run); r6: a few dozen
    cells, all in LDS; cellagg_lds = 0: every addition goes to the global table."""
    x, y, cells = nyc
    ref = truth(cells[res])
    assert (len(ref[0]) > 4096) if res == 9 else (len(ref[0]) < 100)
    with M.default_context(gpu).options(cellagg_lds=lds):
        r = M.grid_cellcount(F(x, gpu), F(y, gpu), res)
    check(r, ref)
    assert int(r.count.sum()) == len(x)


# ---------------------------------------------------------------- 2: near-ties

@pytest.mark.parametrize("libm,column", [(0, "cell_glibc"), (1, "cell_cr")])
def test_near_ties(gpu, libm, column):
    f = np.load(os.path.join(GOLDEN, "h3_edge_points.npz"))
    lon, lat, res = f["lon"], f["lat"], f["res"]
    with M.default_context(gpu).options(h3_libm=libm):
        for r in np.unique(res):
            m = res == r
            got = M.grid_cellcount(F(lon[m], gpu), F(lat[m], gpu), int(r))
            check(got, truth(f[column][m].view(np.int64)))


# ---------------------------------------------------------------- 3: BNG, failing calls

def london_bounds():
    z = M.Polygons.from_npz(os.path.join(GOLDEN, "london_postcode_zones.npz"))
    xy = np.asarray(z.xy).reshape(-1, 2)
    return xy[:, 0].min(), xy[:, 1].min(), xy[:, 0].max(), xy[:, 1].max()


def failure(call):
    with pytest.raises(N.MosaicGpuError) as e:
        call()
    return type(e.value), e.value.code, str(e.value)


def test_bng_london_and_invalid_coordinates(gpu):
    x0, y0, x1, y1 = london_bounds()
    rng = np.random.default_rng(3)
    n = 100_000
    x, y = np.round(rng.uniform(x0, x1, n), 2), np.round(rng.uniform(y0, y1, n), 2)
    ref = truth(O.bng_points_to_cells(x, y, 4))
    agg = M.CellAggregate(BNG, 4)
    agg.add_points(F(x, gpu), F(y, gpu))
    check(agg.result(), ref)
    bad = x.copy()
    bad[n // 2] = np.nan
    want = failure(lambda: M.grid_longlatascellid(F(bad, gpu), F(y, gpu), 4, index_system=BNG))
    assert failure(lambda: agg.add_points(F(bad, gpu), F(y, gpu))) == want
    assert want[0] is N.IllegalStateException and want[1] == N.MGPU_E_NAN
    assert len(agg) == len(ref[0])
    check(agg.result(), ref)
    agg.close()


def test_h3_invalid_latitude(gpu, nyc):
    x, y, cells = nyc
    x, y = x[:50_000], y[:50_000]
    ref = truth(cells[9][:50_000])
    agg = M.CellAggregate(H3, 9)
    agg.add_points(F(x, gpu), F(y, gpu))
    bad = y.copy()
    bad[12345] = np.nan
    want = failure(lambda: M.grid_longlatascellid(F(x, gpu), F(bad, gpu), 9))
    assert failure(lambda: agg.add_points(F(x, gpu), F(bad, gpu))) == want
    assert want[0] is N.IllegalArgumentException
    assert len(agg) == len(ref[0])
    check(agg.result(), ref)
    # a latitude of 91 is no error for grid_longlatascellid (H3 folds it over the pole): the
    # aggregate takes the same cells
    bad[12345] = 91.0
    cells91 = M.grid_longlatascellid(F(x, gpu), F(bad, gpu), 9).cpu().numpy()
    assert np.array_equal(cells91, O.h3_points_to_cells(x, bad, 9))
    agg.clear()
    agg.add_points(F(x, gpu), F(bad, gpu))
    check(agg.result(), truth(cells91))
    agg.close()


# ---------------------------------------------------------------- 4: weights

def test_weights_wrap_unaligned_and_refusals(gpu, nyc):
    x, y, cells = nyc
    rng = np.random.default_rng(4)
    w = rng.integers(I64_MIN, I64_MAX, len(x), endpoint=True)
    for res in (9, 6):  # (r6: thousands of full-range weights per cell: the sums wrap)
        ref = truth(cells[res], w)
        for wt in (L(w, gpu), unaligned(w, gpu)):
            check(M.grid_cellcount(F(x, gpu), F(y, gpu), res, weight=wt), ref)
    xs, ys, ws = F(x[:1000], gpu), F(y[:1000], gpu), L(w[:1000], gpu)
    plain, summed = M.CellAggregate(H3, 9), M.CellAggregate(H3, 9, with_sum=True)
    c = L(cells[9][:1000], gpu)
    for call in (lambda: plain.add_points(xs, ys, weight=ws), lambda: summed.add_points(xs, ys),
                 lambda: plain.add_cells(c, weight=ws), lambda: summed.add_cells(c),
                 lambda: plain.add_counted(c, torch.ones_like(c), ws), lambda: summed.add_counted(c, torch.ones_like(c))):
        kind, code, _ = failure(call)
        assert kind is N.IllegalArgumentException and code == N.MGPU_E_INVALID_ARG
    assert len(plain) == 0 and len(summed) == 0
    plain.close()
    summed.close()


# ---------------------------------------------------------------- 5: streaming

def test_streaming_batches(gpu, nyc):
    x, y, cells = nyc
    rng = np.random.default_rng(5)
    w = rng.integers(I64_MIN, I64_MAX, len(x), endpoint=True)
    xs, ys, ws = F(x, gpu), F(y, gpu), L(w, gpu)
    cuts = [0, 4097, 70_001, 150_000]
    agg = M.CellAggregate(H3, 9, with_sum=True)
    for a, b in zip(cuts[:-1], cuts[1:]):
        agg.add_points(xs[a:b], ys[a:b], weight=ws[a:b])
    one = M.CellAggregate(H3, 9, with_sum=True)
    one.add_points(xs[:150_000], ys[:150_000], weight=ws[:150_000])
    r1, r2 = agg.result(), agg.result()
    same(r1, r2)
    same(r1, one.result())
    check(r1, truth(cells[9][:150_000], w[:150_000]))
    agg.add_points(xs[150_000:], ys[150_000:], weight=ws[150_000:])  # adding after result() continues
    check(agg.result(), truth(cells[9], w))
    agg.clear()
    assert len(agg) == 0
    agg.add_points(xs[150_000:], ys[150_000:], weight=ws[150_000:])
    check(agg.result(), truth(cells[9][150_000:], w[150_000:]))
    agg.close()
    one.close()


# ---------------------------------------------------------------- 6: capped grid

@pytest.mark.parametrize("equal", [False, True])
def test_one_workgroup_strides(gpu, equal):
    """cellagg_groups = 1: one workgroup carries its LDS table over six chunks (a ragged
    tail); 6000 distinct keys overflow the table (4096 entries) into the direct path."""
    rng = np.random.default_rng(6)
    n = 5 * 4096 + 17
    pool = np.unique(rng.integers(I64_MIN, I64_MAX, 6000, endpoint=True))
    assert len(pool) == 6000
    keys = np.full(n, pool[17]) if equal else np.concatenate([pool, rng.choice(pool, n - 6000)])
    w = rng.integers(I64_MIN, I64_MAX, n, endpoint=True)
    for with_sum in (False, True):
        agg = M.CellAggregate(H3, 9, with_sum=with_sum)
        with M.default_context(gpu).options(cellagg_groups=1):
            agg.add_cells(L(keys, gpu), weight=L(w, gpu) if with_sum else None)
        r = agg.result()
        check(r, truth(keys, w if with_sum else None))
        if equal:
            assert len(agg) == 1 and int(r.count[0]) == n
        agg.close()


# ---------------------------------------------------------------- 7: growth

def test_growth_keys_first(gpu):
    """initial_cells = 1: the floor of 1024 entries; 300,000 distinct keys need 2^20 entries
    at a load of 1/2 -- ten doublings, every one found by the keys-first pass.  The same data
    on a table created large enough takes the single pass."""
    rng = np.random.default_rng(7)
    keys = rng.integers(I64_MIN, I64_MAX, 300_000, endpoint=True)
    w = rng.integers(I64_MIN, I64_MAX, len(keys), endpoint=True)
    ref = truth(keys, w)
    assert len(ref[0]) > 299_000
    grown, sized = M.CellAggregate(H3, 9, True, initial_cells=1), M.CellAggregate(H3, 9, True, initial_cells=1_000_000)
    for agg in (grown, sized):
        agg.add_cells(L(keys, gpu), weight=L(w, gpu))
    rg, rs = grown.result(), sized.result()
    check(rg, ref)
    same(rg, rs)
    # growth across batches, with and without the LDS table
    for lds in (1, 0):
        agg = M.CellAggregate(H3, 9, True, initial_cells=1)
        with M.default_context(gpu).options(cellagg_lds=lds):
            for a in range(0, len(keys), 100_000):
                agg.add_cells(L(keys[a:a + 100_000], gpu), weight=L(w[a:a + 100_000], gpu))
        same(agg.result(), rg)
        agg.close()
    grown.close()
    sized.close()


# ---------------------------------------------------------------- 7b: binned columns

@pytest.mark.parametrize("with_sum", [False, True])
def test_binned_columns(gpu, nyc, with_sum):
    """cellagg_bin_min = 1: every column without a bitmap is a candidate for the binning in
    front of the accumulation (by default only columns of 2^22 cells are).  Columns with
    more distinct cells than an LDS table are binned (an odd length: the binned weights'
    offset), columns with few are not, a table at its floor grows under it; all equal
    numpy and the unbinned result."""
    x, y, cells = nyc
    rng = np.random.default_rng(17)
    w = rng.integers(I64_MIN, I64_MAX, len(x), endpoint=True)
    n = 150_001
    wt = (lambda a, b: L(w[a:b], gpu)) if with_sum else (lambda a, b: None)
    wr = w if with_sum else None
    with M.default_context(gpu).options(cellagg_bin_min=1):
        for res in (9, 6):
            agg = M.CellAggregate(H3, res, with_sum, initial_cells=1)
            agg.add_points(F(x[:n], gpu), F(y[:n], gpu), weight=wt(0, n))
            check(agg.result(), truth(cells[res][:n], None if wr is None else wr[:n]))
            agg.add_points(F(x[n:], gpu), F(y[n:], gpu), weight=wt(n, len(x)))  # (the aggregate now knows its cells)
            check(agg.result(), truth(cells[res], wr))
            agg.close()
        keys = np.concatenate([rng.integers(I64_MIN, I64_MAX, 30_000, endpoint=True), [-1, -1, 0, I64_MIN]])
        keys = np.concatenate([keys, rng.choice(keys, 70_003)])
        agg = M.CellAggregate(H3, 9, with_sum, initial_cells=1)
        agg.add_cells(unaligned(keys, gpu), weight=unaligned(w[:len(keys)], gpu) if with_sum else None)
        with M.default_context(gpu).options(cellagg_groups=3):
            agg.add_cells(L(keys, gpu), weight=wt(0, len(keys)))
        k2 = np.concatenate([keys, keys])
        check(agg.result(), truth(k2, np.concatenate([w[:len(keys)]] * 2) if with_sum else None))
        agg.close()


# ---------------------------------------------------------------- 8: arbitrary keys, order

def test_arbitrary_keys_signed_order(gpu):
    rng = np.random.default_rng(8)
    special = np.array([0, -1, I64_MIN, I64_MAX], np.int64)
    reps = [3, 5, 2, 7]
    rand = rng.integers(I64_MIN, I64_MAX, 20_000, endpoint=True)
    assert all(len(np.unique((rand.view(np.uint64) >> np.uint64(8 * b)) & np.uint64(255))) == 256 for b in range(8))
    assert (rand < 0).any() and (rand > 0).any()
    keys = np.concatenate([np.repeat(special, reps), rand, rand[:5000]])
    rng.shuffle(keys)
    w = rng.integers(I64_MIN, I64_MAX, len(keys), endpoint=True)
    for lds in (1, 0):
        agg = M.CellAggregate(H3, 9, with_sum=True)
        with M.default_context(gpu).options(cellagg_lds=lds):
            agg.add_cells(L(keys, gpu), weight=L(w, gpu))
        r = agg.result()
        check(r, truth(keys, w))
        cell, cnt = r.cell.cpu().numpy(), r.count.cpu().numpy()
        assert cell[0] == I64_MIN and cell[-1] == I64_MAX
        for k, c in zip(special, reps):
            i = np.searchsorted(cell, k)
            assert cell[i] == k and cnt[i] >= c and cnt[i] == (keys == k).sum()
        agg.close()


# ---------------------------------------------------------------- 9: validity

def test_validity_bitmap_at_an_offset(gpu):
    rng = np.random.default_rng(9)
    n, off = 3 * 4096 + 1001, 3
    pool = rng.integers(I64_MIN, I64_MAX, 5000, endpoint=True)
    keys = rng.choice(pool, n)
    ok = rng.random(n) > 1 / 3
    keys[~ok] = rng.integers(I64_MIN, I64_MAX, int((~ok).sum()), endpoint=True)  # garbage in the null rows
    keys[np.nonzero(~ok)[0][:10]] = -1
    keys[np.nonzero(ok)[0][:4]] = -1
    w = rng.integers(I64_MIN, I64_MAX, n, endpoint=True)
    bits = np.concatenate([rng.random(off) > 0.5, ok, rng.random(11) > 0.5])
    bm = torch.from_numpy(np.packbits(bits, bitorder="little")).to(gpu)
    agg = M.CellAggregate(BNG, 4, with_sum=True)
    agg.add_cells(unaligned(keys, gpu), weight=L(w, gpu), valid=bm, valid_offset=off)
    ref = truth(keys[ok], w[ok])
    check(agg.result(), ref)
    none = torch.zeros((n + off + 7) // 8, dtype=torch.uint8, device=gpu)
    agg.add_cells(L(keys, gpu), weight=L(w, gpu), valid=none, valid_offset=off)
    check(agg.result(), ref)
    empty = M.CellAggregate(BNG, 4)
    empty.add_cells(L(keys, gpu), valid=none, valid_offset=off)
    assert len(empty) == 0
    agg.close()
    empty.close()


# ---------------------------------------------------------------- 10: fetch capacity, raw ABI

def test_fetch_capacity_raw(gpu):
    rng = np.random.default_rng(10)
    keys = rng.choice(rng.integers(I64_MIN, I64_MAX, 3000, endpoint=True), 10_000)
    w = rng.integers(I64_MIN, I64_MAX, len(keys), endpoint=True)
    u, cnt, sm = truth(keys, w)
    D = len(u)
    agg = M.CellAggregate(H3, 9, with_sum=True)
    agg.add_cells(L(keys, gpu), weight=L(w, gpu))
    lib, ctx = N.lib(), agg.ctx.handle
    SENT = 0x5A5A5A5A5A5A5A5A
    out = [torch.full((D,), SENT, dtype=torch.int64, device=gpu) for _ in range(3)]
    got = ctypes.c_int64(-1)
    st = lib.mgpu_cell_agg_fetch(ctx, agg.handle, D - 1, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                 ctypes.byref(got), None)
    assert st == N.MGPU_E_CAPACITY and got.value == D
    assert all(bool((t == SENT).all()) for t in out)
    with pytest.raises(N.CapacityError) as e:
        N.check(st, required=got.value)
    assert e.value.required == D
    # out_sum is NULL exactly when the aggregate has no sum
    assert lib.mgpu_cell_agg_fetch(ctx, agg.handle, D, out[0].data_ptr(), out[1].data_ptr(), None, ctypes.byref(got),
                                   None) == N.MGPU_E_INVALID_ARG
    assert all(bool((t == SENT).all()) for t in out)
    got = ctypes.c_int64(-1)
    assert lib.mgpu_cell_agg_fetch(ctx, agg.handle, D, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                   ctypes.byref(got), None) == N.MGPU_OK
    assert got.value == D
    check(M.CellCounts(*out), (u, cnt, sm))
    size = ctypes.c_int64(-1)
    assert lib.mgpu_cell_agg_size(ctx, agg.handle, ctypes.byref(size), None) == N.MGPU_OK and size.value == D
    agg.close()


# ---------------------------------------------------------------- 11: add_counted

def test_add_counted_reload_and_merge(gpu, nyc):
    x, y, cells = nyc
    rng = np.random.default_rng(11)
    w = rng.integers(I64_MIN, I64_MAX, len(x), endpoint=True)
    a = M.CellAggregate(H3, 9, with_sum=True)
    a.add_points(F(x, gpu), F(y, gpu), weight=L(w, gpu))
    a.add_cells(L([-1, -1, 0], gpu), weight=L([5, 6, 7], gpu))  # (the marker's side record travels too)
    ra = a.result()
    b = M.CellAggregate(H3, 9, with_sum=True)
    b.add_counted(ra.cell, ra.count, ra.sum)
    b.add_counted(ra.cell, ra.count, ra.sum)
    rb = b.result()
    assert torch.equal(rb.cell, ra.cell) and torch.equal(rb.count, 2 * ra.count) and torch.equal(rb.sum, 2 * ra.sum)
    # a record of count 0 creates no cell
    b.add_counted(L([123456789, -1, ra.cell[0].item()], gpu), L([0, 0, 0], gpu), L([9, 9, 9], gpu))
    same(b.result(), rb)
    c = M.CellAggregate(H3, 9)
    c.add_counted(L([7, 7, 8, -1, 9], gpu), L([2, 3, 0, 4, 1], gpu))
    check(c.result(), (np.array([-1, 7, 9]), np.array([4, 5, 1]), None))
    for agg in (a, b, c):
        agg.close()


# ---------------------------------------------------------------- 12: n == 0

@pytest.mark.parametrize("with_sum", [False, True])
def test_empty(gpu, with_sum):
    agg = M.CellAggregate(H3, 9, with_sum=with_sum)
    e64 = torch.empty(0, dtype=torch.int64, device=gpu)
    e_f = torch.empty(0, dtype=torch.float64, device=gpu)
    wt = e64 if with_sum else None
    agg.add_points(e_f, e_f, weight=wt)
    agg.add_cells(e64, weight=wt)
    agg.add_counted(e64, e64, wt)
    assert len(agg) == 0
    r = agg.result()
    assert r.cell.numel() == 0 and r.count.numel() == 0 and r.cell.dtype == torch.int64 and r.count.dtype == torch.int64
    assert (r.sum.numel() == 0 and r.sum.dtype == torch.int64) if with_sum else r.sum is None
    agg.close()

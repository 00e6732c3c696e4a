"""grid_geometrykring / grid_geometrykloop on the GPU (mgpu_geometry_kring, mosaic_amd/csrc/
geom_ring.hip): the device equals the host twin byte for byte and the set oracle of
tests/geomring_util.py list by list, on the smallest shapes at which the kernels can go wrong: one
border cell, core taken out of a loop, empty lists between neighbours, offsets across waves and
workgroups, a set that overflows LDS, slabs that cut a geometry, a pentagon and its neighbours,
real chip tables, the capacity protocol and the Python surface.  Exact integers: no tolerance."""
import ctypes

import numpy as np
import pytest

import geomring_util as U
import polyfill_util as PU
import mosaic_amd as M
from mosaic_amd import _native as N

pytestmark = pytest.mark.gpu
H3, BNG = M.H3IndexSystem(), M.BNGIndexSystem()


def _triple(gpu, t):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in t)


def _device(gpu, t, k, loop, isys=H3, ctx=None):
    fn = M.grid_geometrykloop if loop else M.grid_geometrykring
    r = fn(_triple(gpu, t), k, isys, ctx=ctx)
    assert r.ids.tolist() == list(range(len(t[0]) - 1))
    return r.cells.cpu().numpy(), r.offsets.cpu().numpy()


def _check(gpu, t, k, loop, isys=H3, ctx=None):
    """device == twin, bytes and offsets; == oracle list by list."""
    cells, off = _device(gpu, t, k, loop, isys, ctx)
    last = U.last()
    tc, toff = U.twin(isys.code, *t, k, loop)
    assert np.array_equal(off, toff) and np.array_equal(cells, tc)
    for g, want in enumerate(U.oracle(isys.code, *t, k, loop)):
        assert np.array_equal(cells[off[g]:off[g + 1]], want), "geometry %d" % g
    return cells, off, last


def test_one_border_cell_is_the_sorted_cell_ring(gpu):
    import torch
    t = U.synthetic()["one_border_cell"]
    c = torch.from_numpy(t[1]).to(gpu)
    for k in (0, 1, 3):
        cells, off, _ = _check(gpu, t, k, False)
        ring, _ = M.grid_cellkring(c, k, H3)
        assert np.array_equal(cells, np.sort(ring.cpu().numpy())) and off.tolist() == [0, 3 * k * (k + 1) + 1]
    for k in (1, 3):
        cells, _, _ = _check(gpu, t, k, True)
        loop, _ = M.grid_cellkloop(c, k, H3)
        assert np.array_equal(cells, np.sort(loop.cpu().numpy())) and len(cells) == 6 * k


@pytest.mark.parametrize("k", [1, 2])
def test_core_is_removed_from_the_loop(gpu, k):
    import oracle as O
    row_off, cell, core = fat = U.synthetic()["fat"]
    cells, _, _ = _check(gpu, fat, k, True)
    got = set(cells.tolist())
    # (the core cells at distance k from a border cell are in that cell's loop, and absent)
    assert not (got & set(cell[core == 1].tolist())) and got == set(O.h3_k_loop(U.manhattan_cell(), 3 + k))
    thin = U.synthetic()["thin"]
    cells, _, _ = _check(gpu, thin, k, True)
    inner = set().union(*[O.h3_k_ring(int(b), k - 1) for b in thin[1]])
    loops = set().union(*[O.h3_k_loop(int(b), k) for b in thin[1]])
    assert loops & inner and not (set(cells.tolist()) & inner)


def test_empty_lists_between_neighbours(gpu):
    t = U.synthetic()["empty_between"]  # small, no rows, core only, small
    _, off, _ = _check(gpu, t, 1, True)
    n = np.diff(off)
    assert n[1] == 0 and n[2] == 0 and n[0] == n[3] > 0
    cells, off, _ = _check(gpu, t, 1, False)
    assert off[1] == off[2] and np.array_equal(cells[off[2]:off[3]], np.sort(t[1][t[0][2]:t[0][3]]))


@pytest.mark.parametrize("loop", [False, True], ids=["ring", "loop"])
def test_sixty_four_copies_cross_waves_and_workgroups(gpu, loop):
    t = U.synthetic()["copies"]
    cells, off, last = _check(gpu, t, 2, loop)
    n = np.diff(off)
    assert n[64] == 0 and np.all(np.delete(n, 64) == n[0]) and n[0] == (18 if loop else 37)
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(n)]))
    for g in list(range(64)) + [65, 66, 67]:
        assert np.array_equal(cells[off[g]:off[g + 1]], cells[:off[1]])
    assert last[0] == 68 and last[1] == 0 and last[2] == 1


@pytest.mark.parametrize("loop", [False, True], ids=["ring", "loop"])
def test_set_that_overflows_lds_takes_the_hbm_path(gpu, loop):
    row_off, cell, core = U.synthetic()["fat"]
    t = U.table([U.small(), (cell[core == 1], cell[core == 0]), U.small()])
    ctx = M.default_context(gpu)
    cells, off, last = _check(gpu, t, 2, loop)
    assert last[:3] == [3, 0, 1]  # three geometries on the LDS path, none on the HBM path, one slab
    with ctx.options(geomring_lds_slots=64):  # 48 cells fit; the disk's lists hold 91 (ring) / 42 + 49 (loop) distinct
        forced, foff, flast = _check(gpu, t, 2, loop, ctx=ctx)
    assert ctx.get_option("geomring_lds_slots") == 0
    assert np.array_equal(foff, off) and np.array_equal(forced, cells)
    assert flast[:3] == [2, 1, 1]


@pytest.mark.parametrize("slab", [1, 5, 18])
def test_slabs_cut_a_geometry(gpu, slab):
    row_off, cell, core = U.synthetic()["fat"]  # 18 border cells
    t = U.table([U.small(), (cell[core == 1], cell[core == 0]), U.small(), U.thin()])
    ctx = M.default_context(gpu)
    for k, loop in [(2, False), (2, True)]:
        cells, off, last = _check(gpu, t, k, loop)
        assert last[2] == 1
        with ctx.options(geomring_slab=slab):
            cut, coff, clast = _check(gpu, t, k, loop, ctx=ctx)
        assert np.array_equal(coff, off) and np.array_equal(cut, cells)
        assert clast[2] == -(-(6 + 18 + 6 + 7) // slab) > 1 and clast[1] >= 1 and clast[0] + clast[1] == 4
    assert ctx.get_option("geomring_slab") == 1 << 16


@pytest.mark.parametrize("k,loop", [(1, False), (2, False), (1, True), (2, True)])
def test_pentagon_and_its_neighbours(gpu, k, loop):
    t = U.synthetic()["pentagon"]
    cells, _, last = _check(gpu, t, k, loop)
    assert last[7] >= 6  # every border cell's walk met the pentagon and took the reference's fallback
    assert len(cells) > 0


def _check_chips(gpu, chips, k, loop, isys):
    fn = M.grid_geometrykloop if loop else M.grid_geometrykring
    r = fn(chips, k, isys)
    ids, row_off, cell, core = U.group(chips)
    assert np.array_equal(r.ids, ids) and r.ids.dtype == np.int32
    cells, off = r.cells.cpu().numpy(), r.offsets.cpu().numpy()
    tc, toff = U.twin(isys.code, row_off, cell, core, k, loop)
    assert np.array_equal(off, toff) and np.array_equal(cells, tc)
    for g, want in enumerate(U.oracle(isys.code, row_off, cell, core, k, loop)):
        assert np.array_equal(cells[off[g]:off[g + 1]], want), "geometry %d" % g
    assert [a.tolist() for a in r.lists()] == [a.tolist() for a in U.lists_of(cells, off)]


@pytest.mark.parametrize("loop", [False, True], ids=["ring", "loop"])
def test_ten_nyc_zones_r9(gpu, loop):
    _check_chips(gpu, U.nyc_chips(100, 10), 2, loop, H3)


def test_ten_london_districts_bng_res4(gpu):
    chips = U.london_chips(tuple(range(0, 180, 18)), 4)
    _check_chips(gpu, chips, 1, False, BNG)
    _check_chips(gpu, chips, 1, True, BNG)


def test_thousand_points_are_their_cells_sorted_rings(gpu):
    import torch
    rng = np.random.default_rng(7)
    x = torch.from_numpy(rng.uniform(-74.25, -73.70, 1000)).to(gpu)
    y = torch.from_numpy(rng.uniform(40.50, 40.91, 1000)).to(gpu)
    r = M.grid_geometrykring((x, y), 2, H3, resolution=9)
    ring, roff = M.grid_cellkring(M.grid_longlatascellid(x, y, 9), 2, H3)
    assert roff.cpu().tolist() == list(range(0, 19001, 19)) and r.offsets.cpu().tolist() == roff.cpu().tolist()
    assert torch.equal(r.cells.view(1000, 19), torch.sort(ring.view(1000, 19), dim=1).values)


def test_capacity_protocol(gpu):
    import torch
    t = U.synthetic()["empty_between"]
    row_off, cell, core = _triple(gpu, t)
    full, foff = U.twin(0, *t, 2, False)
    ctx = M.default_context(gpu)
    s = torch.cuda.current_stream(gpu).cuda_stream

    def call(cap):
        out = torch.full((max(cap, 1),), -1, dtype=torch.int64, device=gpu)
        off = torch.full((5,), -1, dtype=torch.int64, device=gpu)
        tot = ctypes.c_int64(-1)
        st = N.lib().mgpu_geometry_kring(ctx.handle, 0, 4, row_off.data_ptr(), cell.data_ptr(), core.data_ptr(), 2, 0,
                                         out.data_ptr() if cap else None, cap, off.data_ptr(), ctypes.byref(tot), s)
        return st, tot.value, out.cpu().numpy(), off.cpu().numpy()

    st, total, _, off = call(0)  # the size query
    assert st == N.MGPU_E_CAPACITY and total == len(full) and np.array_equal(off, foff)
    st, total, out, off = call(len(full) - 1)
    assert st == N.MGPU_E_CAPACITY and total == len(full) and np.array_equal(off, foff)
    assert np.array_equal(out, full[:-1])
    st, total, out, off = call(len(full))
    assert st == N.MGPU_OK and total == len(full) and np.array_equal(out, full) and np.array_equal(off, foff)
    for k, loop in [(-1, 0), (1025, 0), (0, 1)]:
        tot = ctypes.c_int64()
        assert N.lib().mgpu_geometry_kring(ctx.handle, 0, 4, row_off.data_ptr(), cell.data_ptr(), core.data_ptr(), k, loop,
                                           None, 0, off_buf(gpu).data_ptr(), ctypes.byref(tot), s) == N.MGPU_E_INVALID_ARG
    bad = cell.clone()
    bad[-1] = 12345
    with pytest.raises(N.IllegalArgumentException):
        M.grid_geometrykring((row_off, bad, core), 1, H3)


def off_buf(gpu):
    import torch
    return torch.zeros(5, dtype=torch.int64, device=gpu)


def test_python_surface(gpu):
    import torch
    t = U.synthetic()["empty_between"]
    for explode, plain in [(M.grid_geometrykringexplode, M.grid_geometrykring), (M.grid_geometrykloopexplode, M.grid_geometrykloop)]:
        row, cell = explode(_triple(gpu, t), 1, H3)
        r = plain(_triple(gpu, t), 1, H3)
        n = r.offsets[1:] - r.offsets[:-1]
        assert torch.equal(row, torch.repeat_interleave(torch.arange(4, device=gpu), n)) and torch.equal(cell, r.cells)
    zones = U.nyc().select([100, 101])
    batch = M.grid_geometrykring(zones, 1, H3, resolution=9)
    assert batch.ids.tolist() == sorted(zones.poly_id.tolist()) and len(batch.ids) == 2
    parts = [[[tuple(p) for p in ring] for ring in part] for part in PU.polygon_rings(zones, 0)]
    assert H3.geometry_k_ring(parts, 9, 1) == batch.lists()[0].tolist()
    loops = M.grid_geometrykloop(zones, 1, H3, resolution=9)
    assert H3.geometry_k_loop(parts, 9, 1) == loops.lists()[0].tolist()
    assert not (set(loops.lists()[0].tolist()) & set(M.grid_geometrykring(zones, 0, H3, resolution=9).lists()[0].tolist()))

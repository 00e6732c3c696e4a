"""grid_polyfill on the GPU (mgpu_grid_polyfill, mosaic_amd/csrc/polyfill.hip): the device equals
the host twin element for element, order included, and the oracle of tests/polyfill_util.py as
sets, on the smallest shapes at which the kernel can go wrong: one partial workgroup, rings over
several LDS chunks, slabs that cut polygons, holes, empty lists, offsets across waves and
workgroups, a pentagon, high latitude, BNG, the capacity path.  The certificate counter is zero
in every call; nothing forces it to fire.  The same condition as on the host comes first: no
candidate centre within 1e-9 degrees (BNG: 1e-6 m) of its polygon's boundary."""
import ctypes

import numpy as np
import pytest

import mosaic_amd as M
import polyfill_util as U
from mosaic_amd import _native as N

pytestmark = pytest.mark.gpu
H3, BNG = M.H3IndexSystem(), M.BNGIndexSystem()


def _device(polys, res, isys=H3, ctx=None):
    cells, off = M.grid_polyfill(polys, res, isys, ctx=ctx)
    assert U.last()[2:4] == [0, 1], "certificate failures / attempts: %r" % (U.last(),)
    return cells.cpu().numpy(), off.cpu().numpy()


def _check(gpu, polys, res, isys=H3, ref=None):
    """device == twin in order; == oracle as sets (H3: computed here unless given)."""
    cells, off = _device(polys, res, isys)
    tc, toff = U.twin(polys, res, isys.code)
    assert np.array_equal(off, toff) and np.array_equal(cells, tc)
    if isys is H3:
        ref = ref if ref is not None else U.h3_oracle_set(polys, res)
        assert min(r[2] for r in ref) > U.BOUNDARY_GAP_DEG
        for p, got in enumerate(U.lists_of(cells, off)):
            assert set(got.tolist()) == ref[p][0] and len(set(got.tolist())) == len(got), "polygon %d" % p
    return cells, off


def test_documented_answer_one_partial_workgroup(gpu):
    polys = U.polygons([U.DOC_WKT_PARTS])
    cells, _ = _check(gpu, polys, 0, ref=U.reference("doc", 0))
    assert sorted(cells.tolist()) == sorted([577586652210266111, 578360708396220415, 577269992861466623])
    assert 56 <= U.last()[0] <= 143 and U.last()[1] == 1
    assert sorted(H3.polyfill(U.DOC_WKT_PARTS, 0)) == sorted(cells.tolist())


def test_most_vertices_over_several_lds_chunks(gpu):
    z = U.nyc()
    nv = [z.ring_off[z.part_ring_off[z.poly_part_off[p + 1]]] - z.ring_off[z.part_ring_off[z.poly_part_off[p]]] for p in range(len(z))]
    big = int(np.argmax(nv))
    assert nv[big] > 7000 and 0 < big < len(z) - 1
    _check(gpu, z.select([big - 1, big, big + 1]), 9)


def test_slabs_cut_inside_polygons(gpu):
    polys = U.nyc().select(list(U.NYC20[:10]))
    ctx = M.default_context(gpu)
    whole, woff = _check(gpu, polys, 10, ref=U.reference("nyc20", 10)[:10])
    assert U.last()[1] > 10  # (more tiles than polygons: a slab of one tile cuts them)
    with ctx.options(polyfill_slab=256):
        cells, off = _device(polys, 10, ctx=ctx)
    assert ctx.get_option("polyfill_slab") == 1 << 24
    assert np.array_equal(off, woff) and np.array_equal(cells, whole)


def test_hole_and_empty_list_between_neighbours(gpu):
    holed = U.holed_polygon()
    polys = U.polygons([holed, U.tiny_polygon(), [holed[0][:1]]])
    _, off = _check(gpu, polys, 9)
    n = np.diff(off)
    assert n[1] == 0 and n[0] > 0 and n[2] > n[0] + 5


def test_multipolygons_with_a_hole(gpu):
    """Shell, hole, next part's shell -- the holed part first, last, and with a part inside its hole."""
    multis = U.holed_multipolygons()
    cells, off = _check(gpu, U.polygons(multis + [U.holed_polygon()]), 9)
    first, last_, inhole, holed = [set(c.tolist()) for c in U.lists_of(cells, off)]
    assert first == last_ and holed < first and holed < inhole and len(inhole) < len(first)


def test_sixty_four_copies_cross_a_wave_and_a_workgroup(gpu):
    one = U.box(-73.9912, 40.7003, -73.9801, 40.7094)
    polys = U.polygons([one] * 64 + [U.tiny_polygon()] + [one] * 3)
    ref1 = U.h3_oracle_set(U.polygons([one]), 9)[0]
    ref = [ref1] * 64 + U.h3_oracle_set(U.polygons([U.tiny_polygon()]), 9) + [ref1] * 3
    cells, off = _check(gpu, polys, 9, ref=ref)
    n = np.diff(off)
    assert n[64] == 0 and np.all(n[:64] == n[0]) and n[0] == len(ref1[0]) > 0
    assert np.array_equal(cells[off[66]:off[67]], cells[:off[1]])


def test_chunk_limits_1025_vertices_and_40_parts(gpu):
    """A ring one vertex longer than an LDS chunk, and more ring pieces than a chunk holds."""
    _check(gpu, U.polygons([U.ngon(1025), U.many_parts(40), U.ngon(2048)]), 9)


def test_offcentre_pentagon_box(gpu):
    cells, _ = _check(gpu, U.polygons([U.pentagon_box(14, 3)]), 3)
    assert int(U.CU.h3_cell(3, 14, (0, 0, 0))) in set(cells.tolist())


def test_box_at_84_north(gpu):
    _check(gpu, U.polygons([U.north_box(84)]), 4)


@pytest.mark.parametrize("res", [4, -4])
def test_bng_districts(gpu, res):
    sel = U.london_districts().select(list(range(0, 180, 18)))
    assert len(sel) == 10
    cells, off = _check(gpu, sel, res, BNG)
    for p in range(10):
        full, gap = U.bng_full(U.polygon_rings(sel, p), res)
        assert gap > U.BOUNDARY_GAP_M and set(cells[off[p]:off[p + 1]].tolist()) == full


def test_capacity_path(gpu):
    import torch
    polys = U.polygons([U.DOC_WKT_PARTS, U.box(-74.01, 40.70, -73.99, 40.72)])
    cells, off = _device(polys, 3)
    cap = len(cells) - 1
    out = torch.full((cap,), -1, dtype=torch.int64, device=gpu)
    doff = torch.full((3,), -1, dtype=torch.int64, device=gpu)
    tot = ctypes.c_int64()
    ctx = M.default_context(gpu)
    st = N.lib().mgpu_grid_polyfill(ctx.handle, 0, 3, 2, polys.poly_part_off.ctypes.data, polys.part_ring_off.ctypes.data,
                                    polys.ring_off.ctypes.data, polys.xy.ctypes.data, out.data_ptr(), cap, doff.data_ptr(),
                                    ctypes.byref(tot), torch.cuda.current_stream(gpu).cuda_stream)
    assert st == N.MGPU_E_CAPACITY and tot.value == len(cells)
    assert np.array_equal(doff.cpu().numpy(), off) and np.array_equal(out.cpu().numpy(), cells[:-1])
    with pytest.raises(N.IllegalStateException):
        M.grid_polyfill(polys, 16)
    with pytest.raises(N.MosaicGpuError):
        M.grid_polyfill(U.polygons([U.box(-100, 10, 100, 20)]), 2)

"""grid_polyfill on the CPU: the host twin of the device kernels (mgpu_test_grid_polyfill_host,
the same plan walked by the same code) against the brute-force oracle of tests/polyfill_util.py
-- "the set of grid indices whose centroid is contained in the geometry" -- and, for BNG,
against a restatement of the reference's BFS.

Condition, not tolerance: before any comparison every case asserts that no candidate centre
lies within 1e-9 degrees (BNG: 1e-6 m) of its polygon's boundary, 1000 x the measured gap
between the device's correctly rounded centres and the reference's; under it the two routes
give one verdict.  The certificate counter is zero and the first spacing held in every call
(polyfill_util.twin asserts both)."""
import ctypes
import json
import os

import numpy as np
import pytest

import polyfill_util as U
from mosaic_amd import _native as N


def _check_sets(polys, res, ref, idx=None):
    """twin == oracle as sets, polygon by polygon; no duplicate; the gap condition first."""
    sel = polys if idx is None else polys.select(list(idx))
    cells, off = U.twin(sel, res)
    gap = min(r[2] for r in ref)
    print("polygons %d  candidates %d  cells %d  closest centre-to-boundary %.3g deg  samples %d"
          % (len(sel), sum(r[1] for r in ref), len(cells), gap, U.last()[0]))
    assert gap > U.BOUNDARY_GAP_DEG
    assert off[0] == 0 and off[-1] == len(cells) and np.all(np.diff(off) >= 0)
    for p, got in enumerate(U.lists_of(cells, off)):
        assert len(set(got.tolist())) == len(got), "polygon %d: a cell twice" % p
        assert set(got.tolist()) == ref[p][0], "polygon %d" % p
    return cells, off


def test_documented_answer():
    """docs/source/api/spatial-indexing.rst:191-220: grid_polyfill of the multipolygon at res 0."""
    with open(os.path.join(U.GOLDEN, "polyfill_doc_res0.json")) as f:
        doc = json.load(f)
    polys = U.polygons([[[[tuple(p) for p in ring] for ring in part] for part in doc["parts"]]])
    cells, off = U.twin(polys, doc["resolution"])
    assert sorted(cells.tolist()) == sorted(doc["cells"]) and len(cells) == 3
    assert U.reference("doc", 0)[0][0] == set(doc["cells"])
    assert 56 <= U.last()[0] <= 143  # one partial tile of samples


@pytest.mark.parametrize("res,count", [(0, 3), (1, 11), (2, 74), (3, 502)])
def test_documented_geometry_across_faces(res, count):
    cells, _ = _check_sets(U.polygons([U.DOC_WKT_PARTS]), res, U.reference("doc", res))
    assert len(cells) == count


def test_nyc_res9_all_zones():
    cells, _ = _check_sets(U.nyc(), 9, U.reference("nyc", 9))
    assert len(U.nyc()) == 263


def test_nyc_res10_twenty_zones():
    _check_sets(U.nyc(), 10, U.reference("nyc20", 10), U.NYC20)


def test_london_res8_across_longitude_zero():
    z = U.london_wgs84()
    assert z.xy[:, 0].min() < 0 < z.xy[:, 0].max()
    _check_sets(z, 8, U.reference("london", 8))


@pytest.mark.parametrize("res", [2, 3])
@pytest.mark.parametrize("base_cell", [4, 14, 38, 58])
def test_pentagon_box(base_cell, res):
    polys = U.polygons([U.pentagon_box(base_cell, res)])
    ref = U.h3_oracle_set(polys, res)
    cells, _ = _check_sets(polys, res, ref)
    assert int(U.CU.h3_cell(res, base_cell, (0,) * res)) in set(cells.tolist())


@pytest.mark.parametrize("lat", [60, 75, 84])
def test_high_latitude_box(lat):
    polys = U.polygons([U.north_box(lat)])
    _check_sets(polys, 4, U.h3_oracle_set(polys, 4))


def test_hole_swallows_cells_and_tiny_polygon_is_empty():
    holed = U.holed_polygon()
    polys = U.polygons([holed, U.tiny_polygon(), [holed[0][:1]]])
    ref = U.h3_oracle_set(polys, 9)
    cells, off = _check_sets(polys, 9, ref)
    n = np.diff(off)
    assert n[1] == 0 and n[0] > 0 and n[2] > n[0] + 5  # (the hole's cells are in the shell-only polygon)


def test_multipolygons_with_a_hole():
    """Shell, hole, then another part's shell: a centre in the first part's hole is outside that
    part and matched only where the second part covers it."""
    multis = U.holed_multipolygons()
    polys = U.polygons(multis + [U.holed_polygon(), [U.island()], [U.part_in_hole()], [U.holed_polygon()[0][:1]]])
    cells, off = _check_sets(polys, 9, U.h3_oracle_set(polys, 9))
    first, last_, inhole, holed, island, patch, shell = [set(c.tolist()) for c in U.lists_of(cells, off)]
    assert len(shell - holed) > 5 and patch and patch <= shell - holed  # (the hole swallows cells; the patch lies in it)
    assert first == holed | island == last_ and not holed & island
    assert inhole == holed | patch and len(inhole) < len(shell)
    # the order too: part by part in neither case -- one lattice over the whole multipolygon
    assert sorted(cells[off[0]:off[1]].tolist()) == sorted(cells[off[1]:off[2]].tolist())


@pytest.mark.parametrize("n", [1024, 1025, 1026, 2047, 2048])
def test_ring_lengths_around_the_chunk_size(n):
    """A ring that just fits a chunk of 1024 vertices, overflows it by one and by two, fills two."""
    polys = U.polygons([U.ngon(n), U.ngon(5)])
    _check_sets(polys, 9, U.h3_oracle_set(polys, 9))


def test_more_ring_pieces_than_a_chunk_holds():
    polys = U.polygons([U.many_parts(40), U.many_parts(33)[32:]])
    cells, off = _check_sets(polys, 9, U.h3_oracle_set(polys, 9))
    assert off[1] >= 40 and off[2] > off[1]


@pytest.mark.parametrize("res", [3, -4, 4])
def test_bng_districts_equal_the_reference_bfs(res):
    d = U.london_districts()
    idx = list(range(0, 180, 6))
    sel = d.select(idx)
    cells, off = U.twin(sel, res, code=1)
    assert len(idx) == 30
    for p, got in enumerate(U.lists_of(cells, off)):
        parts = U.polygon_rings(sel, p)
        full, gap = U.bng_full(parts, res)
        assert gap > U.BOUNDARY_GAP_M
        assert U.bng_bfs(parts, res) == full, "polygon %d: the reference's BFS misses cells here" % p
        assert len(set(got.tolist())) == len(got) and set(got.tolist()) == full, "polygon %d" % p
    print("res %d: %d cells over 30 districts" % (res, len(cells)))


def test_errors():
    doc = U.polygons([U.DOC_WKT_PARTS])
    assert U.twin_raw(doc, 16, 0, 64)[0] == N.MGPU_E_RESOLUTION
    assert U.twin_raw(doc, 0, 1, 64)[0] == N.MGPU_E_RESOLUTION  # (BNG has no resolution 0)
    bad = U.polygons([U.DOC_WKT_PARTS])
    bad.xy[2, 1] = np.nan
    assert U.twin_raw(bad, 0, 0, 64)[0] == N.MGPU_E_INVALID_ARG
    unclosed = U.polygons([[[[(30, 20), (45, 40), (10, 40), (30, 21)]]]])
    assert U.twin_raw(unclosed, 0, 0, 64)[0] == N.MGPU_E_INVALID_ARG
    short = U.polygons([[[[(30, 20), (45, 40), (30, 20)]]]])
    assert U.twin_raw(short, 0, 0, 64)[0] == N.MGPU_E_INVALID_ARG
    outside = U.polygons([U.box(170, 10, 181, 20)])
    assert U.twin_raw(outside, 0, 0, 64)[0] == N.MGPU_E_INVALID_ARG
    wide = U.polygons([U.box(-100, 10, 100, 20)])
    assert U.twin_raw(wide, 0, 0, 64)[0] == N.MGPU_E_UNSUPPORTED
    for name, at, value in (("ring_off", 1, 12), ("ring_off", 0, 1), ("part_ring_off", 0, 1), ("poly_part_off", 0, 1)):
        broken = U.polygons([U.DOC_WKT_PARTS])  # (offsets that step back, or do not start at 0)
        getattr(broken, name)[at] = value
        assert U.twin_raw(broken, 0, 0, 64)[0] == N.MGPU_E_INVALID_ARG, name
    huge = U.polygons([U.box(-80, -40, 80, 40)])
    assert U.twin_raw(huge, 12, 0, 64)[0] == N.MGPU_E_INVALID_ARG  # (a lattice beyond 2^31 - 1 samples)


def test_capacity_path():
    polys = U.polygons([U.DOC_WKT_PARTS, U.box(-74.01, 40.70, -73.99, 40.72)])
    cells, off = U.twin(polys, 3)
    st, out, off2, tot = U.twin_raw(polys, 3, 0, len(cells) - 1)
    assert st == N.MGPU_E_CAPACITY and tot == len(cells)
    assert np.array_equal(off2, off) and np.array_equal(out[:len(cells) - 1], cells[:-1])
    st, _, off3, tot = U.twin_raw(polys, 3, 0, 0)
    assert st == N.MGPU_E_CAPACITY and tot == len(cells) and np.array_equal(off3, off)


def test_polygon_without_parts_is_empty():
    import mosaic_amd as M
    a = U.polygons([U.DOC_WKT_PARTS])
    # polygon 0: the multipolygon; polygon 1: no parts; polygon 2: the multipolygon's second part
    polys = M.Polygons([0, 1, 2], [0, 2, 2, 3], [0, 1, 2, 3], [0, 4, 9, 14], np.vstack([a.xy, a.xy[4:9]]))
    cells, off = U.twin(polys, 1)
    n = np.diff(off)
    assert n[0] == 11 and n[1] == 0 and 0 < n[2] < 11
    assert set(cells[off[2]:off[3]].tolist()) <= set(cells[:off[1]].tolist())
    empty = M.Polygons([], [0], [0], [0], np.zeros((0, 2)))
    st, _, off0, tot = U.twin_raw(empty, 1, 0, 8)
    assert st == 0 and tot == 0 and off0[0] == 0

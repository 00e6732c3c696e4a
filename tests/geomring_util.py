"""grid_geometrykring / grid_geometrykloop: the oracle and the shapes of tests/test_geomring_host.py
and tests/test_gpu_geomring.py.

The oracle is Mosaic.geometryKRing / geometryKLoop (core/Mosaic.scala:123-156, getCellSets
:226-238) as Python sets over the project's ring oracle (oracle.h3_k_ring / h3_k_loop / bng_k_ring
/ bng_k_loop), applied to the same chip rows and sorted:

    (core, border) = the geometry's rows split by is_core
    ring(k) = core | U kRing(b, k)
    loop(k) = U kLoop(b, k) - (core | U kRing(b, k - 1))

It shares no code with mgpu_geometry_kring or its host twin.  Exact integers: no tolerance."""
import ctypes
import functools
import os

import numpy as np

import oracle as O

import cellgeom_util as CU
import mosaic_amd as M
from mosaic_amd import _native as N

GOLDEN = CU.GOLDEN
H3, BNG = 0, 1


@functools.lru_cache(maxsize=None)
def _ring(code, cell, k):
    return frozenset(O.h3_k_ring(cell, k) if code == H3 else O.bng_k_ring(cell, k))


@functools.lru_cache(maxsize=None)
def _loop(code, cell, k):
    return frozenset(O.h3_k_loop(cell, k) if code == H3 else O.bng_k_loop(cell, k))


def oracle(code, row_off, cell, is_core, k, loop):
    """One sorted int64 array per geometry."""
    out = []
    for g in range(len(row_off) - 1):
        rows = range(int(row_off[g]), int(row_off[g + 1]))
        core = {int(cell[r]) for r in rows if is_core[r]}
        border = {int(cell[r]) for r in rows if not is_core[r]}
        if loop:
            got = set().union(*[_loop(code, b, k) for b in border]) - core.union(*[_ring(code, b, k - 1) for b in border])
        else:
            got = core.union(*[_ring(code, b, k) for b in border])
        out.append(np.array(sorted(got), dtype=np.int64))
    return out


def table(geoms):
    """[(core cells, border cells), ...] -> (row_off, cell, is_core), the core rows first."""
    row_off, cell, core = [0], [], []
    for c, b in geoms:
        cell += [int(v) for v in c] + [int(v) for v in b]
        core += [1] * len(c) + [0] * len(b)
        row_off.append(len(cell))
    return np.array(row_off, np.int64), np.array(cell, np.int64), np.array(core, np.uint8)


def group(chips):
    """A ChipTable's rows grouped by polygon id (stable): (ids, row_off, cell, is_core)."""
    order = np.argsort(chips.polygon_id, kind="stable")
    pid = chips.polygon_id[order]
    ids = np.unique(pid)
    row_off = np.append(np.searchsorted(pid, ids, side="left"), len(pid)).astype(np.int64)
    return ids.astype(np.int32), row_off, chips.cell[order].copy(), chips.is_core[order].copy()


def twin_raw(code, row_off, cell, is_core, k, loop, capacity, out=None):
    """(status, total, cells buffer, offsets) of mgpu_test_geometry_kring_host."""
    row_off, cell, is_core = (np.ascontiguousarray(row_off, np.int64), np.ascontiguousarray(cell, np.int64),
                              np.ascontiguousarray(is_core, np.uint8))
    n = len(row_off) - 1
    buf = np.full(max(capacity, 1), -1, np.int64) if out is None else out
    off = np.full(n + 1, -1, np.int64)
    tot = ctypes.c_int64(-1)
    st = N.lib().mgpu_test_geometry_kring_host(code, n, row_off.ctypes.data, cell.ctypes.data, is_core.ctypes.data, int(k),
                                               1 if loop else 0, buf.ctypes.data if capacity else None, capacity,
                                               off.ctypes.data, ctypes.byref(tot))
    return st, tot.value, buf, off


def twin(code, row_off, cell, is_core, k, loop):
    """(cells, offsets): a size query, then the exact buffer."""
    st, total, _, _ = twin_raw(code, row_off, cell, is_core, k, loop, 0)
    if st not in (N.MGPU_OK, N.MGPU_E_CAPACITY):
        N.check(st)
    st, total2, buf, off = twin_raw(code, row_off, cell, is_core, k, loop, total)
    N.check(st)
    assert total2 == total
    return buf[:total], off


def lists_of(cells, off):
    return [cells[off[g]:off[g + 1]] for g in range(len(off) - 1)]


def last():
    out = np.zeros(8, np.int64)
    N.check(N.lib().mgpu_test_geometry_kring_last(out.ctypes.data))
    return out.tolist()


def check_twin(code, row_off, cell, is_core, k, loop):
    """twin == oracle, list by list; offsets consistent; returns (cells, offsets)."""
    cells, off = twin(code, row_off, cell, is_core, k, loop)
    ref = oracle(code, row_off, cell, is_core, k, loop)
    assert off[0] == 0 and off[-1] == len(cells) and len(off) == len(ref) + 1
    for g, want in enumerate(ref):
        assert np.array_equal(cells[off[g]:off[g + 1]], want), "geometry %d" % g
    return cells, off


# ---------------------------------------------------------------- shapes

@functools.lru_cache(maxsize=None)
def manhattan_cell(res=9):
    return int(O.h3_points_to_cells(np.array([-73.9857]), np.array([40.7484]), res)[0])


def fat(radius=3, centre=None):
    """A disk: the cells within radius - 1 of the centre are core, its outer ring is border."""
    c = centre or manhattan_cell()
    return O.h3_k_ring(c, radius - 1), O.h3_k_loop(c, radius)


def thin(length=7, centre=None):
    """A line of border cells, no core: each the first cell of the loop around the one before."""
    c = centre or manhattan_cell()
    line = [c]
    while len(line) < length:
        line.append(O.h3_k_loop(line[-1], 1)[0])
    assert len(set(line)) == length
    return [], line


def small(centre=None):
    c = centre or manhattan_cell()
    return [c], O.h3_k_loop(c, 1)


def pentagon_and_neighbours():
    """The res-2 pentagon of base cell 14 and its five neighbours, all border."""
    p = CU.h3_cell(2, 14, (0, 0))
    nb = O.h3_k_loop(p, 1)
    assert len(nb) == 5
    return [], [p] + nb


SYNTHETIC = ("copies", "empty_between", "fat", "one_border_cell", "pentagon", "thin")


@functools.lru_cache(maxsize=None)
def synthetic():
    """The hand-made H3 tables both test files run: name -> (row_off, cell, is_core)."""
    c = manhattan_cell()
    t = {
        "one_border_cell": table([([], [c])]),
        "fat": table([fat()]),
        "thin": table([thin()]),
        "empty_between": table([small(), ([], []), (fat()[0], []), small()]),
        "copies": table([small()] * 64 + [([], [])] + [small()] * 3),
        "pentagon": table([pentagon_and_neighbours()]),
    }
    assert sorted(t) == sorted(SYNTHETIC)
    return t


@functools.lru_cache(maxsize=None)
def nyc():
    return M.Polygons.from_npz(os.path.join(GOLDEN, "nyc_taxi_zones.npz"))


@functools.lru_cache(maxsize=None)
def nyc_chips(first, count, res=9):
    idx = list(range(first, first + count))
    return M.tessellate(nyc().select(idx), M.H3IndexSystem(), res, keep_core_geometries=False)


@functools.lru_cache(maxsize=None)
def london_chips(idx, res):
    import bench_workloads
    return M.tessellate(bench_workloads.london_districts().select(list(idx)), M.BNGIndexSystem(), res, keep_core_geometries=False)

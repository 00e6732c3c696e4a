"""grid_geometrykring / grid_geometrykloop on the CPU: the host twin of the device entry
(mgpu_test_geometry_kring_host: the same contract on host arrays, from the ring code the kernels
run) against the set oracle of tests/geomring_util.py -- Mosaic.geometryKRing / geometryKLoop
over the project's ring oracle.  Exact integers, list by list, order included (ascending)."""
import numpy as np
import pytest

import geomring_util as U
from mosaic_amd import _native as N


@pytest.mark.parametrize("k,loop", [(0, False), (1, False), (2, False), (1, True), (2, True)])
def test_three_nyc_zones_h3_r9(k, loop):
    """(The loop starts at k = 1; test_argument_errors has its k = 0.)"""
    ids, row_off, cell, core = U.group(U.nyc_chips(100, 3))
    assert len(ids) == 3 and core.sum() > 0 and (core == 0).sum() > 0
    cells, off = U.check_twin(U.H3, row_off, cell, core, k, loop)
    assert np.all(np.diff(off) > 0)
    if not loop and k == 0:  # the ring of k = 0 is the geometry's own cells
        for g in range(3):
            assert np.array_equal(cells[off[g]:off[g + 1]], np.unique(cell[row_off[g]:row_off[g + 1]]))


@pytest.mark.parametrize("res", [4, -4])
@pytest.mark.parametrize("k", [1, 2])
def test_two_london_districts_bng(res, k):
    _, row_off, cell, core = U.group(U.london_chips((0, 90), res))
    assert len(row_off) == 3
    print("rows %d  border %d" % (len(cell), int((core == 0).sum())))
    for loop in (False, True):
        U.check_twin(U.BNG, row_off, cell, core, k, loop)


@pytest.mark.parametrize("name", U.SYNTHETIC)
def test_synthetic_tables(name):
    row_off, cell, core = U.synthetic()[name]
    for k, loop in [(0, False), (1, False), (2, False), (3, False), (1, True), (2, True)]:
        U.check_twin(U.H3, row_off, cell, core, k, loop)


def test_one_border_cell_is_the_sorted_cell_ring():
    import oracle as O
    row_off, cell, core = U.synthetic()["one_border_cell"]
    for k in (0, 1, 3):
        cells, _ = U.twin(U.H3, row_off, cell, core, k, False)
        assert cells.tolist() == sorted(O.h3_k_ring(int(cell[0]), k))
    for k in (1, 3):
        cells, _ = U.twin(U.H3, row_off, cell, core, k, True)
        assert cells.tolist() == sorted(O.h3_k_loop(int(cell[0]), k))


def test_core_is_removed_from_the_loop():
    import oracle as O
    row_off, cell, core = U.synthetic()["fat"]
    inner = set(cell[core == 1].tolist())
    for k in (1, 2):
        cells, _ = U.twin(U.H3, row_off, cell, core, k, True)
        got = set(cells.tolist())
        assert not (got & inner) and got == set(O.h3_k_loop(U.manhattan_cell(), 3 + k))
    row_off, cell, core = U.synthetic()["thin"]
    cells, _ = U.twin(U.H3, row_off, cell, core, 1, True)
    assert not (set(cells.tolist()) & set(cell.tolist()))
    assert len(cells) < 6 * len(cell)


def test_empty_lists():
    row_off, cell, core = U.synthetic()["empty_between"]
    _, off = U.twin(U.H3, row_off, cell, core, 1, True)
    n = np.diff(off)
    assert n[1] == 0 and n[2] == 0 and n[0] == n[3] > 0
    cells, off = U.twin(U.H3, row_off, cell, core, 1, False)
    assert np.array_equal(cells[off[2]:off[3]], np.sort(cell[row_off[2]:row_off[3]])) and off[1] == off[2]


def test_argument_errors():
    row_off, cell, core = U.synthetic()["fat"]
    for k, loop in [(-1, False), (1025, False), (0, True), (1025, True)]:
        st, _, _, _ = U.twin_raw(U.H3, row_off, cell, core, k, loop, 0)
        assert st == N.MGPU_E_INVALID_ARG, (k, loop)
    assert U.twin_raw(2, row_off, cell, core, 1, False, 0)[0] == N.MGPU_E_INVALID_ARG
    bad = cell.copy()
    bad[-1] = 12345  # a border row that is no H3 cell id
    assert U.twin_raw(U.H3, row_off, bad, core, 1, False, 0)[0] == N.MGPU_E_INVALID_ARG
    assert U.twin_raw(U.BNG, row_off, cell, core, 1, False, 0)[0] == N.MGPU_E_INVALID_ARG
    assert U.twin_raw(U.H3, row_off[::-1].copy(), cell, core, 1, False, 0)[0] == N.MGPU_E_INVALID_ARG
    with pytest.raises(N.IllegalArgumentException):
        U.twin(U.H3, row_off, bad, core, 1, False)


def test_capacity_protocol():
    row_off, cell, core = U.synthetic()["empty_between"]
    full, foff = U.twin(U.H3, row_off, cell, core, 2, False)
    st, total, _, off = U.twin_raw(U.H3, row_off, cell, core, 2, False, 0)  # the size query
    assert st == N.MGPU_E_CAPACITY and total == len(full) and np.array_equal(off, foff)
    st, total, buf, off = U.twin_raw(U.H3, row_off, cell, core, 2, False, len(full) - 1)
    assert st == N.MGPU_E_CAPACITY and total == len(full) and np.array_equal(off, foff)
    assert np.array_equal(buf[:len(full) - 1], full[:-1])
    st, total, buf, off = U.twin_raw(U.H3, row_off, cell, core, 2, False, len(full))
    assert st == N.MGPU_OK and np.array_equal(buf, full)

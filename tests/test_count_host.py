"""The host part of mgpu_pip_join_count's polygon slots (mosaic_amd/csrc/poly_slots.h through
the hook mgpu_test_poly_slots_host): the distinct polygon ids ascending and each chip row's
slot, against np.unique(..., return_inverse=True).  No GPU."""
import ctypes

import numpy as np
import pytest

from mosaic_amd import _native as N

INT32_MIN = -2 ** 31
INT32_MAX = 2 ** 31 - 1


def poly_slots(pid):
    pid = np.ascontiguousarray(pid, dtype=np.int32)
    n = len(pid)
    ids = np.full(max(n, 1), 12345, np.int32)
    slot = np.full(max(n, 1), 0xDEADBEEF, np.uint32)
    m = ctypes.c_int64(-1)
    N.check(N.lib().mgpu_test_poly_slots_host(pid.ctypes.data if n else None, n, ids.ctypes.data, ctypes.byref(m),
                                              slot.ctypes.data))
    return ids[:m.value], slot[:n]


def check(pid):
    pid = np.asarray(pid, dtype=np.int32)
    ids, slot = poly_slots(pid)
    ref_ids, ref_inv = np.unique(pid, return_inverse=True)
    assert ids.dtype == np.int32 and np.array_equal(ids, ref_ids)
    assert np.array_equal(slot.astype(np.int64), ref_inv.reshape(-1))
    if len(pid):
        assert np.array_equal(ids[slot], pid)
    return ids


def test_symbols_exported():
    for name in ("mgpu_chips_polygons", "mgpu_pip_join_count", "mgpu_test_poly_slots_host"):
        assert name in N.EXPORTS and hasattr(N.lib(), name)


def test_duplicates_negatives_and_int32_min():
    ids = check([5, -3, 5, INT32_MIN, 0, -3, INT32_MAX, 7, INT32_MIN, 5, 0])
    assert ids[0] == INT32_MIN and ids[-1] == INT32_MAX and len(ids) == 6


def test_one_polygon_and_empty():
    assert np.array_equal(check([42] * 17), [42])
    assert np.array_equal(check([INT32_MIN]), [INT32_MIN])
    assert len(check([])) == 0


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_columns(seed):
    rng = np.random.default_rng(seed)
    # dense small ids, ids scaled apart, and the full int32 range, each with many repeats
    check(rng.integers(1, 264, 5000))
    check(-rng.integers(1, 264, 5000) * 1000)
    pool = rng.integers(INT32_MIN, INT32_MAX, 300, endpoint=True)
    check(rng.choice(pool, 4000))


def test_bad_arguments():
    m = ctypes.c_int64()
    assert N.lib().mgpu_test_poly_slots_host(None, 3, None, ctypes.byref(m), None) == N.MGPU_E_INVALID_ARG
    assert N.lib().mgpu_test_poly_slots_host(None, -1, None, ctypes.byref(m), None) == N.MGPU_E_INVALID_ARG

"""The mgpu_cell_agg_* entries without a GPU: the symbols are exported and bound, NULL
handles are refused before a device is touched, and create checks the index system and
the resolution first."""
import ctypes

from mosaic_amd import _native as N

NAMES = ("mgpu_cell_agg_create", "mgpu_cell_agg_add_points", "mgpu_cell_agg_add_cells", "mgpu_cell_agg_add_counted",
         "mgpu_cell_agg_size", "mgpu_cell_agg_fetch", "mgpu_cell_agg_clear", "mgpu_cell_agg_destroy")


def test_symbols_exported_and_bound():
    L = N.lib()
    for name in NAMES:
        assert name in N.EXPORTS and hasattr(L, name)
        f = getattr(L, name)
        assert f.restype is ctypes.c_int32 and f.argtypes, name
    import mosaic_amd as M
    for name in ("CellAggregate", "CellCounts", "grid_cellcount"):
        assert hasattr(M, name) and name in M.__all__


def refused_null(status):
    assert status == N.MGPU_E_INVALID_ARG
    assert "NULL" in N.last_error()


def test_null_ctx_or_handle_is_refused():
    L = N.lib()
    h = ctypes.c_void_p()
    n = ctypes.c_int64(-7)
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: the other handle is NULL
    refused_null(L.mgpu_cell_agg_create(None, N.MGPU_H3, 9, 0, 0, ctypes.byref(h)))
    assert not h.value
    for ctx, agg in ((None, fake), (fake, None), (None, None)):
        refused_null(L.mgpu_cell_agg_add_points(ctx, agg, None, None, None, 0, None, None))
        refused_null(L.mgpu_cell_agg_add_cells(ctx, agg, None, None, 0, None, 0, None))
        refused_null(L.mgpu_cell_agg_add_counted(ctx, agg, None, None, None, 0, None))
        refused_null(L.mgpu_cell_agg_size(ctx, agg, ctypes.byref(n), None))
        refused_null(L.mgpu_cell_agg_fetch(ctx, agg, 0, None, None, None, ctypes.byref(n), None))
        refused_null(L.mgpu_cell_agg_clear(ctx, agg, None))
    assert n.value == -7
    assert L.mgpu_cell_agg_destroy(None) == N.MGPU_OK


def test_create_checks_index_system_and_resolution_first():
    L = N.lib()
    h = ctypes.c_void_p()
    # (a NULL context: were the device touched or the context read first, the status would differ)
    assert L.mgpu_cell_agg_create(None, 7, 9, 0, 0, ctypes.byref(h)) == N.MGPU_E_INVALID_ARG
    assert "unknown index system" in N.last_error()
    assert L.mgpu_cell_agg_create(None, N.MGPU_H3, 16, 0, 0, ctypes.byref(h)) == N.MGPU_E_RESOLUTION
    assert L.mgpu_cell_agg_create(None, N.MGPU_H3, -1, 1, 0, ctypes.byref(h)) == N.MGPU_E_RESOLUTION
    assert L.mgpu_cell_agg_create(None, N.MGPU_BNG, 0, 0, 0, ctypes.byref(h)) == N.MGPU_E_RESOLUTION
    assert L.mgpu_cell_agg_create(None, N.MGPU_BNG, 7, 0, 0, ctypes.byref(h)) == N.MGPU_E_RESOLUTION
    assert not h.value

"""mgpu_pip_join_lookup without a GPU: the symbol is exported and bound, and a NULL context
or chip table is refused before the device is touched."""
import ctypes

import mosaic_amd as M
from mosaic_amd import _native as N


def test_symbol_exported():
    assert "mgpu_pip_join_lookup" in N.EXPORTS and hasattr(N.lib(), "mgpu_pip_join_lookup")
    assert callable(M.pip_join_lookup) and M.LookupResult is not None


def test_null_context_or_chips():
    st = N.MgpuStats()
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: the other handle is NULL
    for ctx, chips in ((None, None), (None, fake), (fake, None)):
        got = N.lib().mgpu_pip_join_lookup(ctx, chips, N.MGPU_H3, 9, None, None, 0, -1, None, None, None,
                                           ctypes.byref(st))
        assert got == N.MGPU_E_INVALID_ARG
        assert "NULL" in N.last_error()

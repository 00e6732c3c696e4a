"""Cell id -> geometry on the host (no GPU): the correctly rounded asin / atan the route
adds (h3_exact.h), the host twin of the cell-geometry kernels
(mgpu_test_cell_geometry_host: h3_boundary.h under its correctly rounded policy, cell_geom.h's
area) against today's glibc route and a numpy restatement of IndexSystem.area, and BNG against
a Python restatement of getX / getY / getEdgeSize.  tests/test_gpu_cellgeom.py asserts that
the device equals the twin bit for bit, so what is pinned here holds for the device.

Measured on the fixed cell set (tests/cellgeom_util.py fixed_h3_cells, 9669 cells; glibc 2.35):
  twin vs glibc route   vertex counts equal everywhere; 0.372 % of the 138,424 coordinates
                        differ in some bit, the largest difference 3.56e-13 degrees
  twin area vs numpy    relative difference, largest per resolution 0..15:
                        4.2e-16 8.2e-16 5.6e-16 2.4e-15 6.5e-15 2.0e-14 2.9e-14 6.9e-14
                        0 7.1e-13 1.6e-12 4.6e-12 1.4e-11 1.5e-16 1.2e-10 3.5e-10
                        (98 % of the areas are equal to the bit: numpy's libm is glibc's, which
                        rounds most arguments correctly; where it does not, the haversine's
                        dx = cos(dph) cos(th1) - cos(th2) cancels to the side's length d, so one
                        ulp becomes 2^-53 / d relative -- 1e-9 at resolution 15.  The reference
                        loses the same digits.)
"""
import numpy as np
import pytest

import cellgeom_util as U
from test_h3_exact_host import elementary

# the measurements above; the assertions allow 4x the maximum and 2x the share (glibc
# versions differ in the last bits), inside the hard conditions 1e-9 degrees and 2 %
TWIN_GLIBC_MAX_DEG = 3.56e-13
TWIN_GLIBC_SHARE = 0.00372
AREA_REL = [4.2e-16, 8.2e-16, 5.6e-16, 2.4e-15, 6.5e-15, 2.0e-14, 2.9e-14, 6.9e-14,
            0.0, 7.1e-13, 1.6e-12, 4.6e-12, 1.4e-11, 1.5e-16, 1.2e-10, 3.5e-10]


def _check_correctly_rounded(fn, x, ref_l):
    """cr(x) is a correct rounding of the 80-bit reference: within half a double ulp of it,
    plus the reference's own error (asinl / atanl: below 1 ulp of the 64-bit significand)."""
    got = elementary(fn, x)
    err = np.abs(got.astype(np.longdouble) - ref_l)
    bound = np.spacing(np.abs(got)).astype(np.longdouble) / 2 + np.abs(ref_l) * np.longdouble(2.0) ** -62
    bad = np.nonzero(~(err <= bound))[0]
    assert bad.size == 0, [(x[i], got[i], ref_l[i]) for i in bad[:3]]
    # and the double nearest to the reference, but for the arguments where that is a near-tie
    near = ref_l.astype(np.float64)
    assert np.count_nonzero(got != near) <= len(x) // 200


def test_cr_asin_equals_asinl():
    assert np.finfo(np.longdouble).nmant == 63  # the host's long double is the x87 format
    rng = np.random.default_rng(301)
    ulps = np.arange(-8, 9) * 2.0 ** -53
    x = np.concatenate([
        rng.uniform(-1.0, 1.0, 200_000),                        # sinlat of _geoAzDistanceRads
        rng.uniform(0.0, 1e-3, 50_000),                         # sqrt(...) / 2 of the haversine
        np.ldexp(rng.uniform(0.5, 1.0, 20_000), rng.integers(-60, 0, 20_000)),
        0.75 + ulps, -0.75 + ulps, 1.0 - np.arange(0, 64) * 2.0 ** -53, -1.0 + np.arange(0, 64) * 2.0 ** -53,
        np.array([5e-324, -5e-324, 2.2250738585072014e-308, 1e-310, -1e-310])])
    _check_correctly_rounded(14, x, np.arcsin(x.astype(np.longdouble)))
    z = elementary(14, np.array([0.0, -0.0, 1.0, -1.0, np.nan, 1.0000000000000002, -1.5, np.inf]))
    assert z[0] == 0 and not np.signbit(z[0]) and z[1] == 0 and np.signbit(z[1])
    assert z[2] == np.pi / 2 and z[3] == -np.pi / 2
    assert np.isnan(z[4:]).all()


def test_cr_atan_equals_atanl():
    rng = np.random.default_rng(302)
    x = np.concatenate([
        rng.uniform(0.0, 0.7, 200_000),                         # r of _hex2dToGeo, t of triangle_area
        rng.uniform(-20.0, 20.0, 50_000),
        np.ldexp(rng.uniform(0.5, 1.0, 20_000), rng.integers(-60, 10, 20_000)),
        np.array([5e-324, -5e-324, 2.2250738585072014e-308, 1e-310, 1.0, -1.0])])
    _check_correctly_rounded(15, x, np.arctan(x.astype(np.longdouble)))
    z = elementary(15, np.array([0.0, -0.0, np.nan, np.inf, -np.inf]))
    assert z[0] == 0 and not np.signbit(z[0]) and z[1] == 0 and np.signbit(z[1])
    assert np.isnan(z[2]) and z[3] == np.pi / 2 and z[4] == -np.pi / 2


def test_twin_against_glibc_route():
    """The correctly rounded route against today's host route (the reference's libm): the
    same topology everywhere, coordinates within the measured, bounded divergence."""
    cells = U.fixed_h3_cells()
    xy, nv, centre, _ = U.fixed_h3_twin()
    gxy, gnv, gcentre = U.glibc_route(cells)
    assert np.array_equal(nv, gnv)
    assert set(np.unique(nv).tolist()) == {5, 6, 7, 8, 10}
    m = np.arange(10)[None, :, None] < nv[:, None, None]
    d = np.concatenate([np.abs(xy - gxy)[np.broadcast_to(m, xy.shape)], np.abs(centre - gcentre).ravel()])
    share, worst = np.count_nonzero(d) / d.size, d.max()
    print("twin vs glibc route: %d coordinates, %.4f %% differ, max %.3e degrees" % (d.size, 100 * share, worst))
    assert worst <= 4 * TWIN_GLIBC_MAX_DEG and worst < 1e-9
    assert share <= 2 * TWIN_GLIBC_SHARE and share < 0.02


def test_twin_area_against_numpy_restatement():
    """IndexSystem.area restated with numpy on the twin's own boundary and centre.  The
    formula loses digits with the resolution (module docstring), so a resolution's bound is
    4x the largest difference measured at it or any coarser one."""
    cells = U.fixed_h3_cells()
    xy, nv, centre, area = U.fixed_h3_twin()
    ref = U.np_area(xy, nv, centre)
    rel = np.abs(area - ref) / ref
    res = (cells >> 52) & 15
    for r in range(16):
        got = rel[res == r].max()
        print("res %2d: %d cells, area rel diff max %.2e" % (r, np.count_nonzero(res == r), got))
        assert got <= 4 * max(AREA_REL[:r + 1]), r
    assert np.all(area > 0)
    doc = U.twin(0, np.array([U.DOC_AREA_CELL]))[3][0]
    print("area(%d) = %.9f (docs: %.8f)" % (U.DOC_AREA_CELL, doc, U.DOC_AREA_KM2))
    assert abs(doc - U.DOC_AREA_KM2) < 1e-6


def test_twin_rejects_invalid_ids():
    from mosaic_amd import IllegalArgumentException
    ok = U.h3_cell(3, 20, (1, 2, 3))
    for bad in (ok & ~(15 << 59) | (2 << 59), U.h3_cell(3, 122, (1, 2, 3)), U.h3_cell(3, 20, (1, 7, 3)),
                ok & ~(7 << 33), U.h3_cell(3, 4, (0, 1, 2)), 0):
        with pytest.raises(IllegalArgumentException):
            U.twin(0, np.array([ok, bad]))
    with pytest.raises(IllegalArgumentException):
        U.twin(1, np.array([123]))


def test_bng_boundaries_and_areas():
    import oracle as O
    rng = np.random.default_rng(303)
    x, y = rng.uniform(0.0, 700000.0, 400), rng.uniform(0.0, 1300000.0, 400)
    seen = set()
    for r in U.BNG_RESOLUTIONS:
        cells = np.unique(O.bng_points_to_cells(x, y, r))
        xy, nv, _, area = U.twin(1, cells)
        assert (nv == 4).all()
        for i, c in enumerate(cells.tolist()):
            corners, a = U.bng_cell_geometry(c)
            assert xy[i, :4].tolist() == [list(p) for p in corners], (r, c)
            assert area[i] == a, (r, c)
        e = xy[0, 1, 0] - xy[0, 0, 0]
        assert e == xy[0, 2, 1] - xy[0, 1, 1]
        seen.add(e)
    assert len(seen) == 12

// Cell id -> geometry, the arithmetic cell_geom.hip's kernels and the host twin
// (mgpu_test_cell_geometry_host, tessellate.cpp) share: IndexSystem.area's spherical
// excess (IndexSystem.scala:248-289), BNG's corners and area (BNGIndexSystem.scala:418-431,
// :510-516) and the size of a cell's WKB row.  The H3 boundary and centre themselves are
// h3_boundary.h's, under its correctly rounded policy (CrMath).
#pragma once
#include <stdint.h>

#include <vector>

#include "bng_core.h"
#include "h3_boundary.h"

namespace mgpu {
namespace cellgeom {

constexpr int kRowDoubles = 20;  // a boundary row: up to 10 (x, y) pairs

struct SinCos {
  double s, c;
};

// sin and cos of `c * lat` (IndexSystem.scala:251-254: c = math.Pi / 180)
template <class M>
MGPU_HD SinCos lat_sincos(double lat_deg) {
  const double c = 3.141592653589793 / 180;
  SinCos r;
  M::sincos(c * lat_deg, &r.s, &r.c);
  return r;
}

// IndexSystem.area's haversine (IndexSystem.scala:250-262), the latitudes' sines and
// cosines taken by lat_sincos
template <class M>
MGPU_HD double haversine(double lng1, SinCos t1, double lng2, SinCos t2) {
  const double c = 3.141592653589793 / 180;
  const double dph = c * (lng1 - lng2);
  double sin_dph, cos_dph;
  M::sincos(dph, &sin_dph, &cos_dph);
  const double dz = t1.s - t2.s;
  const double dx = cos_dph * t1.c - t2.c;
  const double dy = sin_dph * t1.c;
  return M::asin(sqrt(dx * dx + dy * dy + dz * dz) / 2) * 2;
}

// triangle_area (IndexSystem.scala:264-282) of (centre, b0, b1), km^2
template <class M>
MGPU_HD double triangle_area(double clng, SinCos ct, double lng0, SinCos t0, double lng1, SinCos t1) {
  const double a = haversine<M>(clng, ct, lng0, t0);
  const double b = haversine<M>(lng0, t0, lng1, t1);
  const double c = haversine<M>(lng1, t1, clng, ct);
  const double s = (a + b + c) / 2;
  const double t = sqrt(M::tan(s / 2) * M::tan((s - a) / 2) * M::tan((s - b) / 2) * M::tan((s - c) / 2));
  const double e = 4 * M::atan(t);
  const double r = 6371.0088;
  return e * r * r;
}

// IndexSystem.area (IndexSystem.scala:284-288): the triangles of the closed boundary in
// its order, summed from the first.  xy: nv (lng, lat) pairs in degrees.
template <class M>
MGPU_HD double h3_area_km2(const double* xy, int nv, double clng, double clat) {
  const SinCos ct = lat_sincos<M>(clat);
  double sum = 0.0;
  for (int k = 0; k < nv; k++) {
    const int k1 = k + 1 < nv ? k + 1 : 0;
    sum += triangle_area<M>(clng, ct, xy[2 * k], lat_sincos<M>(xy[2 * k + 1]), xy[2 * k1], lat_sincos<M>(xy[2 * k1 + 1]));
  }
  return sum;
}

// BNGIndexSystem.indexToGeometry's corners (x, y), (x + e, y), (x + e, y + e), (x, y + e)
// (JVM Int sums) and BNGIndexSystem.area; false for an id bng::cell_corner cannot decode
MGPU_HD bool bng_cell(int64_t id, double* xy8, double* area_km2) {
  int res, xl, yl;
  int32_t e, x, y;
  if (!bng::cell_corner(id, &res, &e, &x, &y, &xl, &yl)) return false;
  const int32_t x1 = (int32_t)((uint32_t)x + (uint32_t)e), y1 = (int32_t)((uint32_t)y + (uint32_t)e);
  if (xy8) {
    xy8[0] = (double)x, xy8[1] = (double)y;
    xy8[2] = (double)x1, xy8[3] = (double)y;
    xy8[4] = (double)x1, xy8[5] = (double)y1;
    xy8[6] = (double)x, xy8[7] = (double)y1;
  }
  if (area_km2) {
    const double k = (double)e / 1000;
    *area_km2 = k * k;
  }
  return true;
}

// a cell's WKB row when it is one polygon of one ring (the boundary closed with its first
// vertex): byte order, type, ring count, point count, nv + 1 points
MGPU_HD int64_t wkb_row_bytes(int nv) { return 13 + 16 * (int64_t)(nv + 1); }

// H3IndexSystem.indexToGeometry's two special shapes, from a boundary computed elsewhere
// (tessellate.cpp; host): the polar cap of a pole cell (makePoleGeometry) and the parts of
// a cell cut at the antimeridian (makeSafeGeometry), as the chip WKB the tessellator
// writes.  `boundary`: nv (lng, lat) pairs in degrees.
void h3_special_cell_wkb(uint64_t cell, const double* boundary, int nv, std::vector<uint8_t>& out);
// the cell holding the north / south pole at `res` (H3IndexSystem.scala:240-246)
uint64_t h3_pole_cell(bool north, int res);

}  // namespace cellgeom
}  // namespace mgpu

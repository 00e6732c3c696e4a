// H3 v3.7 cell geometry, shared by the host and the device: h3ToGeoBoundary and h3ToGeo,
// for the chip-table builder (host) and the cell-geometry kernels (cell_geom.hip).
// Replaces H3IndexSystem.indexToGeometry (H3IndexSystem.scala:103-111:
// h3.h3ToGeoBoundary(index) closed into a ring), which Mosaic intersects with the polygon
// to make each chip (IndexSystem.getBorderChips / getCoreChips, IndexSystem.scala:178-213),
// and H3IndexSystem.indexToCenter / indexToBoundary (H3IndexSystem.scala:230-237).
//
// Restated from H3 v3.7 (com.uber:h3:3.7.0, not vendored in the reference):
//   _h3ToFaceIjk (base cell home FaceIJK + digits, overage onto the face the centre lies
//   on), _faceIjkToVerts / _faceIjkPentToVerts (the aperture-33r(7r) substrate vertices),
//   _adjustOverageClassII (faceNeighbors: rotate + translate into the adjacent face),
//   _faceIjkToGeoBoundary / _faceIjkPentToGeoBoundary (a vertex per substrate vertex, each
//   projected with the gnomonic of the face it lies on, plus a "distortion" vertex where
//   a Class III edge crosses an icosahedron edge), _hex2dToGeo, _geoAzDistanceRads.
// The faceNeighbors table is H3's; tools/check_h3_face_neighbors.py re-derives every
// entry from the icosahedron geometry.
//
// The floating-point part is parametrised by a math policy M:
//   LibmMath  sin/cos/atan/asin/atan2 of the host's libm, as for H3's JNI library; the
//             long-double expressions as h3_exact.h's ld_* (the x87 unit on an x86-64 host).
//             What the tessellator and the chip-table builder use (host only).
//   CrMath    the correctly rounded exact::cr_* and the integer x87 emulation exact::em_*;
//             sqrt is IEEE.  What the device runs; compiled for the host with
//             -ffp-contract=off it gives the device's bits (the "host twin").
// The boundary is produced edge by edge: vertex a, then the distortion vertex of the edge
// a -> a + 1, each from integer state that is recomputed per vertex, so a device lane can
// take one substrate vertex without the others' results (cell_geom.hip).
#pragma once
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "h3_core.h"

// the projection: out of line on the device (double-double trigonometry, called from
// several places of a kernel)
#ifdef __HIP_DEVICE_COMPILE__
#define MGPU_H3B_COLD __host__ __device__ __attribute__((noinline))
#elif defined(__HIPCC__)
#define MGPU_H3B_COLD __host__ __device__ inline
#else
#define MGPU_H3B_COLD inline
#endif

namespace mgpu {
namespace h3b {

using h3::IJK;
namespace X = mgpu::exact;

struct FaceIJK {
  int face;
  IJK c;
};

// faceNeighbors[face][quadrant]: {neighbour face, translation (res-0 units), ccw 60 rotations}
// quadrants: 0 = central, 1 = IJ, 2 = KI, 3 = JK (H3 faceijk.c)
struct FaceOrient {
  int face;
  int ti, tj, tk;
  int rot;
};
H3T_QUAL FaceOrient kFaceNeighbors[20][4] = {
    {{0, 0, 0, 0, 0}, {4, 2, 0, 2, 1}, {1, 2, 2, 0, 5}, {5, 0, 2, 2, 3}},
    {{1, 0, 0, 0, 0}, {0, 2, 0, 2, 1}, {2, 2, 2, 0, 5}, {6, 0, 2, 2, 3}},
    {{2, 0, 0, 0, 0}, {1, 2, 0, 2, 1}, {3, 2, 2, 0, 5}, {7, 0, 2, 2, 3}},
    {{3, 0, 0, 0, 0}, {2, 2, 0, 2, 1}, {4, 2, 2, 0, 5}, {8, 0, 2, 2, 3}},
    {{4, 0, 0, 0, 0}, {3, 2, 0, 2, 1}, {0, 2, 2, 0, 5}, {9, 0, 2, 2, 3}},
    {{5, 0, 0, 0, 0}, {10, 2, 2, 0, 3}, {14, 2, 0, 2, 3}, {0, 0, 2, 2, 3}},
    {{6, 0, 0, 0, 0}, {11, 2, 2, 0, 3}, {10, 2, 0, 2, 3}, {1, 0, 2, 2, 3}},
    {{7, 0, 0, 0, 0}, {12, 2, 2, 0, 3}, {11, 2, 0, 2, 3}, {2, 0, 2, 2, 3}},
    {{8, 0, 0, 0, 0}, {13, 2, 2, 0, 3}, {12, 2, 0, 2, 3}, {3, 0, 2, 2, 3}},
    {{9, 0, 0, 0, 0}, {14, 2, 2, 0, 3}, {13, 2, 0, 2, 3}, {4, 0, 2, 2, 3}},
    {{10, 0, 0, 0, 0}, {5, 2, 2, 0, 3}, {6, 2, 0, 2, 3}, {15, 0, 2, 2, 3}},
    {{11, 0, 0, 0, 0}, {6, 2, 2, 0, 3}, {7, 2, 0, 2, 3}, {16, 0, 2, 2, 3}},
    {{12, 0, 0, 0, 0}, {7, 2, 2, 0, 3}, {8, 2, 0, 2, 3}, {17, 0, 2, 2, 3}},
    {{13, 0, 0, 0, 0}, {8, 2, 2, 0, 3}, {9, 2, 0, 2, 3}, {18, 0, 2, 2, 3}},
    {{14, 0, 0, 0, 0}, {9, 2, 2, 0, 3}, {5, 2, 0, 2, 3}, {19, 0, 2, 2, 3}},
    {{15, 0, 0, 0, 0}, {16, 2, 0, 2, 1}, {19, 2, 2, 0, 5}, {10, 0, 2, 2, 3}},
    {{16, 0, 0, 0, 0}, {17, 2, 0, 2, 1}, {15, 2, 2, 0, 5}, {11, 0, 2, 2, 3}},
    {{17, 0, 0, 0, 0}, {18, 2, 0, 2, 1}, {16, 2, 2, 0, 5}, {12, 0, 2, 2, 3}},
    {{18, 0, 0, 0, 0}, {19, 2, 0, 2, 1}, {17, 2, 2, 0, 5}, {13, 0, 2, 2, 3}},
    {{19, 0, 0, 0, 0}, {15, 2, 0, 2, 1}, {18, 2, 2, 0, 5}, {14, 0, 2, 2, 3}},
};
enum { kCenter = 0, kIJ = 1, kKI = 2, kJK = 3, kInvalidDir = -1 };

// adjacentFaceDir[from][to]: the quadrant of `from` that borders `to`
MGPU_HD int adjacent_face_dir(int from, int to) {
  int dir = from == to ? kCenter : kInvalidDir;
  for (int q = 1; q <= 3; ++q)
    if (kFaceNeighbors[from][q].face == to) dir = q;
  return dir;
}

// maxDimByCIIres / unitScaleByCIIres of an even (Class II) resolution: 2 * 7^(res/2), 7^(res/2)
MGPU_HD int unit_scale_cii(int res) {
  int u = 1;
  for (int r = 0; r < res; r += 2) u *= 7;
  return u;
}
MGPU_HD int max_dim_cii(int res) { return 2 * unit_scale_cii(res); }

MGPU_HD IJK ijk_add(IJK a, IJK b) { return IJK{a.i + b.i, a.j + b.j, a.k + b.k}; }
MGPU_HD IJK ijk_scale(IJK a, int s) { return IJK{a.i * s, a.j * s, a.k * s}; }
// sum of the three unit-vector images, then normalised (H3's _ijk* lattice maps)
MGPU_HD IJK ijk_map(IJK c, IJK iv, IJK jv, IJK kv) {
  IJK r = ijk_add(ijk_add(ijk_scale(iv, c.i), ijk_scale(jv, c.j)), ijk_scale(kv, c.k));
  h3::ijk_normalize(r);
  return r;
}
MGPU_HD void rotate60ccw(IJK& c) { c = ijk_map(c, {1, 1, 0}, {0, 1, 1}, {1, 0, 1}); }
MGPU_HD void rotate60cw(IJK& c) { c = ijk_map(c, {1, 0, 1}, {1, 1, 0}, {0, 1, 1}); }
MGPU_HD void down_ap3(IJK& c) { c = ijk_map(c, {2, 0, 1}, {1, 2, 0}, {0, 1, 2}); }
MGPU_HD void down_ap3r(IJK& c) { c = ijk_map(c, {2, 1, 0}, {0, 2, 1}, {1, 0, 2}); }
MGPU_HD bool class3(int res) { return res & 1; }

enum Overage { kNoOverage = 0, kFaceEdge = 1, kNewFace = 2 };

MGPU_HD Overage adjust_overage_class2(FaceIJK& f, int res, bool pent_leading4, bool substrate) {
  Overage ov = kNoOverage;
  IJK& ijk = f.c;
  int max_dim = max_dim_cii(res);
  if (substrate) max_dim *= 3;
  const int sum = ijk.i + ijk.j + ijk.k;
  if (substrate && sum == max_dim) {
    ov = kFaceEdge;
  } else if (sum > max_dim) {
    ov = kNewFace;
    int q;
    if (ijk.k > 0) {
      if (ijk.j > 0) {
        q = kJK;
      } else {
        q = kKI;
        if (pent_leading4) {  // the pentagon's missing sequence
          IJK origin{max_dim, 0, 0};
          IJK tmp{ijk.i - origin.i, ijk.j - origin.j, ijk.k - origin.k};
          rotate60cw(tmp);
          ijk = ijk_add(tmp, origin);
        }
      }
    } else {
      q = kIJ;
    }
    const FaceOrient o = kFaceNeighbors[f.face][q];
    f.face = o.face;
    for (int i = 0; i < o.rot; i++) rotate60ccw(ijk);
    int unit = unit_scale_cii(res);
    if (substrate) unit *= 3;
    ijk = ijk_add(ijk, IJK{o.ti * unit, o.tj * unit, o.tk * unit});
    h3::ijk_normalize(ijk);
    if (substrate && ijk.i + ijk.j + ijk.k == max_dim) ov = kFaceEdge;
  }
  return ov;
}

MGPU_HD bool is_pentagon_base(int bc) { return H3T_BASE_CELL_DATA[bc][4] != 0; }
MGPU_HD bool is_pentagon(uint64_t h) {
  const int res = (int)((h >> 52) & 15), bc = (int)((h >> 45) & 127);
  return is_pentagon_base(bc) && h3::leading_nonzero(h, res) == 0;
}

// An H3 cell id as the cell-geometry entries accept it: mode 1, a base cell below 122,
// digits 0..6 up to the resolution and 7 beyond it, and not in a pentagon's deleted
// (K axes) subsequence.  Everything cell_boundary and cell_center index by is then in range.
MGPU_HD bool is_valid_cell(uint64_t h) {
  const int res = (int)((h >> 52) & 15), bc = (int)((h >> 45) & 127);
  bool ok = (h >> 63) == 0 && ((h >> 59) & 15) == 1 && ((h >> 56) & 7) == 0 && bc < H3T_NUM_BASE_CELLS;
  for (int r = 1; r <= h3::kMaxRes; r++) {
    const int d = h3::digit_at(h, r);
    ok = ok && (r <= res ? d != 7 : d == 7);
  }
  if (ok && is_pentagon_base(bc) && h3::leading_nonzero(h, res) == 1) ok = false;
  return ok;
}

// _h3ToFaceIjk
MGPU_HD FaceIJK h3_to_face_ijk(uint64_t h) {
  const int bc = (int)((h >> 45) & 127);
  const int hres = (int)((h >> 52) & 15);
  if (is_pentagon_base(bc) && h3::leading_nonzero(h, hres) == 5) h = h3::rotate_cw(h, hres);
  FaceIJK f{H3T_BASE_CELL_DATA[bc][0], IJK{H3T_BASE_CELL_DATA[bc][1], H3T_BASE_CELL_DATA[bc][2], H3T_BASE_CELL_DATA[bc][3]}};
  // _h3ToFaceIjkWithInitializedFijk
  bool possible_overage = true;
  if (!is_pentagon_base(bc) && (hres == 0 || (f.c.i == 0 && f.c.j == 0 && f.c.k == 0))) possible_overage = false;
  for (int r = 1; r <= hres; ++r) {
    if (class3(r)) h3::down_ap7(f.c);
    else h3::down_ap7r(f.c);
    const int d = h3::digit_at(h, r);
    if (d > 0 && d < 7) {
      f.c.i += (d >> 2) & 1;
      f.c.j += (d >> 1) & 1;
      f.c.k += d & 1;
      h3::ijk_normalize(f.c);
    }
  }
  if (!possible_overage) return f;
  const IJK orig = f.c;
  int res = hres;
  if (class3(res)) {
    h3::down_ap7r(f.c);
    ++res;
  }
  const bool pent_leading4 = is_pentagon_base(bc) && h3::leading_nonzero(h, hres) == 4;
  if (adjust_overage_class2(f, res, pent_leading4, false) != kNoOverage) {
    if (is_pentagon_base(bc))
      while (adjust_overage_class2(f, res, false, false) != kNoOverage) {
      }
    if (res != hres) h3::up_ap7r(f.c);
  } else if (res != hres) {
    f.c = orig;
  }
  return f;
}

struct V2 {
  double x, y;
};
struct LatLon {
  double lat, lon;  // radians
};

// ---------------------------------------------------------------- math policies

// The host's libm, every call where H3 has it (glibc's sincos is not its sin and cos to the
// bit, so an Angle is the angle itself and sin / cos are taken at each use); host functions:
// only host code instantiates the templates below with it.
struct LibmMath {
  typedef double Angle;
  static double angle(double a) { return a; }
  static double sin(double a) { return ::sin(a); }
  static double cos(double a) { return ::cos(a); }
  static double asin(double a) { return ::asin(a); }
  static double atan(double a) { return ::atan(a); }
  static double tan(double a) { return ::tan(a); }
  static double atan2(double y, double x) { return ::atan2(y, x); }
  static double ld_add(double a, X::X80 c) { return X::ld_add(a, c); }
  static double ld_sub(double a, X::X80 c) { return X::ld_sub(a, c); }
  static double ld_mul(double a, X::X80 c) { return X::ld_mul(a, c); }
  static double ld_div(double a, X::X80 c) { return X::ld_div(a, c); }
  static bool ld_lt(double a, X::X80 c) { return X::ld_lt(a, c); }
  static bool ld_ge(double a, X::X80 c) { return X::ld_ge(a, c); }
};

// Correctly rounded functions (out of line on the device, as h3_core.h's lm_*) and the
// integer x87 emulation: the same bits on the host and the device.  An Angle holds its sine
// and cosine, computed once.
MGPU_LIBM double cm_asin(double a) { return X::cr_asin(a); }
struct CrMath {
  struct Angle {
    double s, c;
  };
  MGPU_HD static Angle angle(double a) {
    Angle r;
    h3::lm_sincos(a, &r.s, &r.c);
    return r;
  }
  MGPU_HD static double sin(const Angle& a) { return a.s; }
  MGPU_HD static double cos(const Angle& a) { return a.c; }
  MGPU_HD static void sincos(double a, double* s, double* c) { h3::lm_sincos(a, s, c); }
  MGPU_HD static double asin(double a) { return cm_asin(a); }
  MGPU_HD static double atan(double a) { return h3::lm_atan2(a, 1.0); }
  MGPU_HD static double tan(double a) { return h3::lm_tan(a); }
  MGPU_HD static double atan2(double y, double x) { return h3::lm_atan2(y, x); }
  MGPU_HD static double ld_add(double a, X::X80 c) { return X::em_add(a, c); }
  MGPU_HD static double ld_sub(double a, X::X80 c) { return X::em_sub(a, c); }
  MGPU_HD static double ld_mul(double a, X::X80 c) { return X::em_mul(a, c); }
  MGPU_HD static double ld_div(double a, X::X80 c) { return X::em_div(a, c); }
  MGPU_HD static bool ld_lt(double a, X::X80 c) { return X::em_lt(a, c); }
  MGPU_HD static bool ld_ge(double a, X::X80 c) { return X::em_ge(a, c); }
};

// _posAngleRads (h3::pos_angle under the policy)
template <class M>
MGPU_HD double pos_angle(double rads) {
  double tmp = (rads < 0.0) ? M::ld_add(rads, X::kX2Pi) : rads;
  if (M::ld_ge(rads, X::kX2Pi)) tmp = M::ld_sub(tmp, X::kX2Pi);
  return tmp;
}

// _ijkToHex2d (M_SQRT3_2 is a long double)
template <class M>
MGPU_HD V2 ijk_to_hex2d(IJK c) {
  const int i = c.i - c.k, j = c.j - c.k;
  return V2{i - 0.5 * j, M::ld_mul((double)j, X::kXSin60)};
}

MGPU_HD double constrain_lng(double l) {
  const double kPi = 3.14159265358979323846;
  while (l > kPi) l = l - (2 * kPi);
  while (l < -kPi) l = l + (2 * kPi);
  return l;
}

// _geoAzDistanceRads
template <class M>
MGPU_HD void geo_az_distance(double lat1, double lon1, double az, double dist, double* lat2, double* lon2) {
  const double kPi = 3.14159265358979323846, kPi2 = 1.5707963267948966;
  if (M::ld_lt(dist, X::kXEpsilon)) {
    *lat2 = lat1;
    *lon2 = lon1;
    return;
  }
  az = pos_angle<M>(az);
  if (M::ld_lt(az, X::kXEpsilon) || M::ld_lt(fabs(az - kPi), X::kXEpsilon)) {
    *lat2 = M::ld_lt(az, X::kXEpsilon) ? lat1 + dist : lat1 - dist;
    if (M::ld_lt(fabs(*lat2 - kPi2), X::kXEpsilon)) {
      *lat2 = kPi2;
      *lon2 = 0.0;
    } else if (M::ld_lt(fabs(*lat2 + kPi2), X::kXEpsilon)) {
      *lat2 = -kPi2;
      *lon2 = 0.0;
    } else {
      *lon2 = constrain_lng(lon1);
    }
    return;
  }
  // (M::Angle: the angle itself under libm, whose calls stay where H3 has them; its sine
  // and cosine, taken once, under the correctly rounded policy)
  const typename M::Angle a_lat1 = M::angle(lat1), a_dist = M::angle(dist), a_az = M::angle(az);
  double sinlat = M::sin(a_lat1) * M::cos(a_dist) + M::cos(a_lat1) * M::sin(a_dist) * M::cos(a_az);
  if (sinlat > 1.0) sinlat = 1.0;
  if (sinlat < -1.0) sinlat = -1.0;
  *lat2 = M::asin(sinlat);
  if (M::ld_lt(fabs(*lat2 - kPi2), X::kXEpsilon)) {
    *lat2 = kPi2;
    *lon2 = 0.0;
  } else if (M::ld_lt(fabs(*lat2 + kPi2), X::kXEpsilon)) {
    *lat2 = -kPi2;
    *lon2 = 0.0;
  } else {
    const typename M::Angle a_lat2 = M::angle(*lat2);
    double sinlon = M::sin(a_az) * M::sin(a_dist) / M::cos(a_lat2);
    double coslon = (M::cos(a_dist) - M::sin(a_lat1) * M::sin(a_lat2)) / M::cos(a_lat1) / M::cos(a_lat2);
    if (sinlon > 1.0) sinlon = 1.0;
    if (sinlon < -1.0) sinlon = -1.0;
    if (coslon > 1.0) coslon = 1.0;
    if (coslon < -1.0) coslon = -1.0;
    *lon2 = constrain_lng(lon1 + M::atan2(sinlon, coslon));
  }
}

// _hex2dToGeo -> (lat, lon) radians
template <class M>
MGPU_H3B_COLD void hex2d_to_geo(V2 v, int face, int res, bool substrate, double* lat, double* lon) {
  double r = sqrt(v.x * v.x + v.y * v.y);
  if (M::ld_lt(r, X::kXEpsilon)) {
    *lat = H3T_FACE_CENTER_GEO[face][0];
    *lon = H3T_FACE_CENTER_GEO[face][1];
    return;
  }
  double theta = M::atan2(v.y, v.x);
  for (int i = 0; i < res; i++) r = M::ld_div(r, X::kXSqrt7);
  if (substrate) {
    r /= 3.0;
    if (class3(res)) r = M::ld_div(r, X::kXSqrt7);
  }
  r *= h3::kRes0UGnomonic;
  r = M::atan(r);
  if (!substrate && class3(res)) theta = pos_angle<M>(M::ld_add(theta, X::kXAp7Rot));
  theta = pos_angle<M>(H3T_FACE_AXES_AZ_CII[face][0] - theta);
  geo_az_distance<M>(H3T_FACE_CENTER_GEO[face][0], H3T_FACE_CENTER_GEO[face][1], theta, r, lat, lon);
}

// _v2dIntersect (H3 keeps the parameter in a float)
MGPU_HD V2 v2d_intersect(V2 p0, V2 p1, V2 p2, V2 p3) {
  const V2 s1{p1.x - p0.x, p1.y - p0.y}, s2{p3.x - p2.x, p3.y - p2.y};
  const float t = (float)((s2.x * (p0.y - p2.y) - s2.y * (p0.x - p2.x)) / (-s2.x * s1.y + s1.x * s2.y));
  return V2{p0.x + (t * s1.x), p0.y + (t * s1.y)};
}
MGPU_HD bool v2d_equals(V2 a, V2 b) { return fabs(a.x - b.x) < FLT_EPSILON && fabs(a.y - b.y) < FLT_EPSILON; }

// the icosahedron face edge of the substrate triangle in quadrant `dir`
MGPU_HD void face_edge(int dir, int max_dim, V2* e0, V2* e1) {
  const V2 v0{3.0 * max_dim, 0.0};
  // 3.0 * M_SQRT3_2 * maxDim: long double throughout
  const double yy = X::x80_to_double(X::x80_mul(X::x80_mul(X::x80_from_double(3.0), X::kXSin60),
                                                X::x80_from_double((double)max_dim)));
  const V2 v1{-1.5 * max_dim, yy}, v2{-1.5 * max_dim, -yy};
  if (dir == kIJ) {
    *e0 = v0;
    *e1 = v1;
  } else if (dir == kJK) {
    *e0 = v1;
    *e1 = v2;
  } else {
    *e0 = v2;
    *e1 = v0;
  }
}

// ---------------------------------------------------------------- the boundary, edge by edge

// a cell's substrate frame: _faceIjkToVerts / _faceIjkPentToVerts up to the vertex offsets
struct CellFrame {
  FaceIJK center;  // _h3ToFaceIjk
  IJK sub;         // the centre in the substrate grid (Class II: adj_res)
  int res, adj_res;
  bool pent;
  MGPU_HD int nv() const { return pent ? 5 : 6; }
};

MGPU_HD CellFrame cell_frame(uint64_t h) {
  CellFrame f;
  f.res = f.adj_res = (int)((h >> 52) & 15);
  f.center = h3_to_face_ijk(h);
  f.pent = is_pentagon(h);
  f.sub = f.center.c;
  down_ap3(f.sub);
  down_ap3r(f.sub);
  if (class3(f.res)) {
    h3::down_ap7r(f.sub);
    f.adj_res += 1;
  }
  return f;
}

// the vertex offsets of _faceIjkToVerts (a pentagon takes the first five), a nibble each:
//   Class II  {2,1,0} {1,2,0} {0,2,1} {0,1,2} {1,0,2} {2,0,1}
//   Class III {5,4,0} {1,5,0} {0,5,4} {0,1,5} {4,0,5} {5,0,1}
MGPU_HD IJK vertex_offset(bool c3, int v) {
  const uint32_t pi = c3 ? 0x540015u : 0x210012u, pj = c3 ? 0x001554u : 0x001221u, pk = c3 ? 0x155400u : 0x122100u;
  return IJK{(int)((pi >> (4 * v)) & 15u), (int)((pj >> (4 * v)) & 15u), (int)((pk >> (4 * v)) & 15u)};
}

// substrate vertex v on the centre's face, before any overage
MGPU_HD FaceIJK substrate_vertex(const CellFrame& f, int v) {
  FaceIJK g{f.center.face, ijk_add(f.sub, vertex_offset(class3(f.res), v))};
  h3::ijk_normalize(g.c);
  return g;
}

// ... moved onto the face it lies on (a pentagon's vertex may cross two face edges)
MGPU_HD FaceIJK adjusted_vertex(const CellFrame& f, int v, Overage* ov) {
  FaceIJK g = substrate_vertex(f, v);
  if (f.pent) {
    while (adjust_overage_class2(g, f.adj_res, false, true) == kNewFace) {
    }
    *ov = kNoOverage;
  } else {
    *ov = adjust_overage_class2(g, f.adj_res, false, true);
  }
  return g;
}

// a substrate vertex's position: hex2d_to_geo of its hex2d point (a pure function of the
// face, the normalized ijk and the resolution: callers may memoize it)
template <class M>
struct VertexGeoT {
  MGPU_HD LatLon operator()(const FaceIJK& f, int adj_res) const {
    LatLon p;
    hex2d_to_geo<M>(ijk_to_hex2d<M>(f.c), f.face, adj_res, true, &p.lat, &p.lon);
    return p;
  }
};

// The distortion vertex of the edge from vertex a (fa, its overage ova) to vertex
// b = a + 1 (fb), if the edge has one: a Class III edge that crosses an icosahedron edge.
// *inter on *face is its substrate hex2d point (hex2d_to_geo at adj_res gives its position).
template <class M>
MGPU_HD bool edge_distortion(const CellFrame& f, int a, int b, const FaceIJK& fa, Overage ova, const FaceIJK& fb, V2* inter,
                             int* face) {
  if (!class3(f.res)) return false;
  if (f.pent) {
    // all Class III pentagon edges cross icosahedron edges
    FaceIJK tmp = fb;
    const V2 orig0 = ijk_to_hex2d<M>(fa.c);
    const int dir = adjacent_face_dir(tmp.face, fa.face);
    const FaceOrient o = kFaceNeighbors[tmp.face][dir < 0 ? 0 : dir];  // (the faces of an edge's ends are adjacent)
    tmp.face = o.face;
    for (int i = 0; i < o.rot; i++) rotate60ccw(tmp.c);
    const int unit = unit_scale_cii(f.adj_res) * 3;
    tmp.c = ijk_add(tmp.c, IJK{o.ti * unit, o.tj * unit, o.tk * unit});
    h3::ijk_normalize(tmp.c);
    const V2 orig1 = ijk_to_hex2d<M>(tmp.c);
    V2 e0, e1;
    face_edge(adjacent_face_dir(tmp.face, fb.face), max_dim_cii(f.adj_res), &e0, &e1);
    *inter = v2d_intersect(orig0, orig1, e0, e1);
    *face = tmp.face;
    return true;
  }
  if (fb.face == fa.face || ova == kFaceEdge) return false;
  const V2 orig0 = ijk_to_hex2d<M>(substrate_vertex(f, a).c), orig1 = ijk_to_hex2d<M>(substrate_vertex(f, b).c);
  const int face2 = fa.face == f.center.face ? fb.face : fa.face;
  V2 e0, e1;
  face_edge(adjacent_face_dir(f.center.face, face2), max_dim_cii(f.adj_res), &e0, &e1);
  *inter = v2d_intersect(orig0, orig1, e0, e1);
  *face = f.center.face;
  return !(v2d_equals(orig0, *inter) || v2d_equals(orig1, *inter));
}

// h3ToGeoBoundary: at most 10 vertices (a Class III pentagon's), radians, H3's order, not closed
constexpr int kMaxBoundaryVerts = 10;
struct Boundary {
  int n = 0;
  LatLon v[kMaxBoundaryVerts];
  MGPU_HD size_t size() const { return (size_t)n; }
  MGPU_HD const LatLon& operator[](size_t k) const { return v[k]; }
  MGPU_HD const LatLon* begin() const { return v; }
  MGPU_HD const LatLon* end() const { return v + n; }
  MGPU_HD void push(LatLon p) {
    if (n < kMaxBoundaryVerts) v[n++] = p;
  }
};

// `vertex` computes the cell's own substrate vertices (the distortion vertices on
// icosahedron edges are computed here)
template <class M, class Vertex>
MGPU_HD Boundary cell_boundary_m(uint64_t h, const Vertex& vertex) {
  const CellFrame f = cell_frame(h);
  const int nv = f.nv();
  Boundary g;
  Overage ova;
  FaceIJK fa = adjusted_vertex(f, 0, &ova);
  for (int a = 0; a < nv; a++) {
    g.push(vertex(fa, f.adj_res));
    const int b = a + 1 < nv ? a + 1 : 0;
    Overage ovb;
    const FaceIJK fb = adjusted_vertex(f, b, &ovb);
    V2 inter;
    int face;
    if (edge_distortion<M>(f, a, b, fa, ova, fb, &inter, &face)) {
      LatLon p;
      hex2d_to_geo<M>(inter, face, f.adj_res, true, &p.lat, &p.lon);
      g.push(p);
    }
    fa = fb;
    ova = ovb;
  }
  return g;
}

// h3ToGeo: _h3ToFaceIjk then _faceIjkToGeo (radians)
template <class M>
MGPU_HD LatLon cell_center_m(uint64_t h) {
  const FaceIJK f = h3_to_face_ijk(h);
  LatLon p;
  hex2d_to_geo<M>(ijk_to_hex2d<M>(f.c), f.face, (int)((h >> 52) & 15), false, &p.lat, &p.lon);
  return p;
}

// the libm policy under the names the tessellator and the chip-table builder use (host)
using VertexGeo = VertexGeoT<LibmMath>;
template <class Vertex = VertexGeo>
inline Boundary cell_boundary(uint64_t h, const Vertex& vertex = Vertex()) {
  return cell_boundary_m<LibmMath>(h, vertex);
}
inline LatLon cell_center(uint64_t h) { return cell_center_m<LibmMath>(h); }

// JDK 8 Math.toDegrees (H3-Java converts each coordinate)
MGPU_HD double to_degrees(double rad) { return rad * 180.0 / 3.14159265358979323846; }

}  // namespace h3b
}  // namespace mgpu

// grid_polyfill: the cells of a polygon -- IndexSystem.polyfill (IndexSystem.scala:166;
// H3IndexSystem.scala:134-154; BNGIndexSystem.scala:185-209) as its documented definition,
// "the set of grid indices whose centroid is contained in the geometry".  What the kernels
// of polyfill.hip and the host twin (mgpu_test_grid_polyfill_host, polyfill_host.cpp) share:
// the plan the host lays over a polygon set, a sample's cell / centre / owner, and the
// PointLocator verdict over per-ring RayCrossingCounter bits (pip_core.h count_segment).
//
// H3.  A lon/lat lattice over each polygon's bounding box, padded by a step, spacing
// 0.7 x the smallest centre-to-edge distance (degree space) of the cells at the box's
// corners and middle.  Sample j of the lattice computes its cell c, c's centre (h3ToGeo,
// the correctly rounded route of h3_boundary.h) and the lattice point q nearest that
// centre; it OWNS c iff q == j, so a cell is produced once, by the sample nearest its
// centre, with no sort and no dedupe.  A sample that is not the owner checks that the
// lattice point q maps to c as well (the certificate): then the lane of q owns c.  A cell
// is lost only if no sample falls into it at all.
// BNG.  The lattice is the grid: one sample per cell position of the bounding box, every
// sample an owner; the centre is JTS Centroid of the ring of indexToGeometry's corners.
//
// Containment is planar JTS PointLocator: a part holds the centre iff its shell's ring
// location is INTERIOR and every hole's EXTERIOR; the polygon holds it iff a part does.
// The rings reach the test in chunks (at most kChunkVerts vertices and kChunkPieces ring
// pieces each; a ring longer than a chunk continues in the next, its bits carried).
#pragma once
#include <stdint.h>

#include <vector>

#include "bng_core.h"
#include "cell_geom.h"
#include "geom_decode.h"
#include "h3_boundary.h"
#include "pip_core.h"

namespace mgpu {
namespace polyfill {

constexpr int kTile = 256;          // samples per tile (one workgroup)
constexpr int kChunkVerts = 1024;   // vertices of a ring chunk (16 KiB of LDS)
constexpr int kChunkPieces = 32;    // ring pieces of a chunk (one bit each)
constexpr int kMaxAttempts = 4;     // the first run and three at half the spacing each
constexpr double kSpacing = 0.7;    // lattice step / smallest centre-to-edge distance
constexpr int64_t kMaxSamples = 2147483647LL;

struct PolyParam {
  double x0, y0, sx, sy;  // sample (ix, iy) = (x0 + ix * sx, y0 + iy * sy); BNG: the cell's corner, sx = sy = edge
  double env[4];          // the polygon's envelope: min x, min y, max x, max y
  int32_t nx, ny;
  int32_t n_chunks, pad;
  int64_t chunk0;
};

struct Chunk {
  int64_t v0;  // first vertex (an (x, y) pair of xy)
  int32_t nv;  // vertices
  int32_t np;  // ring pieces
  // bit i: piece i ends its ring / that ring is a shell / it is the last ring of its part
  uint32_t ends, shell, part_last;
  uint16_t start[kChunkPieces + 1];  // piece i = the chunk's vertices [start[i], start[i + 1])
  uint16_t pad;
};
static_assert(sizeof(Chunk) == 96, "the chunk table is uploaded as the host lays it out");

struct Tile {
  int32_t poly;
  uint32_t j0;  // the tile's first sample of that polygon's lattice
};

// PointLocator over the rings in order, a chunk at a time
struct Verdict {
  uint32_t carry_b = 0, carry_p = 0, part_ok = 0, matched = 0;
};

MGPU_HDI void fold_chunk(int np, uint32_t ends, uint32_t shell, uint32_t part_last, uint32_t bnd, uint32_t par, Verdict& v) {
  for (int i = 0; i < np; i++) {
    v.carry_b |= (bnd >> i) & 1u;
    v.carry_p ^= (par >> i) & 1u;
    if (!((ends >> i) & 1u)) continue;
    const int loc = v.carry_b ? pip::kBoundary : (v.carry_p ? pip::kInterior : pip::kExterior);
    if ((shell >> i) & 1u)
      v.part_ok = loc == pip::kInterior;
    else
      v.part_ok &= (uint32_t)(loc == pip::kExterior);
    if ((part_last >> i) & 1u) v.matched |= v.part_ok;
    v.carry_b = v.carry_p = 0;
  }
}

// the bits of the chunk's edges first, first + stride, ... for the point (px, py):
// vtx = the chunk's vertices as (x, y) pairs
MGPU_HDI void chunk_bits(const double* vtx, int nv, const uint16_t* start, double px, double py, int first, int stride,
                         uint32_t* bnd_out, uint32_t* par_out) {
  uint32_t bnd = 0, par = 0;
  int pi = 0;
  for (int e = first; e + 1 < nv; e += stride) {
    while (e >= (int)start[pi + 1]) pi++;
    if (e + 1 >= (int)start[pi + 1]) continue;  // a ring break
    // RayCrossingCounter.locatePointInRing: p1 = ring[i], p2 = ring[i - 1]
    const int bits = pip::count_segment(vtx[2 * e + 2], vtx[2 * e + 3], vtx[2 * e], vtx[2 * e + 1], px, py);
    bnd |= (uint32_t)(bits & 1) << pi;
    par ^= (uint32_t)((bits >> 1) & 1) << pi;
  }
  *bnd_out = bnd;
  *par_out = par;
}

struct Sample {
  bool own = false;        // the sample produces `cell`
  bool cert_fail = false;  // H3: the lattice point nearest the centre maps to another cell
  int64_t cell = 0;
  double cx = 0, cy = 0;
};

MGPU_HDI double clampd(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// geoToH3 of a sample: the fast projection (h3_core.h fast_hex2d), whose cell is the H3
// route's outside its tie band; inside it, the route itself.  (A sample in the band lies on a
// cell edge, at least an inradius from that cell's centre: it owns nothing either way.)
MGPU_HD uint64_t sample_cell(double x, double y, int res, double k_res) {
  const h3::FastHex f = h3::fast_hex2d(h3::to_radians_fast(y), h3::to_radians_fast(x), res, k_res, 0xFFFFFu);
  if (!f.tie) return h3::face_ijk_to_h3_fast(f.face, f.ijk, res);
  bool tie;
  return h3::point_to_cell(x, y, res, &tie);
}

// H3 sample j of polygon P; k_res = h3::k_of_res(res)
template <class M>
MGPU_HD Sample h3_sample(const PolyParam& P, int res, double k_res, uint32_t j) {
  Sample s;
  const uint32_t nx = (uint32_t)P.nx;
  uint32_t at = j;
  uint64_t c = 0;
  uint32_t q = 0;
  bool inside = false;
  // (one call site of the projection: round 1 is the certificate's)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int round = 0; round < 2; round++) {
    const uint32_t ix = at % nx, iy = at / nx;
    // (the padding may leave the globe: the sample is taken at the nearest point on it)
    const double x = clampd(P.x0 + (double)ix * P.sx, -180.0, 180.0), y = clampd(P.y0 + (double)iy * P.sy, -90.0, 90.0);
    const uint64_t h = sample_cell(x, y, res, k_res);
    if (round == 1) {
      s.cert_fail = h != c;
      break;
    }
    c = h;
    if (!c) break;
    const h3b::LatLon g = h3b::cell_center_m<M>(c);
    s.cx = h3b::to_degrees(g.lon);
    s.cy = h3b::to_degrees(g.lat);
    const double rx = rint((s.cx - P.x0) / P.sx), ry = rint((s.cy - P.y0) / P.sy);
    inside = rx >= 0.0 && rx < (double)P.nx && ry >= 0.0 && ry < (double)P.ny;
    if (!inside) break;
    q = (uint32_t)ry * nx + (uint32_t)rx;
    if (q == j) {
      s.own = true;
      break;
    }
    at = q;
  }
  s.cell = (int64_t)c;
  return s;
}

// the closed ring of BNGIndexSystem.indexToGeometry's corners, as a point sequence
struct SquareSeq {
  double x0, y0, x1, y1;
  uint32_t n;
  MGPU_HDI double x(int64_t i) const { return (i == 1 || i == 2) ? x1 : x0; }
  MGPU_HDI double y(int64_t i) const { return (i == 2 || i == 3) ? y1 : y0; }
};

// BNG sample j of polygon P: the cell of that grid position, if isValid accepts it
MGPU_HDI Sample bng_sample(const PolyParam& P, int res, uint32_t j) {
  Sample s;
  const uint32_t nx = (uint32_t)P.nx;
  const uint32_t ix = j % nx, iy = j / nx;
  const double px = P.x0 + ((double)ix + 0.5) * P.sx, py = P.y0 + ((double)iy + 0.5) * P.sy;
  int64_t id = 0;
  if (!bng::point_to_cell(px, py, res, &id) || bng::valid_state(id) != 1) return s;
  int r, xl, yl;
  int32_t e, x, y;
  if (!bng::cell_corner(id, &r, &e, &x, &y, &xl, &yl)) return s;
  const int32_t x1 = (int32_t)((uint32_t)x + (uint32_t)e), y1 = (int32_t)((uint32_t)y + (uint32_t)e);
  const SquareSeq ring{(double)x, (double)y, (double)x1, (double)y1, 5u};
  geom::Centroid c;
  c.add_ring(ring, true);
  if (c.result(&s.cx, &s.cy) != geom::kDecOk) return s;
  s.cell = id;
  s.own = true;
  return s;
}

// What the host lays over a polygon set (polyfill_host.cpp).  `shrink`: 1, then 1/2, 1/4, 1/8
// of the H3 spacing after a certificate failure.
struct Plan {
  std::vector<PolyParam> polys;
  std::vector<Chunk> chunks;
  std::vector<Tile> tiles;
  std::vector<int64_t> first_tile;  // [n_polys + 1] polygon p's tiles are [first_tile[p], first_tile[p + 1])
  int64_t samples = 0, n_verts = 0;
};
int32_t check_polygons(const char* what, int32_t is, int32_t res, int64_t n_polys, const int64_t* poly_part_off,
                       const int64_t* part_ring_off, const int64_t* ring_off, const double* xy);
int32_t build_plan(const char* what, int32_t is, int32_t res, int64_t n_polys, const int64_t* poly_part_off,
                   const int64_t* part_ring_off, const int64_t* ring_off, const double* xy, double shrink, Plan* out);
// the last call's figures on this thread (mgpu_test_grid_polyfill_last): samples, tiles, certificate failures
// (all attempts), attempts, device microseconds of the last attempt's launches (the host twin: 0)
void note_last(int64_t samples, int64_t tiles, int64_t cert_failures, int64_t attempts, int64_t kernel_us);

}  // namespace polyfill
}  // namespace mgpu

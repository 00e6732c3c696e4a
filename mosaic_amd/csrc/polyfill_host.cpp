// grid_polyfill, the host side (polyfill.h has the algorithm): the checks of a polygon set,
// the plan -- lattices, ring chunks and tiles -- that mgpu_grid_polyfill uploads, and the
// kernels' host twin, mgpu_test_grid_polyfill_host, which walks the same plan with the same
// code sample by sample.  Built for the host without FMA contraction: the device's bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/mosaic_gpu.h"
#include "error.h"
#include "parallel.h"
#include "polyfill.h"

namespace mgpu {
namespace polyfill {

namespace {

using M = h3b::CrMath;

thread_local int64_t g_last[8] = {0, 0, 0, 0, 0, 0, 0, 0};

double seg_dist(double px, double py, double ax, double ay, double bx, double by) {
  const double dx = bx - ax, dy = by - ay, l2 = dx * dx + dy * dy;
  double t = l2 > 0.0 ? ((px - ax) * dx + (py - ay) * dy) / l2 : 0.0;
  t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
  return std::hypot(px - (ax + t * dx), py - (ay + t * dy));
}

// the smallest centre-to-edge distance, in degrees of lon / lat, of the cell holding (x, y)
double cell_inradius_deg(double x, double y, int res) {
  bool tie;
  const uint64_t c = h3::point_to_cell(x, y, res, &tie);
  if (!c) return 0.0;
  const h3b::LatLon g = h3b::cell_center_m<M>(c);
  const double cx = h3b::to_degrees(g.lon), cy = h3b::to_degrees(g.lat);
  const h3b::Boundary b = h3b::cell_boundary_m<M>(c, h3b::VertexGeoT<M>());
  double vx[h3b::kMaxBoundaryVerts], vy[h3b::kMaxBoundaryVerts];
  for (int k = 0; k < b.n; k++) {
    double lon = h3b::to_degrees(b.v[k].lon);
    // (a cell across the antimeridian: its vertices on the centre's side)
    if (lon - cx > 180.0) lon -= 360.0;
    if (lon - cx < -180.0) lon += 360.0;
    vx[k] = lon, vy[k] = h3b::to_degrees(b.v[k].lat);
  }
  double r = INFINITY;
  for (int k = 0; k < b.n; k++) {
    const int k1 = k + 1 < b.n ? k + 1 : 0;
    r = std::min(r, seg_dist(cx, cy, vx[k], vy[k], vx[k1], vy[k1]));
  }
  return std::isfinite(r) ? r : 0.0;
}

}  // namespace

void note_last(int64_t samples, int64_t tiles, int64_t cert_failures, int64_t attempts, int64_t kernel_us) {
  g_last[0] = samples, g_last[1] = tiles, g_last[2] = cert_failures, g_last[3] = attempts, g_last[4] = kernel_us;
}

int32_t check_polygons(const char* what, int32_t is, int32_t res, int64_t n_polys, const int64_t* ppo, const int64_t* pro,
                       const int64_t* ro, const double* xy) {
  if (int32_t st = mgpu_check_resolution(is, res)) return st;
  if (n_polys < 0 || (n_polys > 0 && (!ppo || !pro || !ro))) return set_error(MGPU_E_INVALID_ARG, "%s: bad polygon arrays", what);
  // the three offset arrays start at 0 and never step back: parts, rings and vertices are then
  // contiguous, and ring_off's last entry is the number of vertices
  if (n_polys > 0 && (ppo[0] != 0 || pro[0] != 0 || ro[0] != 0))
    return set_error(MGPU_E_INVALID_ARG, "%s: the offset arrays must start at 0", what);
  for (int64_t p = 0; p < n_polys; p++) {
    if (ppo[p + 1] < ppo[p]) return set_error(MGPU_E_INVALID_ARG, "%s: poly_part_off decreases at polygon %lld", what, (long long)p);
    for (int64_t q = ppo[p]; q < ppo[p + 1]; q++) {
      if (pro[q + 1] <= pro[q]) return set_error(MGPU_E_INVALID_ARG, "%s: part %lld has no ring", what, (long long)q);
      for (int64_t r = pro[q]; r < pro[q + 1]; r++) {
        const int64_t a = ro[r], b = ro[r + 1];
        if (a < 0 || b < a) return set_error(MGPU_E_INVALID_ARG, "%s: ring_off decreases at ring %lld", what, (long long)r);
        if (b - a < 4 || !xy) return set_error(MGPU_E_INVALID_ARG, "%s: ring %lld has fewer than 4 points", what, (long long)r);
        for (int64_t v = a; v < b; v++) {
          const double x = xy[2 * v], y = xy[2 * v + 1];
          if (!std::isfinite(x) || !std::isfinite(y))
            return set_error(MGPU_E_INVALID_ARG, "%s: ring %lld has a non-finite coordinate", what, (long long)r);
          if (is == MGPU_H3 && (x < -180.0 || x > 180.0 || y < -90.0 || y > 90.0))
            return set_error(MGPU_E_INVALID_ARG, "%s: ring %lld leaves [-180, 180] x [-90, 90]", what, (long long)r);
        }
        if (xy[2 * a] != xy[2 * (b - 1)] || xy[2 * a + 1] != xy[2 * (b - 1) + 1])
          return set_error(MGPU_E_INVALID_ARG, "%s: ring %lld is not closed", what, (long long)r);
      }
    }
  }
  return MGPU_OK;
}

int32_t build_plan(const char* what, int32_t is, int32_t res, int64_t n_polys, const int64_t* ppo, const int64_t* pro,
                   const int64_t* ro, const double* xy, double shrink, Plan* out) {
  Plan& P = *out;
  P = Plan();
  P.polys.resize((size_t)n_polys);
  P.first_tile.assign((size_t)n_polys + 1, 0);
  // the lattices, polygon by polygon in parallel (H3: five cell boundaries each); errors in polygon order after
  enum { kOk = 0, kWide, kNoSize, kTooMany };
  std::vector<uint8_t> err((size_t)n_polys, kOk);
  parallel_for(n_polys, 16, [&](int64_t pb, int64_t pe, int) {
    for (int64_t p = pb; p < pe; p++) {
      PolyParam& pp = P.polys[(size_t)p];
      pp = PolyParam{};
      if (ppo[p + 1] == ppo[p]) continue;  // no parts: an empty list
      double e[4] = {INFINITY, INFINITY, -INFINITY, -INFINITY};
      for (int64_t q = ppo[p]; q < ppo[p + 1]; q++)
        for (int64_t v = ro[pro[q]]; v < ro[pro[q + 1]]; v++) {
          e[0] = std::min(e[0], xy[2 * v]), e[1] = std::min(e[1], xy[2 * v + 1]);
          e[2] = std::max(e[2], xy[2 * v]), e[3] = std::max(e[3], xy[2 * v + 1]);
        }
      for (int k = 0; k < 4; k++) pp.env[k] = e[k];
      double nx, ny;
      if (is == MGPU_H3) {
        if (e[2] - e[0] >= 180.0) {
          err[(size_t)p] = kWide;
          continue;
        }
        const double mx = e[0] + (e[2] - e[0]) / 2, my = e[1] + (e[3] - e[1]) / 2;
        const double px[5] = {e[0], e[2], e[0], e[2], mx}, py[5] = {e[1], e[1], e[3], e[3], my};
        double r = INFINITY;
        for (int k = 0; k < 5; k++) r = std::min(r, cell_inradius_deg(px[k], py[k], res));
        if (!(r > 0.0) || !std::isfinite(r)) {
          err[(size_t)p] = kNoSize;
          continue;
        }
        const double s = kSpacing * r * shrink;
        pp.sx = pp.sy = s;
        pp.x0 = e[0] - s, pp.y0 = e[1] - s;
        nx = std::ceil((e[2] - e[0]) / s) + 3.0, ny = std::ceil((e[3] - e[1]) / s) + 3.0;
      } else {
        const double edge = (double)bng::edge_of_res(res);
        // the grid positions of the box, inside what isValid accepts: x in [0, 700000], y in [0, 1300000]
        const double ix0 = std::max(std::floor(e[0] / edge), 0.0), iy0 = std::max(std::floor(e[1] / edge), 0.0);
        const double ix1 = std::min(std::floor(e[2] / edge), std::floor(700000.0 / edge));
        const double iy1 = std::min(std::floor(e[3] / edge), std::floor(1300000.0 / edge));
        pp.sx = pp.sy = edge;
        pp.x0 = ix0 * edge, pp.y0 = iy0 * edge;
        nx = ix1 - ix0 + 1.0, ny = iy1 - iy0 + 1.0;
        if (nx < 1.0 || ny < 1.0) nx = ny = 0.0;  // outside the grid
      }
      if (nx * ny > (double)kMaxSamples) {
        err[(size_t)p] = kTooMany;
        continue;
      }
      pp.nx = (int32_t)nx, pp.ny = (int32_t)ny;
    }
  });
  for (int64_t p = 0; p < n_polys; p++) {
    PolyParam& pp = P.polys[(size_t)p];
    if (err[(size_t)p] == kWide)
      return set_error(MGPU_E_UNSUPPORTED, "%s: polygon %lld spans %g degrees of longitude (180 or more: the reference's "
                       "transmeridian heuristics are not built)", what, (long long)p, pp.env[2] - pp.env[0]);
    if (err[(size_t)p] == kNoSize) return set_error(MGPU_E_INTERNAL, "%s: polygon %lld: no cell size at its box", what, (long long)p);
    if (err[(size_t)p] == kTooMany)
      return set_error(MGPU_E_INVALID_ARG, "%s: polygon %lld needs a lattice of more than 2^31 - 1 samples", what, (long long)p);
    P.first_tile[(size_t)p] = (int64_t)P.tiles.size();
    if (ppo[p + 1] == ppo[p]) continue;
    // the rings in chunks: a ring longer than a chunk continues in the next from its last vertex
    pp.chunk0 = (int64_t)P.chunks.size();
    Chunk c{};
    bool open = false;
    auto flush = [&]() {
      if (open) P.chunks.push_back(c);
      open = false;
    };
    for (int64_t q = ppo[p]; q < ppo[p + 1]; q++)
      for (int64_t r = pro[q]; r < pro[q + 1]; r++) {
        int64_t a = ro[r];
        const int64_t b = ro[r + 1];
        while (a < b - 1) {  // vertices [a, b) are left, a the last one already walked to
          // a piece starts where the chunk's vertices end, so the chunk must continue xy there
          if (open && (c.np == kChunkPieces || c.nv > kChunkVerts - 2 || c.v0 + c.nv != a)) flush();
          if (!open) {
            c = Chunk{};
            c.v0 = a;
            open = true;
          }
          const int64_t take = std::min<int64_t>(b - a, kChunkVerts - c.nv);
          const int i = c.np++;
          c.start[i] = (uint16_t)c.nv;
          c.nv += (int32_t)take;
          c.start[i + 1] = (uint16_t)c.nv;
          if (a + take == b) {
            c.ends |= 1u << i;
            if (r == pro[q]) c.shell |= 1u << i;
            if (r + 1 == pro[q + 1]) c.part_last |= 1u << i;
            a = b;
          } else {
            a += take - 1;
            flush();
          }
        }
      }
    flush();
    pp.n_chunks = (int32_t)((int64_t)P.chunks.size() - pp.chunk0);
    const int64_t n = (int64_t)pp.nx * pp.ny;
    for (int64_t j = 0; j < n; j += kTile) P.tiles.push_back(Tile{(int32_t)p, (uint32_t)j});
    P.samples += n;
  }
  P.first_tile[(size_t)n_polys] = (int64_t)P.tiles.size();
  P.n_verts = n_polys > 0 ? ro[pro[ppo[n_polys]]] : 0;
  return MGPU_OK;
}

}  // namespace polyfill
}  // namespace mgpu

extern "C" {

int32_t mgpu_test_grid_polyfill_host(int32_t index_system, int32_t res, int64_t n_polys, const int64_t* poly_part_off,
                                     const int64_t* part_ring_off, const int64_t* ring_off, const double* xy,
                                     int64_t* out_cells, int64_t capacity, int64_t* out_offsets, int64_t* out_total) {
  namespace PF = mgpu::polyfill;
  const char* what = "grid_polyfill (host)";
  if (int32_t st = PF::check_polygons(what, index_system, res, n_polys, poly_part_off, part_ring_off, ring_off, xy)) return st;
  if (!out_offsets || !out_total || capacity < 0 || (capacity > 0 && !out_cells))
    return mgpu::set_error(MGPU_E_INVALID_ARG, "%s: bad output buffers", what);
  int64_t fails_all = 0;
  double shrink = 1.0;
  const double k_res = index_system == MGPU_H3 ? mgpu::h3::k_of_res(res) : 0.0;
  for (int attempt = 1; attempt <= PF::kMaxAttempts; attempt++, shrink /= 2) {
    PF::Plan plan;
    if (int32_t st = PF::build_plan(what, index_system, res, n_polys, poly_part_off, part_ring_off, ring_off, xy, shrink, &plan)) return st;
    // polygons are independent: their lists in parallel, then concatenated in input order
    std::vector<std::vector<int64_t>> lists((size_t)n_polys);
    std::atomic<int64_t> fails_now{0};
    mgpu::parallel_for(n_polys, 1, [&](int64_t pb, int64_t pe, int) {
      for (int64_t p = pb; p < pe; p++) {
        const PF::PolyParam& pp = plan.polys[(size_t)p];
        const int64_t n = (int64_t)pp.nx * pp.ny;
        int64_t f = 0;
        for (int64_t j = 0; j < n; j++) {
          const PF::Sample s = index_system == MGPU_BNG ? PF::bng_sample(pp, res, (uint32_t)j) : PF::h3_sample<mgpu::h3b::CrMath>(pp, res, k_res, (uint32_t)j);
          f += s.cert_fail ? 1 : 0;
          if (!s.own || !mgpu::pip::env_has(pp.env, s.cx, s.cy)) continue;
          PF::Verdict v;
          for (int64_t ci = pp.chunk0; ci < pp.chunk0 + pp.n_chunks; ci++) {
            const PF::Chunk& c = plan.chunks[(size_t)ci];
            uint32_t bnd, par;
            PF::chunk_bits(xy + 2 * c.v0, c.nv, c.start, s.cx, s.cy, 0, 1, &bnd, &par);
            PF::fold_chunk(c.np, c.ends, c.shell, c.part_last, bnd, par, v);
          }
          if (v.matched) lists[(size_t)p].push_back(s.cell);
        }
        fails_now += f;
      }
    });
    int64_t total = 0;
    const int64_t fails = fails_now.load();
    for (int64_t p = 0; p < n_polys; p++) {
      out_offsets[p] = total;
      for (int64_t c : lists[(size_t)p]) {
        if (total < capacity) out_cells[total] = c;
        total++;
      }
    }
    out_offsets[n_polys] = total;
    *out_total = total;
    fails_all += fails;
    PF::note_last(plan.samples, (int64_t)plan.tiles.size(), fails_all, attempt, 0);
    if (fails) continue;  // the spacing was too coarse for some cell: again at half of it
    if (total > capacity)
      return mgpu::set_error(MGPU_E_CAPACITY, "%s: %lld cells needed, %lld given", what, (long long)total, (long long)capacity);
    return MGPU_OK;
  }
  return mgpu::set_error(MGPU_E_INTERNAL, "%s: the certificate failed at every spacing (%lld failures)", what, (long long)fails_all);
}

int32_t mgpu_test_grid_polyfill_last(int64_t* out8) {
  if (!out8) return mgpu::set_error(MGPU_E_INVALID_ARG, "grid_polyfill_last: out8 is NULL");
  for (int k = 0; k < 8; k++) out8[k] = mgpu::polyfill::g_last[k];
  return MGPU_OK;
}

}  // extern "C"

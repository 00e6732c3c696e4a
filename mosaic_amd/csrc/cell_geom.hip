// Cell id -> geometry on the device: centres, boundaries, WKB and areas of a cell column --
// IndexSystem.indexToCenter / indexToBoundary / indexToGeometry / area
// (IndexSystem.scala:223, :239-245, :248-291; H3IndexSystem.scala:103-112, :230-237;
// BNGIndexSystem.scala:418-431, :510-524), what grid_boundaryaswkb, grid_boundary and
// grid_cellarea compute per row (IndexGeometry.scala:65-75, CellArea.scala).  Kernels and
// host entry of the mgpu_cells_* calls (include/mosaic_gpu.h has the contract).
//
// H3.  A cell costs 6 to 10 projections (h3_boundary.h hex2d_to_geo under its correctly
// rounded policy: double-double trigonometry, the x87 expressions in 128-bit integers), so
// cell_boundary_kernel spreads them: 8 lanes per cell, lane v < 6 takes substrate vertex v
// and the distortion vertex of the edge v -> v + 1, lane 7 the centre (h3ToGeo) when it is
// wanted.  The integer part -- the cell's frame, a vertex's face and overage, its
// successor's -- is recomputed by every lane that needs it; all lanes meet in one call of
// the projection, the few with a distortion vertex in a second one.  Output positions come
// from a ballot over the 8 lanes, so no lane indexes a private array (no scratch memory).
// cell_area_kernel has the same shape: lane k the spherical excess of triangle (centre,
// v_k, v_k+1), lanes 0 and 1 a second one for the 9 and 10 vertex cells, summed in boundary
// order.  Both run the code of the host twin (mgpu_test_cell_geometry_host), which the
// tests compare them with bit for bit.
//
// WKB rows have variable length: a count pass gives every row's bytes and lists the special
// H3 rows (pole cells, cells across the antimeridian), whose device-computed boundaries go
// to the host for H3IndexSystem's makePoleGeometry / antimeridian split (tessellate.cpp);
// their sizes are patched in, the lengths are scanned in chunks (per-chunk totals, the
// chunk scan of kernels.hip, a workgroup scan per slice), the write pass stores the
// ordinary rows and a last kernel copies the special rows' bytes into place.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#define H3T_QUAL static __constant__ const
#include "capi_internal.h"
#include "cell_geom.h"

namespace {

namespace CG = mgpu::cellgeom;
namespace HB = mgpu::h3b;
using M = mgpu::h3b::CrMath;

#define CGEO_TRY(expr)                                                                                   \
  do {                                                                                                   \
    hipError_t _e = (expr);                                                                              \
    if (_e != hipSuccess) return mgpu::set_error(MGPU_E_DEVICE, "%s: %s", #expr, hipGetErrorString(_e)); \
  } while (0)

constexpr int kBlock = 256;
constexpr int kCellLanes = 8;                      // lanes per H3 cell (boundary, area)
constexpr int kCellsPerBlock = kBlock / kCellLanes;
constexpr int kWkbLanes = 16;                      // lanes per WKB row: a point each (at most 11)
constexpr int kRowsPerBlock = kBlock / kWkbLanes;
constexpr int kScanSlices = 16;
constexpr int kScanChunk = kBlock * kScanSlices;   // rows per chunk of the length scan
constexpr int64_t kAreaBatch = (int64_t)1 << 20;   // cells whose boundaries the area entry holds in scratch at a time
enum { kBad = 0, kSpecial = 1, kCounterWords = 4 };

struct Poles {
  uint64_t cell[32];  // [2 * res + north]
};

__device__ __forceinline__ bool row_valid(const uint8_t* __restrict__ valid, int64_t voff, int64_t i) {
  return !valid || ((valid[(voff + i) >> 3] >> ((voff + i) & 7)) & 1);
}

__device__ __forceinline__ bool is_cell(int is, int64_t id) {
  return is == MGPU_BNG ? CG::bng_cell(id, nullptr, nullptr) : HB::is_valid_cell((uint64_t)id);
}

// counters[kBad] += the non-null rows that are not cell ids
__global__ __launch_bounds__(kBlock) void cell_validate_kernel(int is, const int64_t* __restrict__ cells,
                                                               const uint8_t* __restrict__ valid, int64_t voff, int64_t n,
                                                               unsigned long long* __restrict__ counters) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool bad = i < n && row_valid(valid, voff, i) && !is_cell(is, cells[i]);
  const unsigned long long b = __ballot(bad);
  if (b && (int)(threadIdx.x & 63) == __ffsll((long long)b) - 1) atomicAdd(&counters[kBad], (unsigned long long)__popcll(b));
}

// h3ToGeo in degrees (lng, lat); NaN for a null row
__global__ __launch_bounds__(kBlock) void cell_center_kernel(const int64_t* __restrict__ cells,
                                                             const uint8_t* __restrict__ valid, int64_t voff, int64_t n,
                                                             double* __restrict__ out_x, double* __restrict__ out_y) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint64_t h = (uint64_t)cells[i];
  double x = __builtin_nan(""), y = x;
  if (row_valid(valid, voff, i) && HB::is_valid_cell(h)) {
    const HB::LatLon c = HB::cell_center_m<M>(h);
    x = HB::to_degrees(c.lon);
    y = HB::to_degrees(c.lat);
  }
  out_x[i] = x;
  out_y[i] = y;
}

// Boundaries: out_xy[i * 20 ..] = the first out_nverts[i] (x, y) pairs; a null row (or an id
// that is no cell: the entries refuse those beforehand) has 0 vertices.  H3 with out_cx:
// the centre as well (NaN for a null row).
template <int IS>
__global__ __launch_bounds__(kBlock) void cell_boundary_kernel(const int64_t* __restrict__ cells,
                                                               const uint8_t* __restrict__ valid, int64_t voff, int64_t n,
                                                               double* __restrict__ out_xy, int32_t* __restrict__ out_nverts,
                                                               double* __restrict__ out_cx, double* __restrict__ out_cy) {
  if (IS == MGPU_BNG) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double xy[8];
    const bool ok = row_valid(valid, voff, i) && CG::bng_cell(cells[i], xy, nullptr);
    if (ok) {
      double2* row = (double2*)(out_xy + i * CG::kRowDoubles);
#pragma unroll
      for (int v = 0; v < 4; v++) row[v] = make_double2(xy[2 * v], xy[2 * v + 1]);
    }
    out_nverts[i] = ok ? 4 : 0;
    return;
  }
  const int lane = threadIdx.x & (kCellLanes - 1);
  const int64_t i = (int64_t)blockIdx.x * kCellsPerBlock + (threadIdx.x / kCellLanes);
  const bool in = i < n;
  const uint64_t h = in ? (uint64_t)cells[i] : 0;
  const bool ok = in && row_valid(valid, voff, i) && HB::is_valid_cell(h);
  const bool want_center = out_cx != nullptr;
  // the lane's first projection: its substrate vertex, or (lane 7) the centre
  HB::CellFrame f{};
  HB::FaceIJK fa{}, fb{};
  HB::Overage ova = HB::kNoOverage, ovb = HB::kNoOverage;
  int nv = 0, b = 0;
  HB::V2 p{0.0, 0.0};
  int face = 0, res = 0;
  bool substrate = true, active = false;
  if (ok) {
    f = HB::cell_frame(h);
    nv = f.nv();
    if (lane < nv) {
      b = lane + 1 < nv ? lane + 1 : 0;
      fa = HB::adjusted_vertex(f, lane, &ova);
      fb = HB::adjusted_vertex(f, b, &ovb);
      p = HB::ijk_to_hex2d<M>(fa.c);
      face = fa.face, res = f.adj_res, active = true;
    } else if (lane == kCellLanes - 1 && want_center) {
      p = HB::ijk_to_hex2d<M>(f.center.c);
      face = f.center.face, res = f.res, substrate = false, active = true;
    }
  }
  double lat = 0.0, lon = 0.0;
  if (active) HB::hex2d_to_geo<M>(p, face, res, substrate, &lat, &lon);
  // the distortion vertex of the edge lane -> lane + 1
  HB::V2 q{0.0, 0.0};
  int qface = 0;
  const bool dist = ok && lane < nv && HB::edge_distortion<M>(f, lane, b, fa, ova, fb, &q, &qface);
  double dlat = 0.0, dlon = 0.0;
  if (dist) HB::hex2d_to_geo<M>(q, qface, f.adj_res, true, &dlat, &dlon);
  // the 8 lanes' distortion flags: positions by a prefix count
  const unsigned long long bal = __ballot(dist);
  const uint32_t mine = (uint32_t)(bal >> ((threadIdx.x & 63) & ~(kCellLanes - 1))) & 0xFFu;
  if (!in) return;
  if (ok && lane < nv) {
    const int pos = lane + __popc(mine & ((1u << lane) - 1u));
    double2* row = (double2*)(out_xy + i * CG::kRowDoubles);
    if (pos < HB::kMaxBoundaryVerts) row[pos] = make_double2(HB::to_degrees(lon), HB::to_degrees(lat));
    if (dist && pos + 1 < HB::kMaxBoundaryVerts) row[pos + 1] = make_double2(HB::to_degrees(dlon), HB::to_degrees(dlat));
  }
  if (lane == 0) {
    const int total = nv + __popc(mine);
    out_nverts[i] = !ok ? 0 : (total < HB::kMaxBoundaryVerts ? total : HB::kMaxBoundaryVerts);
  }
  if (lane == kCellLanes - 1 && want_center) {
    const double nan = __builtin_nan("");
    out_cx[i] = ok ? HB::to_degrees(lon) : nan;
    out_cy[i] = ok ? HB::to_degrees(lat) : nan;
  }
}

// IndexSystem.area.  H3: from the boundaries and centres cell_boundary_kernel left in
// (xy, nverts, cx, cy); 0 vertices (a null row): NaN.  BNG: from the id.
template <int IS>
__global__ __launch_bounds__(kBlock) void cell_area_kernel(const int64_t* __restrict__ cells,
                                                           const uint8_t* __restrict__ valid, int64_t voff, int64_t n,
                                                           const double* __restrict__ xy, const int32_t* __restrict__ nverts,
                                                           const double* __restrict__ cx, const double* __restrict__ cy,
                                                           double* __restrict__ out_area) {
  if (IS == MGPU_BNG) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double a = 0.0;
    const bool ok = row_valid(valid, voff, i) && CG::bng_cell(cells[i], nullptr, &a);
    out_area[i] = ok ? a : __builtin_nan("");
    return;
  }
  const int lane = threadIdx.x & (kCellLanes - 1);
  const int64_t i = (int64_t)blockIdx.x * kCellsPerBlock + (threadIdx.x / kCellLanes);
  const bool in = i < n;
  int nv = in ? nverts[i] : 0;
  if (nv > HB::kMaxBoundaryVerts) nv = HB::kMaxBoundaryVerts;
  const double2* row = (const double2*)(xy + (in ? i : 0) * CG::kRowDoubles);
  double t0 = 0.0, t1 = 0.0;
  if (nv > 0) {
    const double clng = cx[i], clat = cy[i];
    const CG::SinCos ct = CG::lat_sincos<M>(clat);
    // (one call site for both rounds: the second runs for the 9 and 10 vertex cells only)
#pragma unroll 1
    for (int r = 0; r < 2; r++) {
      const int k = lane + r * kCellLanes;
      if (k < nv) {
        const double2 v0 = row[k], v1 = row[k + 1 < nv ? k + 1 : 0];
        const double a = CG::triangle_area<M>(clng, ct, v0.x, CG::lat_sincos<M>(v0.y), v1.x, CG::lat_sincos<M>(v1.y));
        t0 = r == 0 ? a : t0;
        t1 = r == 1 ? a : t1;
      }
    }
  }
  // the triangles in boundary order, from the first (as the reference's .sum)
  double sum = 0.0;
#pragma unroll
  for (int k = 0; k < HB::kMaxBoundaryVerts; k++) {
    const double tk = __shfl(k < kCellLanes ? t0 : t1, k & (kCellLanes - 1), kCellLanes);
    if (k < nv) sum += tk;
  }
  if (in && lane == 0) out_area[i] = nv > 0 ? sum : __builtin_nan("");
}

// ---- WKB

// a row's bytes when it is one ring; the special H3 rows (0 here) to the list
template <int IS>
__global__ __launch_bounds__(kBlock) void wkb_count_kernel(const int64_t* __restrict__ cells, int64_t n,
                                                           const double* __restrict__ xy, const int32_t* __restrict__ nverts,
                                                           Poles poles, uint32_t* __restrict__ len, int64_t* __restrict__ special,
                                                           unsigned long long* __restrict__ counters) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  int nv = nverts[i];
  if (nv > HB::kMaxBoundaryVerts) nv = HB::kMaxBoundaryVerts;
  uint32_t bytes = nv > 0 ? (uint32_t)CG::wkb_row_bytes(nv) : 0u;
  if (IS == MGPU_H3 && nv > 0) {
    const uint64_t h = (uint64_t)cells[i];
    const int res = (int)((h >> 52) & 15);
    bool sp = h == poles.cell[2 * res] || h == poles.cell[2 * res + 1];
    const double2* row = (const double2*)(xy + i * CG::kRowDoubles);
    double lo = INFINITY, hi = -INFINITY;
    for (int v = 0; v < nv; v++) {
      const double x = row[v].x;
      lo = x < lo ? x : lo;
      hi = x > hi ? x : hi;
    }
    sp = sp || (lo < 0 && hi >= 0 && hi - lo > 180.0);
    if (sp) {
      const unsigned long long k = atomicAdd(&counters[kSpecial], 1ull);
      special[k] = i;  // (at most n)
      bytes = 0;
    }
  }
  len[i] = bytes;
}

// the special rows' boundaries, vertex counts and ids, packed for the host
__global__ __launch_bounds__(kBlock) void wkb_gather_kernel(const int64_t* __restrict__ special, int64_t ns,
                                                            const int64_t* __restrict__ cells, const double* __restrict__ xy,
                                                            const int32_t* __restrict__ nverts, double* __restrict__ out_xy,
                                                            int64_t* __restrict__ out_cell, int32_t* __restrict__ out_nv) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t k = t / CG::kRowDoubles;
  const int d = (int)(t % CG::kRowDoubles);
  if (k >= ns) return;
  const int64_t i = special[k];
  out_xy[t] = xy[i * CG::kRowDoubles + d];
  if (d == 0) out_cell[k] = cells[i], out_nv[k] = nverts[i];
}

__global__ __launch_bounds__(kBlock) void wkb_patch_len_kernel(const int64_t* __restrict__ special, int64_t ns,
                                                               const int64_t* __restrict__ sp_off, uint32_t* __restrict__ len) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k < ns) len[special[k]] = (uint32_t)(sp_off[k + 1] - sp_off[k]);
}

// workgroup-wide exclusive scan of one value per thread, and the total
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* s_w, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(incl, d, 64);
    if (lane >= d) incl += t;
  }
  if (lane == 63) s_w[wave] = incl;
  __syncthreads();
  uint32_t off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kBlock / 64; w++) {
    const uint32_t x = s_w[w];
    if (w < wave) off += x;
    tot += x;
  }
  __syncthreads();
  *total = tot;
  return off + incl - v;
}

__global__ __launch_bounds__(kBlock) void wkb_chunk_sum_kernel(const uint32_t* __restrict__ len, int64_t n,
                                                               int64_t* __restrict__ chunk_tot) {
  __shared__ uint32_t s_w[kBlock / 64];
  const int64_t c0 = (int64_t)blockIdx.x * kScanChunk;
  uint32_t sum = 0;
  for (int sl = 0; sl < kScanSlices; sl++) {
    const int64_t i = c0 + sl * kBlock + threadIdx.x;
    if (i < n) sum += len[i];
  }
  uint32_t tot;
  block_excl_scan(sum, s_w, &tot);
  if (threadIdx.x == 0) chunk_tot[blockIdx.x] = tot;
}

// offsets[i] from the scanned chunk totals; offsets[n] = the total
__global__ __launch_bounds__(kBlock) void wkb_offsets_kernel(const uint32_t* __restrict__ len, int64_t n,
                                                             const int64_t* __restrict__ chunk_off,
                                                             int64_t* __restrict__ offsets) {
  __shared__ uint32_t s_w[kBlock / 64];
  const int64_t c0 = (int64_t)blockIdx.x * kScanChunk;
  int64_t carry = chunk_off[blockIdx.x];
  for (int sl = 0; sl < kScanSlices; sl++) {
    const int64_t s0 = c0 + sl * kBlock;
    if (s0 >= n) break;
    const int64_t i = s0 + threadIdx.x;
    const uint32_t v = i < n ? len[i] : 0u;
    uint32_t tot;
    const uint32_t ex = block_excl_scan(v, s_w, &tot);
    if (i < n) {
      offsets[i] = carry + ex;
      if (i == n - 1) offsets[n] = carry + ex + v;
    }
    carry += tot;
  }
}

__device__ __forceinline__ void put_be64(uint8_t* p, double d) {
  const uint64_t v = __builtin_bswap64((uint64_t)__double_as_longlong(d));
  __builtin_memcpy(p, &v, 8);
}
__device__ __forceinline__ void put_be32(uint8_t* p, uint32_t u) {
  const uint32_t v = __builtin_bswap32(u);
  __builtin_memcpy(p, &v, 4);
}

// the ordinary rows: big-endian Polygon, one ring, the boundary closed with its first
// vertex (the byte conventions of wkb.h write_polygons_pts); 16 lanes per row, a point each.
// Rows that would end past out_bytes are left out (the entry then reports MGPU_E_CAPACITY).
__global__ __launch_bounds__(kBlock) void wkb_write_kernel(int64_t n, const double* __restrict__ xy,
                                                           const int32_t* __restrict__ nverts, const uint32_t* __restrict__ len,
                                                           const int64_t* __restrict__ offsets, uint8_t* __restrict__ out,
                                                           int64_t out_bytes) {
  const int lane = threadIdx.x & (kWkbLanes - 1);
  const int64_t i = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x / kWkbLanes);
  if (i >= n) return;
  int nv = nverts[i];
  if (nv > HB::kMaxBoundaryVerts) nv = HB::kMaxBoundaryVerts;
  const int64_t off = offsets[i];
  // (a special row's bytes differ from the one-ring size: the patch kernel writes it)
  if (nv <= 0 || (int64_t)len[i] != CG::wkb_row_bytes(nv) || off < 0 || off + CG::wkb_row_bytes(nv) > out_bytes) return;
  uint8_t* w = out + off;
  if (lane == 0) {
    w[0] = 0;
    put_be32(w + 1, 3u);
    put_be32(w + 5, 1u);
    put_be32(w + 9, (uint32_t)(nv + 1));
  }
  if (lane <= nv) {
    const double2 v = ((const double2*)(xy + i * CG::kRowDoubles))[lane < nv ? lane : 0];
    put_be64(w + 13 + 16 * lane, v.x);
    put_be64(w + 21 + 16 * lane, v.y);
  }
}

// the special rows' bytes (built on the host) into place: a workgroup per row
__global__ __launch_bounds__(64) void wkb_patch_kernel(const int64_t* __restrict__ special, const int64_t* __restrict__ sp_off,
                                                       const uint8_t* __restrict__ sp_bytes, const int64_t* __restrict__ offsets,
                                                       uint8_t* __restrict__ out, int64_t out_bytes) {
  const int64_t k = blockIdx.x;
  const int64_t b0 = sp_off[k], nb = sp_off[k + 1] - b0, off = offsets[special[k]];
  if (off < 0 || off + nb > out_bytes) return;
  for (int64_t q = threadIdx.x; q < nb; q += 64) out[off + q] = sp_bytes[b0 + q];
}

// ---- host

unsigned grid_of(int64_t items, int per_block) { return (unsigned)std::max<int64_t>((items + per_block - 1) / per_block, 1); }
size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

int32_t check_column(const char* what, const mgpu_ctx* ctx, int32_t is, const int64_t* cells, int64_t voff, int64_t n) {
  if (!ctx) return mgpu::set_error(MGPU_E_INVALID_ARG, "%s: ctx is NULL", what);
  if (is != MGPU_H3 && is != MGPU_BNG) return mgpu::set_error(MGPU_E_INVALID_ARG, "%s: unknown index system %d (0 = H3, 1 = BNG)", what, is);
  if (n < 0 || (n > 0 && !cells) || voff < 0) return mgpu::set_error(MGPU_E_INVALID_ARG, "%s: bad cell column", what);
  return MGPU_OK;
}

// the column's non-null rows are cell ids, or MGPU_E_INVALID_ARG; `counters` (device,
// kCounterWords words) is left cleared but for counters[kBad].  Synchronises the stream.
int32_t validate(const char* what, mgpu_ctx* ctx, int32_t is, const int64_t* cells, const uint8_t* valid, int64_t voff,
                 int64_t n, unsigned long long* counters, hipStream_t s) {
  CGEO_TRY(hipMemsetAsync(counters, 0, kCounterWords * 8, s));
  hipLaunchKernelGGL(cell_validate_kernel, dim3(grid_of(n, kBlock)), dim3(kBlock), 0, s, is, cells, valid, voff, n, counters);
  CGEO_TRY(hipGetLastError());
  CGEO_TRY(hipMemcpyAsync(ctx->pin, counters, kCounterWords * 8, hipMemcpyDeviceToHost, s));
  CGEO_TRY(hipStreamSynchronize(s));
  if (ctx->pin[kBad])
    return mgpu::set_error(MGPU_E_INVALID_ARG, "%s: %llu rows are not %s cell ids", what, (unsigned long long)ctx->pin[kBad],
                           is == MGPU_BNG ? "BNG" : "H3");
  return MGPU_OK;
}

hipError_t launch_boundaries(int32_t is, const int64_t* cells, const uint8_t* valid, int64_t voff, int64_t n, double* xy,
                             int32_t* nverts, double* cx, double* cy, hipStream_t s) {
  if (is == MGPU_BNG)
    hipLaunchKernelGGL(cell_boundary_kernel<MGPU_BNG>, dim3(grid_of(n, kBlock)), dim3(kBlock), 0, s, cells, valid, voff, n, xy,
                       nverts, nullptr, nullptr);
  else
    hipLaunchKernelGGL(cell_boundary_kernel<MGPU_H3>, dim3(grid_of(n, kCellsPerBlock)), dim3(kBlock), 0, s, cells, valid, voff,
                       n, xy, nverts, cx, cy);
  return hipGetLastError();
}

hipError_t write_valid(const uint8_t* valid, int64_t voff, int64_t n, uint8_t* out_valid, hipStream_t s) {
  if (!out_valid || n <= 0) return hipSuccess;
  return mgpu::launch_valid_and(valid, voff, nullptr, 0, n, out_valid, s);
}

}  // namespace

extern "C" {

int32_t mgpu_cells_to_centers(mgpu_ctx* ctx, int32_t index_system, const int64_t* cells, const uint8_t* valid,
                              int64_t valid_offset, int64_t n, double* out_x, double* out_y, uint8_t* out_valid, void* stream) {
  if (int32_t st = check_column("cells_to_centers", ctx, index_system, cells, valid_offset, n)) return st;
  if (index_system == MGPU_BNG)
    return mgpu::set_error(MGPU_E_UNSUPPORTED, "cells_to_centers: BNGIndexSystem.indexToCenter is not implemented (NotImplementedError)");
  if (n == 0) return MGPU_OK;
  if (!out_x || !out_y) return mgpu::set_error(MGPU_E_INVALID_ARG, "cells_to_centers: out_x / out_y is NULL");
  CGEO_TRY(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  if (int32_t st = ensure_scratch(ctx, 256)) return st;
  if (int32_t st = validate("cells_to_centers", ctx, index_system, cells, valid, valid_offset, n, (unsigned long long*)ctx->scratch, s)) return st;
  hipLaunchKernelGGL(cell_center_kernel, dim3(grid_of(n, kBlock)), dim3(kBlock), 0, s, cells, valid, valid_offset, n, out_x, out_y);
  CGEO_TRY(hipGetLastError());
  CGEO_TRY(write_valid(valid, valid_offset, n, out_valid, s));
  return MGPU_OK;
}

int32_t mgpu_cells_to_boundaries(mgpu_ctx* ctx, int32_t index_system, const int64_t* cells, const uint8_t* valid,
                                 int64_t valid_offset, int64_t n, double* out_xy, int32_t* out_nverts, uint8_t* out_valid,
                                 void* stream) {
  if (int32_t st = check_column("cells_to_boundaries", ctx, index_system, cells, valid_offset, n)) return st;
  if (n == 0) return MGPU_OK;
  if (!out_xy || !out_nverts) return mgpu::set_error(MGPU_E_INVALID_ARG, "cells_to_boundaries: out_xy / out_nverts is NULL");
  if (((uintptr_t)out_xy) & 15) return mgpu::set_error(MGPU_E_INVALID_ARG, "cells_to_boundaries: out_xy must be 16-byte aligned");
  CGEO_TRY(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  if (int32_t st = ensure_scratch(ctx, 256)) return st;
  if (int32_t st = validate("cells_to_boundaries", ctx, index_system, cells, valid, valid_offset, n, (unsigned long long*)ctx->scratch, s)) return st;
  CGEO_TRY(launch_boundaries(index_system, cells, valid, valid_offset, n, out_xy, out_nverts, nullptr, nullptr, s));
  CGEO_TRY(write_valid(valid, valid_offset, n, out_valid, s));
  return MGPU_OK;
}

int32_t mgpu_cells_area(mgpu_ctx* ctx, int32_t index_system, const int64_t* cells, const uint8_t* valid, int64_t valid_offset,
                        int64_t n, double* out_area_km2, uint8_t* out_valid, void* stream) {
  if (int32_t st = check_column("cells_area", ctx, index_system, cells, valid_offset, n)) return st;
  if (n == 0) return MGPU_OK;
  if (!out_area_km2) return mgpu::set_error(MGPU_E_INVALID_ARG, "cells_area: out_area_km2 is NULL");
  CGEO_TRY(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  // scratch: counters | xy | cx | cy | nverts of one batch
  const int64_t batch = std::min(n, kAreaBatch);
  const size_t xy_b = align256((size_t)batch * CG::kRowDoubles * 8), c_b = align256((size_t)batch * 8), nv_b = align256((size_t)batch * 4);
  if (int32_t st = ensure_scratch(ctx, 256 + (index_system == MGPU_H3 ? xy_b + 2 * c_b + nv_b : 0))) return st;
  uint8_t* base = (uint8_t*)ctx->scratch;
  if (int32_t st = validate("cells_area", ctx, index_system, cells, valid, valid_offset, n, (unsigned long long*)base, s)) return st;
  if (index_system == MGPU_BNG) {
    hipLaunchKernelGGL(cell_area_kernel<MGPU_BNG>, dim3(grid_of(n, kBlock)), dim3(kBlock), 0, s, cells, valid, valid_offset, n,
                       nullptr, nullptr, nullptr, nullptr, out_area_km2);
    CGEO_TRY(hipGetLastError());
  } else {
    double* xy = (double*)(base + 256);
    double* cx = (double*)(base + 256 + xy_b);
    double* cy = (double*)(base + 256 + xy_b + c_b);
    int32_t* nv = (int32_t*)(base + 256 + xy_b + 2 * c_b);
    for (int64_t o = 0; o < n; o += batch) {
      const int64_t m = std::min(batch, n - o);
      CGEO_TRY(launch_boundaries(MGPU_H3, cells + o, valid, valid_offset + o, m, xy, nv, cx, cy, s));
      hipLaunchKernelGGL(cell_area_kernel<MGPU_H3>, dim3(grid_of(m, kCellsPerBlock)), dim3(kBlock), 0, s, cells + o, valid,
                         valid_offset + o, m, xy, nv, cx, cy, out_area_km2 + o);
      CGEO_TRY(hipGetLastError());
    }
  }
  CGEO_TRY(write_valid(valid, valid_offset, n, out_valid, s));
  return MGPU_OK;
}

int32_t mgpu_cells_boundary_wkb(mgpu_ctx* ctx, int32_t index_system, const int64_t* cells, const uint8_t* valid,
                                int64_t valid_offset, int64_t n, uint8_t* out, int64_t out_bytes, int64_t* out_offsets,
                                int64_t* out_total, uint8_t* out_valid, void* stream) {
  if (int32_t st = check_column("cells_boundary_wkb", ctx, index_system, cells, valid_offset, n)) return st;
  if (!out_offsets || out_bytes < 0 || (out_bytes > 0 && !out))
    return mgpu::set_error(MGPU_E_INVALID_ARG, "cells_boundary_wkb: bad output buffers");
  CGEO_TRY(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  if (out_total) *out_total = 0;
  if (n == 0) {
    CGEO_TRY(hipMemsetAsync(out_offsets, 0, 8, s));
    CGEO_TRY(hipStreamSynchronize(s));
    return MGPU_OK;
  }
  // scratch: counters | xy | nverts | len | special list | chunk totals
  const int64_t nc = (n + kScanChunk - 1) / kScanChunk;
  const size_t xy_b = align256((size_t)n * CG::kRowDoubles * 8), nv_b = align256((size_t)n * 4), sp_b = align256((size_t)n * 8),
               ch_b = align256((size_t)nc * 8);
  if (int32_t st = ensure_scratch(ctx, 256 + xy_b + 2 * nv_b + sp_b + ch_b)) return st;
  uint8_t* base = (uint8_t*)ctx->scratch;
  unsigned long long* counters = (unsigned long long*)base;
  double* xy = (double*)(base + 256);
  int32_t* nv = (int32_t*)(base + 256 + xy_b);
  uint32_t* len = (uint32_t*)(base + 256 + xy_b + nv_b);
  int64_t* special = (int64_t*)(base + 256 + xy_b + 2 * nv_b);
  int64_t* chunk = (int64_t*)(base + 256 + xy_b + 2 * nv_b + sp_b);
  if (int32_t st = validate("cells_boundary_wkb", ctx, index_system, cells, valid, valid_offset, n, counters, s)) return st;
  CGEO_TRY(launch_boundaries(index_system, cells, valid, valid_offset, n, xy, nv, nullptr, nullptr, s));
  Poles poles{};
  if (index_system == MGPU_H3) {
    for (int r = 0; r < 16; r++) poles.cell[2 * r] = CG::h3_pole_cell(false, r), poles.cell[2 * r + 1] = CG::h3_pole_cell(true, r);
    hipLaunchKernelGGL(wkb_count_kernel<MGPU_H3>, dim3(grid_of(n, kBlock)), dim3(kBlock), 0, s, cells, n, xy, nv, poles, len, special, counters);
  } else {
    hipLaunchKernelGGL(wkb_count_kernel<MGPU_BNG>, dim3(grid_of(n, kBlock)), dim3(kBlock), 0, s, cells, n, xy, nv, poles, len, special, counters);
  }
  CGEO_TRY(hipGetLastError());
  // the special rows: boundaries to the host, rings and bytes there, sizes back
  int64_t ns = 0;
  struct Dev {  // the special rows' device buffers, freed on every return path
    void* p = nullptr;
    ~Dev() {
      if (p) hipFree(p);
    }
  } sp_dev;
  int64_t* sp_off = nullptr;
  uint8_t* sp_bytes = nullptr;
  if (index_system == MGPU_H3) {
    CGEO_TRY(hipMemcpyAsync(ctx->pin, counters, kCounterWords * 8, hipMemcpyDeviceToHost, s));
    CGEO_TRY(hipStreamSynchronize(s));
    ns = (int64_t)ctx->pin[kSpecial];
  }
  if (ns > 0) {
    const size_t gx_b = align256((size_t)ns * CG::kRowDoubles * 8), gc_b = align256((size_t)ns * 8), gn_b = align256((size_t)ns * 4);
    Dev gather;
    CGEO_TRY(hipMalloc(&gather.p, gx_b + gc_b + gn_b));
    double* g_xy = (double*)gather.p;
    int64_t* g_cell = (int64_t*)((uint8_t*)gather.p + gx_b);
    int32_t* g_nv = (int32_t*)((uint8_t*)gather.p + gx_b + gc_b);
    hipLaunchKernelGGL(wkb_gather_kernel, dim3(grid_of(ns * CG::kRowDoubles, kBlock)), dim3(kBlock), 0, s, special, ns, cells, xy, nv, g_xy, g_cell, g_nv);
    CGEO_TRY(hipGetLastError());
    std::vector<double> h_xy((size_t)ns * CG::kRowDoubles);
    std::vector<int64_t> h_cell((size_t)ns);
    std::vector<int32_t> h_nv((size_t)ns);
    CGEO_TRY(hipMemcpyAsync(h_xy.data(), g_xy, h_xy.size() * 8, hipMemcpyDeviceToHost, s));
    CGEO_TRY(hipMemcpyAsync(h_cell.data(), g_cell, h_cell.size() * 8, hipMemcpyDeviceToHost, s));
    CGEO_TRY(hipMemcpyAsync(h_nv.data(), g_nv, h_nv.size() * 4, hipMemcpyDeviceToHost, s));
    CGEO_TRY(hipStreamSynchronize(s));
    std::vector<uint8_t> bytes;
    std::vector<int64_t> off((size_t)ns + 1, 0);
    for (int64_t k = 0; k < ns; k++) {
      const int v = std::min(std::max(h_nv[k], 0), (int32_t)HB::kMaxBoundaryVerts);
      CG::h3_special_cell_wkb((uint64_t)h_cell[k], h_xy.data() + k * CG::kRowDoubles, v, bytes);
      off[k + 1] = (int64_t)bytes.size();
    }
    const size_t off_b = align256(off.size() * 8);
    CGEO_TRY(hipMalloc(&sp_dev.p, off_b + std::max<size_t>(bytes.size(), 1)));
    sp_off = (int64_t*)sp_dev.p;
    sp_bytes = (uint8_t*)sp_dev.p + off_b;
    CGEO_TRY(hipMemcpyAsync(sp_off, off.data(), off.size() * 8, hipMemcpyHostToDevice, s));
    CGEO_TRY(hipMemcpyAsync(sp_bytes, bytes.data(), bytes.size(), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(wkb_patch_len_kernel, dim3(grid_of(ns, kBlock)), dim3(kBlock), 0, s, special, ns, sp_off, len);
    CGEO_TRY(hipGetLastError());
    CGEO_TRY(hipStreamSynchronize(s));  // (the host vectors are read by the copies above)
  }
  hipLaunchKernelGGL(wkb_chunk_sum_kernel, dim3((unsigned)nc), dim3(kBlock), 0, s, len, n, chunk);
  CGEO_TRY(hipGetLastError());
  CGEO_TRY(mgpu::launch_scan_sums(chunk, nc, s));
  hipLaunchKernelGGL(wkb_offsets_kernel, dim3((unsigned)nc), dim3(kBlock), 0, s, len, n, chunk, out_offsets);
  CGEO_TRY(hipGetLastError());
  if (out_bytes > 0) {
    hipLaunchKernelGGL(wkb_write_kernel, dim3(grid_of(n, kRowsPerBlock)), dim3(kBlock), 0, s, n, xy, nv, len, out_offsets, out, out_bytes);
    CGEO_TRY(hipGetLastError());
    if (ns > 0) {
      hipLaunchKernelGGL(wkb_patch_kernel, dim3((unsigned)ns), dim3(64), 0, s, special, sp_off, sp_bytes, out_offsets, out, out_bytes);
      CGEO_TRY(hipGetLastError());
    }
  }
  CGEO_TRY(write_valid(valid, valid_offset, n, out_valid, s));
  int64_t total = 0;
  CGEO_TRY(hipMemcpyAsync(&total, out_offsets + n, 8, hipMemcpyDeviceToHost, s));
  CGEO_TRY(hipStreamSynchronize(s));
  if (out_total) *out_total = total;
  if (total > out_bytes)
    return mgpu::set_error(MGPU_E_CAPACITY, "cells_boundary_wkb: %lld bytes needed, %lld given", (long long)total, (long long)out_bytes);
  return MGPU_OK;
}

}  // extern "C"

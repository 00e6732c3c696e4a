// grid_polyfill on the device: mgpu_grid_polyfill's kernels and host entry (polyfill.h has
// the algorithm and the code shared with the host twin; include/mosaic_gpu.h the contract).
//
// polyfill_kernel, one workgroup per tile of 256 consecutive lattice samples of one polygon:
//   phase 1  every lane its sample: cell, centre, owner (H3: or the certificate's second
//            projection); the owners inside the polygon's envelope are compacted into an LDS
//            list by ballot rank, in lattice order
//   phase 2  the polygon's ring chunks staged through LDS (16-byte loads); with k owners,
//            groups of 256 / k lanes split a chunk's edges for one owner and combine their
//            RayCrossingCounter bits per ring piece by OR (boundary) and XOR (parity) in LDS;
//            the owner's lane folds them into the PointLocator verdict, ring by ring
//   output   the matches, in lattice order, to the tile's 256-entry slot, and their count
// then per slab of tiles: launch_scan_sums over the counts, and polyfill_gather_kernel writes
// out_cells; polyfill_offsets_kernel reads each polygon's offset at its first tile.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#define H3T_QUAL static __constant__ const
#include "capi_internal.h"
#include "polyfill.h"

namespace {

namespace PF = mgpu::polyfill;
using M = mgpu::h3b::CrMath;

#define PFILL_TRY(expr)                                                                                  \
  do {                                                                                                   \
    hipError_t _e = (expr);                                                                              \
    if (_e != hipSuccess) return mgpu::set_error(MGPU_E_DEVICE, "%s: %s", #expr, hipGetErrorString(_e)); \
  } while (0)

constexpr int kBlock = PF::kTile;
enum { kCertFail = 0, kBase0 = 1, kBase1 = 2, kCounterWords = 4 };

struct Args {
  const PF::Tile* tiles;      // the slab's tiles
  const PF::PolyParam* polys;
  const PF::Chunk* chunks;
  const double2* xy;
  int64_t n_tiles;            // of the slab
  int res;
  double k_res;               // H3: h3::k_of_res(res)
  int64_t* slot;              // [n_tiles * 256] the tiles' matches
  uint32_t* tile_cnt;         // [n_tiles]
  int64_t* tile_scan;         // [n_tiles] the counts again, for the scan
  unsigned long long* counters;
};

// rank of the lanes with `flag` over the workgroup, in lane order, and their number
__device__ __forceinline__ uint32_t block_rank(bool flag, uint32_t* s_w, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long b = __ballot(flag);
  if (lane == 0) s_w[wave] = (uint32_t)__popcll(b);
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
  return off + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
}

template <int IS>
__global__ __launch_bounds__(kBlock) void polyfill_kernel(Args a) {
  __shared__ double2 s_v[PF::kChunkVerts];
  __shared__ double s_cx[kBlock], s_cy[kBlock];
  __shared__ int64_t s_cell[kBlock];
  __shared__ uint32_t s_bnd[kBlock], s_par[kBlock];
  __shared__ uint16_t s_start[PF::kChunkPieces + 2];
  __shared__ uint32_t s_w[kBlock / 64];
  const int tid = threadIdx.x;
  const int64_t t = blockIdx.x;
  if (t >= a.n_tiles) return;
  const PF::Tile tile = a.tiles[t];
  const PF::PolyParam& P = a.polys[tile.poly];
  const uint32_t n = (uint32_t)P.nx * (uint32_t)P.ny;  // (at most 2^31 - 1)
  // ---- phase 1
  const uint32_t j = tile.j0 + (uint32_t)tid;
  PF::Sample s;
  if (j < n) s = IS == MGPU_BNG ? PF::bng_sample(P, a.res, j) : PF::h3_sample<M>(P, a.res, a.k_res, j);
  if (IS == MGPU_H3) {
    const unsigned long long fb = __ballot(s.cert_fail);
    if (fb && (tid & 63) == __ffsll((long long)fb) - 1) atomicAdd(&a.counters[kCertFail], (unsigned long long)__popcll(fb));
  }
  const bool cand = s.own && mgpu::pip::env_has(P.env, s.cx, s.cy);
  uint32_t k;
  const uint32_t rank = block_rank(cand, s_w, &k);
  if (k == 0) {
    if (tid == 0) a.tile_cnt[t] = 0, a.tile_scan[t] = 0;
    return;
  }
  if (cand) s_cx[rank] = s.cx, s_cy[rank] = s.cy, s_cell[rank] = s.cell;
  // ---- phase 2: owner o < k is walked by the lanes [o * G, (o + 1) * G), decided by lane o
  const int G = kBlock / (int)k, o = tid / G, sub = tid - o * G;
  PF::Verdict v;
  const int64_t c1 = P.chunk0 + P.n_chunks;
  for (int64_t ci = P.chunk0; ci < c1; ci++) {
    const PF::Chunk& C = a.chunks[ci];
    const int nv = C.nv, np = C.np;
    __syncthreads();  // (the owner list written; the last chunk's vertices and bits read)
    for (int i = tid; i < nv; i += kBlock) s_v[i] = a.xy[C.v0 + i];
    if (tid <= np) s_start[tid] = C.start[tid];
    if (tid < (int)k) s_bnd[tid] = 0, s_par[tid] = 0;
    __syncthreads();
    if (o < (int)k) {
      uint32_t bnd, par;
      PF::chunk_bits((const double*)s_v, nv, s_start, s_cx[o], s_cy[o], sub, G, &bnd, &par);
      if (bnd) atomicOr(&s_bnd[o], bnd);
      if (par) atomicXor(&s_par[o], par);
    }
    __syncthreads();
    if (tid < (int)k) PF::fold_chunk(np, C.ends, C.shell, C.part_last, s_bnd[tid], s_par[tid], v);
  }
  // ---- output
  const bool hit = tid < (int)k && v.matched;
  uint32_t m;
  const uint32_t pos = block_rank(hit, s_w, &m);
  if (hit) a.slot[t * kBlock + pos] = s_cell[tid];
  if (tid == 0) a.tile_cnt[t] = m, a.tile_scan[t] = (int64_t)m;
}

// the slab's matches into out_cells: tile t's at base + scan[t], base = counters[base_in];
// goff[t] = that offset (goff: the slab's part of the per-tile offsets); the slab's last
// tile leaves the next slab's base in counters[base_out]
__global__ __launch_bounds__(kBlock) void polyfill_gather_kernel(const int64_t* __restrict__ slot, const uint32_t* __restrict__ tile_cnt,
                                                                 const int64_t* __restrict__ tile_scan, int64_t n_tiles,
                                                                 unsigned long long* __restrict__ counters, int base_in, int base_out,
                                                                 int64_t* __restrict__ goff, int64_t* __restrict__ out_cells,
                                                                 int64_t capacity) {
  const int64_t t = blockIdx.x;
  if (t >= n_tiles) return;
  const int64_t off = (int64_t)counters[base_in] + tile_scan[t];
  const uint32_t m = tile_cnt[t];
  if (threadIdx.x == 0) {
    goff[t] = off;
    if (t == n_tiles - 1) counters[base_out] = (unsigned long long)(off + m);
  }
  if (threadIdx.x < m && off + threadIdx.x < capacity) out_cells[off + threadIdx.x] = slot[t * kBlock + threadIdx.x];
}

// out_offsets[p] = the offset of polygon p's first tile (a polygon without tiles: the next one's), p <= n_polys
__global__ __launch_bounds__(kBlock) void polyfill_offsets_kernel(const int64_t* __restrict__ first_tile, int64_t n_polys,
                                                                  const int64_t* __restrict__ goff, int64_t n_tiles,
                                                                  const unsigned long long* __restrict__ counters, int base_final,
                                                                  int64_t* __restrict__ out_offsets) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p > n_polys) return;
  const int64_t ft = first_tile[p];
  out_offsets[p] = ft < n_tiles ? goff[ft] : (int64_t)counters[base_final];
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

int32_t mgpu_grid_polyfill(mgpu_ctx* ctx, int32_t index_system, int32_t res, int64_t n_polys, const int64_t* poly_part_off,
                           const int64_t* part_ring_off, const int64_t* ring_off, const double* xy, int64_t* out_cells,
                           int64_t capacity, int64_t* out_offsets, int64_t* out_total, void* stream) {
  const char* what = "grid_polyfill";
  if (!ctx) return mgpu::set_error(MGPU_E_INVALID_ARG, "%s: ctx is NULL", what);
  if (int32_t st = PF::check_polygons(what, index_system, res, n_polys, poly_part_off, part_ring_off, ring_off, xy)) return st;
  if (!out_offsets || !out_total || capacity < 0 || (capacity > 0 && !out_cells))
    return mgpu::set_error(MGPU_E_INVALID_ARG, "%s: bad output buffers", what);
  PFILL_TRY(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  *out_total = 0;
  const int64_t slab_tiles = std::max<int64_t>(ctx->opt.polyfill_slab / kBlock, 1);
  int64_t fails_all = 0;
  double shrink = 1.0;
  const double k_res = index_system == MGPU_H3 ? mgpu::h3::k_of_res(res) : 0.0;
  for (int attempt = 1; attempt <= PF::kMaxAttempts; attempt++, shrink /= 2) {
    PF::Plan plan;
    if (int32_t st = PF::build_plan(what, index_system, res, n_polys, poly_part_off, part_ring_off, ring_off, xy, shrink, &plan)) return st;
    const int64_t nt = (int64_t)plan.tiles.size(), st_tiles = std::min(slab_tiles, std::max<int64_t>(nt, 1));
    // scratch: counters | tiles | polygons | chunks | first tiles | tile offsets | xy | slab: slots, counts, scan
    const size_t b_tiles = align256((size_t)std::max<int64_t>(nt, 1) * sizeof(PF::Tile));
    const size_t b_polys = align256((size_t)std::max<int64_t>(n_polys, 1) * sizeof(PF::PolyParam));
    const size_t b_chunks = align256(std::max<size_t>(plan.chunks.size(), 1) * sizeof(PF::Chunk));
    const size_t b_first = align256((size_t)(n_polys + 1) * 8), b_goff = align256((size_t)std::max<int64_t>(nt, 1) * 8);
    const size_t b_xy = align256((size_t)std::max<int64_t>(plan.n_verts, 1) * 16);
    const size_t b_slot = align256((size_t)st_tiles * kBlock * 8), b_cnt = align256((size_t)st_tiles * 4), b_scan = align256((size_t)st_tiles * 8);
    if (int32_t st = ensure_scratch(ctx, 256 + b_tiles + b_polys + b_chunks + b_first + b_goff + b_xy + b_slot + b_cnt + b_scan)) return st;
    uint8_t* w = (uint8_t*)ctx->scratch;
    unsigned long long* counters = (unsigned long long*)w;
    w += 256;
    PF::Tile* d_tiles = (PF::Tile*)w;
    w += b_tiles;
    PF::PolyParam* d_polys = (PF::PolyParam*)w;
    w += b_polys;
    PF::Chunk* d_chunks = (PF::Chunk*)w;
    w += b_chunks;
    int64_t* d_first = (int64_t*)w;
    w += b_first;
    int64_t* d_goff = (int64_t*)w;
    w += b_goff;
    double2* d_xy = (double2*)w;
    w += b_xy;
    int64_t* d_slot = (int64_t*)w;
    w += b_slot;
    uint32_t* d_cnt = (uint32_t*)w;
    w += b_cnt;
    int64_t* d_scan = (int64_t*)w;
    PFILL_TRY(hipMemsetAsync(counters, 0, kCounterWords * 8, s));
    if (nt) PFILL_TRY(hipMemcpyAsync(d_tiles, plan.tiles.data(), (size_t)nt * sizeof(PF::Tile), hipMemcpyHostToDevice, s));
    if (n_polys) PFILL_TRY(hipMemcpyAsync(d_polys, plan.polys.data(), (size_t)n_polys * sizeof(PF::PolyParam), hipMemcpyHostToDevice, s));
    if (!plan.chunks.empty())
      PFILL_TRY(hipMemcpyAsync(d_chunks, plan.chunks.data(), plan.chunks.size() * sizeof(PF::Chunk), hipMemcpyHostToDevice, s));
    PFILL_TRY(hipMemcpyAsync(d_first, plan.first_tile.data(), (size_t)(n_polys + 1) * 8, hipMemcpyHostToDevice, s));
    if (plan.n_verts) PFILL_TRY(hipMemcpyAsync(d_xy, xy, (size_t)plan.n_verts * 16, hipMemcpyHostToDevice, s));
    PFILL_TRY(hipEventRecord(ctx->ev0, s));  // (the launches' device time, for mgpu_test_grid_polyfill_last)
    int base = kBase0;
    for (int64_t t0 = 0; t0 < nt; t0 += st_tiles) {
      const int64_t m = std::min(st_tiles, nt - t0);
      Args a{d_tiles + t0, d_polys, d_chunks, d_xy, m, res, k_res, d_slot, d_cnt, d_scan, counters};
      if (index_system == MGPU_BNG)
        hipLaunchKernelGGL(polyfill_kernel<MGPU_BNG>, dim3((unsigned)m), dim3(kBlock), 0, s, a);
      else
        hipLaunchKernelGGL(polyfill_kernel<MGPU_H3>, dim3((unsigned)m), dim3(kBlock), 0, s, a);
      PFILL_TRY(hipGetLastError());
      PFILL_TRY(mgpu::launch_scan_sums(d_scan, m, s));
      const int next = base == kBase0 ? kBase1 : kBase0;
      hipLaunchKernelGGL(polyfill_gather_kernel, dim3((unsigned)m), dim3(kBlock), 0, s, d_slot, d_cnt, d_scan, m, counters, base,
                         next, d_goff + t0, out_cells, capacity);
      PFILL_TRY(hipGetLastError());
      base = next;
    }
    hipLaunchKernelGGL(polyfill_offsets_kernel, dim3((unsigned)((n_polys + 1 + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, d_first,
                       n_polys, d_goff, nt, counters, base, out_offsets);
    PFILL_TRY(hipGetLastError());
    PFILL_TRY(hipEventRecord(ctx->ev1, s));
    PFILL_TRY(hipMemcpyAsync(ctx->pin, counters, kCounterWords * 8, hipMemcpyDeviceToHost, s));
    PFILL_TRY(hipStreamSynchronize(s));  // (the plan's vectors are read by the copies above)
    const int64_t fails = (int64_t)ctx->pin[kCertFail], total = (int64_t)ctx->pin[base];
    fails_all += fails;
    float kernel_ms = 0.0f;
    PFILL_TRY(hipEventElapsedTime(&kernel_ms, ctx->ev0, ctx->ev1));
    PF::note_last(plan.samples, nt, fails_all, attempt, (int64_t)(kernel_ms * 1000.0f));
    *out_total = total;
    if (fails) continue;  // the spacing was too coarse for some cell: again at half of it
    if (total > capacity)
      return mgpu::set_error(MGPU_E_CAPACITY, "%s: %lld cells needed, %lld given", what, (long long)total, (long long)capacity);
    return MGPU_OK;
  }
  return mgpu::set_error(MGPU_E_INTERNAL, "%s: the certificate failed at every spacing (%lld failures)", what, (long long)fails_all);
}

}  // extern "C"

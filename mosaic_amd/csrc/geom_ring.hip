// grid_geometrykring / grid_geometrykloop on the device: mgpu_geometry_kring's kernels and host
// entry (geom_ring.h has the definition and the record; include/mosaic_gpu.h the contract).
//
// The border cells of all geometries are compacted, geometry by geometry, and processed in slabs
// of at most `geomring_slab` cells.  Per slab:
//   ring lists   the three launch steps of mgpu_grid_kring (kernels.h launch_kring_*, pentagon
//                fallbacks included) over the slab's border cells: kRing(b, k), or for the loop
//                kLoop(b, k) and kRing(b, k - 1), as lists in scratch
//   LDS path     georing_lds_kernel, one workgroup per geometry of the slab: its lists and its
//                rows inserted as records into an open-addressing set in LDS (lowest key per id),
//                the set packed and sorted there (bitonic), the ids that kept member 1 to staging
//   HBM path     a geometry whose set overflowed, or that a slab boundary cuts: its records (and
//                the distinct keys carried from its earlier slabs) emitted to memory, sorted by
//                cell_agg.hip's radix sort, made distinct by a count / scan / write pass; a cut
//                geometry carries its distinct keys to the next slab, a finished one its ids
//   gather       launch_scan_sums over the geometries' counts, the lists copied to out_cells
//                behind the slabs before, out_offsets written
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#define H3T_QUAL static __constant__ const
#include "capi_internal.h"
#include "geom_ring.h"

namespace {

namespace GR = mgpu::geomring;
using u64 = unsigned long long;

#define GRING_TRY(expr)                                                                                  \
  do {                                                                                                   \
    hipError_t _e = (expr);                                                                              \
    if (_e != hipSuccess) return mgpu::set_error(MGPU_E_DEVICE, "%s: %s", #expr, hipGetErrorString(_e)); \
  } while (0)

constexpr int kBlock = GR::kBlock;
constexpr int kCopyBlock = 256;
constexpr int kUniqSlices = 16;                         // a chunk of the distinct pass: 16 slices of 256 keys
constexpr int64_t kUniqChunk = kCopyBlock * kUniqSlices;
constexpr int64_t kMaxSegs = 1 << 16;                   // geometries (or pieces) of a slab
// counters (u64): the ring steps' own sixteen first (kernels.hip: [2] invalid, [3] fallback cells,
// [4] overflowed walks), then this unit's
enum { kRingWords = 16, kBadRow = 16, kBase0 = 17, kBase1 = 18, kHbmCount = 19, kCounterWords = 24 };
enum { kFirst = 1u, kLast = 2u };
enum { kStatusLds = 0u, kStatusOverflow = 1u, kStatusCut = 2u };

// a geometry's part in one slab
struct Seg {
  int64_t row0, row1;   // its rows (the first piece only: else row0 == row1)
  int64_t b0, b1;       // its border cells, as positions in the slab
  int64_t stage_rows;   // rows of the slab's pieces before it (its place in staging)
  int32_t geom;
  uint32_t flags;       // kFirst | kLast
};

struct LdsArgs {
  const Seg* segs;          // the slab's
  const int64_t* cell;
  const int64_t *roff_a, *ring_a;   // member-1 lists of the slab's border cells
  const int64_t *roff_b, *ring_b;   // loop: their member-0 lists (else null)
  uint32_t max_slots;               // a power of two in [kLdsSlotsMin, kLdsSlots]
  uint32_t row_member;              // the member bit of a row's own cell (ring: 1, loop: 0)
  int64_t* staging;
  int64_t* seg_cnt;
  u64* seg_src;
  uint32_t* seg_status;
};

// rank of the lanes with `flag` over the workgroup, in lane order, and their number
template <int BLOCK>
__device__ __forceinline__ uint32_t block_rank(bool flag, uint32_t* s_w, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u64 b = __ballot(flag);
  if (lane == 0) s_w[wave] = (uint32_t)__popcll(b);
  __syncthreads();
  uint32_t off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < BLOCK / 64; w++) {
    const uint32_t x = s_w[w];
    if (w < wave) off += x;
    tot += x;
  }
  __syncthreads();
  *total = tot;
  return off + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
}

// wave per geometry: nb[g] = its border rows; counters[kBadRow] += core rows outside [0, 2^62)
__global__ __launch_bounds__(kCopyBlock) void georing_count_kernel(const int64_t* __restrict__ row_off, const int64_t* __restrict__ cell,
                                                                   const uint8_t* __restrict__ is_core, int64_t n_geoms,
                                                                   int64_t* __restrict__ nb, u64* __restrict__ counters) {
  const int lane = threadIdx.x & 63;
  const int64_t g = (int64_t)blockIdx.x * (kCopyBlock / 64) + (threadIdx.x >> 6);
  if (g >= n_geoms) return;
  const int64_t r0 = row_off[g], r1 = row_off[g + 1];
  int64_t border = 0, bad = 0;
  for (int64_t r = r0 + lane; r < r1; r += 64) {
    const bool core = is_core[r] != 0;
    const int64_t id = cell[r];
    border += core ? 0 : 1;
    bad += (core && (id < 0 || id >= GR::kIdLimit)) ? 1 : 0;
  }
  for (int o = 32; o > 0; o >>= 1) border += __shfl_xor(border, o, 64), bad += __shfl_xor(bad, o, 64);
  if (lane == 0) {
    nb[g] = border;
    if (bad) atomicAdd(&counters[kBadRow], (u64)bad);
  }
}

// wave per geometry: its border rows' cells to bcell[bstart[g] ..], in row order
__global__ __launch_bounds__(kCopyBlock) void georing_compact_kernel(const int64_t* __restrict__ row_off, const int64_t* __restrict__ cell,
                                                                     const uint8_t* __restrict__ is_core, int64_t n_geoms,
                                                                     const int64_t* __restrict__ bstart, int64_t* __restrict__ bcell) {
  const int lane = threadIdx.x & 63;
  const int64_t g = (int64_t)blockIdx.x * (kCopyBlock / 64) + (threadIdx.x >> 6);
  if (g >= n_geoms) return;
  const int64_t r0 = row_off[g], r1 = row_off[g + 1], end = bstart[g + 1];
  int64_t at = bstart[g];
  for (int64_t q = r0; q < r1; q += 64) {
    const int64_t r = q + lane;
    const bool border = r < r1 && is_core[r] == 0;
    const u64 b = __ballot(border);
    const int64_t pos = at + __popcll(b & ((1ull << lane) - 1ull));
    if (border && pos < end) bcell[pos] = cell[r];  // (pos < end always: bstart is the scan of these counts)
    at += __popcll(b);
  }
}

// One workgroup per piece of the slab.  A whole geometry (first and last piece): its records into
// the LDS set, lowest key per id; the set packed and sorted; the ids with member 1 to staging.
// The set has 2^j slots, the fewest that hold twice the records, at most max_slots; it overflows
// when more than 3/4 of the slots are taken (status kStatusOverflow, nothing written).
__global__ __launch_bounds__(kBlock) void georing_lds_kernel(LdsArgs a) {
  __shared__ u64 s_tab[GR::kLdsSlots];
  __shared__ uint32_t s_w[kBlock / 64];
  __shared__ uint32_t s_cnt, s_over;
  const int tid = threadIdx.x;
  const int64_t si = blockIdx.x;
  const Seg seg = a.segs[si];
  if ((seg.flags & (kFirst | kLast)) != (kFirst | kLast)) {
    if (tid == 0) a.seg_status[si] = kStatusCut, a.seg_cnt[si] = 0, a.seg_src[si] = 0;
    return;
  }
  const int64_t a0 = a.roff_a[seg.b0], n_a = a.roff_a[seg.b1] - a0;
  const int64_t b0 = a.roff_b ? a.roff_b[seg.b0] : 0, n_b = a.roff_b ? a.roff_b[seg.b1] - b0 : 0;
  const int64_t n_in = n_a + n_b + (seg.row1 - seg.row0);
  uint32_t slots = a.max_slots;
  while (slots > GR::kLdsSlotsMin && (int64_t)(slots >> 1) >= 2 * n_in) slots >>= 1;
  const int shift = 64 - (__ffs((int)slots) - 1);
  const uint32_t limit = slots - slots / 4;
  for (uint32_t i = tid; i < slots; i += kBlock) s_tab[i] = GR::kEmpty;
  if (tid == 0) s_cnt = 0, s_over = 0;
  __syncthreads();
  for (int64_t i = tid; i < n_in; i += kBlock) {
    u64 key;
    if (i < n_a)
      key = ((u64)a.ring_a[a0 + i] << 1) | 1ull;
    else if (i < n_a + n_b)
      key = (u64)a.ring_b[b0 + (i - n_a)] << 1;
    else  // a row's own cell: core, or a border cell, which its own list holds with this member too
      key = ((u64)a.cell[seg.row0 + (i - n_a - n_b)] << 1) | a.row_member;
    const u64 id = key >> 1;
    uint32_t h = (uint32_t)((id * 0x9E3779B97F4A7C15ull) >> shift);
    bool done = *(volatile uint32_t*)&s_over != 0;
    uint32_t probes = 0;
    for (; probes < slots && !done; probes++) {
      const u64 old = atomicCAS(&s_tab[h], GR::kEmpty, key);
      if (old == GR::kEmpty) {
        if (atomicAdd(&s_cnt, 1u) + 1u > limit) s_over = 1;
        done = true;
      } else if ((old >> 1) == id) {
        if (key < old) atomicMin(&s_tab[h], key);
        done = true;
      }
      h = (h + 1) & (slots - 1);
    }
    if (!done) s_over = 1;  // (every slot probed: the set is full)
  }
  __syncthreads();
  if (s_over) {
    if (tid == 0) a.seg_status[si] = kStatusOverflow, a.seg_cnt[si] = 0, a.seg_src[si] = 0;
    return;
  }
  // the taken slots moved to the front, in place: a round reads kBlock slots into registers
  // before any lane writes, and writes at or before the slots it has read
  const uint32_t n = s_cnt;
  uint32_t packed = 0;
  for (uint32_t i0 = 0; i0 < slots; i0 += kBlock) {
    const uint32_t i = i0 + tid;
    const u64 key = i < slots ? s_tab[i] : GR::kEmpty;
    uint32_t m;
    const uint32_t rank = block_rank<kBlock>(key != GR::kEmpty, s_w, &m);  // (its first barrier follows the reads)
    if (key != GR::kEmpty) s_tab[packed + rank] = key;
    packed += m;
  }
  uint32_t sort_n = 2;  // the power of two that holds them; the slots between are unused ones
  while (sort_n < n) sort_n <<= 1;
  __syncthreads();
  for (uint32_t i = n + tid; i < sort_n; i += kBlock) s_tab[i] = GR::kEmpty;
  __syncthreads();
  // bitonic sort of those slots, unused ones (the largest value) last
  for (uint32_t k2 = 2; k2 <= sort_n; k2 <<= 1)
    for (uint32_t j = k2 >> 1; j > 0; j >>= 1) {
      for (uint32_t i = tid; i < sort_n; i += kBlock) {
        const uint32_t p = i ^ j;
        if (p > i) {
          const u64 x = s_tab[i], y = s_tab[p];
          if ((x > y) == ((i & k2) == 0)) s_tab[i] = y, s_tab[p] = x;
        }
      }
      __syncthreads();
    }
  int64_t* const out =a.staging + a0 + b0 + seg.stage_rows;
  uint32_t written = 0;
  for (uint32_t i0 = 0; i0 < n; i0 += kBlock) {
    const uint32_t i = i0 + tid;
    const u64 key = i < n ? s_tab[i] : 0ull;
    const bool keep = i < n && (key & 1ull);
    uint32_t m;
    const uint32_t rank = block_rank<kBlock>(keep, s_w, &m);
    if (keep) out[written + rank] = (int64_t)(key >> 1);
    written += m;
  }
  if (tid == 0) a.seg_status[si] = kStatusLds, a.seg_cnt[si] = (int64_t)written, a.seg_src[si] = (u64)out;
}

// the HBM path's records of one piece: the keys carried from its earlier pieces, its lists, its rows
__global__ __launch_bounds__(kCopyBlock) void georing_emit_kernel(const u64* __restrict__ carry, int64_t n_carry,
                                                                  const int64_t* __restrict__ ring_a, int64_t n_a,
                                                                  const int64_t* __restrict__ ring_b, int64_t n_b,
                                                                  const int64_t* __restrict__ rows, int64_t n_rows, uint32_t row_member,
                                                                  u64* __restrict__ out) {
  const int64_t n = n_carry + n_a + n_b + n_rows;
  for (int64_t i = (int64_t)blockIdx.x * kCopyBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kCopyBlock) {
    u64 key;
    if (i < n_carry)
      key = carry[i];
    else if (i < n_carry + n_a)
      key = ((u64)ring_a[i - n_carry] << 1) | 1ull;
    else if (i < n_carry + n_a + n_b)
      key = (u64)ring_b[i - n_carry - n_a] << 1;
    else
      key = ((u64)rows[i - n_carry - n_a - n_b] << 1) | row_member;
    out[i] = key;
  }
}

// sorted keys -> the first (lowest) key of every id; final: only those with member 1, as ids.
// Pass 1 (dest == null): chunk_tot[c] = the chunk's kept keys, *total += them; pass 2 (chunk_tot
// scanned): they are written to dest in order.
__global__ __launch_bounds__(kCopyBlock) void georing_distinct_kernel(const u64* __restrict__ key, int64_t n, int final_ids,
                                                                      int64_t* __restrict__ chunk_tot, u64* __restrict__ total,
                                                                      u64* __restrict__ dest) {
  __shared__ uint32_t s_w[kCopyBlock / 64];
  const int64_t c0 = (int64_t)blockIdx.x * kUniqChunk;
  int64_t at = dest ? chunk_tot[blockIdx.x] : 0;
  for (int sl = 0; sl < kUniqSlices; sl++) {
    const int64_t i = c0 + (int64_t)sl * kCopyBlock + threadIdx.x;
    u64 k = 0;
    bool keep = false;
    if (i < n) {
      k = key[i];
      keep = (i == 0 || (key[i - 1] >> 1) != (k >> 1)) && (!final_ids || (k & 1ull));
    }
    uint32_t m;
    const uint32_t rank = block_rank<kCopyBlock>(keep, s_w, &m);
    if (dest && keep) dest[at + rank] = final_ids ? k >> 1 : k;
    at += m;
  }
  if (!dest && threadIdx.x == 0) {
    chunk_tot[blockIdx.x] = at;
    if (at) atomicAdd(total, (u64)at);
  }
}

// the slab's lists into out_cells: piece i's at base + scan[i], base = counters[base_in]; a
// geometry's first piece writes its offset; the slab's last piece leaves the next slab's base
__global__ __launch_bounds__(kCopyBlock) void georing_gather_kernel(const Seg* __restrict__ segs, const int64_t* __restrict__ seg_cnt,
                                                                    const int64_t* __restrict__ seg_scan, const u64* __restrict__ seg_src,
                                                                    int64_t n_segs, u64* __restrict__ counters, int base_in, int base_out,
                                                                    int64_t* __restrict__ out_cells, int64_t capacity,
                                                                    int64_t* __restrict__ out_offsets) {
  const int64_t si = blockIdx.x;
  if (si >= n_segs) return;
  const int64_t cnt = seg_cnt[si], off = (int64_t)counters[base_in] + seg_scan[si];
  const int64_t* src = (const int64_t*)seg_src[si];
  if (threadIdx.x == 0) {
    if (segs[si].flags & kFirst) out_offsets[segs[si].geom] = off;
    if (si == n_segs - 1) counters[base_out] = (u64)(off + cnt);
  }
  for (int64_t i = threadIdx.x; i < cnt; i += kCopyBlock)
    if (off + i < capacity) out_cells[off + i] = src[i];
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// device allocations of one call outside the context's scratch (the HBM path), freed on every return path
struct Owned {
  std::vector<void*> p;
  ~Owned() {
    for (void* q : p)
      if (q) hipFree(q);
  }
  void drop(void* q) {
    for (void*& x : p)
      if (x == q && q) hipFree(q), x = nullptr;
  }
};

struct RingBufs {
  int64_t *mc, *chunk, *roff, *ring;
  uint32_t* fb_idx;
};

// mgpu_grid_kring's steps (capi.cpp) over n border cells: lists at ring[roff[i] .. roff[i + 1]),
// *total = roff[n] (at most n * list_bound by construction)
int32_t ring_lists(mgpu_ctx* ctx, const char* what, int is, const int64_t* cells, int64_t n, int k, int loop_only, const RingBufs& B,
                   int64_t cap, u64* counters, hipStream_t s, int64_t* total, int64_t* n_fallback) {
  GRING_TRY(hipMemsetAsync(counters, 0, kRingWords * 8, s));
  GRING_TRY(mgpu::launch_kring_count(is, cells, n, k, loop_only, B.mc, B.chunk, B.fb_idx, counters, s));
  u64 h[6] = {0, 0, 0, 0, 0, 0};
  GRING_TRY(hipMemcpyAsync(h, counters, sizeof h, hipMemcpyDeviceToHost, s));
  GRING_TRY(hipStreamSynchronize(s));
  if (h[2] && is == MGPU_H3) return mgpu::set_error(MGPU_E_INVALID_ARG, "%s: %llu border rows are not H3 cell ids", what, h[2]);
  if (h[2])
    return mgpu::set_error(MGPU_E_INVALID_ARG, "%s: %llu border rows are not BNG cells or reach ids BNGIndexSystem.isValid cannot parse",
                           what, h[2]);
  const int64_t n_fb = (int64_t)h[3];
  *n_fallback += n_fb;
  Owned fb;
  uint64_t* scratch = nullptr;
  int64_t batch = 0;
  if (n_fb) {
    const int64_t words = mgpu::kring_fallback_words(k);
    batch = std::max<int64_t>(1, std::min<int64_t>(n_fb, ((int64_t)256 << 20) / 8 / words));
    if (ctx->opt.kring_batch > 0) batch = std::min(batch, ctx->opt.kring_batch);
    GRING_TRY(hipMalloc(&scratch, (size_t)batch * words * 8));
    fb.p.push_back(scratch);
    for (int64_t j0 = 0; j0 < n_fb; j0 += batch)
      GRING_TRY(mgpu::launch_kring_fallback(cells, B.fb_idx, j0, std::min(n_fb, j0 + batch), k, loop_only, B.mc, B.chunk, B.roff,
                                            B.ring, cap, scratch, 0, counters, s));
  }
  GRING_TRY(mgpu::launch_kring_write(is, cells, n, k, loop_only, B.mc, B.chunk, B.roff, B.ring, cap, s));
  for (int64_t j0 = 0; j0 < n_fb; j0 += batch)
    GRING_TRY(mgpu::launch_kring_fallback(cells, B.fb_idx, j0, std::min(n_fb, j0 + batch), k, loop_only, B.mc, B.chunk, B.roff, B.ring,
                                          cap, scratch, 1, counters, s));
  GRING_TRY(hipMemcpyAsync(h, counters, sizeof h, hipMemcpyDeviceToHost, s));
  GRING_TRY(hipMemcpyAsync(total, B.roff + n, 8, hipMemcpyDeviceToHost, s));
  GRING_TRY(hipStreamSynchronize(s));
  if (h[4]) return mgpu::set_error(MGPU_E_INTERNAL, "%s: %llu pentagon walks overflowed their hash set (inconsistent tables)", what, h[4]);
  if (*total > cap) return mgpu::set_error(MGPU_E_INTERNAL, "%s: %lld ring ids for room of %lld", what, (long long)*total, (long long)cap);
  return MGPU_OK;
}

struct Slab {
  int64_t b0, b1;  // border cells (positions in the compacted list)
  int64_t s0, s1;  // pieces
  int64_t rows;    // rows of its first pieces
};

}  // namespace

extern "C" {

int32_t mgpu_geometry_kring(mgpu_ctx* ctx, int32_t index_system, int64_t n_geoms, const int64_t* row_off, const int64_t* cell,
                            const uint8_t* is_core, int32_t k, int32_t loop_only, int64_t* out_cells, int64_t capacity,
                            int64_t* out_offsets, int64_t* out_total, void* stream) {
  const char* what = "geometry_kring";
  if (!ctx) return mgpu::set_error(MGPU_E_INVALID_ARG, "%s: ctx is NULL", what);
  if (int32_t st = GR::check_args(what, index_system, n_geoms, row_off, cell, is_core, k, loop_only, out_cells, capacity, out_offsets,
                                  out_total))
    return st;
  GRING_TRY(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  *out_total = 0;
  int64_t last[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<int64_t> h_row((size_t)n_geoms + 1);
  GRING_TRY(hipMemcpyAsync(h_row.data(), row_off, (size_t)(n_geoms + 1) * 8, hipMemcpyDeviceToHost, s));
  GRING_TRY(hipStreamSynchronize(s));
  for (int64_t g = 0; g < n_geoms; g++)
    if (h_row[g] < 0 || h_row[g + 1] < h_row[g])
      return mgpu::set_error(MGPU_E_INVALID_ARG, "%s: row_off must start at or above 0 and not decrease", what);
  const int64_t n_rows = h_row[n_geoms] - h_row[0];
  if (n_rows > 0 && (!cell || !is_core)) return mgpu::set_error(MGPU_E_INVALID_ARG, "%s: cell / is_core is NULL", what);
  if (n_geoms == 0) {
    GRING_TRY(hipMemsetAsync(out_offsets, 0, 8, s));
    GRING_TRY(hipStreamSynchronize(s));
    GR::note_last(last);
    return MGPU_OK;
  }
  // ---- the border cells, geometry by geometry
  const size_t b_cnt = align256(kCounterWords * 8), b_nb = align256((size_t)(n_geoms + 1) * 8);
  const size_t b_bcell = align256((size_t)std::max<int64_t>(n_rows, 1) * 8);
  if (int32_t st = ensure_scratch(ctx, b_cnt + 2 * b_nb + b_bcell)) return st;
  {
    uint8_t* w = (uint8_t*)ctx->scratch;
    u64* counters = (u64*)w;
    int64_t* d_nb = (int64_t*)(w + b_cnt);
    GRING_TRY(hipMemsetAsync(counters, 0, kCounterWords * 8, s));
    hipLaunchKernelGGL(georing_count_kernel, dim3((unsigned)((n_geoms + 3) / 4)), dim3(kCopyBlock), 0, s, row_off, cell, is_core, n_geoms,
                       d_nb, counters);
    GRING_TRY(hipGetLastError());
  }
  std::vector<int64_t> bstart((size_t)n_geoms + 1);
  {
    uint8_t* w = (uint8_t*)ctx->scratch;
    GRING_TRY(hipMemcpyAsync(bstart.data(), w + b_cnt, (size_t)n_geoms * 8, hipMemcpyDeviceToHost, s));
    GRING_TRY(hipMemcpyAsync(ctx->pin, w, kCounterWords * 8, hipMemcpyDeviceToHost, s));
    GRING_TRY(hipStreamSynchronize(s));
  }
  if (ctx->pin[kBadRow])
    return mgpu::set_error(MGPU_E_INVALID_ARG, "%s: %llu core rows hold no cell id (outside [0, 2^62))", what, (u64)ctx->pin[kBadRow]);
  int64_t n_border = 0;
  for (int64_t g = 0; g < n_geoms; g++) {
    const int64_t c = bstart[g];
    bstart[g] = n_border;
    n_border += c;
  }
  bstart[n_geoms] = n_border;
  // ---- the plan: slabs of border cells, pieces of geometries
  const int64_t bound_a = GR::list_bound(index_system, k, loop_only);
  const int64_t bound_b = loop_only ? GR::list_bound(index_system, k - 1, 0) : 0;
  const int64_t slab_cells =
      std::max<int64_t>(1, std::min<int64_t>(ctx->opt.geomring_slab, GR::kSlabRecords / std::max(bound_a, bound_b)));
  std::vector<Seg> segs;
  std::vector<Slab> slabs;
  Slab cur{0, 0, 0, 0, 0};
  auto close = [&]() {
    cur.s1 = (int64_t)segs.size();
    slabs.push_back(cur);
    cur = Slab{cur.b1, cur.b1, cur.s1, cur.s1, 0};
  };
  for (int64_t g = 0; g < n_geoms; g++) {
    int64_t done = 0;
    const int64_t nb = bstart[g + 1] - bstart[g];
    do {
      if (cur.b1 - cur.b0 >= slab_cells || (int64_t)segs.size() - cur.s0 >= kMaxSegs) close();
      const int64_t take = std::min(nb - done, slab_cells - (cur.b1 - cur.b0));
      Seg sg;
      const bool first = done == 0;
      sg.row0 = h_row[g], sg.row1 = first ? h_row[g + 1] : h_row[g];
      sg.b0 = cur.b1 - cur.b0, sg.b1 = sg.b0 + take;
      sg.stage_rows = cur.rows;
      sg.geom = (int32_t)g;
      sg.flags = (first ? kFirst : 0u) | (done + take == nb ? kLast : 0u);
      cur.rows += sg.row1 - sg.row0;
      cur.b1 += take;
      done += take;
      segs.push_back(sg);
    } while (done < nb);
  }
  close();
  int64_t max_cells = 1, max_rows = 0, max_segs = 1;
  for (const Slab& sl : slabs) {
    max_cells = std::max(max_cells, sl.b1 - sl.b0);
    max_rows = std::max(max_rows, sl.rows);
    max_segs = std::max(max_segs, sl.s1 - sl.s0);
  }
  // scratch: counters | border starts | border cells | pieces | per slab: the ring steps' arrays,
  // the two lists, staging, the pieces' counts, scans, sources and status
  const int64_t cap_a = max_cells * bound_a, cap_b = max_cells * bound_b;
  const size_t b_segs = align256(segs.size() * sizeof(Seg));
  const size_t b_mc = align256((size_t)max_cells * 8), b_fb = align256((size_t)max_cells * 4);
  const size_t b_chunk = align256((size_t)(mgpu::format_chunks(max_cells) + 1) * 8), b_roff = align256((size_t)(max_cells + 1) * 8);
  const size_t b_ring_a = align256((size_t)std::max<int64_t>(cap_a, 1) * 8), b_ring_b = align256((size_t)std::max<int64_t>(cap_b, 1) * 8);
  const size_t b_stage = align256((size_t)std::max<int64_t>(cap_a + cap_b + max_rows, 1) * 8);
  const size_t b_seg8 = align256((size_t)max_segs * 8), b_seg4 = align256((size_t)max_segs * 4);
  if (int32_t st = ensure_scratch(ctx, b_cnt + 2 * b_nb + b_bcell + b_segs + b_mc + b_fb + b_chunk + 2 * b_roff + b_ring_a + b_ring_b +
                                           b_stage + 3 * b_seg8 + b_seg4))
    return st;
  uint8_t* w = (uint8_t*)ctx->scratch;  // (a grown scratch is a new allocation: nothing before is kept but what is on the host)
  u64* counters = (u64*)w;
  w += b_cnt + b_nb;
  int64_t* d_bstart = (int64_t*)w;
  w += b_nb;
  int64_t* d_bcell = (int64_t*)w;
  w += b_bcell;
  Seg* d_segs = (Seg*)w;
  w += b_segs;
  RingBufs A, B;
  A.mc = B.mc = (int64_t*)w;
  w += b_mc;
  A.fb_idx = B.fb_idx = (uint32_t*)w;
  w += b_fb;
  A.chunk = B.chunk = (int64_t*)w;
  w += b_chunk;
  A.roff = (int64_t*)w;
  w += b_roff;
  B.roff = (int64_t*)w;
  w += b_roff;
  A.ring = (int64_t*)w;
  w += b_ring_a;
  B.ring = (int64_t*)w;
  w += b_ring_b;
  int64_t* d_stage = (int64_t*)w;
  w += b_stage;
  int64_t* d_seg_cnt = (int64_t*)w;
  w += b_seg8;
  int64_t* d_seg_scan = (int64_t*)w;
  w += b_seg8;
  u64* d_seg_src = (u64*)w;
  w += b_seg8;
  uint32_t* d_seg_status = (uint32_t*)w;
  GRING_TRY(hipMemsetAsync(counters, 0, kCounterWords * 8, s));
  GRING_TRY(hipMemcpyAsync(d_bstart, bstart.data(), (size_t)(n_geoms + 1) * 8, hipMemcpyHostToDevice, s));
  GRING_TRY(hipMemcpyAsync(d_segs, segs.data(), segs.size() * sizeof(Seg), hipMemcpyHostToDevice, s));
  GRING_TRY(hipEventRecord(ctx->ev0, s));
  if (n_border) {
    hipLaunchKernelGGL(georing_compact_kernel, dim3((unsigned)((n_geoms + 3) / 4)), dim3(kCopyBlock), 0, s, row_off, cell, is_core,
                       n_geoms, d_bstart, d_bcell);
    GRING_TRY(hipGetLastError());
  }
  uint32_t max_slots = GR::kLdsSlots;
  if (ctx->opt.geomring_lds_slots > 0)
    while ((int64_t)max_slots > ctx->opt.geomring_lds_slots && max_slots > GR::kLdsSlotsMin) max_slots >>= 1;
  const uint32_t row_member = loop_only ? 0u : 1u;
  Owned own;
  u64* carry = nullptr;  // the distinct keys of the geometry a slab boundary has cut, so far
  int64_t n_carry = 0;
  std::vector<uint32_t> h_status;
  std::vector<int64_t> h_roff_a, h_roff_b;
  int base = kBase0;
  last[GR::kLastBorder] = n_border;
  last[GR::kLastGenerated] = n_rows;
  for (const Slab& sl : slabs) {
    const int64_t nc = sl.b1 - sl.b0, ns = sl.s1 - sl.s0;
    if (ns == 0) continue;
    last[GR::kLastSlabs]++;
    // ---- ring lists
    int64_t tot_a = 0, tot_b = 0;
    if (nc) {
      if (int32_t st = ring_lists(ctx, what, index_system, d_bcell + sl.b0, nc, k, loop_only, A, cap_a, counters, s, &tot_a,
                                  &last[GR::kLastFallback]))
        return st;
      if (loop_only)
        if (int32_t st = ring_lists(ctx, what, index_system, d_bcell + sl.b0, nc, k - 1, 0, B, cap_b, counters, s, &tot_b,
                                    &last[GR::kLastFallback]))
          return st;
    } else {
      GRING_TRY(hipMemsetAsync(A.roff, 0, 8, s));
      GRING_TRY(hipMemsetAsync(B.roff, 0, 8, s));
    }
    last[GR::kLastGenerated] += tot_a + tot_b;
    // ---- LDS path
    LdsArgs la{d_segs + sl.s0, cell,        A.roff,    A.ring,     loop_only ? B.roff : nullptr, loop_only ? B.ring : nullptr,
               max_slots,      row_member,  d_stage,   d_seg_cnt,  d_seg_src,                    d_seg_status};
    hipLaunchKernelGGL(georing_lds_kernel, dim3((unsigned)ns), dim3(kBlock), 0, s, la);
    GRING_TRY(hipGetLastError());
    h_status.resize((size_t)ns);
    GRING_TRY(hipMemcpyAsync(h_status.data(), d_seg_status, (size_t)ns * 4, hipMemcpyDeviceToHost, s));
    GRING_TRY(hipStreamSynchronize(s));
    // ---- HBM path
    bool have_roff = false;
    std::vector<void*> finished;
    for (int64_t i = 0; i < ns; i++) {
      if (h_status[(size_t)i] == kStatusLds) {
        last[GR::kLastLds]++;
        continue;
      }
      const Seg& sg = segs[(size_t)(sl.s0 + i)];
      if (!have_roff) {
        h_roff_a.assign((size_t)nc + 1, 0), h_roff_b.assign((size_t)nc + 1, 0);
        GRING_TRY(hipMemcpyAsync(h_roff_a.data(), A.roff, (size_t)(nc + 1) * 8, hipMemcpyDeviceToHost, s));
        if (loop_only) GRING_TRY(hipMemcpyAsync(h_roff_b.data(), B.roff, (size_t)(nc + 1) * 8, hipMemcpyDeviceToHost, s));
        GRING_TRY(hipStreamSynchronize(s));
        have_roff = true;
      }
      const int64_t a0 = h_roff_a[(size_t)sg.b0], n_a = h_roff_a[(size_t)sg.b1] - a0;
      const int64_t b0 = h_roff_b[(size_t)sg.b0], n_b = h_roff_b[(size_t)sg.b1] - b0;
      const int64_t n_r = sg.row1 - sg.row0, n_c = (sg.flags & kFirst) ? 0 : n_carry;
      const int64_t n = n_c + n_a + n_b + n_r;
      if (n >= ((int64_t)1 << 31))
        return mgpu::set_error(MGPU_E_UNSUPPORTED, "%s: a geometry with 2^31 records or more in one slab (lower geomring_slab)", what);
      const bool fin = (sg.flags & kLast) != 0;
      u64* dest = nullptr;
      int64_t m = 0;
      if (n > 0) {
        const size_t col = align256((size_t)n * 8), b_hist = align256((size_t)mgpu::sort_pairs_hist_words(n) * 4);
        const int64_t chunks = (n + kUniqChunk - 1) / kUniqChunk;
        uint8_t* hb = nullptr;
        GRING_TRY(hipMalloc(&hb, 4 * col + b_hist + align256((size_t)chunks * 8)));
        own.p.push_back(hb);
        u64 *k0 = (u64*)hb, *v0 = (u64*)(hb + col), *k1 = (u64*)(hb + 2 * col), *v1 = (u64*)(hb + 3 * col);
        uint32_t* hist = (uint32_t*)(hb + 4 * col);
        int64_t* chunk_tot = (int64_t*)(hb + 4 * col + b_hist);
        GRING_TRY(hipMemsetAsync(v0, 0, col, s));
        hipLaunchKernelGGL(georing_emit_kernel, dim3((unsigned)std::min<int64_t>((n + kCopyBlock - 1) / kCopyBlock, 4096)),
                           dim3(kCopyBlock), 0, s, carry, n_c, A.ring + a0, n_a, B.ring + b0, n_b, cell + sg.row0, n_r, row_member, k0);
        GRING_TRY(hipGetLastError());
        GRING_TRY(mgpu::launch_sort_pairs(&k0, &v0, &k1, &v1, n, ~0ull >> 1, hist, s));
        GRING_TRY(hipMemsetAsync(&counters[kHbmCount], 0, 8, s));
        hipLaunchKernelGGL(georing_distinct_kernel, dim3((unsigned)chunks), dim3(kCopyBlock), 0, s, k0, n, fin ? 1 : 0, chunk_tot,
                           &counters[kHbmCount], (u64*)nullptr);
        GRING_TRY(hipGetLastError());
        GRING_TRY(mgpu::launch_scan_sums(chunk_tot, chunks, s));
        GRING_TRY(hipMemcpyAsync(ctx->pin, &counters[kHbmCount], 8, hipMemcpyDeviceToHost, s));
        GRING_TRY(hipStreamSynchronize(s));
        m = (int64_t)ctx->pin[0];
        if (m > 0) {
          GRING_TRY(hipMalloc(&dest, (size_t)m * 8));
          own.p.push_back(dest);
          hipLaunchKernelGGL(georing_distinct_kernel, dim3((unsigned)chunks), dim3(kCopyBlock), 0, s, k0, n, fin ? 1 : 0, chunk_tot,
                             &counters[kHbmCount], dest);
          GRING_TRY(hipGetLastError());
        }
        GRING_TRY(hipStreamSynchronize(s));
        own.drop(hb);
      }
      if (carry) own.drop(carry);
      carry = nullptr, n_carry = 0;
      if (fin) {
        last[GR::kLastHbm]++;
        const u64 src = (u64)dest;
        GRING_TRY(hipMemcpy(d_seg_cnt + i, &m, 8, hipMemcpyHostToDevice));
        GRING_TRY(hipMemcpy(d_seg_src + i, &src, 8, hipMemcpyHostToDevice));
        if (dest) finished.push_back(dest);
      } else {
        carry = dest, n_carry = m;
      }
    }
    // ---- gather
    GRING_TRY(hipMemcpyAsync(d_seg_scan, d_seg_cnt, (size_t)ns * 8, hipMemcpyDeviceToDevice, s));
    GRING_TRY(mgpu::launch_scan_sums(d_seg_scan, ns, s));
    const int next = base == kBase0 ? kBase1 : kBase0;
    hipLaunchKernelGGL(georing_gather_kernel, dim3((unsigned)ns), dim3(kCopyBlock), 0, s, d_segs + sl.s0, d_seg_cnt, d_seg_scan,
                       d_seg_src, ns, counters, base, next, out_cells, capacity, out_offsets);
    GRING_TRY(hipGetLastError());
    base = next;
    if (!finished.empty()) {
      GRING_TRY(hipStreamSynchronize(s));
      for (void* q : finished) own.drop(q);
    }
  }
  GRING_TRY(hipMemcpyAsync(out_offsets + n_geoms, &counters[base], 8, hipMemcpyDeviceToDevice, s));
  GRING_TRY(hipEventRecord(ctx->ev1, s));
  GRING_TRY(hipMemcpyAsync(ctx->pin, &counters[base], 8, hipMemcpyDeviceToHost, s));
  GRING_TRY(hipStreamSynchronize(s));
  const int64_t total = (int64_t)ctx->pin[0];
  float ms = 0.0f;
  GRING_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  last[GR::kLastReturned] = total;
  last[GR::kLastKernelUs] = (int64_t)(ms * 1000.0f);
  GR::note_last(last);
  *out_total = total;
  if (total > capacity)
    return mgpu::set_error(MGPU_E_CAPACITY, "%s: %lld cells needed, %lld given", what, (long long)total, (long long)capacity);
  return MGPU_OK;
}

}  // extern "C"

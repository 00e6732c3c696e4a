// CellAggregate: per-cell counts and sums of a point stream -- the groupBy("index_id")
// .count() / .agg(count, sum) a grid user runs on a cell column before any polygon exists
// (notebooks/examples/python/TransformBNG/transform_join_bng.ipynb:5321, the gridded-EO
// notebooks' EOGriddedSTAC/03. Gridded EO Data.ipynb:3194-3233), as a hash aggregation in
// LDS and HBM instead of a sort of the 8 B/point column.  Kernels and host entry of the
// mgpu_cell_agg_* calls (include/mosaic_gpu.h has the contract).
//
// The table (device, one allocation): keys u64[cap] | count u64[cap] | sum u64[cap] (with a
// sum), cap a power of two, open addressing with linear probes from mix(key) & (cap - 1).
// A free slot's key is kEmpty (all ones: the clear is a memset); the aggregate of the key
// that equals kEmpty lives in a side record (meta[kSideCount], meta[kSideSum]), so every
// int64 is a key.  A slot's key is claimed once by a 64-bit compare-and-swap and never
// changes; counts and sums are 64-bit adds; all device-scope atomics.  Integer arithmetic
// throughout: the results do not depend on scheduling, batch boundaries or growth.
//
// Accumulation (agg_cells_kernel) follows count_kernels.inc's measured shape: a resident
// grid of 1024-thread workgroups at 8 waves per SIMD strides over chunks of 4096 cells,
// two 16-byte loads per thread and column, all in flight before the first probe.  Each
// workgroup keeps an LDS hash table in front of the global one (tag = the cell, u32 count,
// u64 sum; buckets of 4, 8 probes), flushed once per workgroup; a cell that finds no place
// within the probes goes straight to the global table (device-scope atomics run at the
// memory side, ~19 G/s, DESIGN 3.5: the LDS table is what keeps the default path off
// that rate).  A large column with many distinct cells is binned by hash first, so that
// the LDS tables do catch its additions (agg_bin_kernel below).
//
// Growth without losing exactness (host: agg_run).  The load is kept at or below 1/2.  A
// launch of n items onto a table with claimed + n <= cap / 2 cannot overflow and runs as
// one pass.  Otherwise keys first: an insert-only pass (ADD = false) claims slots and adds
// nothing, so it can be repeated; it gives up a key after kProbeLimit probes and raises
// meta[kOverflow]; on that flag, or more than cap / 2 slots claimed, the host doubles the
// table, rehashes with the add_counted kernel (whose source is then the old table itself:
// free slots hold count 0, and a record of count 0 adds nothing) and repeats the pass.  The
// adding pass then finds every key where the insert pass left it and cannot fail.  Keys a
// failing call claimed hold count 0 and are never reported (a rehash drops them).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "capi_internal.h"

struct mgpu_cell_agg {
  int device = 0;
  int32_t is = 0, res = 0;
  bool with_sum = false;
  void* mem = nullptr;  // keys | count | sum
  int64_t cap = 0;
  unsigned long long* meta = nullptr;  // kMetaWords device words
  int64_t claimed = 0;                 // slots claimed at the last synchronisation
};

namespace {

#define CA_TRY(expr)                                                                                     \
  do {                                                                                                   \
    hipError_t _e = (expr);                                                                              \
    if (_e != hipSuccess) return mgpu::set_error(MGPU_E_DEVICE, "%s: %s", #expr, hipGetErrorString(_e)); \
  } while (0)

constexpr unsigned long long kEmpty = ~0ull;
enum { kSideCount = 0, kSideSum = 1, kOverflow = 2, kClaimed = 3, kCursor = 4, kOr = 5, kAnd = 6, kMetaWords = 8 };
constexpr int64_t kFloorEntries = 1024;
constexpr uint32_t kProbeLimit = 1024;  // (<= kFloorEntries: a full table is found out)
constexpr int kAggBlock = 1024;
constexpr int kAggChunk = 4096;
constexpr int kAggLoads = kAggChunk / (kAggBlock * 2);  // 16-byte loads per thread, column and chunk
constexpr int kAggProbes = 8;
// LDS u32 counts: one launch takes at most this many items (launch_agg_cells slices longer
// columns), so no workgroup's share of a launch reaches 2^32
constexpr int64_t kLaunchItems = (int64_t)1 << 31;
static_assert(kLaunchItems % kAggChunk == 0 && kLaunchItems % 8 == 0, "slices keep chunk and bitmap-byte alignment");

struct AggTable {
  unsigned long long* keys;
  unsigned long long* count;
  unsigned long long* sum;  // nullptr: no sum
  unsigned long long* meta;
  uint64_t mask;  // cap - 1
};

__device__ __forceinline__ uint64_t agg_mix(uint64_t c) {
  c ^= c >> 33;
  c *= 0xff51afd7ed558ccdULL;
  c ^= c >> 33;
  c *= 0xc4ceb9fe1a85ec53ULL;
  c ^= c >> 33;
  return c;
}

// key (!= kEmpty) into the global table: find or claim its slot, ADD: add k and w to it.
// ADD = false gives up after kProbeLimit probes (the table is then too full: meta[kOverflow]);
// ADD = true is only launched where a place is certain (see the head comment).
template <bool W, bool ADD>
__device__ __forceinline__ void agg_global(const AggTable& t, unsigned long long key, uint64_t hash,
                                           unsigned long long k, unsigned long long w, uint32_t* s_claimed) {
  uint64_t h = hash & t.mask;
  uint32_t probes = 0;
#pragma unroll 1
  for (;;) {
    unsigned long long cur = __hip_atomic_load(&t.keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kEmpty) {
      cur = atomicCAS(&t.keys[h], kEmpty, key);
      if (cur == kEmpty) {
        atomicAdd(s_claimed, 1u);
        cur = key;
      }
    }
    if (cur == key) break;
    h = (h + 1) & t.mask;
    if (!ADD && ++probes > kProbeLimit) {
      __hip_atomic_store(&t.meta[kOverflow], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return;
    }
  }
  if (ADD) {
    atomicAdd(&t.count[h], k);
    if (W) atomicAdd(&t.sum[h], w);
  }
}

template <bool W>
struct AggLds {
  // 4096 entries of {u64 tag, u32 count}: 48 KiB; with u64 sums 2048 entries: 40 KiB --
  // either way two workgroups of 1024 threads per CU (8 waves per SIMD)
  static constexpr uint32_t kEntries = W ? 2048 : 4096;
  static constexpr int kShift = W ? 53 : 52;  // the hash's top bits
};

// a thread's share of a chunk of an int64 column: two 16-byte loads (vec: the chunk is whole
// and the column 16-byte aligned), else element by element, 0 past the end
__device__ __forceinline__ void agg_load_chunk(const int64_t* __restrict__ col, bool vec, int64_t c0, int64_t n,
                                               unsigned long long* v) {
  if (vec) {
#pragma unroll
    for (int q = 0; q < kAggLoads; q++) {
      const ulonglong2 u = *(const ulonglong2*)(col + c0 + ((int64_t)q * kAggBlock + threadIdx.x) * 2);
      v[2 * q] = u.x, v[2 * q + 1] = u.y;
    }
  } else {
#pragma unroll
    for (int q = 0; q < kAggLoads; q++)
#pragma unroll
      for (int j = 0; j < 2; j++) {
        const int64_t p = c0 + ((int64_t)q * kAggBlock + threadIdx.x) * 2 + j;
        v[2 * q + j] = p < n ? (unsigned long long)col[p] : 0ull;
      }
  }
}
__device__ __forceinline__ int64_t agg_item(int64_t c0, int i) {
  return c0 + ((int64_t)(i >> 1) * kAggBlock + threadIdx.x) * 2 + (i & 1);
}

// W: sums; ADD: see agg_global; LDS: the workgroup's table in front (option cellagg_lds).
// valid: optional Arrow bitmap at bit offset voff.  weight is read only with W && ADD.
// run = 0: the workgroups stride over the chunks; run > 0: each takes `run` consecutive
// chunks (a binned column: a run meets the cells of a few bins, which its table holds).
template <bool W, bool ADD, bool LDS>
__global__ __launch_bounds__(kAggBlock) __attribute__((amdgpu_waves_per_eu(8, 8)))
void agg_cells_kernel(AggTable t, const int64_t* __restrict__ cells, const uint8_t* __restrict__ valid, int64_t voff,
                      const int64_t* __restrict__ weight, int64_t n, int64_t n_chunks, int64_t run) {
  constexpr uint32_t H = AggLds<W>::kEntries;
  __shared__ unsigned long long s_tag[LDS ? H : 1];
  __shared__ uint32_t s_cnt[LDS ? H : 1];
  __shared__ unsigned long long s_sum[(LDS && W) ? H : 1];
  __shared__ unsigned long long s_side_sum;
  __shared__ uint32_t s_side_cnt, s_claimed;
  if (LDS) {
    for (uint32_t i = threadIdx.x; i < H; i += kAggBlock) {
      s_tag[i] = kEmpty;
      s_cnt[i] = 0;
      if (W) s_sum[i] = 0;
    }
  }
  if (threadIdx.x == 0) s_side_sum = 0, s_side_cnt = 0, s_claimed = 0;
  __syncthreads();
  const bool cells16 = (((uintptr_t)cells) & 15) == 0, weight16 = (((uintptr_t)weight) & 15) == 0;
  const int64_t c_begin = run ? (int64_t)blockIdx.x * run : (int64_t)blockIdx.x, c_step = run ? 1 : (int64_t)gridDim.x;
  const int64_t c_end = run && c_begin + run < n_chunks ? c_begin + run : n_chunks;
  for (int64_t chunk = c_begin; chunk < c_end; chunk += c_step) {
    // (an insert-only pass that has overflowed is repeated on a larger table: stop early)
    if (!ADD && __hip_atomic_load(&t.meta[kOverflow], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
    const int64_t c0 = chunk * kAggChunk;
    const bool whole = c0 + kAggChunk <= n;
    unsigned long long key[2 * kAggLoads], w[2 * kAggLoads];
    agg_load_chunk(cells, whole && cells16, c0, n, key);
    if (W && ADD) {
      agg_load_chunk(weight, whole && weight16, c0, n, w);
    } else {
#pragma unroll
      for (int i = 0; i < 2 * kAggLoads; i++) w[i] = 0;
    }
#pragma unroll
    for (int i = 0; i < 2 * kAggLoads; i++) {
      const int64_t p = agg_item(c0, i);
      bool has = p < n;
      if (has && valid) has = (valid[(voff + p) >> 3] >> ((voff + p) & 7)) & 1;
      if (!has) continue;
      const unsigned long long c = key[i];
      if (c == kEmpty) {
        if (ADD) {
          atomicAdd(&s_side_cnt, 1u);
          if (W) atomicAdd(&s_side_sum, w[i]);
        }
        continue;
      }
      const uint64_t hash = agg_mix(c);
      bool placed = false;
      if (LDS) {
        // a tag is set once (free -> cell) and never changes: a read of a set tag is final
        uint32_t e = (uint32_t)(hash >> AggLds<W>::kShift) & ~3u;
#pragma unroll 1
        for (int pr = 0; pr < kAggProbes; pr++, e = (e + 1) & (H - 1)) {
          unsigned long long tg = __hip_atomic_load(&s_tag[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          if (tg == kEmpty) {
            tg = atomicCAS(&s_tag[e], kEmpty, c);
            if (tg == kEmpty) tg = c;
          }
          if (tg == c) {
            if (ADD) {
              atomicAdd(&s_cnt[e], 1u);
              if (W) atomicAdd(&s_sum[e], w[i]);
            }
            placed = true;
            break;
          }
        }
      }
      if (!placed) agg_global<W, ADD>(t, c, hash, 1ull, w[i], &s_claimed);
    }
  }
  __syncthreads();
  if (LDS) {
    for (uint32_t i = threadIdx.x; i < H; i += kAggBlock) {
      const unsigned long long tg = s_tag[i];
      if (tg != kEmpty) agg_global<W, ADD>(t, tg, agg_mix(tg), (unsigned long long)s_cnt[i], W ? s_sum[i] : 0ull, &s_claimed);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (s_claimed) atomicAdd(&t.meta[kClaimed], (unsigned long long)s_claimed);
    if (ADD && s_side_cnt) {
      atomicAdd(&t.meta[kSideCount], (unsigned long long)s_side_cnt);
      if (W) atomicAdd(&t.meta[kSideSum], s_side_sum);
    }
  }
}

// Binning in front of the accumulation (host: agg_bin).  With more distinct cells than an
// LDS table holds and no order in the input, nearly every addition would be a device-scope
// atomic (1e8 of them: 5 to 8 ms).  So a large column is first dealt into kBins bins by
// hash bits the tables do not index with -- a counting sort: per-workgroup bin histograms
// over runs of chunks, their scan (scan_rows_kernel), a scatter of cells and weights
// through per-workgroup LDS cursors -- and the accumulation then takes the binned column in
// runs: a workgroup meets the cells of a few bins only, and its table holds them.
constexpr int kBins = 512;
constexpr int kBinShift = 40;  // hash bits 40..48 (the LDS tables use 52.., the global table the low bits)
__device__ __forceinline__ uint32_t agg_bin(unsigned long long cell) {
  return (uint32_t)(agg_mix(cell) >> kBinShift) & (kBins - 1);
}

// SCATTER = false: hist[bin * groups + group] = the group's cells per bin; SCATTER = true:
// hist and tot hold the scan of that (scan_rows_kernel), the cells (W: and weights) go to their places
template <bool SCATTER, bool W>
__global__ __launch_bounds__(kAggBlock) void agg_bin_kernel(const int64_t* __restrict__ cells,
                                                            const int64_t* __restrict__ weight, int64_t n, int64_t n_chunks,
                                                            int64_t run, uint32_t* __restrict__ hist,
                                                            const uint32_t* __restrict__ tot,
                                                            int64_t* __restrict__ out_cells, int64_t* __restrict__ out_weight) {
  __shared__ uint32_t s_b[kBins];
  for (int i = threadIdx.x; i < kBins; i += kAggBlock) s_b[i] = SCATTER ? tot[i] + hist[(int64_t)i * gridDim.x + blockIdx.x] : 0u;
  __syncthreads();
  const bool cells16 = (((uintptr_t)cells) & 15) == 0, weight16 = (((uintptr_t)weight) & 15) == 0;
  const int64_t c_begin = (int64_t)blockIdx.x * run;
  const int64_t c_end = c_begin + run < n_chunks ? c_begin + run : n_chunks;
  for (int64_t chunk = c_begin; chunk < c_end; chunk++) {
    const int64_t c0 = chunk * kAggChunk;
    const bool whole = c0 + kAggChunk <= n;
    unsigned long long key[2 * kAggLoads], w[2 * kAggLoads];
    agg_load_chunk(cells, whole && cells16, c0, n, key);
    if (SCATTER && W) agg_load_chunk(weight, whole && weight16, c0, n, w);
#pragma unroll
    for (int i = 0; i < 2 * kAggLoads; i++) {
      if (agg_item(c0, i) >= n) continue;
      const uint32_t pos = atomicAdd(&s_b[agg_bin(key[i])], 1u);
      if (SCATTER && (int64_t)pos < n) {  // (always: the histograms were taken from the same column)
        out_cells[pos] = (int64_t)key[i];
        if (W) out_weight[pos] = (int64_t)w[i];
      }
    }
  }
  if (!SCATTER) {
    __syncthreads();
    for (int i = threadIdx.x; i < kBins; i += kAggBlock) hist[(int64_t)i * gridDim.x + blockIdx.x] = s_b[i];
  }
}

// (cell, count, sum) records, one per thread; count <= 0 adds nothing.  Reloads a fetched
// result, merges another aggregate's, and rehashes the table itself on growth.
template <bool W, bool ADD>
__global__ __launch_bounds__(256) void agg_counted_kernel(AggTable t, const int64_t* __restrict__ cells,
                                                          const int64_t* __restrict__ count,
                                                          const int64_t* __restrict__ sum, int64_t n) {
  __shared__ uint32_t s_claimed;
  if (threadIdx.x == 0) s_claimed = 0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const int64_t k = count[i];
    if (k > 0) {
      const unsigned long long c = (unsigned long long)cells[i];
      const unsigned long long w = W ? (unsigned long long)sum[i] : 0ull;
      if (c == kEmpty) {
        if (ADD) {
          atomicAdd(&t.meta[kSideCount], (unsigned long long)k);
          if (W) atomicAdd(&t.meta[kSideSum], w);
        }
      } else {
        agg_global<W, ADD>(t, c, agg_mix(c), (unsigned long long)k, w, &s_claimed);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_claimed) atomicAdd(&t.meta[kClaimed], (unsigned long long)s_claimed);
}

// ---- fetch: count, compact, radix sort, split

__device__ __forceinline__ unsigned long long wave_or_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v |= (unsigned long long)__shfl_xor((long long)v, o, 64);
  return v;
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}

// the slots with count > 0: their number to meta[kCursor]; WRITE: the records {key, slot}
// to (out_key, out_slot), the OR and AND of the keys to meta[kOr], meta[kAnd]; the side
// record as slot = cap.  A wave counts its run of slots, takes its place from the cursor
// with one atomic, and reads the run again to write (any order: the sort follows).
template <bool WRITE>
__global__ __launch_bounds__(256) void agg_compact_kernel(AggTable t, int64_t cap, unsigned long long* __restrict__ out_key,
                                                          unsigned long long* __restrict__ out_slot) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
  const int64_t seg = ((cap + n_waves - 1) / n_waves + 63) & ~(int64_t)63;
  const int64_t b = wave * seg < cap ? wave * seg : cap, e = b + seg < cap ? b + seg : cap;
  uint32_t mine = 0;
  for (int64_t i = b + lane; i < e; i += 64) mine += t.count[i] != 0 ? 1u : 0u;
  const uint32_t total = wave_sum_u32(mine);
  unsigned long long vor = 0, vand = ~0ull;
  if (total) {
    unsigned long long run = 0;
    if (lane == 0) run = atomicAdd(&t.meta[kCursor], (unsigned long long)total);
    if (WRITE) {
      run = (unsigned long long)__shfl((long long)run, 0, 64);
      for (int64_t i0 = b; i0 < e; i0 += 64) {
        const int64_t i = i0 + lane;
        const bool has = i < e && t.count[i] != 0;
        const unsigned long long m = __ballot(has);
        if (has) {
          const unsigned long long pos = run + (unsigned long long)__popcll(m & ((1ull << lane) - 1));
          const unsigned long long key = t.keys[i];
          out_key[pos] = key;
          out_slot[pos] = (unsigned long long)i;
          vor |= key, vand &= key;
        }
        run += (unsigned long long)__popcll(m);
      }
    }
  }
  if (WRITE) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && t.meta[kSideCount] != 0) {
      const unsigned long long pos = atomicAdd(&t.meta[kCursor], 1ull);
      out_key[pos] = kEmpty;
      out_slot[pos] = (unsigned long long)cap;
      vor |= kEmpty, vand &= kEmpty;
    }
    vor = wave_or_u64(vor);
    vand = ~wave_or_u64(~vand);
    if (lane == 0) {
      if (vor) atomicOr(&t.meta[kOr], vor);
      if (vand != ~0ull) atomicAnd(&t.meta[kAnd], vand);
    }
  }
}

// LSD radix sort, 8-bit digits, one wave per tile of kSortTile records (four tiles per
// workgroup).  A pass: per-tile digit histograms (digit-major: hist[digit * tiles + tile]),
// their exclusive scan (scan_rows_kernel), a stable scatter.  The host skips a pass whose digit is equal in
// all keys.  Signed order: the top digit is taken with its sign bit flipped.
constexpr int kSortTile = 1024;
constexpr int kSortWaves = 4;

__device__ __forceinline__ uint32_t sort_digit(unsigned long long key, int d) {
  const uint32_t v = (uint32_t)(key >> (8 * d)) & 0xFFu;
  return d == 7 ? v ^ 0x80u : v;
}

__global__ __launch_bounds__(64 * kSortWaves) void sort_hist_kernel(const unsigned long long* __restrict__ key, int64_t n,
                                                                     int64_t tiles, int d, uint32_t* __restrict__ hist) {
  __shared__ uint32_t s_cnt[kSortWaves][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = lane; i < 256; i += 64) s_cnt[wave][i] = 0;
  __syncthreads();
  const int64_t tile = (int64_t)blockIdx.x * kSortWaves + wave;
  const int64_t t0 = tile * kSortTile;
  for (int r = 0; r < kSortTile / 64; r++) {
    const int64_t i = t0 + r * 64 + lane;
    if (tile < tiles && i < n) atomicAdd(&s_cnt[wave][sort_digit(key[i], d)], 1u);
  }
  __syncthreads();
  if (tile < tiles)
    for (int i = lane; i < 256; i += 64) hist[(int64_t)i * tiles + tile] = s_cnt[wave][i];
}

// Exclusive scan of a histogram of `rows` rows (digits, bins) of `len` entries, row-major:
// every row in place by its own workgroup (tot[row] = the row's sum), then tot in place by
// one workgroup; an entry's offset is tot[row] + its own.  rows <= 1024.
__global__ __launch_bounds__(256) void scan_rows_kernel(uint32_t* __restrict__ v, int64_t len, uint32_t* __restrict__ tot) {
  __shared__ uint32_t s_v[256];
  uint32_t* const row = v + (int64_t)blockIdx.x * len;
  uint32_t carry = 0;
  for (int64_t i0 = 0; i0 < len; i0 += 256) {
    const int64_t i = i0 + threadIdx.x;
    const uint32_t x = i < len ? row[i] : 0u;
    s_v[threadIdx.x] = x;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const uint32_t add = (int)threadIdx.x >= o ? s_v[threadIdx.x - o] : 0u;
      __syncthreads();
      s_v[threadIdx.x] += add;
      __syncthreads();
    }
    if (i < len) row[i] = carry + s_v[threadIdx.x] - x;
    carry += s_v[255];
    __syncthreads();
  }
  if (threadIdx.x == 0) tot[blockIdx.x] = carry;
}
__global__ __launch_bounds__(1024) void scan_tot_kernel(uint32_t* __restrict__ tot, int rows) {
  __shared__ uint32_t s_v[1024];
  const uint32_t x = (int)threadIdx.x < rows ? tot[threadIdx.x] : 0u;
  s_v[threadIdx.x] = x;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const uint32_t add = (int)threadIdx.x >= o ? s_v[threadIdx.x - o] : 0u;
    __syncthreads();
    s_v[threadIdx.x] += add;
    __syncthreads();
  }
  if ((int)threadIdx.x < rows) tot[threadIdx.x] = s_v[threadIdx.x] - x;
}

__global__ __launch_bounds__(64 * kSortWaves) void sort_scatter_kernel(const unsigned long long* __restrict__ key,
                                                                        const unsigned long long* __restrict__ val,
                                                                        int64_t n, int64_t tiles, int d,
                                                                        const uint32_t* __restrict__ hist,
                                                                        const uint32_t* __restrict__ tot,
                                                                        unsigned long long* __restrict__ out_key,
                                                                        unsigned long long* __restrict__ out_val) {
  __shared__ uint32_t s_base[kSortWaves][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t tile = (int64_t)blockIdx.x * kSortWaves + wave;
  for (int i = lane; i < 256; i += 64) s_base[wave][i] = tile < tiles ? tot[i] + hist[(int64_t)i * tiles + tile] : 0u;
  __syncthreads();
  const int64_t t0 = tile * kSortTile;
  for (int r = 0; r < kSortTile / 64; r++) {
    const int64_t i = t0 + r * 64 + lane;
    const bool in = tile < tiles && i < n;
    const unsigned long long k = in ? key[i] : 0ull;
    const unsigned long long v = in ? val[i] : 0ull;
    const uint32_t dg = sort_digit(k, d);
    // the lanes of this round with the same digit; the rank among them keeps the order
    unsigned long long peers = __ballot(in);
#pragma unroll
    for (int b = 0; b < 8; b++) {
      const bool bit = (dg >> b) & 1u;
      const unsigned long long m = __ballot(in && bit);
      peers &= bit ? m : ~m;
    }
    const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1));
    if (in) {
      const uint32_t pos = s_base[wave][dg] + rank;
      if ((int64_t)pos < n) {  // (always: the histograms were taken from the same keys)
        out_key[pos] = k;
        out_val[pos] = v;
      }
    }
    __syncthreads();
    if (in && rank == 0) s_base[wave][dg] += (uint32_t)__popcll(peers);
    __syncthreads();
  }
}

// the sorted records into the output columns
__global__ __launch_bounds__(256) void agg_split_kernel(AggTable t, int64_t cap, const unsigned long long* __restrict__ key,
                                                        const unsigned long long* __restrict__ slot, int64_t n,
                                                        int64_t* __restrict__ out_cell, int64_t* __restrict__ out_count,
                                                        int64_t* __restrict__ out_sum) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned long long s = slot[i];
  const bool side = s >= (unsigned long long)cap;
  out_cell[i] = (int64_t)key[i];
  out_count[i] = (int64_t)(side ? t.meta[kSideCount] : t.count[s]);
  if (out_sum) out_sum[i] = (int64_t)(side ? t.meta[kSideSum] : t.sum[s]);
}

// ---- host

AggTable table_of(const mgpu_cell_agg* a) {
  AggTable t;
  t.keys = (unsigned long long*)a->mem;
  t.count = t.keys + a->cap;
  t.sum = a->with_sum ? t.count + a->cap : nullptr;
  t.meta = a->meta;
  t.mask = (uint64_t)a->cap - 1;
  return t;
}

size_t table_bytes(const mgpu_cell_agg* a, int64_t cap) { return (size_t)cap * (a->with_sum ? 24 : 16); }

hipError_t clear_table(void* mem, int64_t cap, bool with_sum, hipStream_t s) {
  if (hipError_t e = hipMemsetAsync(mem, 0xFF, (size_t)cap * 8, s)) return e;
  return hipMemsetAsync((uint8_t*)mem + (size_t)cap * 8, 0, (size_t)cap * (with_sum ? 16 : 8), s);
}

// meta -> the context's pinned page; synchronises the stream
int32_t read_meta(mgpu_ctx* ctx, const mgpu_cell_agg* a, hipStream_t s) {
  CA_TRY(hipMemcpyAsync(ctx->pin, a->meta, kMetaWords * 8, hipMemcpyDeviceToHost, s));
  CA_TRY(hipStreamSynchronize(s));
  return MGPU_OK;
}

int resident_groups() {
  static int groups = 0;
  if (groups == 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      n = 256;
    groups = 2 * std::max(n, 1);  // two workgroups of 1024 threads per CU
  }
  return groups;
}

template <bool W, bool ADD>
hipError_t launch_cells_lds(bool lds, int64_t grid, hipStream_t s, const AggTable& t, const int64_t* cells,
                            const uint8_t* valid, int64_t voff, const int64_t* weight, int64_t n, int64_t nc, int64_t run) {
  if (lds)
    hipLaunchKernelGGL((agg_cells_kernel<W, ADD, true>), dim3((unsigned)grid), dim3(kAggBlock), 0, s, t, cells, valid, voff, weight, n, nc, run);
  else
    hipLaunchKernelGGL((agg_cells_kernel<W, ADD, false>), dim3((unsigned)grid), dim3(kAggBlock), 0, s, t, cells, valid, voff, weight, n, nc, run);
  return hipGetLastError();
}

// a cell column onto the table, in launches of at most kLaunchItems; runs: a binned column,
// every workgroup takes consecutive chunks
hipError_t launch_agg_cells(const mgpu_ctx* ctx, const mgpu_cell_agg* a, bool add, const int64_t* cells, const uint8_t* valid,
                            int64_t voff, const int64_t* weight, int64_t n, hipStream_t s, bool runs = false) {
  const AggTable t = table_of(a);
  const bool lds = ctx->opt.cellagg_lds != 0;
  for (int64_t off = 0; off < n; off += kLaunchItems) {
    const int64_t m = std::min(n - off, kLaunchItems);
    const int64_t nc = (m + kAggChunk - 1) / kAggChunk;
    int64_t grid = std::min<int64_t>(nc, resident_groups());
    if (ctx->opt.cellagg_groups) grid = std::min<int64_t>(grid, ctx->opt.cellagg_groups);
    const int64_t* w = weight ? weight + off : nullptr;
    const int64_t run = runs ? (nc + grid - 1) / grid : 0;
    hipError_t e;
    if (!add)
      e = launch_cells_lds<false, false>(lds, grid, s, t, cells + off, valid, voff + off, nullptr, m, nc, run);
    else if (a->with_sum)
      e = launch_cells_lds<true, true>(lds, grid, s, t, cells + off, valid, voff + off, w, m, nc, run);
    else
      e = launch_cells_lds<false, true>(lds, grid, s, t, cells + off, valid, voff + off, nullptr, m, nc, run);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_agg_counted(const AggTable& t, bool with_sum, bool add, const int64_t* cells, const int64_t* count,
                              const int64_t* sum, int64_t n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (!add)
    hipLaunchKernelGGL((agg_counted_kernel<false, false>), grid, dim3(256), 0, s, t, cells, count, sum, n);
  else if (with_sum)
    hipLaunchKernelGGL((agg_counted_kernel<true, true>), grid, dim3(256), 0, s, t, cells, count, sum, n);
  else
    hipLaunchKernelGGL((agg_counted_kernel<false, true>), grid, dim3(256), 0, s, t, cells, count, sum, n);
  return hipGetLastError();
}

// double the table and rehash: the old table's arrays are the add_counted records.  They
// are distinct and at most old cap = new cap / 2, so the single pass cannot overflow.
int32_t grow(mgpu_ctx* ctx, mgpu_cell_agg* a, hipStream_t s) {
  if (a->cap >= ((int64_t)1 << 40)) return mgpu::set_error(MGPU_E_INTERNAL, "cell aggregate: table of 2^40 entries overflowed");
  const int64_t cap2 = a->cap * 2;
  void* mem2 = nullptr;
  CA_TRY(hipMalloc(&mem2, table_bytes(a, cap2)));
  mgpu_cell_agg b = *a;
  b.mem = mem2, b.cap = cap2;
  const AggTable old = table_of(a);
  hipError_t e = clear_table(mem2, cap2, a->with_sum, s);
  if (e == hipSuccess) e = hipMemsetAsync(a->meta + kOverflow, 0, 16, s);  // (kOverflow, kClaimed)
  // (the side record stays in meta: the kernel meets no kEmpty key with a count)
  if (e == hipSuccess)
    e = launch_agg_counted(table_of(&b), a->with_sum, true, (const int64_t*)old.keys, (const int64_t*)old.count,
                           (const int64_t*)old.sum, a->cap, s);
  int32_t st = MGPU_OK;
  if (e != hipSuccess) st = mgpu::set_error(MGPU_E_DEVICE, "cell aggregate rehash: %s", hipGetErrorString(e));
  if (!st) st = read_meta(ctx, &b, s);
  if (st) {
    hipFree(mem2);
    return st;
  }
  hipFree(a->mem);
  a->mem = mem2;
  a->cap = cap2;
  a->claimed = (int64_t)ctx->pin[kClaimed];
  return MGPU_OK;
}

// n items through `launch(add)` (see the head comment); synchronises the stream
template <class F>
int32_t agg_run(mgpu_ctx* ctx, mgpu_cell_agg* a, int64_t n, hipStream_t s, F launch) {
  if (a->claimed + n > a->cap / 2) {
    for (;;) {
      CA_TRY(hipMemsetAsync(a->meta + kOverflow, 0, 8, s));
      CA_TRY(launch(false));
      if (int32_t st = read_meta(ctx, a, s)) return st;
      a->claimed = (int64_t)ctx->pin[kClaimed];
      if (!ctx->pin[kOverflow] && a->claimed <= a->cap / 2) break;
      if (int32_t st = grow(ctx, a, s)) return st;
    }
  }
  CA_TRY(launch(true));
  if (int32_t st = read_meta(ctx, a, s)) return st;
  a->claimed = (int64_t)ctx->pin[kClaimed];
  return MGPU_OK;
}

// Binning (see agg_bin_kernel).  A column qualifies by its size (option cellagg_bin_min) --
// one launch, no validity bitmap; it is binned when the aggregate is known to hold more
// cells than an LDS table does, or, while it holds few, when an insert-only pass over the
// column's head finds that many (the keys it claims are wanted anyway).
constexpr int64_t kBinCells = 2048;
constexpr int64_t kBinSample = 1 << 20;

bool bin_candidate(const mgpu_ctx* ctx, const uint8_t* valid, int64_t n) {
  return ctx->opt.cellagg_bin_min > 0 && n >= ctx->opt.cellagg_bin_min && n <= kLaunchItems && !valid;
}
int64_t bin_groups(int64_t n, int64_t* run) {
  const int64_t nc = (n + kAggChunk - 1) / kAggChunk;
  *run = (nc + resident_groups() - 1) / resident_groups();
  return (nc + *run - 1) / *run;
}
// scratch a binned column needs: the binned cells, the binned weights, the histograms
size_t bin_column(int64_t n) { return ((size_t)n * 8 + 255) & ~(size_t)255; }
size_t bin_bytes(int64_t n, bool with_sum) {
  int64_t run;
  return bin_column(n) * (with_sum ? 2 : 1) + ((size_t)bin_groups(n, &run) + 1) * kBins * 4;
}

// cells (and weight) dealt into out (bin_bytes of scratch): *b_cells, *b_weight
hipError_t agg_bin(bool with_sum, const int64_t* cells, const int64_t* weight, int64_t n, void* out, hipStream_t s,
                   const int64_t** b_cells, const int64_t** b_weight) {
  int64_t run;
  const int64_t groups = bin_groups(n, &run), nc = (n + kAggChunk - 1) / kAggChunk;
  int64_t* oc = (int64_t*)out;
  int64_t* ow = with_sum ? (int64_t*)((uint8_t*)out + bin_column(n)) : nullptr;
  uint32_t* hist = (uint32_t*)((uint8_t*)out + bin_column(n) * (with_sum ? 2 : 1));
  const dim3 grid((unsigned)groups), block(kAggBlock);
  uint32_t* tot = hist + groups * kBins;
  hipLaunchKernelGGL((agg_bin_kernel<false, false>), grid, block, 0, s, cells, nullptr, n, nc, run, hist, nullptr, nullptr, nullptr);
  hipLaunchKernelGGL(scan_rows_kernel, dim3(kBins), dim3(256), 0, s, hist, groups, tot);
  hipLaunchKernelGGL(scan_tot_kernel, dim3(1), dim3(1024), 0, s, tot, kBins);
  if (with_sum)
    hipLaunchKernelGGL((agg_bin_kernel<true, true>), grid, block, 0, s, cells, weight, n, nc, run, hist, tot, oc, ow);
  else
    hipLaunchKernelGGL((agg_bin_kernel<true, false>), grid, block, 0, s, cells, nullptr, n, nc, run, hist, tot, oc, nullptr);
  *b_cells = oc, *b_weight = ow;
  return hipGetLastError();
}

// a device cell column onto the aggregate (the body of add_cells and add_points); bins: a
// bin_candidate's scratch of bin_bytes, or nullptr
int32_t agg_add_column(mgpu_ctx* ctx, mgpu_cell_agg* a, const int64_t* cells, const uint8_t* valid, int64_t voff,
                       const int64_t* weight, int64_t n, void* bins, hipStream_t s) {
  bool runs = false;
  if (bins) {
    bool many = a->claimed > kBinCells;
    if (!many) {
      CA_TRY(hipMemsetAsync(a->meta + kOverflow, 0, 8, s));
      CA_TRY(launch_agg_cells(ctx, a, false, cells, nullptr, 0, nullptr, std::min(n, kBinSample), s));
      if (int32_t st = read_meta(ctx, a, s)) return st;
      a->claimed = (int64_t)ctx->pin[kClaimed];
      many = ctx->pin[kOverflow] || a->claimed > kBinCells;
    }
    if (many) {
      CA_TRY(agg_bin(a->with_sum, cells, weight, n, bins, s, &cells, &weight));
      runs = true;
    }
  }
  return agg_run(ctx, a, n, s, [&](bool add) { return launch_agg_cells(ctx, a, add, cells, valid, voff, weight, n, s, runs); });
}

int32_t check_handles(const mgpu_ctx* ctx, const mgpu_cell_agg* a, const char* what) {
  if (!ctx || !a) return mgpu::set_error(MGPU_E_INVALID_ARG, "%s: ctx / aggregate is NULL", what);
  if (ctx->device != a->device)
    return mgpu::set_error(MGPU_E_INVALID_ARG, "%s: the aggregate lives on device %d, the context on %d", what, a->device, ctx->device);
  return MGPU_OK;
}

int32_t check_weight(const mgpu_cell_agg* a, const void* weight, const char* what, const char* name) {
  if ((weight != nullptr) != a->with_sum)
    return mgpu::set_error(MGPU_E_INVALID_ARG, "%s: %s is given exactly on an aggregate created with a sum", what, name);
  return MGPU_OK;
}

// the number of cells with count > 0; synchronises the stream
int32_t agg_size(mgpu_ctx* ctx, const mgpu_cell_agg* a, hipStream_t s, int64_t* out) {
  CA_TRY(hipMemsetAsync(a->meta + kCursor, 0, 8, s));
  const int64_t grid = std::min<int64_t>((a->cap + 255) / 256, 512);
  hipLaunchKernelGGL((agg_compact_kernel<false>), dim3((unsigned)grid), dim3(256), 0, s, table_of(a), a->cap, nullptr, nullptr);
  CA_TRY(hipGetLastError());
  if (int32_t st = read_meta(ctx, a, s)) return st;
  *out = (int64_t)ctx->pin[kCursor] + (ctx->pin[kSideCount] ? 1 : 0);
  return MGPU_OK;
}

}  // namespace

namespace mgpu {

// kernels.h: the radix sort above for another unit (geom_ring.hip's HBM path)
int64_t sort_pairs_hist_words(int64_t n) { return ((n + kSortTile - 1) / kSortTile + 1) * 256; }

hipError_t launch_sort_pairs(unsigned long long** k0, unsigned long long** v0, unsigned long long** k1,
                             unsigned long long** v1, int64_t n, unsigned long long differ, uint32_t* hist, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int64_t tiles = (n + kSortTile - 1) / kSortTile;
  uint32_t* tot = hist + tiles * 256;
  const dim3 sgrid((unsigned)((tiles + kSortWaves - 1) / kSortWaves));
  for (int d = 0; d < 8; d++) {
    if (((differ >> (8 * d)) & 0xFFu) == 0) continue;  // this digit is equal in all keys
    hipLaunchKernelGGL(sort_hist_kernel, sgrid, dim3(64 * kSortWaves), 0, s, *k0, n, tiles, d, hist);
    hipLaunchKernelGGL(scan_rows_kernel, dim3(256), dim3(256), 0, s, hist, tiles, tot);
    hipLaunchKernelGGL(scan_tot_kernel, dim3(1), dim3(1024), 0, s, tot, 256);
    hipLaunchKernelGGL(sort_scatter_kernel, sgrid, dim3(64 * kSortWaves), 0, s, *k0, *v0, n, tiles, d, hist, tot, *k1, *v1);
    if (hipError_t e = hipGetLastError()) return e;
    std::swap(*k0, *k1);
    std::swap(*v0, *v1);
  }
  return hipSuccess;
}

}  // namespace mgpu

extern "C" {

int32_t mgpu_cell_agg_create(mgpu_ctx* ctx, int32_t index_system, int32_t res, int32_t with_sum, int64_t initial_cells,
                             mgpu_cell_agg** out) {
  if (int32_t st = mgpu_check_resolution(index_system, res)) return st;
  if (!ctx || !out) return mgpu::set_error(MGPU_E_INVALID_ARG, "cell_agg_create: ctx / out is NULL");
  if (initial_cells < 0 || initial_cells > ((int64_t)1 << 38))
    return mgpu::set_error(MGPU_E_INVALID_ARG, "cell_agg_create: initial_cells %lld out of range", (long long)initial_cells);
  CA_TRY(hipSetDevice(ctx->device));
  int64_t cap = kFloorEntries;
  while (cap < 2 * initial_cells) cap *= 2;
  mgpu_cell_agg* a = new mgpu_cell_agg();
  a->device = ctx->device;
  a->is = index_system, a->res = res, a->with_sum = with_sum != 0;
  a->cap = cap;
  hipError_t e = hipMalloc(&a->mem, table_bytes(a, cap));
  if (e == hipSuccess) e = hipMalloc((void**)&a->meta, kMetaWords * 8);
  if (e == hipSuccess) e = clear_table(a->mem, cap, a->with_sum, nullptr);
  if (e == hipSuccess) e = hipMemsetAsync(a->meta, 0, kMetaWords * 8, nullptr);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess) {
    mgpu_cell_agg_destroy(a);
    return mgpu::set_error(MGPU_E_DEVICE, "cell_agg_create: %s", hipGetErrorString(e));
  }
  *out = a;
  return MGPU_OK;
}

int32_t mgpu_cell_agg_destroy(mgpu_cell_agg* a) {
  if (!a) return MGPU_OK;
  hipSetDevice(a->device);
  if (a->mem) hipFree(a->mem);
  if (a->meta) hipFree(a->meta);
  delete a;
  return MGPU_OK;
}

int32_t mgpu_cell_agg_clear(mgpu_ctx* ctx, mgpu_cell_agg* a, void* stream) {
  if (int32_t st = check_handles(ctx, a, "cell_agg_clear")) return st;
  CA_TRY(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  CA_TRY(clear_table(a->mem, a->cap, a->with_sum, s));
  CA_TRY(hipMemsetAsync(a->meta, 0, kMetaWords * 8, s));
  CA_TRY(hipStreamSynchronize(s));
  a->claimed = 0;
  return MGPU_OK;
}

int32_t mgpu_cell_agg_add_cells(mgpu_ctx* ctx, mgpu_cell_agg* a, const int64_t* cells, const uint8_t* valid,
                                int64_t valid_offset, const int64_t* weight, int64_t n, void* stream) {
  if (int32_t st = check_handles(ctx, a, "cell_agg_add_cells")) return st;
  if (n < 0 || (n > 0 && !cells) || valid_offset < 0) return mgpu::set_error(MGPU_E_INVALID_ARG, "cell_agg_add_cells: bad cell column");
  if (n == 0) return MGPU_OK;
  if (int32_t st = check_weight(a, weight, "cell_agg_add_cells", "weight")) return st;
  CA_TRY(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  void* bins = nullptr;
  if (bin_candidate(ctx, valid, n)) {
    if (int32_t st = ensure_scratch(ctx, bin_bytes(n, a->with_sum))) return st;
    bins = ctx->scratch;
  }
  return agg_add_column(ctx, a, cells, valid, valid_offset, weight, n, bins, s);
}

int32_t mgpu_cell_agg_add_points(mgpu_ctx* ctx, mgpu_cell_agg* a, const double* x, const double* y, const int64_t* weight,
                                 int64_t n, void* stream, mgpu_stats* stats) {
  if (int32_t st = check_handles(ctx, a, "cell_agg_add_points")) return st;
  if (n < 0 || (n > 0 && (!x || !y))) return mgpu::set_error(MGPU_E_INVALID_ARG, "cell_agg_add_points: bad point arrays");
  if (n == 0) {
    if (stats) *stats = mgpu_stats{};
    return MGPU_OK;
  }
  if (int32_t st = check_weight(a, weight, "cell_agg_add_points", "weight")) return st;
  hipStream_t s = (hipStream_t)stream;
  if (int32_t st = mgpu::begin_call(ctx)) return st;
  const bool binned = bin_candidate(ctx, nullptr, n);
  if (int32_t st = ensure_scratch(ctx, bin_column(n) + (binned ? bin_bytes(n, a->with_sum) : 0))) return st;
  int64_t* cells = (int64_t*)ctx->scratch;
  // the cells settle first (fast path, near-tie queue, host libm pass; invalid coordinates
  // fail here): the aggregate is touched only after that
  if (int32_t st = cells_impl(ctx, a->is, a->res, x, y, n, cells, s, nullptr, 0, stats)) return st;
  CA_TRY(hipEventRecord(ctx->ev2, s));
  if (int32_t st = agg_add_column(ctx, a, cells, nullptr, 0, weight, n, binned ? (uint8_t*)cells + bin_column(n) : nullptr, s)) return st;
  CA_TRY(hipEventRecord(ctx->ev3, s));
  CA_TRY(hipEventSynchronize(ctx->ev3));
  if (stats) {
    float ms = 0;
    hipEventElapsedTime(&ms, ctx->ev2, ctx->ev3);
    stats->emit_kernel_ms = ms;
    stats->kernel_ms += ms;
  }
  return MGPU_OK;
}

int32_t mgpu_cell_agg_add_counted(mgpu_ctx* ctx, mgpu_cell_agg* a, const int64_t* cells, const int64_t* count,
                                  const int64_t* sum, int64_t n, void* stream) {
  if (int32_t st = check_handles(ctx, a, "cell_agg_add_counted")) return st;
  if (n < 0 || (n > 0 && (!cells || !count))) return mgpu::set_error(MGPU_E_INVALID_ARG, "cell_agg_add_counted: bad record columns");
  if (n == 0) return MGPU_OK;
  if (int32_t st = check_weight(a, sum, "cell_agg_add_counted", "sum")) return st;
  CA_TRY(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  return agg_run(ctx, a, n, s, [&](bool add) { return launch_agg_counted(table_of(a), a->with_sum, add, cells, count, sum, n, s); });
}

int32_t mgpu_cell_agg_size(mgpu_ctx* ctx, const mgpu_cell_agg* a, int64_t* n_cells, void* stream) {
  if (int32_t st = check_handles(ctx, a, "cell_agg_size")) return st;
  if (!n_cells) return mgpu::set_error(MGPU_E_INVALID_ARG, "cell_agg_size: n_cells is NULL");
  CA_TRY(hipSetDevice(ctx->device));
  return agg_size(ctx, a, (hipStream_t)stream, n_cells);
}

int32_t mgpu_cell_agg_fetch(mgpu_ctx* ctx, const mgpu_cell_agg* a, int64_t capacity, int64_t* out_cell, int64_t* out_count,
                            int64_t* out_sum, int64_t* out_n, void* stream) {
  if (int32_t st = check_handles(ctx, a, "cell_agg_fetch")) return st;
  if (!out_n || capacity < 0) return mgpu::set_error(MGPU_E_INVALID_ARG, "cell_agg_fetch: out_n is NULL or capacity negative");
  CA_TRY(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  int64_t D = 0;
  if (int32_t st = agg_size(ctx, a, s, &D)) return st;
  *out_n = D;
  if (D == 0) return MGPU_OK;
  if (int32_t st = check_weight(a, out_sum, "cell_agg_fetch", "out_sum")) return st;
  if (D > capacity) return mgpu::set_error(MGPU_E_CAPACITY, "cell_agg_fetch: %lld cells, capacity %lld", (long long)D, (long long)capacity);
  if (!out_cell || !out_count) return mgpu::set_error(MGPU_E_INVALID_ARG, "cell_agg_fetch: out_cell / out_count is NULL");
  if (D >= ((int64_t)1 << 31)) return mgpu::set_error(MGPU_E_UNSUPPORTED, "cell_agg_fetch: 2^31 cells or more");
  // scratch: keys and slots, twice (the sort's two sides), then the tile histograms
  const int64_t tiles = (D + kSortTile - 1) / kSortTile;
  const size_t col = ((size_t)D * 8 + 255) & ~(size_t)255;
  if (int32_t st = ensure_scratch(ctx, 4 * col + ((size_t)tiles + 1) * 256 * 4)) return st;
  uint8_t* base = (uint8_t*)ctx->scratch;
  unsigned long long *k0 = (unsigned long long*)base, *v0 = (unsigned long long*)(base + col);
  unsigned long long *k1 = (unsigned long long*)(base + 2 * col), *v1 = (unsigned long long*)(base + 3 * col);
  uint32_t* hist = (uint32_t*)(base + 4 * col);
  uint32_t* tot = hist + tiles * 256;
  const AggTable t = table_of(a);
  CA_TRY(hipMemsetAsync(a->meta + kCursor, 0, 16, s));  // (kCursor, kOr)
  CA_TRY(hipMemsetAsync(a->meta + kAnd, 0xFF, 8, s));
  const int64_t cgrid = std::min<int64_t>((a->cap + 255) / 256, 512);
  hipLaunchKernelGGL((agg_compact_kernel<true>), dim3((unsigned)cgrid), dim3(256), 0, s, t, a->cap, k0, v0);
  CA_TRY(hipGetLastError());
  if (int32_t st = read_meta(ctx, a, s)) return st;
  if ((int64_t)ctx->pin[kCursor] != D) return mgpu::set_error(MGPU_E_INTERNAL, "cell_agg_fetch: the aggregate changed during the call");
  const unsigned long long differ = ctx->pin[kOr] ^ ctx->pin[kAnd];
  const dim3 sgrid((unsigned)((tiles + kSortWaves - 1) / kSortWaves));
  for (int d = 0; d < 8; d++) {
    if (((differ >> (8 * d)) & 0xFFu) == 0) continue;  // this digit is equal in all keys
    hipLaunchKernelGGL(sort_hist_kernel, sgrid, dim3(64 * kSortWaves), 0, s, k0, D, tiles, d, hist);
    hipLaunchKernelGGL(scan_rows_kernel, dim3(256), dim3(256), 0, s, hist, tiles, tot);
    hipLaunchKernelGGL(scan_tot_kernel, dim3(1), dim3(1024), 0, s, tot, 256);
    hipLaunchKernelGGL(sort_scatter_kernel, sgrid, dim3(64 * kSortWaves), 0, s, k0, v0, D, tiles, d, hist, tot, k1, v1);
    CA_TRY(hipGetLastError());
    std::swap(k0, k1);
    std::swap(v0, v1);
  }
  hipLaunchKernelGGL(agg_split_kernel, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, s, t, a->cap, k0, v0, D, out_cell,
                     out_count, out_sum);
  CA_TRY(hipGetLastError());
  CA_TRY(hipStreamSynchronize(s));
  return MGPU_OK;
}

}  // extern "C"

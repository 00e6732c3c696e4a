// mgpu_pip_join_count's aggregation kernels (included at the end of kernels.hip, inside
// namespace mgpu: they share the emit kernels' constants and helpers).  One kernel per
// pipeline, each reading what that pipeline's emit kernel reads -- the split pipeline's
// codes and mixed answers, the fused join's tile records, the binned answers in slot
// order -- and adding every pair to its polygon's slot (count, and the point's weight to
// sum) instead of writing it out.  The additions are integer, so their order does not
// matter: no output offsets, no gather back to input order.
//
// Accumulation (count_add): a resident grid strides over the units (chunks / tiles), so a
// workgroup flushes once.  Up to CountArgs.lds_slots polygons the workgroup keeps the
// histogram in LDS (u32 counts, u64 sums) and flushes each non-zero slot with one 64-bit
// global atomic add.  Above it a 64-bit global atomic per addition is far too slow
// (device-scope atomics run at the memory side, ~19 G/s: C3's 1.25e8 took 6.7 ms), so the
// workgroup keeps an LDS hash table of kCountHash entries {slot, u32 count, u64 sum} in
// front of them: the slots it meets first live there and are flushed once, the rest go to
// global atomics (hash_slots == 0: global atomics only).  Either way the
// wave merges first -- real data is skewed, most lanes of a wave hit one or two slots:
// the first active lane's slot is broadcast, the lanes equal to it are balloted, one
// lane adds the popcount (and the wave's weights of those lanes); at most kCountRounds
// rounds, and none after a leader that was alone (uniform data: merging finds nothing),
// then the lanes left add on their own.  A wave-iteration of 64 points costs 4 cycles per
// instruction, so the rounds are kept few: with four unconditional rounds and a butterfly
// reduction of the weights the C2 aggregation took 0.41 ms (1.06 ms weighted) against
// the emit's 0.25 ms.

constexpr int kCountBlock = 256;
constexpr int kCountRounds = 2;
constexpr int kCountFewLanes = 8;  // weights of at most this many lanes are summed lane by lane
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
constexpr int kCountProbes = 8;
static_assert(kCountHash == 4096, "the hash keeps the product's top 12 bits");

// The workgroup's LDS (dynamic): [sum u64 x S (weighted)] [count u32 x S] [tag u32 x H]
// [lookup u32 x stage_n], S = lds_slots or, with the hash table, H = hash_slots entries
// (kept as word offsets into the one LDS block, not as pointers: every access is then an
// LDS instruction -- pointers chosen between LDS and global memory compiled to flat loads)
struct CountLds {
  uint32_t cnt;   // u32 index of the counts (the sums are the block's first u64s)
  uint32_t tag;   // ... of the hash table's tags: the slot an entry holds (kNoSlot: free)
  uint32_t look;  // ... of the staged copy of the dense table / of the sorted ids (stage_n entries)
};
__device__ __forceinline__ unsigned long long* count_lds_u64() {
  extern __shared__ __attribute__((aligned(16))) unsigned long long s_count_dyn[];
  return s_count_dyn;
}
__device__ __forceinline__ uint32_t* count_lds_u32() { return (uint32_t*)count_lds_u64(); }

template <bool W>
__device__ __forceinline__ CountLds count_lds_init(const CountArgs& c) {
  CountLds L;
  const uint32_t S = c.lds_slots + c.hash_slots;  // (one of them)
  L.cnt = W ? 2u * S : 0u;
  L.tag = L.cnt + S;
  L.look = L.tag + c.hash_slots;
  uint32_t* const s32 = count_lds_u32();
  for (uint32_t i = threadIdx.x; i < S; i += blockDim.x) {
    s32[L.cnt + i] = 0;
    if (W) count_lds_u64()[i] = 0;
    if (c.hash_slots) s32[L.tag + i] = kNoSlot;
  }
  const uint32_t* src = c.dense ? c.dense : (const uint32_t*)c.ids;
  for (uint32_t i = threadIdx.x; i < c.stage_n; i += blockDim.x) s32[L.look + i] = src[i];
  __syncthreads();
  return L;
}

template <bool W>
__device__ __forceinline__ void count_flush(const CountArgs& c, const CountLds& L) {
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < c.lds_slots + c.hash_slots; i += blockDim.x) {
    const uint32_t v = count_lds_u32()[L.cnt + i];
    if (v) {
      uint32_t slot = i;
      if (c.hash_slots) slot = count_lds_u32()[L.tag + i];
      atomicAdd(&c.count[slot], (unsigned long long)v);
      if (W) atomicAdd(&c.sum[slot], count_lds_u64()[i]);
    }
  }
}

// (an atomic load: a plain one is merged with the global alternative into one flat load)
__device__ __forceinline__ uint32_t count_lds_look(const CountLds& L, uint32_t k) {
  return __hip_atomic_load(&count_lds_u32()[L.look + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// polygon id -> slot: contiguous ids (min .. min + P - 1, the common case) by subtraction,
// else the dense table over [min id, max id], else a binary search of the sorted ids (every id looked up is one of them); either from LDS when staged
__device__ __forceinline__ uint32_t count_slot_of(const CountArgs& c, const CountLds& L, int32_t id) {
  if (c.contiguous) return (uint32_t)id - (uint32_t)c.min_id;
  if (c.dense) {
    const uint32_t k = (uint32_t)id - (uint32_t)c.min_id;
    if (c.stage_n) return count_lds_look(L, k);
    return c.dense[k];
  }
  uint32_t lo = 0, hi = c.n_slots;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    int32_t v;
    if (c.stage_n)
      v = (int32_t)count_lds_look(L, mid);
    else
      v = c.ids[mid];
    if (v < id)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo < c.n_slots ? lo : c.n_slots - 1;
}

// a slot's home: the first entry of a bucket of 4 (kCountHash = 2^12 entries, 2^10 buckets)
__device__ __forceinline__ uint32_t count_hash(uint32_t slot) {
  return ((slot * 2654435761u) >> 20) & ~3u;
}

template <bool W>
__device__ __forceinline__ void count_add_one(const CountArgs& c, const CountLds& L, uint32_t slot, uint32_t k,
                                              unsigned long long w) {
  uint32_t* const s32 = count_lds_u32();
  if (c.lds_slots) {
    atomicAdd(&s32[L.cnt + slot], k);
    if (W) atomicAdd(&count_lds_u64()[slot], w);
    return;
  }
  if (c.hash_slots) {
    // open addressing, kCountProbes linear probes from the slot's home bucket; an entry's
    // tag is set once (free -> slot) and never changes, so a read of a set tag is final
    uint32_t i = count_hash(slot);
#pragma unroll 1
    for (int p = 0; p < kCountProbes; p++, i = (i + 1) & (kCountHash - 1)) {
      uint32_t t = __hip_atomic_load(&s32[L.tag + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (t == kNoSlot) {
        t = atomicCAS(&s32[L.tag + i], kNoSlot, slot);
        if (t == kNoSlot) t = slot;
      }
      if (t == slot) {
        atomicAdd(&s32[L.cnt + i], k);
        if (W) atomicAdd(&count_lds_u64()[i], w);
        return;
      }
    }
  }
  atomicAdd(&c.count[slot], (unsigned long long)k);
  if (W) atomicAdd(&c.sum[slot], w);
}

__device__ __forceinline__ unsigned long long count_readlane_u64(unsigned long long v, int lane) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
  return (unsigned long long)lo | ((unsigned long long)hi << 32);
}

// One pair per lane with `has` (slot < n_slots, its point's weight).  Every lane of the
// wave calls this together.
template <bool W>
__device__ __forceinline__ void count_add(const CountArgs& c, const CountLds& L, bool has, uint32_t slot,
                                          unsigned long long w) {
  const int lane = threadIdx.x & 63;
  unsigned long long active = __ballot(has);
#pragma unroll
  for (int r = 0; r < kCountRounds; r++) {
    if (!active) break;
    const int leader = __ffsll((long long)active) - 1;
    const uint32_t ls = (uint32_t)__builtin_amdgcn_readlane((int)slot, leader);
    const bool eq = has && slot == ls;
    const unsigned long long m = __ballot(eq);
    const int np = __popcll(m);
    if (np == 1) break;  // (the leader is alone: it and the rest add on their own below)
    unsigned long long ws = 0;
    if (W) {
      if (np <= kCountFewLanes) {
        for (unsigned long long mm = m; mm; mm &= mm - 1) ws += count_readlane_u64(w, __ffsll((long long)mm) - 1);
      } else {
        ws = wave_sum_u64(eq ? w : 0ull);
      }
    }
    if (lane == leader) count_add_one<W>(c, L, ls, (uint32_t)np, ws);
    active &= ~m;
    has = has && !eq;
  }
  if (has) count_add_one<W>(c, L, slot, 1u, w);
}

// The pairs of one answer per lane (first chip | match mask << 32; mask 0: none): bit j
// is chip first + j, whose slot is chip_slot[].  one_is_poly: a mask of exactly 1 holds
// the polygon id in `first` (JoinArgs.poly_answers).
template <bool W>
__device__ __forceinline__ void count_answer(const CountArgs& c, const CountLds& L, uint64_t v, unsigned long long w,
                                             bool one_is_poly) {
  const uint32_t first = (uint32_t)v;
  uint32_t m = (uint32_t)(v >> 32);
  if (one_is_poly) {  // (uniform: the whole wave takes count_add together)
    const bool one = m == 1u;
    const uint32_t slot = one ? count_slot_of(c, L, (int32_t)first) : 0u;
    count_add<W>(c, L, one, slot, w);
    if (one) m = 0;
  }
  while (__ballot(m != 0u)) {
    const bool has = m != 0u;
    const uint32_t slot = has ? c.chip_slot[first + (uint32_t)__builtin_ctz(m)] : 0u;
    m &= m - 1u;
    count_add<W>(c, L, has, slot, w);
  }
}

// kPer consecutive weights of a thread (16-byte loads when whole and aligned)
template <int kPer>
__device__ __forceinline__ void count_weights(const CountArgs& c, int64_t p0, int64_t n, unsigned long long* w) {
  if (p0 + kPer <= n && (((uintptr_t)c.weight) & 15) == 0) {
    const ulonglong2* src = (const ulonglong2*)(c.weight + p0);  // (p0 is a multiple of kPer: even)
#pragma unroll
    for (int i = 0; i < kPer / 2; i++) {
      const ulonglong2 q = src[i];
      w[2 * i] = q.x, w[2 * i + 1] = q.y;
    }
  } else {
#pragma unroll
    for (int k = 0; k < kPer; k++) w[k] = p0 + k < n ? (unsigned long long)c.weight[p0 + k] : 0ull;
  }
}

// Split pipeline: a chunk's codes (16 bytes per lane and load, every load of the chunk in
// flight at once), then its mixed answers with their points from the chunk's list.  H3
// classes with one match take their slot from an LDS table built once per workgroup;
// the rare classes with more go through raster_cls in a second pass over the load.
template <int IS, bool W>
__global__ __launch_bounds__(kCountBlock) void split_count_kernel(SplitArgs sa, CountArgs c, int64_t n_chunks) {
  using Code = typename CodeOf<IS>::T;
  constexpr int kPer = 16 / (int)sizeof(Code);  // codes per 16-byte load
  constexpr int kLoads = kChunk / (kCountBlock * kPer);
  const JoinArgs& a = sa.j;
  const ChipTableView& t = a.chips;
  __shared__ uint32_t s_cs[IS == MGPU_H3 ? kEmitCls : 1];  // class -> slot (kNoSlot: not one match)
  uint32_t ncs = 0;
  if (IS == MGPU_H3) {
    ncs = min(t.raster_ncls, (uint32_t)kEmitCls);
    for (uint32_t i = threadIdx.x; i < ncs; i += kCountBlock) {
      const uint64_t v = t.raster_cls[i];
      const uint32_t m = (uint32_t)(v >> 32);
      s_cs[i] = (i && __popc(m) == 1) ? c.chip_slot[(uint32_t)v + (uint32_t)__builtin_ctz(m)] : kNoSlot;
    }
  }
  const CountLds L = count_lds_init<W>(c);
  const Code kMixed = IS == MGPU_H3 ? (Code)kPixMixed : (Code)kCodeMixed32;
  for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
    const int64_t c0 = chunk * kChunk;
    uint4 raw[kLoads];
    // (the codes buffer holds whole chunks: the loads stay inside it, p < n masks the tail)
#pragma unroll
    for (int q = 0; q < kLoads; q++)
      raw[q] = *(const uint4*)((const Code*)sa.codes + c0 + ((int64_t)q * kCountBlock + threadIdx.x) * kPer);
#pragma unroll
    for (int q = 0; q < kLoads; q++) {
      const int64_t p0 = c0 + ((int64_t)q * kCountBlock + threadIdx.x) * kPer;
      const uint32_t cw[4] = {raw[q].x, raw[q].y, raw[q].z, raw[q].w};
      unsigned long long w[kPer];
      if (W)
        count_weights<kPer>(c, p0, a.n, w);
      else
#pragma unroll
        for (int k = 0; k < kPer; k++) w[k] = 0;
      Code code[kPer];
      bool pure[kPer];
#pragma unroll
      for (int k = 0; k < kPer; k++) {
        code[k] = sizeof(Code) == 2 ? (Code)(cw[k >> 1] >> ((k & 1) * 16)) : (Code)cw[k];
        pure[k] = p0 + k < a.n && code[k] != 0 && code[k] != kMixed;
      }
      if (IS == MGPU_H3) {
        uint32_t one[kPer];
        bool multi = false;
#pragma unroll
        for (int k = 0; k < kPer; k++) {
          one[k] = (pure[k] && (uint32_t)code[k] < ncs) ? s_cs[(uint32_t)code[k]] : kNoSlot;
          multi |= pure[k] && one[k] == kNoSlot;
        }
#pragma unroll
        for (int k = 0; k < kPer; k++) count_add<W>(c, L, one[k] != kNoSlot, one[k], w[k]);
        if (__ballot(multi)) {
#pragma unroll
          for (int k = 0; k < kPer; k++) {
            const uint64_t v = (pure[k] && one[k] == kNoSlot) ? t.raster_cls[(uint32_t)code[k]] : 0ull;
            count_answer<W>(c, L, v, w[k], false);
          }
        }
      } else {
#pragma unroll
        for (int k = 0; k < kPer; k++) {
          const uint64_t v =
              pure[k] ? (uint64_t)((uint32_t)code[k] >> 8) | ((uint64_t)((uint32_t)code[k] & 0xFFu) << 32) : 0ull;
          count_answer<W>(c, L, v, w[k], false);
        }
      }
    }
    const uint32_t nm = sa.chunk_mixed[chunk];
    for (uint32_t i0 = 0; i0 < nm; i0 += kCountBlock) {
      const uint32_t i = i0 + threadIdx.x;
      const bool in = i < nm;
      const uint64_t v = in ? a.mixed_res[c0 + i] : 0ull;
      unsigned long long w = 0;
      if (W && in && (v >> 32)) w = (unsigned long long)c.weight[c0 + sa.mixed_idx[c0 + i]];
      count_answer<W>(c, L, v, w, false);
    }
  }
  if (c.lds_slots + c.hash_slots) count_flush<W>(c, L);
}

// Fused join: a wave takes 64 consecutive tiles at a time -- their counts and record
// positions in one load per lane -- then walks each tile's records {point in tile << 32 |
// polygon id}, kTileRecs loads in flight.  A tile whose records the overflow pool dropped
// sets *c.dropped.
constexpr int kTileRecs = 4;
template <bool W>
__global__ __launch_bounds__(kCountBlock) void tile_count_kernel(EmitArgs e, CountArgs c, int64_t n_tiles) {
  const CountLds L = count_lds_init<W>(c);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int kWaves = kCountBlock / 64;
  const int64_t n_groups = (n_tiles + 63) / 64;
  for (int64_t g = (int64_t)blockIdx.x * kWaves + wave; g < n_groups; g += (int64_t)gridDim.x * kWaves) {
    const int64_t t0 = g * 64;
    const bool tin = t0 + lane < n_tiles;
    const uint32_t my_cnt = tin ? e.tile_count[t0 + lane] : 0u;
    const uint64_t my_where = tin ? e.tile_where[t0 + lane] : 0ull;
    if (__ballot(my_cnt != 0u && my_where == kNoDst)) {
      if (lane == 0) atomicOr(c.dropped, 1u);
    }
    const int nt = (int)(n_tiles - t0 < 64 ? n_tiles - t0 : 64);
    for (int j = 0; j < nt; j++) {
      const uint32_t cnt = (uint32_t)__builtin_amdgcn_readlane((int)my_cnt, j);
      const uint64_t where = count_readlane_u64(my_where, j);
      if (cnt == 0 || where == kNoDst) continue;
      const int64_t pt0 = (t0 + j) * kTile;
      for (uint32_t i0 = 0; i0 < cnt; i0 += 64 * kTileRecs) {
        uint64_t r[kTileRecs];
#pragma unroll
        for (int u = 0; u < kTileRecs; u++) {
          const uint32_t i = i0 + u * 64 + lane;
          r[u] = i < cnt ? e.recs[where + i] : kNoDst;
        }
        uint32_t slot[kTileRecs];
        unsigned long long w[kTileRecs];
#pragma unroll
        for (int u = 0; u < kTileRecs; u++) {
          const bool in = i0 + u * 64 + lane < cnt;
          slot[u] = in ? count_slot_of(c, L, (int32_t)(uint32_t)r[u]) : 0u;
          w[u] = (W && in) ? (unsigned long long)c.weight[pt0 + (int64_t)(r[u] >> 32)] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < kTileRecs; u++) {
          if (i0 + u * 64 >= cnt) break;
          count_add<W>(c, L, i0 + u * 64 + lane < cnt, slot[u], w[u]);
        }
      }
    }
  }
  if (c.lds_slots + c.hash_slots) count_flush<W>(c, L);
}

// Binned pipeline: the answers in binned slot order, kBinRecs loads in flight per thread;
// perm[slot] only fetches the weight.  A workgroup is 1024 threads at 8 waves per SIMD,
// two per CU: its histogram or hash table is per workgroup (32 to 64 KiB for C3's 74,000
// tracts), so with 256 threads the LDS held a CU to 4 waves per SIMD, and the loads, the
// ~1 instruction per point and the LDS round trips added up instead of overlapping.
constexpr int kBinCountBlock = 1024;
constexpr int kBinRecs = kChunk / kBinCountBlock;
template <bool W>
__global__ __launch_bounds__(kBinCountBlock) __attribute__((amdgpu_waves_per_eu(8, 8)))
void bin_count_kernel(BinArgs b, CountArgs c, int64_t n_chunks) {
  const JoinArgs& a = b.s.j;
  const CountLds L = count_lds_init<W>(c);
  static_assert(kBinRecs * kBinCountBlock == kChunk, "one batch of loads per chunk");
  // a contiguous run of chunks per workgroup: binned slots are sorted by bin, so the run
  // meets few polygons (the hash table holds them)
  const int64_t per = (n_chunks + gridDim.x - 1) / gridDim.x;
  const int64_t c_end = ((int64_t)blockIdx.x + 1) * per < n_chunks ? ((int64_t)blockIdx.x + 1) * per : n_chunks;
  for (int64_t chunk = (int64_t)blockIdx.x * per; chunk < c_end; chunk++) {
    {
      constexpr int q0 = 0;
      uint64_t v[kBinRecs];
      unsigned long long w[kBinRecs];
#pragma unroll
      for (int u = 0; u < kBinRecs; u++) {
        const int64_t s = chunk * kChunk + (int64_t)(q0 + u) * kBinCountBlock + threadIdx.x;
        v[u] = s < a.n ? a.mixed_res[s] : 0ull;
      }
#pragma unroll
      for (int u = 0; u < kBinRecs; u++) {
        const int64_t s = chunk * kChunk + (int64_t)(q0 + u) * kBinCountBlock + threadIdx.x;
        w[u] = (W && (v[u] >> 32)) ? (unsigned long long)c.weight[b.perm[s]] : 0ull;
      }
      if (c.hash_slots && a.poly_answers) {
        // The hash table's common case without a dependent round trip per answer: the
        // home buckets (4 tags, one 16-byte read) of the batch's one-match answers are read
        // together; a bucket entry that holds the slot takes the addition at once.  The
        // answers that miss (a first touch, a full bucket) are only noted, and go through
        // the probes in one loop after the batch: a wave waits for that loop's LDS round
        // trips whenever any of its lanes is in it, so running it per answer (0.74 ms on
        // C3, 0.19 ms of it the loads) serialised eight of them per batch.  (No wave merge
        // here: the LDS atomics serialise equal slots themselves.)  A stale read only
        // sends an answer to the probes, which decide with atomics.
        uint32_t sl[kBinRecs], hh[kBinRecs];
        uint4 tg[kBinRecs];
        uint32_t* const s32 = count_lds_u32();
#pragma unroll
        for (int u = 0; u < kBinRecs; u++) {
          const bool one = (uint32_t)(v[u] >> 32) == 1u;
          sl[u] = one ? count_slot_of(c, L, (int32_t)(uint32_t)v[u]) : kNoSlot;
          hh[u] = one ? count_hash(sl[u]) : 0u;
          tg[u] = *(const uint4*)&s32[L.tag + hh[u]];
        }
        uint32_t pending = 0;
#pragma unroll
        for (int u = 0; u < kBinRecs; u++) {
          if (sl[u] == kNoSlot) continue;
          const int j = tg[u].x == sl[u] ? 0 : tg[u].y == sl[u] ? 1 : tg[u].z == sl[u] ? 2 : tg[u].w == sl[u] ? 3 : -1;
          if (j >= 0) {
            atomicAdd(&s32[L.cnt + hh[u] + j], 1u);
            if (W) atomicAdd(&count_lds_u64()[hh[u] + j], w[u]);
          } else {
            pending |= 1u << u;
          }
          v[u] = 0;
        }
        if (__ballot(pending != 0u)) {
#pragma unroll
          for (int u = 0; u < kBinRecs; u++)
            if (pending >> u & 1u) count_add_one<W>(c, L, sl[u], 1u, w[u]);
        }
#pragma unroll
        for (int u = 0; u < kBinRecs; u++) count_answer<W>(c, L, v[u], w[u], false);
      } else {
#pragma unroll
        for (int u = 0; u < kBinRecs; u++) count_answer<W>(c, L, v[u], w[u], a.poly_answers != 0);
      }
    }
  }
  if (c.lds_slots + c.hash_slots) count_flush<W>(c, L);
}

static size_t count_lds_bytes(const CountArgs& c) {
  return (size_t)c.lds_slots * (c.weight ? 12 : 4) + (size_t)c.hash_slots * (c.weight ? 16 : 8) + (size_t)c.stage_n * 4;
}

// The resident grid: workgroups per CU = what the CU's 160 KiB of LDS hold beside the
// split kernel's 8 KiB class table, at most 32 waves and 8 workgroups per CU (the default
// bound of 4096 slots with sums is 48 KiB: two workgroups of 256 threads per CU; NYC's 263
// slots: eight).  A kernel's opt-in to more than 48 KiB of dynamic LDS is made once.
template <class K, class... A>
static hipError_t launch_count_grid(K kernel, int block, int64_t units, const CountArgs& c, hipStream_t s, A... args) {
  const size_t lds = count_lds_bytes(c);
  static std::mutex mu;
  static std::map<const void*, size_t> opted;  // kernel -> dynamic LDS it was opted in for
  static int cus = 0;
  {
    std::lock_guard<std::mutex> lock(mu);
    if (cus == 0) {
      int dev = 0, n = 0;
      if (hipError_t e = hipGetDevice(&dev)) return e;
      if (hipError_t e = hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev)) return e;
      cus = std::max(n, 1);
    }
    size_t& have = opted[(const void*)kernel];
    if (lds > 48 * 1024 && lds > have) {
      if (hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))
        return e;
      have = lds;
    }
  }
  const int64_t by_lds = (160 * 1024) / (int64_t)(lds + 8192), by_waves = 32 / (block / 64);
  const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(8, std::min(by_lds, by_waves)));
  int64_t grid = std::min<int64_t>(units, per_cu * cus);
  if (c.max_groups) grid = std::min<int64_t>(grid, c.max_groups);  // (option count_groups: the stride loops under test)
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(block), lds, s, args...);
  return hipSuccess;
}

hipError_t launch_split_count(int is, const SplitArgs& a, const CountArgs& c, hipStream_t s) {
  if (a.j.n <= 0) return hipSuccess;
  hipError_t e_ = hipSuccess;
  const int64_t nc = split_chunks(a.j.n);
  if (is == MGPU_H3) {
    if (c.weight)
      e_ = launch_count_grid(split_count_kernel<MGPU_H3, true>, kCountBlock, nc, c, s, a, c, nc);
    else
      e_ = launch_count_grid(split_count_kernel<MGPU_H3, false>, kCountBlock, nc, c, s, a, c, nc);
  } else {
    if (c.weight)
      e_ = launch_count_grid(split_count_kernel<MGPU_BNG, true>, kCountBlock, nc, c, s, a, c, nc);
    else
      e_ = launch_count_grid(split_count_kernel<MGPU_BNG, false>, kCountBlock, nc, c, s, a, c, nc);
  }
  return e_ != hipSuccess ? e_ : hipGetLastError();
}

hipError_t launch_tile_count(const EmitArgs& e, int64_t n_tiles, const CountArgs& c, hipStream_t s) {
  if (n_tiles <= 0) return hipSuccess;
  hipError_t e_ = hipSuccess;
  const int64_t units = (n_tiles + kCountBlock - 1) / kCountBlock;  // 64 tiles per wave and round
  if (c.weight)
    e_ = launch_count_grid(tile_count_kernel<true>, kCountBlock, units, c, s, e, c, n_tiles);
  else
    e_ = launch_count_grid(tile_count_kernel<false>, kCountBlock, units, c, s, e, c, n_tiles);
  return e_ != hipSuccess ? e_ : hipGetLastError();
}

hipError_t launch_bin_count(const BinArgs& b, const CountArgs& c, hipStream_t s) {
  if (b.s.j.n <= 0) return hipSuccess;
  hipError_t e_ = hipSuccess;
  const int64_t nc = split_chunks(b.s.j.n);
  if (c.weight)
    e_ = launch_count_grid(bin_count_kernel<true>, kBinCountBlock, nc, c, s, b, c, nc);
  else
    e_ = launch_count_grid(bin_count_kernel<false>, kBinCountBlock, nc, c, s, b, c, nc);
  return e_ != hipSuccess ? e_ : hipGetLastError();
}

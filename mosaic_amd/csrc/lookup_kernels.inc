// mgpu_pip_join_lookup's kernels (included at the end of kernels.hip, inside namespace
// mgpu, after count_kernels.inc: they share the emit kernels' constants and helpers).  One
// kernel per pipeline, each reading what that pipeline's count kernel reads -- the split
// pipeline's codes and mixed answers, the fused join's tile records, the binned answers in
// slot order -- and writing, per INPUT position, the point's lowest matching polygon id
// (null_id: none) and its match count.  Chips are sorted by (cell, polygon id, row)
// (chip_table.h), so the lowest set bit of a match mask is the lowest polygon id, and a
// tile's records are in (point, polygon) order (join_tile's phase 3: a lane owns
// consecutive points and writes their matches chip by chip at positions from an
// exclusive scan in lane order).
//
// Every element of [0, n) is written by every launch, and nothing else.  No resident
// grid: there is no per-workgroup state to flush, so one unit per workgroup.

constexpr int kLookBlock = 256;

// 16-byte stores of 4 consecutive answers where the array allows them (a caller's array
// may start at any 4-byte boundary)
__device__ __forceinline__ bool look_aligned(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// kPer = 4 consecutive values at out[p0 ..], p0 a multiple of 4; the tail masked by n.
// Plain stores: non-temporal ones took the C2 split kernel from 0.22 to 0.36 ms with the
// match counts (0.14 to 0.15 without), see DESIGN.md section 3.6.
template <int kPer>
__device__ __forceinline__ void look_store(int32_t* out, bool vec, int64_t p0, int64_t n, const int32_t* v) {
  if (vec && p0 + kPer <= n) {
#pragma unroll
    for (int i = 0; i < kPer / 4; i++)
      *(int4*)(out + p0 + 4 * i) = make_int4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
  } else {
#pragma unroll
    for (int k = 0; k < kPer; k++)
      if (p0 + k < n) out[p0 + k] = v[k];
  }
}

// an answer (first chip | match mask << 32) -> lowest polygon id and match count.
// one_is_poly: a mask of exactly 1 holds the polygon id in `first` (JoinArgs.poly_answers)
__device__ __forceinline__ void look_answer(const ChipTableView& t, uint64_t v, bool one_is_poly, int32_t null_id,
                                            int32_t* poly, int32_t* cnt) {
  const uint32_t first = (uint32_t)v, m = (uint32_t)(v >> 32);
  *cnt = __popc(m);
  if (m == 0u)
    *poly = null_id;
  else if (one_is_poly && m == 1u)
    *poly = (int32_t)first;
  else
    *poly = t.chip_poly[first + (uint32_t)__builtin_ctz(m)];
}

// Split pipeline: one workgroup per chunk.  The chunk's codes are loaded 4 per lane and
// load (every load in flight at once, as split_count_kernel); a pure H3 class answers from an
// LDS table class -> (lowest polygon id, match count) built once per workgroup (classes
// beyond the table: raster_cls), a BNG code (first << 8 | mask) from chip_poly, code 0 is
// (null_id, 0).  A mixed point takes its answer from mixed_res by its RANK in the chunk's
// list: the list is in point order (split_emit_kernel reads it the same way), so the rank
// is the number of mixed codes before the point in the chunk -- a block scan of the
// threads' mixed counts -- and mixed_idx is not needed.  Each thread then writes its 4
// consecutive points with one 16-byte store per column: consecutive lanes, consecutive
// addresses.
// Write ordering: none is needed.  The two forms that write a mixed position twice -- a
// placeholder inside the owner's 16-byte store, then the mixed answer scattered to
// c0 + mixed_idx[c0 + i] by another thread, the two ordered by a workgroup barrier; or the
// chunk's 4096 answers staged in LDS (32 KiB for both columns: 5 workgroups per CU instead
// of 8) -- were weighed against this one; the barrier form was built and measured: 0.204 ms
// on C2 against 0.187 ms (its ~200 scattered 4-byte stores per chunk and column are as many
// memory transactions again as the chunk's 512 full lines).  Here every element has one
// writer and one store, and a mixed point without a match (mask 0) is (null_id, 0) like
// any other answer.
template <int IS>
__global__ __launch_bounds__(kLookBlock) void split_lookup_kernel(SplitArgs sa, LookupArgs o) {
  using Code = typename CodeOf<IS>::T;
  // 4 consecutive points per thread and load: one 16-byte store per column, so that a
  // wave's store covers 1 KiB without gaps (the columns are 4 to 8 times the codes' bytes:
  // the H3 codes come by 8-byte loads for it; with 16-byte loads of 8 codes a thread's two
  // stores per column each left every other 16 bytes to the next instruction)
  constexpr int kPer = 4;
  constexpr int kWords = kPer * (int)sizeof(Code) / 4;  // 32-bit words per load: 2 (H3), 4 (BNG)
  constexpr int kLoads = kChunk / (kLookBlock * kPer);
  const JoinArgs& a = sa.j;
  const ChipTableView& t = a.chips;
  __shared__ int32_t s_poly[IS == MGPU_H3 ? kEmitCls : 1];  // class -> lowest polygon id
  __shared__ uint8_t s_cnt[IS == MGPU_H3 ? kEmitCls : 1];   // class -> matches (<= 32)
  __shared__ uint32_t s_w[2][kLookBlock / 64];
  const Code kMixed = IS == MGPU_H3 ? (Code)kPixMixed : (Code)kCodeMixed32;
  const int64_t c0 = (int64_t)blockIdx.x * kChunk;
  const bool vp = look_aligned(o.out_polygon), vm = look_aligned(o.out_matches);
  uint32_t raw[kLoads][kWords];
  // (the codes buffer holds whole chunks: the loads stay inside it, p < n masks the tail;
  // issued before the class table is built, so that they are in flight behind it)
#pragma unroll
  for (int q = 0; q < kLoads; q++) {
    const Code* src = (const Code*)sa.codes + c0 + ((int64_t)q * kLookBlock + threadIdx.x) * kPer;
    if (kWords == 2) {
      const uint2 v = *(const uint2*)src;
      raw[q][0] = v.x, raw[q][1] = v.y;
    } else {
      const uint4 v = *(const uint4*)src;
      raw[q][0] = v.x, raw[q][1] = v.y, raw[q][kWords - 2] = v.z, raw[q][kWords - 1] = v.w;
    }
  }
  const uint32_t nm = sa.chunk_mixed[blockIdx.x];
  auto code_of = [&](int q, int k) -> Code {
    return sizeof(Code) == 2 ? (Code)(raw[q][k >> 1] >> ((k & 1) * 16)) : (Code)raw[q][k];
  };
  auto is_mixed = [&](int q, int k) -> bool {
    return c0 + ((int64_t)q * kLookBlock + threadIdx.x) * kPer + k < a.n && code_of(q, k) == kMixed;
  };
  // the rank of each mixed point in the chunk's list: the mixed points before it in point
  // order, i.e. of the loads before (whole), of the lower threads in its load, and of the
  // thread's own earlier points -- four block scans at once, 16 bits each (<= 1024 a load)
  static_assert(kLoads == 4, "two packed scans of two 16-bit counts");
  uint32_t pk[2] = {0, 0};
#pragma unroll
  for (int q = 0; q < kLoads; q++)
#pragma unroll
    for (int k = 0; k < kPer; k++) pk[q >> 1] += (is_mixed(q, k) ? 1u : 0u) << ((q & 1) * 16);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t incl[2] = {wave_incl_scan(pk[0]), wave_incl_scan(pk[1])};
  if (lane == 63) s_w[0][wave] = incl[0], s_w[1][wave] = incl[1];
  uint32_t ncs = 0;
  if (IS == MGPU_H3) {
    // a one-match class (below raster_pc[0]) has its polygon in raster_cls_poly: one load,
    // no raster_cls -> chip_poly chain; the few classes with more matches take that chain
    ncs = min(t.raster_ncls, (uint32_t)kEmitCls);
    for (uint32_t i = threadIdx.x; i < ncs; i += kLookBlock) {
      int32_t p = t.raster_cls_poly[i], c = 1;
      if (i == 0 || i >= t.raster_pc[0]) look_answer(t, t.raster_cls[i], false, o.null_id, &p, &c);
      s_poly[i] = p;
      s_cnt[i] = (uint8_t)c;
    }
  }
  __syncthreads();  // the class table and the waves' mixed counts
  uint32_t rank[kLoads];
  {
    uint32_t before[2] = {incl[0] - pk[0], incl[1] - pk[1]}, all[2] = {0, 0};
#pragma unroll
    for (int w = 0; w < kLookBlock / 64; w++)
#pragma unroll
      for (int h = 0; h < 2; h++) {
        before[h] += w < wave ? s_w[h][w] : 0u;
        all[h] += s_w[h][w];
      }
    uint32_t whole = 0;  // the loads before
#pragma unroll
    for (int q = 0; q < kLoads; q++) {
      rank[q] = whole + ((before[q >> 1] >> ((q & 1) * 16)) & 0xFFFFu);
      whole += (all[q >> 1] >> ((q & 1) * 16)) & 0xFFFFu;
    }
  }
  // the mixed points' answers, every load of the thread in flight together
  uint64_t mv[kLoads][kPer];
#pragma unroll
  for (int q = 0; q < kLoads; q++)
#pragma unroll
    for (int k = 0; k < kPer; k++) {
      mv[q][k] = 0;
      if (is_mixed(q, k)) {
        const uint32_t r = rank[q]++;
        if (r < nm) mv[q][k] = a.mixed_res[c0 + r];
      }
    }
#pragma unroll
  for (int q = 0; q < kLoads; q++) {
    const int64_t p0 = c0 + ((int64_t)q * kLookBlock + threadIdx.x) * kPer;
    int32_t poly[kPer], cnt[kPer];
#pragma unroll
    for (int k = 0; k < kPer; k++) {
      const Code code = code_of(q, k);
      poly[k] = o.null_id, cnt[k] = 0;
      if (p0 + k >= a.n || code == 0) continue;
      if (code == kMixed) {
        look_answer(t, mv[q][k], false, o.null_id, &poly[k], &cnt[k]);
      } else if (IS == MGPU_H3) {
        if ((uint32_t)code < ncs)
          poly[k] = s_poly[(uint32_t)code], cnt[k] = s_cnt[(uint32_t)code];
        else
          look_answer(t, t.raster_cls[(uint32_t)code], false, o.null_id, &poly[k], &cnt[k]);
      } else {
        const uint64_t v = (uint64_t)((uint32_t)code >> 8) | ((uint64_t)((uint32_t)code & 0xFFu) << 32);
        look_answer(t, v, false, o.null_id, &poly[k], &cnt[k]);
      }
    }
    look_store<kPer>(o.out_polygon, vp, p0, a.n, poly);
    if (o.out_matches) look_store<kPer>(o.out_matches, vm, p0, a.n, cnt);
  }
}

// Fused join: one wave per tile of kTile points, kLookBlock / 64 tiles per workgroup.
// The wave fills its tile's (null_id, 0) in LDS, walks the tile's records {point in tile
// << 32 | polygon id}, 64 at a time, and places them there: the records are in (point,
// polygon) order, so a record is its point's first -- the lowest id -- exactly when its
// predecessor names another point (the predecessor of a lane's record is the lane
// below's, of lane 0's the last record of the batch before: a run may cross both), and
// the match count is the run's length, counted by an LDS add per record.  A tile's
// records are contiguous, in its slot or in the overflow pool (tile_where).
// Write ordering: fill, placement and read-out are separated by workgroup barriers
// (outside the record loop, whose trip count differs per wave), and global memory is
// written once, from LDS, 16 bytes per lane.  A tile whose records the pool dropped sets
// *o.dropped (its points are written as unmatched; the entry fails).
constexpr int kLookTiles = kLookBlock / 64;
static_assert(kTile % 256 == 0, "a wave writes its tile 4 points per lane");
__global__ __launch_bounds__(kLookBlock) void tile_lookup_kernel(EmitArgs e, LookupArgs o, int64_t n, int64_t n_tiles) {
  __shared__ __attribute__((aligned(16))) int32_t s_poly[kLookTiles][kTile];
  __shared__ __attribute__((aligned(16))) int32_t s_cnt[kLookTiles][kTile];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t tile = (int64_t)blockIdx.x * kLookTiles + wave;
  for (int j = lane; j < kTile; j += 64) s_poly[wave][j] = o.null_id, s_cnt[wave][j] = 0;
  __syncthreads();
  if (tile < n_tiles) {
    const uint32_t cnt = e.tile_count[tile];
    const uint64_t where = e.tile_where[tile];
    if (cnt != 0 && where == kNoDst) {
      if (lane == 0) atomicOr(o.dropped, 1u);
    } else {
      uint32_t carry = 0xFFFFFFFFu;  // the point of the record before this batch
      for (uint32_t i0 = 0; i0 < cnt; i0 += 64) {
        const uint32_t i = i0 + lane;
        const uint64_t r = i < cnt ? e.recs[where + i] : kNoDst;
        const uint32_t pt = (uint32_t)(r >> 32);
        uint32_t prev = (uint32_t)__shfl_up((int)pt, 1, 64);
        if (lane == 0) prev = carry;
        carry = (uint32_t)__shfl((int)pt, 63, 64);
        if (i < cnt && pt < (uint32_t)kTile) {
          if (pt != prev) s_poly[wave][pt] = (int32_t)(uint32_t)r;
          atomicAdd(&s_cnt[wave][pt], 1);
        }
      }
    }
  }
  __syncthreads();
  if (tile >= n_tiles) return;
  const int64_t pt0 = tile * kTile;
  const bool vp = look_aligned(o.out_polygon), vm = look_aligned(o.out_matches);
  for (int j = lane * 4; j < kTile; j += 256) {
    look_store<4>(o.out_polygon, vp, pt0 + j, n, &s_poly[wave][j]);
    if (o.out_matches) look_store<4>(o.out_matches, vm, pt0 + j, n, &s_cnt[wave][j]);
  }
}

// Binned pipeline.  The answers are in binned slot order and perm[slot] is the input
// position; every slot holds exactly one input point, so every output element is written
// once, with no fill and no hazard.  One workgroup per INPUT chunk, as
// bin_emit_gather_kernel's front half: the chunk's bin runs of answers are read whole
// (consecutive lanes, consecutive slots) and placed by perm[] into LDS in input order
// (bin_runs, bin_gather_lds: they read the binning's counts and offsets beside the answers
// and perm[]), then written out 16 bytes per lane.  The plain scatter -- a workgroup per
// 2048 consecutive slots, out[perm[slot]] = answer, 4-byte stores -- measured 8.0 ms on C3
// (3.2 ms without the match counts) against this kernel's 0.46 ms: a wave's 64 stores fall
// on 64 different lines of an input chunk, and the lines' other words arrive from other
// workgroups at other times (DESIGN.md section 3.6).
__global__ __launch_bounds__(kBinBlock) void bin_lookup_kernel(BinArgs b, LookupArgs o) {
  __shared__ uint64_t s_v[kBinChunk];
  __shared__ uint32_t s_off[kBinMax];
  __shared__ uint32_t s_loc[kBinMax];
  __shared__ uint32_t s_w[kBinBlock / 64];
  const JoinArgs& a = b.s.j;
  const int nb = b.nbx * b.nby;
  const int64_t k = blockIdx.x, c0 = k * kBinChunk;
  bin_runs(b, k, s_off, s_loc, s_w);
  const int64_t left = a.n - c0;
  const uint32_t m = left < kBinChunk ? (uint32_t)left : (uint32_t)kBinChunk;
  bin_gather_lds(b, c0, m, nb, s_off, s_loc, s_v);
  __syncthreads();
  static_assert(kBgItems % 4 == 0, "16-byte stores of 4 consecutive points");
  // 4 consecutive points per thread and pass: a wave's store covers 1 KiB without gaps
  const bool vp = look_aligned(o.out_polygon), vm = look_aligned(o.out_matches);
#pragma unroll
  for (int g = 0; g < kBgItems / 4; g++) {
    const int l0 = (g * kBinBlock + (int)threadIdx.x) * 4;
    int32_t poly[4], cnt[4];
#pragma unroll
    for (int q = 0; q < 4; q++)
      look_answer(a.chips, (uint32_t)(l0 + q) < m ? s_v[l0 + q] : 0ull, a.poly_answers != 0, o.null_id, &poly[q], &cnt[q]);
    look_store<4>(o.out_polygon, vp, c0 + l0, a.n, poly);
    if (o.out_matches) look_store<4>(o.out_matches, vm, c0 + l0, a.n, cnt);
  }
}

hipError_t launch_split_lookup(int is, const SplitArgs& a, const LookupArgs& o, hipStream_t s) {
  if (a.j.n <= 0) return hipSuccess;
  const unsigned nc = (unsigned)split_chunks(a.j.n);
  if (is == MGPU_H3)
    hipLaunchKernelGGL(split_lookup_kernel<MGPU_H3>, dim3(nc), dim3(kLookBlock), 0, s, a, o);
  else
    hipLaunchKernelGGL(split_lookup_kernel<MGPU_BNG>, dim3(nc), dim3(kLookBlock), 0, s, a, o);
  return hipGetLastError();
}

hipError_t launch_tile_lookup(const EmitArgs& e, int64_t n, int64_t n_tiles, const LookupArgs& o, hipStream_t s) {
  if (n <= 0 || n_tiles <= 0) return hipSuccess;
  const unsigned grid = (unsigned)((n_tiles + kLookTiles - 1) / kLookTiles);
  hipLaunchKernelGGL(tile_lookup_kernel, dim3(grid), dim3(kLookBlock), 0, s, e, o, n, n_tiles);
  return hipGetLastError();
}

hipError_t launch_bin_lookup(const BinArgs& b, const LookupArgs& o, hipStream_t s) {
  const int64_t n = b.s.j.n;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(bin_lookup_kernel, dim3((unsigned)bin_chunks(n)), dim3(kBinBlock), 0, s, b, o);
  return hipGetLastError();
}

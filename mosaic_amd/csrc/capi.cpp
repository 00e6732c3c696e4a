// C-ABI of the MI355X point-in-polygon join (include/mosaic_gpu.h).
//
// Host-side responsibilities: argument validation with the reference's error
// classes, contexts and options, workspace management, kernel launches and the
// join's settle / override logic.  The chip table is built by chip_build.cpp
// (host only); this file stages its blob to the device.  No computation on the
// data path happens here; every per-point operation runs in kernels.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <string>
#include <memory>
#include <functional>
#include <mutex>
#include <vector>

#include "../../include/mosaic_arrow.h"
#include "../../include/mosaic_gpu.h"
#include "error.h"
#include "h3_core.h"
#include "kernels.h"
#include "parallel.h"
#include "poly_slots.h"
#include "capi_internal.h"
#include "chip_build.h"
#include "geom_decode.h"
#include "h3_glibc.h"

namespace {

thread_local std::string g_err;

int32_t fail(int32_t code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) return fail(MGPU_E_DEVICE, "%s: %s", #expr, hipGetErrorString(_e)); \
  } while (0)

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

constexpr double kPi = 3.14159265358979323846;

}  // namespace

namespace mgpu {
int32_t set_error(int32_t code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
}  // namespace mgpu

namespace {

// Workspace layout (each region 256-byte aligned):
//   [counters 16 x u64] [fast-path tie queue u64 x (1 + kTieCap)] [tile_count u32 x T]
//   [tile_where u64 x T] [group_off u64 x T/32 (T)] [group_sum u32 x T/32] [dirty tiles u32 x T]
//   [records u64 x (T * slot records + pool)]
// counters: [0] pairs [1] route near-ties [2] invalid points [3] candidates (tile_scan_kernel)
//           [4] kWsCountDropped (mgpu_pip_join_count's aggregation: a fused tile's records were
//           dropped by the pool; no join kernel writes it) [5] pool records used
//           [6] dirty tiles (u32) [7] split: extra mixed tiles (u32) [8..] MGPU_STATS
// T = tiles of the largest point batch reserved; pool = overflow records (tiles with
// more pairs than points), at most the output capacity.
constexpr size_t kWsCounters = 128;  // 16 x u64
constexpr int kWsCountDropped = 4;   // (reserved: zeroed with the counters at every join)

struct WsLayout {
  size_t count, where, off, gsum, dirty, ties, recs, total;
};
// mgpu_points_to_cells' queue of the points its fast projection hands to the H3 route
// (overflow: the route pass redoes every point)
constexpr int64_t kTieCap = 1 << 16;

WsLayout ws_layout(int64_t n_tiles, int64_t pool) {
  WsLayout L;
  size_t T = (size_t)std::max<int64_t>(n_tiles, 1);
  L.ties = align_up(kWsCounters, 256);
  L.count = align_up(L.ties + (size_t)(kTieCap + 1) * 8, 256);
  L.where = align_up(L.count + T * 4, 256);
  L.off = align_up(L.where + T * 8, 256);
  L.gsum = align_up(L.off + T * 8, 256);
  L.dirty = align_up(L.gsum + 2 * (T / 32 + 1) * 4, 256);  // group pair sums, group candidate sums
  L.recs = align_up(L.dirty + T * 4 * 4, 256);  // (the split pipeline's mixed tiles: 64 points)
  L.total = align_up(L.recs + (T * (size_t)mgpu::join_slot_records() + (size_t)std::max<int64_t>(pool, 0)) * 8, 256);
  return L;
}

int32_t ensure_ws(mgpu_ctx* ctx, int64_t n_tiles, int64_t pool = 0) {
  ctx->last.valid = false;  // every call that uses the workspace ends the last join's lifetime
  ctx->last.async_pending = false;
  size_t need = ws_layout(n_tiles, pool).total;
  if (need <= ctx->ws_bytes) return MGPU_OK;
  if (ctx->ws) HIP_TRY(hipFree(ctx->ws));
  ctx->ws = nullptr;
  ctx->ws_bytes = 0;
  HIP_TRY(hipMalloc(&ctx->ws, need));
  ctx->ws_bytes = need;
  return MGPU_OK;
}

// The H3 route's near-tie queue (kernels.h JoinArgs.tie_queue): 2 header words, then
// 4 words per record.  The head the synchronous calls copy back with the counters.
constexpr int64_t kTqInit = 1 << 12;
constexpr int64_t kTqHead = 64;
constexpr size_t kPinWords = 16 + 2 + 4 * kTqHead;

int32_t ensure_tq(mgpu_ctx* ctx, int64_t cap) {
  if (cap <= ctx->tq_cap) return MGPU_OK;
  if (ctx->tq) HIP_TRY(hipFree(ctx->tq));
  ctx->tq = nullptr;
  ctx->tq_cap = 0;
  HIP_TRY(hipMalloc(&ctx->tq, (size_t)(2 + 4 * cap) * 8));
  ctx->tq_cap = cap;
  return MGPU_OK;
}

int32_t ensure_ovr(mgpu_ctx* ctx, int64_t words) {
  if (words <= ctx->ovr_cap) return MGPU_OK;
  if (ctx->ovr) HIP_TRY(hipFree(ctx->ovr));
  ctx->ovr = nullptr;
  ctx->ovr_cap = 0;
  HIP_TRY(hipMalloc(&ctx->ovr, (size_t)words * 8));
  ctx->ovr_cap = words;
  return MGPU_OK;
}

// The synchronous calls' host wait (option spin_us): poll the stream, yielding the core
// between polls, for at most spin_us, then block.  The poll saves the blocking wake-up
// (1.3-1.9% of C2's 1.5 ms step, profiles/r2_spin_ab.txt); the bound keeps a long join
// (or a stuck one) from holding a host core.
hipError_t stream_wait(const mgpu_ctx* ctx, hipStream_t s) {
  const int64_t us = ctx->opt.spin_us;
  if (us > 0) {
    const auto t0 = std::chrono::steady_clock::now();
    const auto lim = std::chrono::microseconds(us);
    for (;;) {
      const hipError_t q = hipStreamQuery(s);
      if (q != hipErrorNotReady) return q;
      if (std::chrono::steady_clock::now() - t0 > lim) break;
      sched_yield();
    }
  }
  return hipStreamSynchronize(s);
}

// A near-tie record of the queue (kernels.h JoinArgs.tie_queue)
struct TieRec {
  int64_t pos;
  double x, y;
  uint64_t key;
};

// Records of the queue: the head from the pinned copy, the rest read back.
int32_t read_ties(mgpu_ctx* ctx, int64_t n, std::vector<TieRec>& out) {
  out.resize((size_t)n);
  const uint64_t* head = ctx->pin + 16;
  const int64_t nh = std::min(n, kTqHead);
  if (nh) memcpy(out.data(), head + 2, (size_t)nh * 32);
  if (n > nh) HIP_TRY(hipMemcpy(out.data() + nh, ctx->tq + 2 + 4 * nh, (size_t)(n - nh) * 32, hipMemcpyDeviceToHost));
  return MGPU_OK;
}

// The reference's lattice key of every queued point (h3_glibc.cpp), by record; and the
// (position, key) list sorted by position for the override table.
std::vector<std::pair<int64_t, uint64_t>> libm_reference_keys(std::vector<TieRec>& ties, int res) {
  std::sort(ties.begin(), ties.end(), [](const TieRec& a, const TieRec& b) { return a.pos < b.pos; });
  std::vector<std::pair<int64_t, uint64_t>> out(ties.size());
  mgpu::parallel_for((int64_t)ties.size(), 256, [&](int64_t b, int64_t e, int) {
    for (int64_t k = b; k < e; k++) out[k] = {ties[k].pos, mgpu::h3glibc::lattice_key(ties[k].x, ties[k].y, res)};
  });
  return out;
}

// The reference's libm for the near-ties (h3_glibc.cpp); cells = true: keys are cell
// ids, else lattice keys.  Returns the records whose answer differs as (pos, key),
// sorted by position.
std::vector<std::pair<int64_t, uint64_t>> libm_second_opinion(const std::vector<TieRec>& ties, int res, bool cells) {
  std::vector<uint64_t> ref(ties.size());
  mgpu::parallel_for((int64_t)ties.size(), 256, [&](int64_t b, int64_t e, int) {
    for (int64_t k = b; k < e; k++)
      ref[k] = cells ? mgpu::h3glibc::point_to_cell(ties[k].x, ties[k].y, res)
                     : mgpu::h3glibc::lattice_key(ties[k].x, ties[k].y, res);
  });
  std::vector<std::pair<int64_t, uint64_t>> diff;
  for (size_t k = 0; k < ties.size(); k++)
    if (ref[k] != ties[k].key) diff.push_back({ties[k].pos, ref[k]});
  std::sort(diff.begin(), diff.end());
  return diff;
}

int32_t check_res(int32_t is, int32_t res) {
  if (is == MGPU_H3) {
    if (res < 0 || res > 15) return fail(MGPU_E_RESOLUTION, "H3 resolution has to be between 0 and 15; found %d", res);
    return MGPU_OK;
  }
  if (is == MGPU_BNG) {
    if (res == 0 || res < -6 || res > 6) return fail(MGPU_E_RESOLUTION, "BNG resolution not supported; found %d", res);
    return MGPU_OK;
  }
  return fail(MGPU_E_INVALID_ARG, "unknown index system %d (0 = H3, 1 = BNG)", is);
}

int32_t set_device(int dev) {
  HIP_TRY(hipSetDevice(dev));
  return MGPU_OK;
}

}  // namespace

namespace mgpu {
int32_t begin_call(mgpu_ctx* ctx) {
  if (int32_t st = set_device(ctx->device)) return st;
  return ensure_ws(ctx, 1);
}
}  // namespace mgpu

extern "C" {

const char* mgpu_last_error(void) { return g_err.c_str(); }
const char* mgpu_version(void) { return "mosaic-mi355x 0.1.0 (gfx950)"; }
int32_t mgpu_join_tile_points(void) { return (int32_t)mgpu::join_tile_points(); }

int32_t mgpu_check_resolution(int32_t index_system, int32_t res) { return check_res(index_system, res); }

int32_t mgpu_ctx_create(int32_t device_id, mgpu_ctx** out) {
  if (!out) return fail(MGPU_E_INVALID_ARG, "out is NULL");
  int n = 0;
  HIP_TRY(hipGetDeviceCount(&n));
  if (device_id < 0 || device_id >= n) return fail(MGPU_E_INVALID_ARG, "device %d not present (%d GPUs)", device_id, n);
  HIP_TRY(hipSetDevice(device_id));
  mgpu_ctx* c = new mgpu_ctx();
  c->device = device_id;
  int32_t st = MGPU_OK;
  if (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
      hipEventCreate(&c->ev2) != hipSuccess || hipEventCreate(&c->ev3) != hipSuccess ||
      hipHostMalloc((void**)&c->pin, kPinWords * 8, hipHostMallocDefault) != hipSuccess)
    st = fail(MGPU_E_DEVICE, "mgpu_ctx_create: events / pinned page");
  if (!st && hipHostGetDevicePointer((void**)&c->pin_dev, c->pin, 0) != hipSuccess)
    st = fail(MGPU_E_DEVICE, "mgpu_ctx_create: the pinned page is not device-visible");
  if (!st) st = ensure_ws(c, 1);
  if (!st) st = ensure_tq(c, kTqInit);
  if (st) {
    mgpu_ctx_destroy(c);
    return st;
  }
  *out = c;
  return MGPU_OK;
}

int32_t mgpu_ctx_destroy(mgpu_ctx* ctx) {
  if (!ctx) return MGPU_OK;
  mgpu_comm_destroy(ctx);
  hipSetDevice(ctx->device);
  if (ctx->split_ws) hipFree(ctx->split_ws);
  if (ctx->bin_ws) hipFree(ctx->bin_ws);
  if (ctx->scratch) hipFree(ctx->scratch);
  if (ctx->redo) hipFree(ctx->redo);
  if (ctx->tq) hipFree(ctx->tq);
  if (ctx->ovr) hipFree(ctx->ovr);
  if (ctx->ws) hipFree(ctx->ws);
  if (ctx->pin) hipHostFree(ctx->pin);
  if (ctx->ev0) hipEventDestroy(ctx->ev0);
  if (ctx->ev1) hipEventDestroy(ctx->ev1);
  if (ctx->ev2) hipEventDestroy(ctx->ev2);
  if (ctx->ev3) hipEventDestroy(ctx->ev3);
  delete ctx;
  return MGPU_OK;
}

int32_t mgpu_ctx_set_option(mgpu_ctx* ctx, const char* key, int64_t v) {
  if (!ctx || !key) return fail(MGPU_E_INVALID_ARG, "ctx/key is NULL");
  mgpu_options& o = ctx->opt;
  const std::string k = key;
  auto bad = [&]() { return fail(MGPU_E_INVALID_ARG, "option %s: value %lld out of range", key, (long long)v); };
  if (k == "h3_libm") {
    if (v != MGPU_LIBM_REFERENCE && v != MGPU_LIBM_CORRECTLY_ROUNDED) return bad();
    o.h3_libm = v;
  } else if (k == "pipeline") {
    if (v < MGPU_PIPELINE_AUTO || v > MGPU_PIPELINE_BINNED) return bad();
    o.pipeline = v;
  } else if (k == "bin_count") {
    if (v < 1 || v > mgpu::bin_max()) return bad();
    o.bin_count = v;
  } else if (k == "bin_min_mb") {
    if (v < 0) return bad();
    o.bin_min_mb = v;
  } else if (k == "bin_min_points") {
    if (v < 0) return bad();
    o.bin_min_points = v;
  } else if (k == "bin_xcd") {
    if (v != 0 && v != 1) return bad();
    o.bin_xcd = v;
  } else if (k == "bin_keys") {
    if (v != 0 && v != 1) return bad();
    o.bin_keys = v;
  } else if (k == "ring_batch") {
    if (v < 1) return bad();
    o.ring_batch = v;
  } else if (k == "bng_split") {
    if (v != 0 && v != 1) return bad();
    o.bng_split = v;
  } else if (k == "cfy_fine") {
    if (v != 0 && v != 1) return bad();
    o.cfy_fine = v;
  } else if (k == "count_lds_slots") {
    if (v < 0 || v > mgpu::kCountLdsSlotsMax) return bad();
    o.count_lds_slots = v;
  } else if (k == "count_groups") {
    if (v < 0 || v > mgpu::kCountGroupsMax) return bad();
    o.count_groups = v;
  } else if (k == "cellagg_groups") {
    if (v < 0 || v > mgpu::kCountGroupsMax) return bad();
    o.cellagg_groups = v;
  } else if (k == "cellagg_bin_min") {
    if (v < 0) return bad();
    o.cellagg_bin_min = v;
  } else if (k == "cellagg_lds") {
    if (v != 0 && v != 1) return bad();
    o.cellagg_lds = v;
  } else if (k == "kring_batch") {
    if (v < 0 || v > 2147483647LL) return bad();
    o.kring_batch = v;
  } else if (k == "polyfill_slab") {
    if (v < 256 || v > ((int64_t)1 << 28)) return bad();
    o.polyfill_slab = v;
  } else if (k == "geomring_slab") {
    if (v < 1 || v > ((int64_t)1 << 24)) return bad();
    o.geomring_slab = v;
  } else if (k == "geomring_lds_slots") {
    if (v != 0 && v < 64) return bad();  // (geom_ring.h kLdsSlotsMin; above kLdsSlots: capped)
    o.geomring_lds_slots = v;
  } else if (k == "spin_us") {
    if (v < 0 || v > 10000000) return bad();
    o.spin_us = v;
  } else if (k == "raster" || k == "raster_bng") {
    if (v != 0 && v != 1) return bad();
    (k == "raster" ? o.raster : o.raster_bng) = v;
  } else if (k == "raster_sub") {
    if (!(v == 0 || (v >= 2 && v <= 16))) return bad();
    o.raster_sub = v;
  } else if (k == "raster_milli") {
    if (v < 10 || v > 1000) return bad();
    o.raster_milli = v;
  } else {
    return fail(MGPU_E_INVALID_ARG, "unknown option %s", key);
  }
  return MGPU_OK;
}

int32_t mgpu_ctx_get_option(const mgpu_ctx* ctx, const char* key, int64_t* v) {
  if (!ctx || !key || !v) return fail(MGPU_E_INVALID_ARG, "NULL argument");
  const mgpu_options& o = ctx->opt;
  const std::pair<const char*, int64_t> all[] = {
      {"h3_libm", o.h3_libm},       {"pipeline", o.pipeline}, {"bin_count", o.bin_count},
      {"bin_min_mb", o.bin_min_mb}, {"bin_min_points", o.bin_min_points}, {"bin_xcd", o.bin_xcd},
      {"bin_keys", o.bin_keys},     {"spin_us", o.spin_us},   {"ring_batch", o.ring_batch},       {"raster", o.raster},     {"raster_bng", o.raster_bng},
      {"bng_split", o.bng_split},   {"cfy_fine", o.cfy_fine}, {"count_lds_slots", o.count_lds_slots}, {"count_groups", o.count_groups},
      {"kring_batch", o.kring_batch}, {"cellagg_groups", o.cellagg_groups}, {"cellagg_lds", o.cellagg_lds}, {"cellagg_bin_min", o.cellagg_bin_min},
      {"raster_sub", o.raster_sub}, {"raster_milli", o.raster_milli}, {"polyfill_slab", o.polyfill_slab},
      {"geomring_slab", o.geomring_slab}, {"geomring_lds_slots", o.geomring_lds_slots}};
  for (const auto& kv : all)
    if (strcmp(kv.first, key) == 0) {
      *v = kv.second;
      return MGPU_OK;
    }
  return fail(MGPU_E_INVALID_ARG, "unknown option %s", key);
}

int32_t mgpu_ctx_reserve(mgpu_ctx* ctx, int64_t max_points) {
  if (!ctx) return fail(MGPU_E_INVALID_ARG, "ctx is NULL");
  if (int32_t st = set_device(ctx->device)) return st;
  const int64_t tiles = mgpu::join_tiles(max_points);
  return ensure_ws(ctx, tiles, max_points);
}

}  // extern "C"

// IndexSystem.pointToIndex over a batch: the kernels (fast path + the H3 route for the
// points it cannot decide), then -- H3 with the reference's libm -- the route's near-ties
// recomputed on the host (h3_glibc.cpp) and the cells that moves written back.  A
// near-tie queue that overflowed is grown and the call redone.
int32_t cells_impl(mgpu_ctx* ctx, int32_t is, int32_t res, const double* x, const double* y, int64_t n,
                          int64_t* out_cell, hipStream_t s, const uint8_t* valid, int64_t voff, mgpu_stats* stats) {
  auto* counters = (unsigned long long*)ctx->ws;
  auto* ties = (unsigned long long*)((uint8_t*)ctx->ws + ws_layout(1, 0).ties);
  int64_t n_ties = 0, n_fixed = 0;
  for (int attempt = 0;; attempt++) {
    HIP_TRY(hipMemsetAsync(counters, 0, kWsCounters, s));
    HIP_TRY(hipMemsetAsync(ties, 0, 8, s));
    HIP_TRY(hipMemsetAsync(ctx->tq, 0, 16, s));
    HIP_TRY(hipEventRecord(ctx->ev0, s));
    HIP_TRY(mgpu::launch_cells(is, res, x, y, n, out_cell, counters, ties, kTieCap, ctx->tq, ctx->tq_cap, s, valid, voff));
    HIP_TRY(hipEventRecord(ctx->ev1, s));
    // invalid coordinates must reach the caller as IllegalArgument / IllegalState, so the
    // status is read back (the cell column itself stays on the device)
    HIP_TRY(hipMemcpyAsync(ctx->pin, counters, 16 * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(ctx->pin + 16, ctx->tq, (2 + 4 * kTqHead) * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(stream_wait(ctx, s));
    if (ctx->pin[2]) {
      if (is == MGPU_BNG) return fail(MGPU_E_NAN, "NaN coordinates are not supported. (%llu points)", (unsigned long long)ctx->pin[2]);
      return fail(MGPU_E_INVALID_ARG, "Latitude or longitude were invalid. (%llu points)", (unsigned long long)ctx->pin[2]);
    }
    n_ties = (int64_t)ctx->pin[16];
    if (n_ties > ctx->tq_cap) {
      if (attempt >= 2) return fail(MGPU_E_INTERNAL, "near-tie queue overflowed twice");
      if (int32_t st = ensure_tq(ctx, n_ties + n_ties / 4 + 1024)) return st;
      continue;
    }
    break;
  }
  if (stats) {
    memset(stats, 0, sizeof *stats);
    stats->n_points = n;
    stats->n_near_ties = n_ties;
    float ms = 0;
    hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    stats->kernel_ms = stats->stream_kernel_ms = ms;
  }
  if (is == MGPU_H3 && n_ties > 0 && ctx->opt.h3_libm == MGPU_LIBM_REFERENCE) {
    std::vector<TieRec> tr;
    if (int32_t st = read_ties(ctx, n_ties, tr)) return st;
    const auto diff = libm_second_opinion(tr, res, true);
    n_fixed = (int64_t)diff.size();
    if (n_fixed) {
      std::vector<int64_t> hv(2 * diff.size());
      for (size_t k = 0; k < diff.size(); k++) hv[k] = diff[k].first, hv[diff.size() + k] = (int64_t)diff[k].second;
      if (int32_t st = ensure_ovr(ctx, (int64_t)hv.size())) return st;
      HIP_TRY(hipMemcpyAsync(ctx->ovr, hv.data(), hv.size() * 8, hipMemcpyHostToDevice, s));
      HIP_TRY(mgpu::launch_scatter_i64((const int64_t*)ctx->ovr, (const int64_t*)ctx->ovr + n_fixed, n_fixed, out_cell, s));
      HIP_TRY(stream_wait(ctx, s));
    }
  }
  if (stats) stats->libm_overrides = (int32_t)n_fixed;
  return MGPU_OK;
}

extern "C" {

int32_t mgpu_points_to_cells(mgpu_ctx* ctx, int32_t is, int32_t res, const double* x, const double* y, int64_t n,
                             int64_t* out_cell, void* stream, mgpu_stats* stats) {
  if (!ctx) return fail(MGPU_E_INVALID_ARG, "ctx is NULL");
  if (int32_t r = check_res(is, res)) return r;
  if (n < 0 || (n > 0 && (!x || !y || !out_cell))) return fail(MGPU_E_INVALID_ARG, "bad point arrays");
  if (int32_t st = set_device(ctx->device)) return st;
  if (int32_t st = ensure_ws(ctx, 1)) return st;
  return cells_impl(ctx, is, res, x, y, n, out_cell, (hipStream_t)stream, nullptr, 0, stats);
}

int32_t mgpu_format_cells_device(mgpu_ctx* ctx, int32_t index_system, const int64_t* cells, int64_t n, char* out,
                                 int64_t out_bytes, int64_t* out_offsets, int64_t* out_total, void* stream) {
  if (!ctx || n < 0 || (n > 0 && (!cells || !out)) || !out_offsets || out_bytes < 0)
    return fail(MGPU_E_INVALID_ARG, "format_cells_device: bad arguments");
  if (index_system != MGPU_H3 && index_system != MGPU_BNG)
    return fail(MGPU_E_INVALID_ARG, "unknown index system %d (0 = H3, 1 = BNG)", index_system);
  if (int32_t st = set_device(ctx->device)) return st;
  hipStream_t s = (hipStream_t)stream;
  // per-chunk totals live in the workspace's tile_where region (one int64 per 256 ids
  // there, one per 4096 needed)
  if (int32_t st = ensure_ws(ctx, mgpu::join_tiles(n))) return st;
  auto* counters = (unsigned long long*)ctx->ws;
  auto* chunk = (int64_t*)((uint8_t*)ctx->ws + ws_layout(mgpu::join_tiles(n), 0).where);
  HIP_TRY(hipMemsetAsync(counters, 0, kWsCounters, s));
  HIP_TRY(mgpu::launch_format_cells(index_system, cells, n, out, out_bytes, out_offsets, chunk, counters, s));
  unsigned long long h[4] = {0};
  int64_t total = 0;
  HIP_TRY(hipMemcpyAsync(h, counters, sizeof h, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&total, out_offsets + n, sizeof total, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (out_total) *out_total = total;
  if (h[2]) return fail(MGPU_E_INVALID_ARG, "%llu BNG cell ids have no string form", h[2]);
  if (total > out_bytes) return fail(MGPU_E_CAPACITY, "format_cells_device: %lld bytes needed, %lld given",
                                     (long long)total, (long long)out_bytes);
  return MGPU_OK;
}

int32_t mgpu_grid_kring(mgpu_ctx* ctx, int32_t index_system, const int64_t* cells, int64_t n, int32_t k,
                        int32_t loop_only, int64_t* out_cells, int64_t capacity, int64_t* out_offsets,
                        int64_t* out_total, void* stream) {
  if (!ctx || n < 0 || (n > 0 && !cells) || !out_offsets || capacity < 0 || (capacity > 0 && !out_cells))
    return fail(MGPU_E_INVALID_ARG, "grid_kring: bad arguments");
  if (index_system != MGPU_BNG && index_system != MGPU_H3)
    return fail(MGPU_E_INVALID_ARG, "grid_kring: unknown index system %d", index_system);
  if (k < 0 || k > 1024) return fail(MGPU_E_INVALID_ARG, "grid_kring: k must be in [0, 1024]");
  if (int32_t st = set_device(ctx->device)) return st;
  hipStream_t s = (hipStream_t)stream;
  if (int32_t st = ensure_ws(ctx, mgpu::join_tiles(n))) return st;
  // workspace: counters, the chunk sums (tile_where region), per-cell counts mc[n] and the
  // fallback list fb_idx[n] (the records region, >= 16 n bytes)
  const WsLayout L = ws_layout(mgpu::join_tiles(n), 0);
  auto* base = (uint8_t*)ctx->ws;
  auto* counters = (unsigned long long*)base;
  auto* chunk = (int64_t*)(base + L.where);
  auto* mc = (int64_t*)(base + L.recs);
  auto* fb_idx = (uint32_t*)(base + L.recs + (size_t)std::max<int64_t>(n, 1) * 8);
  HIP_TRY(hipMemsetAsync(counters, 0, kWsCounters, s));
  HIP_TRY(mgpu::launch_kring_count(index_system, cells, n, k, loop_only, mc, chunk, fb_idx, counters, s));
  unsigned long long h[6] = {0};
  HIP_TRY(hipMemcpyAsync(h, counters, sizeof h, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (h[2] && index_system == MGPU_H3)
    return fail(MGPU_E_INVALID_ARG, "%llu cells are not H3 cell ids", h[2]);
  if (h[2])
    return fail(MGPU_E_INVALID_ARG, "%llu cells are not BNG cells or reach ids BNGIndexSystem.isValid cannot parse "
                "(NumberFormatException in the reference)", h[2]);
  // H3 walks that met a pentagon: H3's _kRingInternal / Mosaic's kLoop fallback, in
  // batches of cells whose scratch fits 256 MB, once for the lengths, once (after the
  // offsets) for the lists
  const int64_t n_fb = (int64_t)h[3];
  uint64_t* scratch = nullptr;
  struct Free {  // the fallback scratch is freed on every return path
    uint64_t*& p;
    ~Free() {
      if (p) hipFree(p);
    }
  } free_scratch{scratch};
  int64_t batch = 0;
  if (n_fb) {
    const int64_t words = mgpu::kring_fallback_words(k);
    batch = std::max<int64_t>(1, std::min<int64_t>(n_fb, ((int64_t)256 << 20) / 8 / words));
    if (ctx->opt.kring_batch > 0) batch = std::min(batch, ctx->opt.kring_batch);  // (option kring_batch)
    HIP_TRY(hipMalloc(&scratch, (size_t)batch * words * 8));
    for (int64_t j0 = 0; j0 < n_fb; j0 += batch)
      HIP_TRY(mgpu::launch_kring_fallback(cells, fb_idx, j0, std::min(n_fb, j0 + batch), k, loop_only, mc, chunk,
                                          out_offsets, out_cells, capacity, scratch, 0, counters, s));
  }
  HIP_TRY(mgpu::launch_kring_write(index_system, cells, n, k, loop_only, mc, chunk, out_offsets, out_cells, capacity,
                                   s));
  for (int64_t j0 = 0; j0 < n_fb; j0 += batch)
    HIP_TRY(mgpu::launch_kring_fallback(cells, fb_idx, j0, std::min(n_fb, j0 + batch), k, loop_only, mc, chunk,
                                        out_offsets, out_cells, capacity, scratch, 1, counters, s));
  int64_t total = 0;
  HIP_TRY(hipMemcpyAsync(h, counters, sizeof h, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&total, out_offsets + n, sizeof total, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (out_total) *out_total = total;
  if (h[4])
    return fail(MGPU_E_INTERNAL, "grid_kring: %llu pentagon walks overflowed their hash set (inconsistent tables)", h[4]);
  if (total > capacity)
    return fail(MGPU_E_CAPACITY, "grid_kring: %lld ids, capacity %lld", (long long)total, (long long)capacity);
  return MGPU_OK;
}

int32_t mgpu_bng_format_device(mgpu_ctx* ctx, const int64_t* cells, int64_t n, char* out, int64_t out_bytes,
                               int64_t* out_offsets, int64_t* out_total, void* stream) {
  return mgpu_format_cells_device(ctx, MGPU_BNG, cells, n, out, out_bytes, out_offsets, out_total, stream);
}

int32_t mgpu_points_to_cells_host(mgpu_ctx* ctx, int32_t is, int32_t res, const double* x, const double* y, int64_t n,
                                  int64_t* out_cell) {
  if (!ctx) return fail(MGPU_E_INVALID_ARG, "ctx is NULL");
  if (n == 0) return check_res(is, res);
  if (int32_t st = set_device(ctx->device)) return st;
  double *dx = nullptr, *dy = nullptr;
  int64_t* dc = nullptr;
  HIP_TRY(hipMalloc(&dx, n * 8));
  HIP_TRY(hipMalloc(&dy, n * 8));
  HIP_TRY(hipMalloc(&dc, n * 8));
  HIP_TRY(hipMemcpy(dx, x, n * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dy, y, n * 8, hipMemcpyHostToDevice));
  int32_t st = mgpu_points_to_cells(ctx, is, res, dx, dy, n, dc, nullptr, nullptr);
  if (st == MGPU_OK) HIP_TRY(hipMemcpy(out_cell, dc, n * 8, hipMemcpyDeviceToHost));
  hipFree(dx);
  hipFree(dy);
  hipFree(dc);
  return st;
}

// ------------------------------------------------------------------ chips

}  // extern "C"

static mgpu_build_opts build_opts_of(const mgpu_ctx* ctx) {
  mgpu_build_opts o;
  o.raster = (int32_t)ctx->opt.raster;
  o.raster_bng = (int32_t)ctx->opt.raster_bng;
  o.raster_sub = (int32_t)ctx->opt.raster_sub;
  o.raster_milli = (int32_t)ctx->opt.raster_milli;
  return o;
}

namespace mgpu {
int32_t adopt_device_blob(mgpu_ctx* ctx, void* dev_blob, int64_t bytes, mgpu_chips** out) {
  BlobHeader hdr;
  HIP_TRY(hipMemcpy(&hdr, dev_blob, sizeof hdr, hipMemcpyDeviceToHost));
  if (int32_t st = check_header(hdr, bytes)) return st;
  mgpu_chips* ch = new mgpu_chips();
  ch->device = ctx->device;
  ch->blob = dev_blob;
  ch->bytes = (size_t)bytes;
  ch->index_system = hdr.index_system;
  ch->view = view_from_header(hdr, (uint8_t*)ch->blob);
  ch->n_vertices = hdr.n_vertices;
  // the classify kernels' finer block table, derived from the blob's pixel classes and kept
  // on the handle beside the blob (the blob's own bytes are pinned: every way a table
  // reaches a device passes through here)
  uint32_t sx = 0, sy = 0, bnx = 0, bny = 0;
  if (ch->index_system == MGPU_H3 && fine_table_shape(ch->view, &sx, &sy, &bnx, &bny)) {
    void* fine = nullptr;
    hipError_t e = hipMalloc(&fine, ((size_t)bnx * bny + 3) & ~(size_t)3);
    if (e == hipSuccess) e = launch_fine_table(ch->view, sx, sy, bnx, bny, (uint8_t*)fine, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
      if (fine) hipFree(fine);
      delete ch;
      return fail(MGPU_E_DEVICE, "fine block table: %s", hipGetErrorString(e));
    }
    ch->fine = fine;
    ch->view.raster_fine = (const uint8_t*)fine;
    ch->view.fine_sx = sx, ch->view.fine_sy = sy, ch->view.fine_bnx = bnx, ch->view.fine_bny = bny;
  }
  *out = ch;
  return MGPU_OK;
}
}  // namespace mgpu

// mgpu_pip_join_count's polygon slots of a chip table (poly_slots.h), on the device: built
// at the first use from the table's chip_poly -- read back from the blob, so handles made
// from a device blob or a broadcast have them too -- and kept on the handle, outside the
// blob (mgpu_chips.slots).
struct PolySlotsDev {
  std::vector<int32_t> ids;        // host copy (mgpu_chips_polygons)
  int32_t* d_ids = nullptr;        // [P]
  uint32_t* d_chip_slot = nullptr; // [n_chips]
  uint32_t* d_dense = nullptr;     // [max id - min id + 1] or null (poly_slots_dense)
};

static std::mutex g_slots_mu;

static void free_poly_slots(mgpu_chips* chips) {
  auto* ps = (PolySlotsDev*)chips->slots;
  if (!ps) return;
  if (ps->d_ids) hipFree(ps->d_ids);
  if (ps->d_chip_slot) hipFree(ps->d_chip_slot);
  if (ps->d_dense) hipFree(ps->d_dense);
  delete ps;
  chips->slots = nullptr;
}

static int32_t ensure_poly_slots(const mgpu_chips* chips, const PolySlotsDev** out) {
  std::lock_guard<std::mutex> lock(g_slots_mu);
  if (chips->slots) {
    *out = (const PolySlotsDev*)chips->slots;
    return MGPU_OK;
  }
  if (int32_t st = set_device(chips->device)) return st;
  const int64_t nch = chips->view.n_chips;
  std::vector<int32_t> poly((size_t)nch);
  if (nch) HIP_TRY(hipMemcpy(poly.data(), chips->view.chip_poly, (size_t)nch * 4, hipMemcpyDeviceToHost));
  mgpu::PolySlots hs = mgpu::poly_slots(poly.data(), nch);
  auto ps = std::make_unique<PolySlotsDev>();
  auto upload = [&](auto** d, const void* src, size_t bytes) -> hipError_t {
    if (hipError_t e = hipMalloc((void**)d, std::max<size_t>(bytes, 4))) return e;
    return bytes ? hipMemcpy(*d, src, bytes, hipMemcpyHostToDevice) : hipSuccess;
  };
  hipError_t e = upload(&ps->d_ids, hs.ids.data(), hs.ids.size() * 4);
  if (e == hipSuccess) e = upload(&ps->d_chip_slot, hs.slot_of_row.data(), hs.slot_of_row.size() * 4);
  if (e == hipSuccess && mgpu::poly_slots_dense(hs.ids)) {
    std::vector<uint32_t> dense((size_t)((int64_t)hs.ids.back() - hs.ids.front() + 1), 0u);
    for (size_t k = 0; k < hs.ids.size(); k++) dense[(size_t)((int64_t)hs.ids[k] - hs.ids.front())] = (uint32_t)k;
    e = upload(&ps->d_dense, dense.data(), dense.size() * 4);
  }
  if (e != hipSuccess) {
    if (ps->d_ids) hipFree(ps->d_ids);
    if (ps->d_chip_slot) hipFree(ps->d_chip_slot);
    if (ps->d_dense) hipFree(ps->d_dense);
    return fail(MGPU_E_DEVICE, "polygon slots: %s", hipGetErrorString(e));
  }
  ps->ids = std::move(hs.ids);
  chips->slots = ps.release();
  *out = (const PolySlotsDev*)chips->slots;
  return MGPU_OK;
}

// Host -> device copy of `bytes` bytes that fill(dst, off, n) produces, through two pinned
// 64 MiB staging buffers: the host threads fill one piece while the DMA engine moves the
// other (a pageable hipMemcpy of C3's 5.3 GB blob ran at ~4.6 GB/s on the box).
static hipError_t stage_to_device(void* d, size_t bytes, const std::function<void(uint8_t*, size_t, size_t)>& fill) {
  constexpr size_t kPiece = (size_t)64 << 20;
  if (bytes <= 2 * kPiece) {  // (small: one pageable buffer)
    std::vector<uint8_t> tmp(bytes);
    mgpu::parallel_for((int64_t)((bytes + (1 << 20) - 1) >> 20), 1, [&](int64_t b, int64_t en, int) {
      const size_t lo = (size_t)b << 20, hi = std::min(bytes, (size_t)en << 20);
      fill(tmp.data() + lo, lo, hi - lo);
    });
    return hipMemcpy(d, tmp.data(), bytes, hipMemcpyHostToDevice);
  }
  void* stage[2] = {nullptr, nullptr};
  hipEvent_t done[2] = {nullptr, nullptr};
  hipStream_t s = nullptr;
  hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
  for (int k = 0; k < 2 && e == hipSuccess; k++) {
    e = hipHostMalloc(&stage[k], kPiece, hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&done[k], hipEventDisableTiming);
  }
  for (size_t off = 0, k = 0; off < bytes && e == hipSuccess; off += kPiece, k ^= 1) {
    const size_t n = std::min(kPiece, bytes - off);
    if (off >= 2 * kPiece) e = hipEventSynchronize(done[k]);  // the piece this buffer held is on the device
    if (e != hipSuccess) break;
    auto* dst = (uint8_t*)stage[k];
    mgpu::parallel_for((int64_t)((n + (1 << 20) - 1) >> 20), 1, [&](int64_t b, int64_t en, int) {
      const size_t lo = (size_t)b << 20, hi = std::min(n, (size_t)en << 20);
      fill(dst + lo, off + lo, hi - lo);
    });
    e = hipMemcpyAsync((uint8_t*)d + off, stage[k], n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipEventRecord(done[k], s);
  }
  if (s) {
    const hipError_t e2 = hipStreamSynchronize(s);
    if (e == hipSuccess) e = e2;
    hipStreamDestroy(s);
  }
  for (int k = 0; k < 2; k++) {
    if (done[k]) hipEventDestroy(done[k]);
    if (stage[k]) hipHostFree(stage[k]);
  }
  return e;
}

extern "C" {

int32_t mgpu_chips_upload_blob(mgpu_ctx* ctx, const void* host_blob, int64_t bytes, mgpu_chips** out) {
  if (!ctx || !out) return fail(MGPU_E_INVALID_ARG, "ctx/out is NULL");
  if (int32_t st = mgpu_host_blob_info(host_blob, bytes, nullptr, nullptr, nullptr, nullptr)) return st;
  if (int32_t st = set_device(ctx->device)) return st;
  void* d = nullptr;
  HIP_TRY(hipMalloc(&d, (size_t)bytes));
  hipError_t e = stage_to_device(d, (size_t)bytes, [&](uint8_t* dst, size_t off, size_t n) {
    memcpy(dst, (const uint8_t*)host_blob + off, n);
  });
  if (e != hipSuccess) {
    hipFree(d);
    return fail(MGPU_E_DEVICE, "hipMemcpy: %s", hipGetErrorString(e));
  }
  int32_t st = mgpu::adopt_device_blob(ctx, d, bytes, out);
  if (st) hipFree(d);
  return st;
}

int32_t mgpu_chips_upload(mgpu_ctx* ctx, int32_t index_system, int64_t n_chips, const int64_t* cell,
                          const int32_t* polygon_id, const uint8_t* is_core, const int64_t* wkb_offsets,
                          const uint8_t* wkb, mgpu_chips** out) {
  if (!ctx || !out) return fail(MGPU_E_INVALID_ARG, "ctx/out is NULL");
  mgpu::HostBlob host;
  mgpu::BlobHeader hdr;
  if (int32_t st = set_device(ctx->device)) return st;
  // the blob's pieces staged straight to the device (no whole host blob)
  void* d = nullptr;
  size_t bytes = 0;
  const mgpu::BlobSink sink = [&](size_t total, const std::vector<mgpu::BlobPiece>& pieces) -> int32_t {
    BLOB_T0();
    HIP_TRY(hipMalloc(&d, total));
    BLOB_MARK("sink:malloc");
    bytes = total;
    const hipError_t e = stage_to_device(d, total, [&](uint8_t* dst, size_t off, size_t n) {
      mgpu::fill_from_pieces(pieces, dst, off, n);
    });
    if (e != hipSuccess) return fail(MGPU_E_DEVICE, "hipMemcpy: %s", hipGetErrorString(e));
    return MGPU_OK;
  };
  BLOB_T0();
  int32_t st = mgpu::build_blob(index_system, n_chips, cell, polygon_id, is_core, wkb_offsets, wkb, host, hdr,
                                build_opts_of(ctx), &sink);
  BLOB_MARK("upl:build");
  if (st == MGPU_OK) st = mgpu::adopt_device_blob(ctx, d, (int64_t)bytes, out);
  BLOB_MARK("upl:adopt");
  if (st && d) hipFree(d);
  return st;
}

int32_t mgpu_chips_destroy(mgpu_chips* chips) {
  if (!chips) return MGPU_OK;
  hipSetDevice(chips->device);
  if (chips->blob) hipFree(chips->blob);
  if (chips->fine) hipFree(chips->fine);
  free_poly_slots(chips);
  delete chips;
  return MGPU_OK;
}

int32_t mgpu_chips_info(const mgpu_chips* chips, int64_t* n_chips, int64_t* n_cells, int64_t* n_vertices) {
  if (!chips) return fail(MGPU_E_INVALID_ARG, "chips is NULL");
  if (n_chips) *n_chips = chips->view.n_chips;
  if (n_cells) *n_cells = chips->view.n_cells;
  if (n_vertices) *n_vertices = chips->n_vertices;
  return MGPU_OK;
}

int32_t mgpu_chips_raster_info(const mgpu_chips* chips, int64_t* mode, int64_t* n_classes) {
  if (!chips) return fail(MGPU_E_INVALID_ARG, "chips is NULL");
  if (mode) *mode = chips->view.raster_mode;
  if (n_classes) *n_classes = chips->view.raster_mode != mgpu::kRasterNone ? (int64_t)chips->view.raster_ncls : 0;
  return MGPU_OK;
}

int32_t mgpu_chips_device_blob(const mgpu_chips* chips, void** device_ptr, int64_t* bytes) {
  if (!chips || !device_ptr || !bytes) return fail(MGPU_E_INVALID_ARG, "NULL argument");
  *device_ptr = chips->blob;
  *bytes = (int64_t)chips->bytes;
  return MGPU_OK;
}

int32_t mgpu_chips_from_device_blob(mgpu_ctx* ctx, const void* device_ptr, int64_t bytes, mgpu_chips** out) {
  if (!ctx || !device_ptr || !out || bytes <= 0) return fail(MGPU_E_INVALID_ARG, "NULL argument");
  if (int32_t st = set_device(ctx->device)) return st;
  if (bytes < (int64_t)mgpu::kBlobHeaderBytes) return fail(MGPU_E_INVALID_ARG, "blob too small");
  mgpu::BlobHeader hdr;
  HIP_TRY(hipMemcpy(&hdr, device_ptr, sizeof hdr, hipMemcpyDeviceToHost));
  if (int32_t st = mgpu::check_header(hdr, bytes)) return st;
  void* d = nullptr;
  HIP_TRY(hipMalloc(&d, bytes));
  hipError_t e = hipMemcpy(d, device_ptr, bytes, hipMemcpyDeviceToDevice);
  if (e != hipSuccess) {
    hipFree(d);
    return fail(MGPU_E_DEVICE, "hipMemcpy: %s", hipGetErrorString(e));
  }
  int32_t st = mgpu::adopt_device_blob(ctx, d, bytes, out);
  if (st) hipFree(d);
  return st;
}

int32_t mgpu_st_contains(mgpu_ctx* ctx, const mgpu_chips* chips, const int64_t* chip_row, const double* x,
                         const double* y, int64_t n, int8_t* out, void* stream) {
  if (!ctx || !chips) return fail(MGPU_E_INVALID_ARG, "ctx/chips is NULL");
  if (n < 0 || (n > 0 && (!chip_row || !x || !y || !out))) return fail(MGPU_E_INVALID_ARG, "bad arrays");
  if (int32_t st = set_device(ctx->device)) return st;
  if (chips->device != ctx->device)
    return fail(MGPU_E_INVALID_ARG, "chip table lives on device %d, context on device %d", chips->device, ctx->device);
  hipStream_t s = (hipStream_t)stream;
  if (int32_t st = ensure_ws(ctx, 1)) return st;
  auto* counters = (unsigned long long*)ctx->ws;
  HIP_TRY(hipMemsetAsync(counters, 0, kWsCounters, s));
  HIP_TRY(mgpu::launch_st_contains(chips->view, chip_row, x, y, n, out, counters, s));
  unsigned long long h[4] = {0};
  HIP_TRY(hipMemcpyAsync(h, counters, sizeof h, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (h[2])
    return fail(MGPU_E_INVALID_ARG, "st_contains: %llu chip rows outside [0, %u)", h[2], chips->view.n_chips);
  return MGPU_OK;
}

// ------------------------------------------------------------------ join

// The binned pipeline's planner (kernels.h BinArgs): a chip table far larger than the
// caches and a large batch of points.  Option pipeline = MGPU_PIPELINE_BINNED forces it
// whenever it applies; auto takes it for tables of at least bin_min_mb (256 MB -- the
// Infinity Cache) and batches of at least bin_min_points (2^21).  The bins tile the chip
// table's extent (H3: the lon/lat box of the chip cells; BNG: the dense grid's box),
// about bin_count of them (default 64), roughly square on the ground.
static bool plan_bins(const mgpu_options& o, const mgpu_chips* chips, int32_t is, int32_t res, int64_t n,
                      const uint8_t* valid, const mgpu::JoinArgs& a, mgpu::BinArgs& b) {
  const bool forced = o.pipeline == MGPU_PIPELINE_BINNED;
  if (!(forced || o.pipeline == MGPU_PIPELINE_AUTO) || n <= 0 || valid || !a.res_match) return false;
  if (n >= (int64_t)1 << 32 || chips->view.max_cell_chips > 32) return false;
  const mgpu::ChipTableView& v = chips->view;
  double x0, y0, W, H, aspect;
  if (is == MGPU_H3) {
    if (v.probe_mode == mgpu::kProbeCellId || !(v.bbox[2] - v.bbox[0] < 360.0) || !(v.bbox[3] - v.bbox[1] < 180.0))
      return false;
    x0 = v.bbox[0], y0 = v.bbox[1], W = v.bbox[2] - v.bbox[0], H = v.bbox[3] - v.bbox[1];
    const double latc = std::min(std::max(std::fabs(v.bbox[1]), std::fabs(v.bbox[3])), 85.0);
    aspect = W * std::cos(latc * kPi / 180.0) / std::max(H, 1e-12);
  } else {
    if (v.probe_mode != mgpu::kProbeDense || res != v.res || v.bng_edge == 0) return false;
    const mgpu::DenseFace& D = v.dense[0];
    x0 = (double)D.a0 * v.bng_edge, y0 = (double)D.b0 * v.bng_edge;
    W = (double)D.w * v.bng_edge, H = (double)D.h * v.bng_edge;
    aspect = W / std::max(H, 1e-12);
  }
  if (!(W > 0) || !(H > 0)) return false;
  if (!forced && ((double)chips->bytes < (double)o.bin_min_mb * 1048576.0 || n < o.bin_min_points)) return false;
  const int nb = (int)std::min<int64_t>(std::max<int64_t>(o.bin_count, 1), mgpu::bin_max());
  int nbx = (int)std::lround(std::sqrt(nb * aspect));
  nbx = std::min(std::max(nbx, 1), nb);
  const int nby = std::max(nb / nbx, 1);
  b.x0 = x0, b.y0 = y0;
  b.nbx = nbx, b.nby = nby;
  b.inv_bx = nbx / W, b.inv_by = nby / H;
  b.xcd_runs = (int32_t)o.bin_xcd;
  return true;
}

// Launch one join on `s` (nothing waits here).  n_ovr > 0: the route's near-ties take
// the first n_ovr libm overrides of ctx->ovr (ascending input positions, lattice keys).
static int32_t join_impl(mgpu_ctx* ctx, const mgpu_chips* chips, int32_t is, int32_t res, const double* x,
                         const double* y, const int64_t* point_id, int64_t id_base, int64_t n, int64_t capacity,
                         int64_t* out_point, int32_t* out_poly, hipStream_t s, bool timed,
                         const uint8_t* valid = nullptr, int64_t valid_off = 0, int64_t n_ovr = 0,
                         int tie_host = 0, int64_t count_pool = -1) {
  if (!ctx || !chips) return fail(MGPU_E_INVALID_ARG, "ctx/chips is NULL");
  if (int32_t r = check_res(is, res)) return r;
  if (chips->index_system != is)
    return fail(MGPU_E_INVALID_ARG, "chip table built for index system %d, join asked for %d", chips->index_system, is);
  if (chips->device != ctx->device)
    return fail(MGPU_E_INVALID_ARG, "chip table lives on device %d, context on device %d", chips->device, ctx->device);
  if (n < 0 || (n > 0 && (!x || !y))) return fail(MGPU_E_INVALID_ARG, "bad point arrays");
  if (capacity < 0 || (capacity > 0 && (!out_point || !out_poly))) return fail(MGPU_E_INVALID_ARG, "bad output arrays");
  if (int32_t st = set_device(ctx->device)) return st;
  int64_t tiles = mgpu::join_tiles(n);
  // pool: the records of tiles with more pairs than points (bounded by the capacity; a
  // total beyond it is reported as MGPU_E_CAPACITY either way).  Count mode
  // (mgpu_pip_join_count, count_pool >= 0) has no capacity: its pool is count_pool, and
  // nothing that writes pairs is launched.
  const bool emit = count_pool < 0;
  const int64_t pool = emit ? capacity : count_pool;
  if (int32_t st = ensure_ws(ctx, tiles, pool)) return st;
  auto* base = (uint8_t*)ctx->ws;
  const WsLayout L = ws_layout(tiles, pool);
  const mgpu_options& o = ctx->opt;
  mgpu::JoinArgs a;
  a.x = x;
  a.y = y;
  a.n = n;
  a.n_tiles = tiles;
  a.res = res;
  a.res_match = (is == MGPU_BNG || chips->view.res < 0 || chips->view.res == res) ? 1 : 0;
  a.chips = chips->view;
  if (!o.cfy_fine) a.chips.raster_fine = nullptr;  // (the classify kernels then stage raster_blk)
  a.counters = (unsigned long long*)base;
  a.pool_used = a.counters + 5;
  a.n_dirty = (uint32_t*)(a.counters + 6);
  a.dirty = (uint32_t*)(base + L.dirty);
  a.pool_cap = pool;
  a.tile_count = (uint32_t*)(base + L.count);
  a.tile_where = (uint64_t*)(base + L.where);
  a.recs = (uint64_t*)(base + L.recs);
  a.tie_queue = ctx->tq;
  a.tie_cap = ctx->tq_cap;
  a.ovr = ctx->ovr;
  a.n_ovr = n_ovr;
  a.tie_host = (is == MGPU_H3 && tie_host) ? 1 : 0;
  a.pos_of = nullptr;
  mgpu::EmitArgs e;
  e.tile_count = a.tile_count;
  e.group_off = (uint64_t*)(base + L.off);
  a.group_sum = (uint32_t*)(base + L.gsum);
  a.group_cand = a.group_sum + (tiles / 32 + 1);
  e.tile_where = a.tile_where;
  e.recs = a.recs;
  e.point_id = point_id;
  e.id_base = id_base;
  e.capacity = capacity;
  e.out_point = out_point;
  e.out_poly = out_poly;
  a.valid = valid;
  a.valid_off = valid_off;
  a.mixed_idx = nullptr;
  a.mixed_res = nullptr;
  a.chunk_mixed = nullptr;
  a.extra = nullptr;
  a.n_extra = nullptr;
  a.poly_answers = 0;
  static_assert(kWsCounters == mgpu::kCounterWords * 8, "launch_join_clear clears the counters");
  HIP_TRY(mgpu::launch_join_clear(a.counters, ctx->tq, s));  // (counters + the queue's header: one launch)
  // the split pipeline (kernels.h SplitArgs) when the chip table has a pixel index for
  // this resolution and no cell holds more than 32 chips
  // (BNG dense tables without a pixel index: the grid entry is the code -- a cell whose
  // chips are all core answers its points, the rest are mixed; option bng_split)
  const bool bng_grid = is == MGPU_BNG && chips->view.raster_mode == mgpu::kRasterNone &&
                        chips->view.probe_mode == mgpu::kProbeDense && o.bng_split;
  const bool split = (o.pipeline == MGPU_PIPELINE_AUTO || o.pipeline == MGPU_PIPELINE_SPLIT) && n > 0 &&
                     (chips->view.raster_mode != mgpu::kRasterNone || bng_grid) && a.res_match &&
                     (is == MGPU_H3 || res == chips->view.res) && chips->view.max_cell_chips <= 32;
  mgpu::SplitArgs sa{};
  if (split) {
    const int64_t nc = mgpu::split_chunks(n), C = mgpu::split_chunk();
    size_t off = 0;
    auto carve = [&](size_t bytes) {
      const size_t o_ = off;
      off = align_up(off + bytes, 256);
      return o_;
    };
    const size_t o_codes = carve((size_t)nc * C * 4), o_idx = carve((size_t)nc * C * 2), o_res = carve((size_t)nc * C * 8);
    const size_t o_pairs = carve(nc * 4), o_mixed = carve(nc * 4), o_cand = carve(nc * 4), o_off = carve(nc * 8);
    const size_t o_extra = carve((size_t)nc * (C / mgpu::join_tile_points()) * 4);
    if (off > ctx->split_bytes) {
      if (ctx->split_ws) HIP_TRY(hipFree(ctx->split_ws));
      ctx->split_ws = nullptr;
      ctx->split_bytes = 0;
      HIP_TRY(hipMalloc(&ctx->split_ws, off));
      ctx->split_bytes = off;
    }
    auto* sb = (uint8_t*)ctx->split_ws;
    sa.codes = sb + o_codes;
    sa.mixed_idx = (uint16_t*)(sb + o_idx);
    sa.chunk_pairs = (uint32_t*)(sb + o_pairs);
    sa.chunk_mixed = (uint32_t*)(sb + o_mixed);
    sa.chunk_off = (uint64_t*)(sb + o_off);
    a.extra = sa.extra = (uint32_t*)(sb + o_extra);
    a.n_extra = (uint32_t*)(a.counters + 7);  // (zeroed with the counters)
    a.group_sum = sa.chunk_pairs;
    a.group_cand = (uint32_t*)(sb + o_cand);  // (zeroed per chunk by the classify kernels)
    a.mixed_idx = sa.mixed_idx;
    a.mixed_res = (uint64_t*)(sb + o_res);
    a.chunk_mixed = sa.chunk_mixed;
    sa.point_id = point_id;
    sa.id_base = id_base;
    sa.capacity = capacity;
    sa.out_point = out_point;
    sa.out_poly = out_poly;
    sa.j = a;
  }
  mgpu::BinArgs ba{};
  const bool binned = !split && plan_bins(o, chips, is, res, n, valid, a, ba);
  if (binned) {
    const int64_t nc = mgpu::split_chunks(n), C = mgpu::split_chunk();
    const int64_t K = mgpu::bin_chunks(n), G = mgpu::bin_groups(n), nb = (int64_t)ba.nbx * ba.nby;
    size_t off = 0;
    auto carve = [&](size_t bytes) {
      const size_t o_ = off;
      off = align_up(off + bytes, 256);
      return o_;
    };
    const size_t o_perm = carve((size_t)n * 4), o_rorig = carve((size_t)n * 8);
    const size_t o_bx = carve((size_t)n * 8), o_by = carve((size_t)n * 8),
                 o_pre = carve((size_t)K * nb * 4), o_res = carve((size_t)nc * C * 8), o_cnt = carve((size_t)K * nb * 4),
                 o_gs = carve((size_t)G * nb * 4), o_pairs = carve(nc * 4), o_off = carve(nc * 8),
                 o_gperm = carve(nc * 4), o_gcand = carve(nc * 4);
    // H3 over a dense grid: the scatter kernel's per-slot grid keys (kernels.hip bin_key_of)
    const mgpu::ChipTableView& cv = chips->view;
    uint64_t grid_entries = 0;
    for (int f = 0; f < 20; f++) grid_entries = std::max<uint64_t>(grid_entries, (uint64_t)cv.dense[f].base + (uint64_t)cv.dense[f].w * cv.dense[f].h);
    const bool keyed = is == MGPU_H3 && cv.probe_mode == mgpu::kProbeDense && o.bin_keys && grid_entries < (1ull << 30);
    const size_t o_key = keyed ? carve((size_t)n * 4) : 0;
    if (off > ctx->bin_bytes) {
      if (ctx->bin_ws) HIP_TRY(hipFree(ctx->bin_ws));
      ctx->bin_ws = nullptr;
      ctx->bin_bytes = 0;
      HIP_TRY(hipMalloc(&ctx->bin_ws, off));
      ctx->bin_bytes = off;
    }
    auto* bb = (uint8_t*)ctx->bin_ws;
    ba.x = x;
    ba.y = y;
    ba.bx = (double*)(bb + o_bx);
    ba.by = (double*)(bb + o_by);
    ba.pre = (uint32_t*)(bb + o_pre);
    ba.perm = (uint32_t*)(bb + o_perm);
    ba.res = (uint64_t*)(bb + o_rorig);
    ba.cnt = (uint32_t*)(bb + o_cnt);
    ba.gsum = (uint32_t*)(bb + o_gs);
    ba.key = keyed ? (uint32_t*)(bb + o_key) : nullptr;
    mgpu::JoinArgs j = a;
    j.bin_key = ba.key;
    j.x = ba.bx;
    j.y = ba.by;
    j.mixed_idx = nullptr;
    j.chunk_mixed = nullptr;
    j.poly_answers = 1;
    j.pos_of = ba.perm;
    j.mixed_res = (uint64_t*)(bb + o_res);
    j.group_sum = (uint32_t*)(bb + o_gperm);
    j.group_cand = (uint32_t*)(bb + o_gcand);
    ba.s.j = j;
    ba.s.chunk_pairs = (uint32_t*)(bb + o_pairs);
    ba.s.chunk_off = (uint64_t*)(bb + o_off);
    ba.s.point_id = point_id;
    ba.s.id_base = id_base;
    ba.s.capacity = capacity;
    ba.s.out_point = out_point;
    ba.s.out_poly = out_poly;
    HIP_TRY(hipMemsetAsync(bb + o_gperm, 0, align_up(nc * 4, 256) + nc * 4, s));  // group_sum, group_cand
  } else if (!split) {
    HIP_TRY(hipMemsetAsync(base + L.gsum, 0, 2 * ((size_t)tiles / 32 + 1) * 4, s));
  }
  if (timed) HIP_TRY(hipEventRecord(ctx->ev0, s));
  if (split)
    HIP_TRY(mgpu::launch_split(is, sa, s, timed ? ctx->ev2 : nullptr, timed ? ctx->ev3 : nullptr, emit));
  else if (binned)
    HIP_TRY(mgpu::launch_binned(is, ba, s, timed ? ctx->ev3 : nullptr, timed ? ctx->ev2 : nullptr, emit));
  else
    HIP_TRY(mgpu::launch_join(is, a, e, s, timed ? ctx->ev2 : nullptr, emit));
  if (timed) HIP_TRY(hipEventRecord(ctx->ev1, s));
  auto& L2 = ctx->last;
  L2.split = split;
  L2.sargs = sa;
  L2.binned = binned;
  L2.bargs = ba;
  L2.chips = chips;
  L2.is = is;
  L2.res = res;
  L2.x = x;
  L2.y = y;
  L2.point_id = point_id;
  L2.id_base = id_base;
  L2.n = n;
  L2.pts_valid = valid;
  L2.pts_valid_off = valid_off;
  L2.emit = e;
  L2.jargs = a;
  L2.n_tiles = tiles;
  L2.n_ovr = n_ovr;
  L2.tie_host = a.tie_host;
  L2.pool_ok = false;
  L2.pool = pool;
  L2.pool_used = 0;
  L2.total = -1;
  L2.valid = true;
  L2.stream = (void*)s;
  L2.capacity = capacity;
  L2.out_point = out_point;
  L2.out_poly = out_poly;
  return MGPU_OK;
}

int32_t mgpu_last_near_ties(mgpu_ctx* ctx, int64_t* out_index, int64_t cap, int64_t* out_n) {
  if (!ctx || !out_n || cap < 0 || (cap > 0 && !out_index)) return fail(MGPU_E_INVALID_ARG, "bad arguments");
  *out_n = 0;
  if (!ctx->tq) return MGPU_OK;
  if (int32_t st = set_device(ctx->device)) return st;
  if (ctx->last.valid && ctx->last.n_ovr > 0) {
    // the last join was rerun with the reference's cell of every point its first pass
    // queued: the override table (ascending positions) is the list
    const int64_t n = ctx->last.n_ovr;
    *out_n = n;
    if (n > cap) return fail(MGPU_E_CAPACITY, "%lld near-tie points, capacity %lld", (long long)n, (long long)cap);
    std::vector<uint64_t> hv((size_t)n * 2);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(hv.data(), ctx->ovr, hv.size() * 8, hipMemcpyDeviceToHost));
    for (int64_t k = 0; k < n; k++) out_index[k] = (int64_t)hv[2 * k];
    return MGPU_OK;
  }
  uint64_t cnt = 0;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(&cnt, ctx->tq, 8, hipMemcpyDeviceToHost));
  const int64_t n = (int64_t)cnt;
  *out_n = n;
  if (n > ctx->tq_cap)
    return fail(MGPU_E_INTERNAL, "%lld near-tie points: more than the queue of an asynchronous join holds (%lld)",
                (long long)n, (long long)ctx->tq_cap);
  if (n > cap) return fail(MGPU_E_CAPACITY, "%lld near-tie points, capacity %lld", (long long)n, (long long)cap);
  std::vector<uint64_t> rec((size_t)n * 4);
  if (n) HIP_TRY(hipMemcpy(rec.data(), ctx->tq + 2, (size_t)n * 32, hipMemcpyDeviceToHost));
  for (int64_t k = 0; k < n; k++) out_index[k] = (int64_t)rec[4 * k];
  std::sort(out_index, out_index + n);
  return MGPU_OK;
}

}  // extern "C"

// mgpu_pip_join with an optional validity bitmap of the points (the Arrow entry's nulls).
// H3 with the reference's libm: one join in which every point whose fast projection
// falls in its tie band is queued and joined with the fast cell (JoinArgs.tie_host);
// the host recomputes the queued points with the reference's arithmetic (h3_glibc.cpp:
// glibc libm + x87, as H3-Java's JNI library on this host) and, only if a cell moves
// -- the fast path's last bits, or glibc misrounding an argument that decides it --
// runs the join again with the reference's cell of EVERY queued point as an override
// (the fix kernels then take the override without computing the device route).  With
// the correctly rounded libm (option h3_libm) the fix kernels decide the ties by the
// device route.  A near-tie queue that overflowed is grown and the join redone.
// One join's arguments (the synchronous call's, or an asynchronous call's kept until
// mgpu_pip_join_finish).
struct JoinCall {
  const mgpu_chips* chips;
  int32_t is, res;
  const double *x, *y;
  const int64_t* point_id;
  int64_t id_base, n, capacity;
  int64_t* out_point;
  int32_t* out_poly;
  hipStream_t s;
  const uint8_t* valid;
  int64_t valid_off;
  int64_t* d_n_pairs;  // the asynchronous form's device count (or null)
  int64_t count_pool = -1;  // >= 0: mgpu_pip_join_count's join (join_impl's count mode) with this overflow pool
};

static int32_t launch_call(mgpu_ctx* ctx, const JoinCall& c, bool timed, int64_t n_ovr, int tie_host) {
  int32_t st = join_impl(ctx, c.chips, c.is, c.res, c.x, c.y, c.point_id, c.id_base, c.n, c.capacity, c.out_point,
                         c.out_poly, c.s, timed, c.valid, c.valid_off, n_ovr, tie_host, c.count_pool);
  if (st) return st;
  if (c.d_n_pairs) HIP_TRY(hipMemcpyAsync(c.d_n_pairs, ctx->ws, 8, hipMemcpyDeviceToDevice, c.s));
  return MGPU_OK;
}

// The override pass of a join whose host libm pass moved a cell: only the units holding
// the overridden points run again (the fused join's tiles; the split pipeline's chunks),
// then -- if some unit's pair count changed -- the scan and the whole emit, else only
// those units' output (kernels.hip launch_join_redo).  The binned pipeline -- its tiles
// hold binned slots -- and a fused join whose first pass used the overflow pool (a rerun
// would take more of it) run whole.
static int32_t launch_override_pass(mgpu_ctx* ctx, const JoinCall& c, bool timed, int64_t n_ovr,
                                    const std::vector<int64_t>& pos, uint64_t pool_used) {
  auto& L = ctx->last;
  if (!L.valid || L.binned || (!L.split && pool_used > 0)) return launch_call(ctx, c, timed, n_ovr, 0);
  // the units, ascending (the positions ascend)
  const int64_t unit = L.split ? mgpu::split_chunk() : mgpu::join_tile_points();
  const int64_t n_units = L.split ? mgpu::split_chunks(L.n) : L.n_tiles;
  std::vector<uint32_t> list;
  for (int64_t p : pos)
    if (list.empty() || list.back() != (uint32_t)(p / unit)) list.push_back((uint32_t)(p / unit));
  if ((int64_t)list.size() * (L.split ? mgpu::split_chunk_tiles() : 1) > L.n_tiles)
    return launch_call(ctx, c, timed, n_ovr, 0);
  const size_t o_aff = 256, o_list = align_up(o_aff + (size_t)n_units, 256), o_old = o_list + list.size() * 4;
  // [0] changed flag, [4] first changed unit (~0), [256] flags per unit, the list, the old counts
  const size_t bytes = o_old + list.size() * 4;
  if (bytes > ctx->redo_bytes) {
    if (ctx->redo) HIP_TRY(hipFree(ctx->redo));
    ctx->redo = nullptr;
    ctx->redo_bytes = 0;
    HIP_TRY(hipMalloc(&ctx->redo, bytes));
    ctx->redo_bytes = bytes;
  }
  auto* rb = (uint8_t*)ctx->redo;
  mgpu::RedoArgs R{(const uint32_t*)(rb + o_list), (uint32_t*)(rb + o_old), rb + o_aff, (uint32_t*)rb,
                   (uint32_t*)(rb + 4)};
  mgpu::JoinArgs a = L.split ? L.sargs.j : L.jargs;
  a.ovr = ctx->ovr;
  a.n_ovr = n_ovr;
  a.tie_host = 0;
  // (the first pass has finished: settle_join waited for its counters)
  HIP_TRY(hipMemsetAsync(rb, 0, o_list, c.s));
  HIP_TRY(hipMemsetAsync(rb + 4, 0xFF, 4, c.s));
  HIP_TRY(hipMemcpyAsync(rb + o_list, list.data(), list.size() * 4, hipMemcpyHostToDevice, c.s));
  const uint32_t nd = L.split ? 0u : (uint32_t)list.size();  // (split: the unpair kernel lists the tiles)
  HIP_TRY(hipMemcpyAsync(a.n_dirty, &nd, 4, hipMemcpyHostToDevice, c.s));
  HIP_TRY(hipStreamSynchronize(c.s));  // (the pageable sources above)
  if (L.split) {
    mgpu::SplitArgs sa = L.sargs;
    sa.j = a;
    HIP_TRY(mgpu::launch_split_redo(c.is, sa, R, (int64_t)list.size(), c.s, c.count_pool < 0));
    L.sargs = sa;
  } else {
    HIP_TRY(mgpu::launch_join_redo(c.is, a, L.emit, R, (int64_t)list.size(), c.s, c.count_pool < 0));
    L.jargs = a;
  }
  if (timed) HIP_TRY(hipEventRecord(ctx->ev1, c.s));
  if (c.d_n_pairs) HIP_TRY(hipMemcpyAsync(c.d_n_pairs, ctx->ws, 8, hipMemcpyDeviceToDevice, c.s));
  L.n_ovr = n_ovr;
  L.tie_host = 0;
  return MGPU_OK;
}

// After a join's first launch (near-ties queued for the host when reference_libm): read
// its counters; grow an overflowed near-tie queue and launch again; recompute the queued
// points with the reference's libm and, only if a cell moves, launch once more with the
// reference's cell of every queued point as an override.  Overflow relaunches are bounded
// separately from the one override pass, so a completed pass is never reported as a
// failure.  Fills out_n_pairs / stats and the context's record of the last join.
static int32_t settle_join(mgpu_ctx* ctx, const JoinCall& c, bool timed, bool reference_libm, int64_t* out_n_pairs,
                           mgpu_stats* stats) {
  const hipStream_t s = c.s;
  int64_t n_ovr = 0, n_ties = 0, n_moved = 0;
  int overflows = 0;
  uint64_t h[8] = {0};
  for (;;) {
    // the counters and the queue's head, written into the pinned page by one launch
    static_assert(kPinWords == mgpu::kCounterWords + 2 + 4 * kTqHead, "launch_join_readback fills the pinned page");
    HIP_TRY(mgpu::launch_join_readback((const unsigned long long*)ctx->ws, ctx->tq, (int)(2 + 4 * kTqHead), ctx->pin_dev, s));
    HIP_TRY(stream_wait(ctx, s));
    memcpy(h, ctx->pin, sizeof h);
    const int64_t queued = (int64_t)ctx->pin[16];
    if (h[2]) break;  // invalid coordinates: reported below
    if (queued > ctx->tq_cap) {
      // the queue is sized from this pass's count, so one regrowth holds the next pass
      if (++overflows > 2) return fail(MGPU_E_INTERNAL, "pip_join: the near-tie queue overflowed %d times", overflows);
      if (int32_t e = ensure_tq(ctx, queued + queued / 4 + 1024)) return e;
      if (int32_t e = launch_call(ctx, c, timed, n_ovr, reference_libm && n_ovr == 0)) return e;
      continue;
    }
    if (n_ovr > 0) break;  // the pass with the reference's cells
    n_ties = queued;
    if (!reference_libm || n_ties == 0) break;
    std::vector<TieRec> tr;
    if (int32_t e = read_ties(ctx, n_ties, tr)) return e;
    // (queued once per point: the fix kernels do not queue a tile's points again)
    const auto ref = libm_reference_keys(tr, c.res);
    n_moved = 0;
    for (size_t k = 0; k < tr.size(); k++) n_moved += ref[k].second != tr[k].key;
    if (n_moved == 0) break;
    std::vector<uint64_t> hv(2 * ref.size());
    for (size_t k = 0; k < ref.size(); k++) hv[2 * k] = (uint64_t)ref[k].first, hv[2 * k + 1] = ref[k].second;
    if (int32_t e = ensure_ovr(ctx, (int64_t)hv.size())) return e;
    HIP_TRY(hipMemcpy(ctx->ovr, hv.data(), hv.size() * 8, hipMemcpyHostToDevice));
    n_ovr = (int64_t)ref.size();
    std::vector<int64_t> pos(ref.size());
    for (size_t k = 0; k < ref.size(); k++) pos[k] = (int64_t)ref[k].first;
    if (int32_t e = launch_override_pass(ctx, c, timed, n_ovr, pos, h[5])) return e;
  }
  const int32_t is = c.is;
  const int64_t n = c.n, capacity = c.capacity;
  if (out_n_pairs) *out_n_pairs = (int64_t)h[0];
  if (stats) {
    stats->n_points = n;
    stats->n_pairs = (int64_t)h[0];
    stats->n_near_ties = n_ties;
    stats->n_candidates = (int64_t)h[3];
    stats->libm_overrides = (int32_t)n_moved;
    float ms = 0, ms2 = 0;
    if (timed) {
      hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
      if (n > 0) hipEventElapsedTime(&ms2, ctx->ev0, ctx->ev2);
    }
    stats->kernel_ms = ms;
    stats->stream_kernel_ms = ms2;
    stats->mixed_kernel_ms = stats->emit_kernel_ms = 0;
    if (!timed) {
      // (an asynchronous join records no events)
    } else if (ctx->last.split && n > 0) {
      float m3 = 0;
      hipEventElapsedTime(&m3, ctx->ev0, ctx->ev3);
      stats->mixed_kernel_ms = m3 - ms2;
      stats->emit_kernel_ms = ms - m3;
    } else if (ctx->last.binned && n > 0) {
      // ev0 | binning | ev3 | pip_binned_kernel | ev2 | fix, count, scan, emit | ev1
      float m3 = 0;
      hipEventElapsedTime(&m3, ctx->ev0, ctx->ev3);
      stats->mixed_kernel_ms = m3;
      stats->stream_kernel_ms = ms2 - m3;
      stats->emit_kernel_ms = ms - ms2;
    }
    stats->pipeline = ctx->last.split ? MGPU_PIPELINE_SPLIT
                      : ctx->last.binned ? MGPU_PIPELINE_BINNED : MGPU_PIPELINE_FUSED;
  }
  // pool records used (counters[5]) within the pool: every record is still in the
  // workspace, so a larger output can be written by mgpu_pip_join_fetch alone (the split
  // and binned pipelines keep their answers: always)
  ctx->last.total = (int64_t)h[0];
  ctx->last.pool_used = (int64_t)h[5];
  ctx->last.pool_ok = ctx->last.split || ctx->last.binned || (int64_t)h[5] <= ctx->last.pool;
  if (h[2]) {
    ctx->last.valid = false;
    if (is == MGPU_BNG) return fail(MGPU_E_NAN, "NaN coordinates are not supported. (%llu points)", (unsigned long long)h[2]);
    return fail(MGPU_E_INVALID_ARG, "Latitude or longitude were invalid. (%llu points)", (unsigned long long)h[2]);
  }
  if (c.count_pool < 0 && (int64_t)h[0] > capacity)
    return fail(MGPU_E_CAPACITY, "%lld pairs do not fit capacity %lld", (long long)h[0], (long long)capacity);
  return MGPU_OK;
}

static int32_t pip_join_sync(mgpu_ctx* ctx, const mgpu_chips* chips, int32_t is, int32_t res, const double* x,
                             const double* y, const int64_t* point_id, int64_t point_id_base, int64_t n,
                             int64_t capacity, int64_t* out_n_pairs, int64_t* out_point_id, int32_t* out_polygon_id,
                             void* stream, mgpu_stats* stats, const uint8_t* valid, int64_t valid_off) {
  const JoinCall c{chips, is, res, x, y, point_id, point_id_base, n, capacity, out_point_id, out_polygon_id,
                   (hipStream_t)stream, valid, valid_off, nullptr};
  const bool reference_libm = is == MGPU_H3 && ctx && ctx->opt.h3_libm == MGPU_LIBM_REFERENCE;
  if (int32_t st = launch_call(ctx, c, true, 0, reference_libm)) return st;
  return settle_join(ctx, c, true, reference_libm, out_n_pairs, stats);
}

extern "C" {

int32_t mgpu_pip_join(mgpu_ctx* ctx, const mgpu_chips* chips, int32_t is, int32_t res, const double* x,
                      const double* y, const int64_t* point_id, int64_t point_id_base, int64_t n, int64_t capacity,
                      int64_t* out_n_pairs, int64_t* out_point_id, int32_t* out_polygon_id, void* stream,
                      mgpu_stats* stats) {
  return pip_join_sync(ctx, chips, is, res, x, y, point_id, point_id_base, n, capacity, out_n_pairs, out_point_id,
                       out_polygon_id, stream, stats, nullptr, 0);
}

// The asynchronous form: the same first launch as the synchronous call (H3 near-ties
// queued with the fast cell), nothing waits; mgpu_pip_join_finish settles it.
int32_t mgpu_pip_join_async(mgpu_ctx* ctx, const mgpu_chips* chips, int32_t is, int32_t res, const double* x,
                            const double* y, const int64_t* point_id, int64_t point_id_base, int64_t n,
                            int64_t capacity, int64_t* d_n_pairs, int64_t* out_point_id, int32_t* out_polygon_id,
                            void* stream) {
  const JoinCall c{chips, is, res, x, y, point_id, point_id_base, n, capacity, out_point_id, out_polygon_id,
                   (hipStream_t)stream, nullptr, 0, d_n_pairs};
  const bool reference_libm = is == MGPU_H3 && ctx && ctx->opt.h3_libm == MGPU_LIBM_REFERENCE;
  if (int32_t st = launch_call(ctx, c, false, 0, reference_libm)) return st;
  ctx->last.async_pending = true;
  ctx->last.d_n_pairs = d_n_pairs;
  return MGPU_OK;
}

int32_t mgpu_pip_join_finish(mgpu_ctx* ctx, int64_t* out_n_pairs, mgpu_stats* stats) {
  if (!ctx) return fail(MGPU_E_INVALID_ARG, "ctx is NULL");
  auto& L = ctx->last;
  if (!L.valid || !L.async_pending)
    return fail(MGPU_E_INVALID_ARG, "pip_join_finish: no asynchronous join pending on this context");
  if (int32_t st = set_device(ctx->device)) return st;
  const JoinCall c{L.chips, L.is, L.res, L.x, L.y, L.point_id, L.id_base, L.n, L.capacity, L.out_point, L.out_poly,
                   (hipStream_t)L.stream, nullptr, 0, L.d_n_pairs};
  const bool reference_libm = L.tie_host != 0;
  L.async_pending = false;
  return settle_join(ctx, c, false, reference_libm, out_n_pairs, stats);
}

int32_t mgpu_pip_join_fetch(mgpu_ctx* ctx, int64_t capacity, int64_t* out_n_pairs, int64_t* out_point_id,
                            int32_t* out_polygon_id, void* stream) {
  if (!ctx) return fail(MGPU_E_INVALID_ARG, "ctx is NULL");
  auto& L = ctx->last;
  if (!L.valid || L.total < 0) return fail(MGPU_E_INVALID_ARG, "pip_join_fetch: no completed join on this context");
  if (out_n_pairs) *out_n_pairs = L.total;
  if (capacity < L.total)
    return fail(MGPU_E_CAPACITY, "%lld pairs do not fit capacity %lld", (long long)L.total, (long long)capacity);
  if (L.total > 0 && (!out_point_id || !out_polygon_id)) return fail(MGPU_E_INVALID_ARG, "bad output arrays");
  if (int32_t st = set_device(ctx->device)) return st;
  hipStream_t s = (hipStream_t)stream;
  if (!L.pool_ok) {
    // the overflow pool had dropped records: redo the join with a pool that holds them
    const auto c = L;
    int64_t cnt = 0;
    return pip_join_sync(ctx, c.chips, c.is, c.res, c.x, c.y, c.point_id, c.id_base, c.n, capacity,
                         out_n_pairs ? out_n_pairs : &cnt, out_point_id, out_polygon_id, stream, nullptr, c.pts_valid,
                         c.pts_valid_off);
  }
  if (L.binned) {
    mgpu::BinArgs ba = L.bargs;
    ba.s.capacity = capacity;
    ba.s.out_point = out_point_id;
    ba.s.out_poly = out_polygon_id;
    HIP_TRY(mgpu::launch_bin_emit(ba, s));
    HIP_TRY(hipStreamSynchronize(s));
    return MGPU_OK;
  }
  if (L.split) {
    mgpu::SplitArgs sa = L.sargs;
    sa.capacity = capacity;
    sa.out_point = out_point_id;
    sa.out_poly = out_polygon_id;
    HIP_TRY(mgpu::launch_split_emit(L.is, sa, s));
    HIP_TRY(hipStreamSynchronize(s));
    return MGPU_OK;
  }
  mgpu::EmitArgs e = L.emit;
  e.capacity = capacity;
  e.out_point = out_point_id;
  e.out_poly = out_polygon_id;
  HIP_TRY(mgpu::launch_emit(e, L.n_tiles, s));
  HIP_TRY(hipStreamSynchronize(s));
  return MGPU_OK;
}

int32_t mgpu_chips_polygons(const mgpu_chips* chips, int32_t* out_ids, int64_t cap, int64_t* out_n) {
  if (!chips || !out_n || cap < 0) return fail(MGPU_E_INVALID_ARG, "bad arguments");
  const PolySlotsDev* ps = nullptr;
  if (int32_t st = ensure_poly_slots(chips, &ps)) return st;
  const int64_t P = (int64_t)ps->ids.size();
  *out_n = P;
  if (P > cap || (P > 0 && !out_ids))
    return fail(MGPU_E_CAPACITY, "%lld polygons, capacity %lld", (long long)P, (long long)(out_ids ? cap : 0));
  if (P) memcpy(out_ids, ps->ids.data(), (size_t)P * 4);
  return MGPU_OK;
}

// mgpu_pip_join in count mode (join_impl: nothing that writes pairs is launched), settled
// as the pair join is -- near-tie queue, host libm pass, override rerun -- then one
// aggregation launch over what the join left in device memory (kernels.h CountArgs).
// Aggregating only after settle_join keeps reruns free of un-counting, and a failing call
// never touches count / sum.  The fused pipeline's overflow pool has no capacity to size
// it: n records first, and one rerun with the size the first run asked for.
int32_t mgpu_pip_join_count(mgpu_ctx* ctx, const mgpu_chips* chips, int32_t is, int32_t res, const double* x,
                            const double* y, const int64_t* weight, int64_t n, int64_t n_slots, int64_t* count,
                            int64_t* sum, int32_t accumulate, void* stream, mgpu_stats* stats) {
  if (!ctx || !chips) return fail(MGPU_E_INVALID_ARG, "ctx/chips is NULL");
  if ((weight && !sum) || (sum && !weight && n > 0))  // (an empty batch's weight column may be NULL)
    return fail(MGPU_E_INVALID_ARG, "pip_join_count: weight and sum go together (both or neither)");
  const PolySlotsDev* ps = nullptr;
  if (int32_t st = ensure_poly_slots(chips, &ps)) return st;
  const int64_t P = (int64_t)ps->ids.size();
  if (n_slots != P)
    return fail(MGPU_E_INVALID_ARG, "pip_join_count: n_slots %lld, the chip table has %lld polygons", (long long)n_slots,
                (long long)P);
  if (P > 0 && !count) return fail(MGPU_E_INVALID_ARG, "pip_join_count: count is NULL");
  const hipStream_t s = (hipStream_t)stream;
  JoinCall c{chips, is, res, x, y, nullptr, 0, n, 0, nullptr, nullptr, s, nullptr, 0, nullptr, std::max<int64_t>(n, 0)};
  const bool reference_libm = is == MGPU_H3 && ctx->opt.h3_libm == MGPU_LIBM_REFERENCE;
  int64_t pairs = 0;
  if (int32_t st = launch_call(ctx, c, true, 0, reference_libm)) return st;
  if (int32_t st = settle_join(ctx, c, true, reference_libm, &pairs, stats)) return st;
  auto& L = ctx->last;
  if (!L.pool_ok) {
    c.count_pool = L.pool_used;
    if (int32_t st = launch_call(ctx, c, true, 0, reference_libm)) return st;
    if (int32_t st = settle_join(ctx, c, true, reference_libm, &pairs, stats)) return st;
    if (!L.pool_ok)
      return fail(MGPU_E_INTERNAL, "pip_join_count: the overflow pool of %lld records is short again (%lld asked for)",
                  (long long)L.pool, (long long)L.pool_used);
  }
  mgpu::CountArgs ca{};
  ca.ids = ps->d_ids;
  ca.n_slots = (uint32_t)P;
  ca.chip_slot = ps->d_chip_slot;
  ca.dense = ps->d_dense;
  ca.min_id = P ? ps->ids.front() : 0;
  ca.contiguous = (P > 0 && (int64_t)ps->ids.back() - ps->ids.front() + 1 == P) ? 1u : 0u;
  // LDS histograms hold u32 counts: only while no slot of a workgroup can pass 2^32
  ca.lds_slots = (P > 0 && P <= ctx->opt.count_lds_slots && pairs < ((int64_t)1 << 32)) ? (uint32_t)P : 0u;
  // more polygons than LDS slots: an LDS hash table per workgroup in front of the global
  // atomics (device-scope atomics run at the memory side: C3's 1.25e8 took 6.7 ms)
  ca.hash_slots = (!ca.lds_slots && ctx->opt.count_lds_slots > 0 && P > 0 && pairs < ((int64_t)1 << 32))
                      ? mgpu::kCountHash : 0u;
  const int64_t look_n = ca.dense ? (int64_t)ps->ids.back() - ps->ids.front() + 1 : P;
  ca.stage_n = (look_n <= mgpu::kCountStageMax && !ca.hash_slots && !ca.contiguous) ? (uint32_t)look_n : 0u;
  ca.max_groups = (uint32_t)ctx->opt.count_groups;
  ca.weight = weight;
  ca.count = (unsigned long long*)count;
  ca.sum = (unsigned long long*)sum;
  ca.dropped = (uint32_t*)((unsigned long long*)ctx->ws + kWsCountDropped);
  if (!accumulate && P > 0) {
    HIP_TRY(hipMemsetAsync(count, 0, (size_t)P * 8, s));
    if (sum) HIP_TRY(hipMemsetAsync(sum, 0, (size_t)P * 8, s));
  }
  HIP_TRY(hipEventRecord(ctx->ev2, s));
  if (L.split)
    HIP_TRY(mgpu::launch_split_count(is, L.sargs, ca, s));
  else if (L.binned)
    HIP_TRY(mgpu::launch_bin_count(L.bargs, ca, s));
  else
    HIP_TRY(mgpu::launch_tile_count(L.emit, L.n_tiles, ca, s));
  HIP_TRY(hipEventRecord(ctx->ev3, s));
  HIP_TRY(hipMemcpyAsync(ctx->pin, ca.dropped, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(stream_wait(ctx, s));
  if (ctx->pin[0]) return fail(MGPU_E_INTERNAL, "pip_join_count: a tile's records were dropped by the overflow pool");
  if (stats) {
    float ms = 0;
    hipEventElapsedTime(&ms, ctx->ev2, ctx->ev3);
    stats->emit_kernel_ms = ms;
    stats->kernel_ms += ms;
  }
  return MGPU_OK;
}

// As mgpu_pip_join_count: the join in count mode, settled as the pair join is, the fused
// pipeline's one rerun with the pool it asked for -- then one lookup launch over what the
// join left in device memory (kernels.h LookupArgs), which writes every element of the
// outputs once.  Writing only after settle_join keeps a failing call's outputs untouched.
int32_t mgpu_pip_join_lookup(mgpu_ctx* ctx, const mgpu_chips* chips, int32_t is, int32_t res, const double* x,
                             const double* y, int64_t n, int32_t null_id, int32_t* out_polygon, int32_t* out_matches,
                             void* stream, mgpu_stats* stats) {
  if (!ctx || !chips) return fail(MGPU_E_INVALID_ARG, "ctx/chips is NULL");
  if (n > 0 && !out_polygon) return fail(MGPU_E_INVALID_ARG, "pip_join_lookup: out_polygon is NULL");
  const hipStream_t s = (hipStream_t)stream;
  JoinCall c{chips, is, res, x, y, nullptr, 0, n, 0, nullptr, nullptr, s, nullptr, 0, nullptr, std::max<int64_t>(n, 0)};
  const bool reference_libm = is == MGPU_H3 && ctx->opt.h3_libm == MGPU_LIBM_REFERENCE;
  int64_t pairs = 0;
  if (int32_t st = launch_call(ctx, c, true, 0, reference_libm)) return st;
  if (int32_t st = settle_join(ctx, c, true, reference_libm, &pairs, stats)) return st;
  auto& L = ctx->last;
  if (!L.pool_ok) {
    c.count_pool = L.pool_used;
    if (int32_t st = launch_call(ctx, c, true, 0, reference_libm)) return st;
    if (int32_t st = settle_join(ctx, c, true, reference_libm, &pairs, stats)) return st;
    if (!L.pool_ok)
      return fail(MGPU_E_INTERNAL, "pip_join_lookup: the overflow pool of %lld records is short again (%lld asked for)",
                  (long long)L.pool, (long long)L.pool_used);
  }
  if (n == 0) return MGPU_OK;
  mgpu::LookupArgs la{out_polygon, out_matches, null_id, (uint32_t*)((unsigned long long*)ctx->ws + kWsCountDropped)};
  HIP_TRY(hipEventRecord(ctx->ev2, s));
  if (L.split)
    HIP_TRY(mgpu::launch_split_lookup(is, L.sargs, la, s));
  else if (L.binned)
    HIP_TRY(mgpu::launch_bin_lookup(L.bargs, la, s));
  else
    HIP_TRY(mgpu::launch_tile_lookup(L.emit, n, L.n_tiles, la, s));
  HIP_TRY(hipEventRecord(ctx->ev3, s));
  const bool fused = !L.split && !L.binned;  // (only tile_lookup_kernel sets the flag)
  if (fused) HIP_TRY(hipMemcpyAsync(ctx->pin, la.dropped, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(stream_wait(ctx, s));
  if (fused && ctx->pin[0])
    return fail(MGPU_E_INTERNAL, "pip_join_lookup: a tile's records were dropped by the overflow pool");
  if (stats) {
    float ms = 0;
    hipEventElapsedTime(&ms, ctx->ev2, ctx->ev3);
    stats->emit_kernel_ms = ms;
    stats->kernel_ms += ms;
  }
  return MGPU_OK;
}

int32_t mgpu_test_poly_slots_host(const int32_t* polygon_id, int64_t n, int32_t* out_ids, int64_t* out_n,
                                  uint32_t* out_slot_of_row) {
  if (n < 0 || !out_n || (n > 0 && (!polygon_id || !out_ids || !out_slot_of_row)))
    return fail(MGPU_E_INVALID_ARG, "bad arguments");
  const mgpu::PolySlots hs = mgpu::poly_slots(polygon_id, n);
  *out_n = (int64_t)hs.ids.size();
  if (n) {
    memcpy(out_ids, hs.ids.data(), hs.ids.size() * 4);
    memcpy(out_slot_of_row, hs.slot_of_row.data(), (size_t)n * 4);
  }
  return MGPU_OK;
}

int32_t mgpu_pip_join_host(mgpu_ctx* ctx, const mgpu_chips* chips, int32_t is, int32_t res, const double* x,
                           const double* y, const int64_t* point_id, int64_t n, int64_t capacity, int64_t* out_n_pairs,
                           int64_t* out_point_id, int32_t* out_polygon_id) {
  if (!ctx) return fail(MGPU_E_INVALID_ARG, "ctx is NULL");
  if (int32_t st = set_device(ctx->device)) return st;
  double *dx = nullptr, *dy = nullptr;
  int64_t *dpid = nullptr, *dop = nullptr;
  int32_t* dpo = nullptr;
  size_t nb = (size_t)std::max<int64_t>(n, 1) * 8, cb = (size_t)std::max<int64_t>(capacity, 1);
  HIP_TRY(hipMalloc(&dx, nb));
  HIP_TRY(hipMalloc(&dy, nb));
  HIP_TRY(hipMalloc(&dop, cb * 8));
  HIP_TRY(hipMalloc(&dpo, cb * 4));
  if (n) {
    HIP_TRY(hipMemcpy(dx, x, n * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dy, y, n * 8, hipMemcpyHostToDevice));
  }
  if (point_id && n) {
    HIP_TRY(hipMalloc(&dpid, nb));
    HIP_TRY(hipMemcpy(dpid, point_id, n * 8, hipMemcpyHostToDevice));
  }
  int64_t cnt = 0;
  int32_t st = mgpu_pip_join(ctx, chips, is, res, dx, dy, dpid, 0, n, capacity, &cnt, dop, dpo, nullptr, nullptr);
  if (out_n_pairs) *out_n_pairs = cnt;
  if (st == MGPU_OK || st == MGPU_E_CAPACITY) {
    int64_t m = std::min(cnt, capacity);
    if (m > 0) {
      hipMemcpy(out_point_id, dop, m * 8, hipMemcpyDeviceToHost);
      hipMemcpy(out_polygon_id, dpo, m * 4, hipMemcpyDeviceToHost);
    }
  }
  hipFree(dx);
  hipFree(dy);
  hipFree(dop);
  hipFree(dpo);
  if (dpid) hipFree(dpid);
  return st;
}

}  // extern "C"

// ------------------------------------------------------------------ geometry columns, Arrow

int32_t ensure_scratch(mgpu_ctx* ctx, size_t bytes) {
  if (bytes <= ctx->scratch_bytes) return MGPU_OK;
  if (ctx->scratch) HIP_TRY(hipFree(ctx->scratch));
  ctx->scratch = nullptr;
  ctx->scratch_bytes = 0;
  HIP_TRY(hipMalloc(&ctx->scratch, bytes));
  ctx->scratch_bytes = bytes;
  return MGPU_OK;
}

// decode into (x, y) and check the decode counters
// the decode kernels' counters -> the reference's exception classes
static int32_t decode_status(mgpu_ctx* ctx, int32_t format, hipStream_t s) {
  static const char* names[] = {"WKB", "WKT", "hex WKB", "GeoJSON", "internal geometry"};
  unsigned long long h[8] = {0};
  HIP_TRY(hipMemcpyAsync(h, ctx->ws, sizeof h, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const char* name = names[format >= 0 && format <= 4 ? format : 0];
  if (h[4]) return fail(MGPU_E_WKB, "%llu rows are not well-formed %s", h[4], name);
  if (h[5])
    return fail(MGPU_E_UNSUPPORTED, "%llu %s rows are of a geometry type whose centroid is not built for this format",
                h[5], name);
  if (h[6]) return fail(MGPU_E_EMPTY, "getX called on empty Point (%llu rows: empty geometries)", h[6]);
  return MGPU_OK;
}

static int32_t decode_points(mgpu_ctx* ctx, int32_t format, const uint8_t* data, const void* offsets, int off32,
                             const uint8_t* valid, int64_t voff, int64_t n, double* x, double* y, hipStream_t s) {
  if (format < MGPU_GEOM_WKB || format > MGPU_GEOM_GEOJSON) return fail(MGPU_E_INVALID_ARG, "geometry format %d", format);
  if (n < 0 || (n > 0 && (!data || !offsets || !x || !y))) return fail(MGPU_E_INVALID_ARG, "bad geometry arrays");
  if (int32_t st = ensure_ws(ctx, 1)) return st;
  auto* counters = (unsigned long long*)ctx->ws;
  HIP_TRY(hipMemsetAsync(counters, 0, kWsCounters, s));
  HIP_TRY(mgpu::launch_decode_points(format, data, offsets, off32, valid, voff, n, x, y, counters, s));
  return decode_status(ctx, format, s);
}

extern "C" {

int32_t mgpu_points_from_geometry(mgpu_ctx* ctx, int32_t format, const uint8_t* data, const int64_t* offsets,
                                  const uint8_t* valid, int64_t valid_offset, int64_t n, double* out_x, double* out_y,
                                  void* stream) {
  if (!ctx) return fail(MGPU_E_INVALID_ARG, "ctx is NULL");
  if (int32_t st = set_device(ctx->device)) return st;
  return decode_points(ctx, format, data, offsets, 0, valid, valid_offset, n, out_x, out_y, (hipStream_t)stream);
}

}  // extern "C"

static int32_t geometry_cells(mgpu_ctx* ctx, int32_t is, int32_t res, int32_t format, const uint8_t* data,
                              const void* offsets, int off32, const uint8_t* valid, int64_t voff, int64_t n,
                              int64_t* out_cell, uint8_t* out_valid, hipStream_t s, mgpu_stats* stats) {
  if (!ctx) return fail(MGPU_E_INVALID_ARG, "ctx is NULL");
  if (int32_t r = check_res(is, res)) return r;
  if (n < 0 || (n > 0 && !out_cell)) return fail(MGPU_E_INVALID_ARG, "bad output array");
  if (int32_t st = set_device(ctx->device)) return st;
  if (int32_t st = ensure_scratch(ctx, (size_t)std::max<int64_t>(n, 1) * 16)) return st;
  double* x = (double*)ctx->scratch;
  double* y = x + std::max<int64_t>(n, 1);
  if (int32_t st = decode_points(ctx, format, data, offsets, off32, valid, voff, n, x, y, s)) return st;
  if (int32_t st = cells_impl(ctx, is, res, x, y, n, out_cell, s, valid, voff, stats)) return st;
  if (out_valid) {
    HIP_TRY(mgpu::launch_valid_and(valid, voff, nullptr, 0, n, out_valid, s));
    HIP_TRY(stream_wait(ctx, s));
  }
  return MGPU_OK;
}

// an Arrow array on this context's GPU with the given format; *data = its values (offset
// applied), *valid / *voff = its validity bitmap (null: no nulls)
static int32_t arrow_column(mgpu_ctx* ctx, const ArrowDeviceArray* a, size_t elem, const void** data,
                            const uint8_t** valid, int64_t* voff, const char* what) {
  if (!a) return fail(MGPU_E_INVALID_ARG, "%s: NULL array", what);
  if (a->device_type != ARROW_DEVICE_ROCM || a->device_id != ctx->device)
    return fail(MGPU_E_INVALID_ARG, "%s: not on this context's GPU (device type %d, id %lld)", what, a->device_type,
                (long long)a->device_id);
  if (a->array.n_buffers < 2 || !a->array.buffers || a->array.length < 0 || a->array.offset < 0)
    return fail(MGPU_E_INVALID_ARG, "%s: not a primitive Arrow array", what);
  if (a->sync_event) HIP_TRY(hipEventSynchronize((hipEvent_t)a->sync_event));
  *data = (const uint8_t*)a->array.buffers[1] + (size_t)a->array.offset * elem;
  *valid = a->array.null_count != 0 ? (const uint8_t*)a->array.buffers[0] : nullptr;
  *voff = a->array.offset;
  return MGPU_OK;
}

extern "C" {

int32_t mgpu_geometry_to_cells(mgpu_ctx* ctx, int32_t index_system, int32_t res, int32_t format, const uint8_t* data,
                               const int64_t* offsets, const uint8_t* valid, int64_t valid_offset, int64_t n,
                               int64_t* out_cell, uint8_t* out_valid, void* stream, mgpu_stats* stats) {
  return geometry_cells(ctx, index_system, res, format, data, offsets, 0, valid, valid_offset, n, out_cell, out_valid,
                        (hipStream_t)stream, stats);
}

int32_t mgpu_internal_geometry_to_cells(mgpu_ctx* ctx, int32_t index_system, int32_t res, int64_t n,
                                        const int32_t* type_id, const int64_t* row_part, const int64_t* part_ring,
                                        const int64_t* ring_off, const double* xy, const uint8_t* valid,
                                        int64_t valid_offset, int64_t* out_cell, uint8_t* out_valid, void* stream,
                                        mgpu_stats* stats) {
  if (!ctx) return fail(MGPU_E_INVALID_ARG, "ctx is NULL");
  if (int32_t r = check_res(index_system, res)) return r;
  if (n < 0 || (n > 0 && (!out_cell || !type_id || !row_part || !part_ring || !ring_off || !xy)))
    return fail(MGPU_E_INVALID_ARG, "bad internal geometry arrays");
  if (int32_t st = set_device(ctx->device)) return st;
  hipStream_t s = (hipStream_t)stream;
  if (int32_t st = ensure_ws(ctx, 1)) return st;
  if (int32_t st = ensure_scratch(ctx, (size_t)std::max<int64_t>(n, 1) * 16)) return st;
  double* x = (double*)ctx->scratch;
  double* y = x + std::max<int64_t>(n, 1);
  HIP_TRY(hipMemsetAsync(ctx->ws, 0, kWsCounters, s));
  HIP_TRY(mgpu::launch_decode_internal(type_id, row_part, part_ring, ring_off, xy, valid, valid_offset, n, x, y,
                                       (unsigned long long*)ctx->ws, s));
  if (int32_t st = decode_status(ctx, 4, s)) return st;
  if (int32_t st = cells_impl(ctx, index_system, res, x, y, n, out_cell, s, valid, valid_offset, stats)) return st;
  if (out_valid) {
    HIP_TRY(mgpu::launch_valid_and(valid, valid_offset, nullptr, 0, n, out_valid, s));
    HIP_TRY(stream_wait(ctx, s));
  }
  return MGPU_OK;
}

int32_t mgpu_geometry_to_cells_arrow(mgpu_ctx* ctx, int32_t index_system, int32_t res,
                                     const struct ArrowDeviceArray* geom, const struct ArrowSchema* schema,
                                     int64_t* out_cell, uint8_t* out_valid, void* stream) {
  if (!ctx || !geom || !schema || !schema->format) return fail(MGPU_E_INVALID_ARG, "NULL argument");
  const char f = schema->format[0];
  if (!((f == 'z' || f == 'Z' || f == 'u' || f == 'U') && schema->format[1] == 0))
    return fail(MGPU_E_INVALID_ARG, "geometry column format '%s': binary (WKB) or utf8 (WKT) expected", schema->format);
  if (geom->device_type != ARROW_DEVICE_ROCM || geom->device_id != ctx->device)
    return fail(MGPU_E_INVALID_ARG, "geometry column not on this context's GPU");
  if (geom->array.n_buffers < 3 || !geom->array.buffers) return fail(MGPU_E_INVALID_ARG, "not a binary Arrow array");
  if (geom->sync_event) HIP_TRY(hipEventSynchronize((hipEvent_t)geom->sync_event));
  const bool o32 = f == 'z' || f == 'u';
  const uint8_t* offs = (const uint8_t*)geom->array.buffers[1] + (size_t)geom->array.offset * (o32 ? 4 : 8);
  const uint8_t* valid = geom->array.null_count != 0 ? (const uint8_t*)geom->array.buffers[0] : nullptr;
  return geometry_cells(ctx, index_system, res, (f == 'z' || f == 'Z') ? MGPU_GEOM_WKB : MGPU_GEOM_WKT,
                        (const uint8_t*)geom->array.buffers[2], offs, o32 ? 1 : 0, valid, geom->array.offset,
                        geom->array.length, out_cell, out_valid, (hipStream_t)stream, nullptr);
}

int32_t mgpu_pip_join_arrow(mgpu_ctx* ctx, const mgpu_chips* chips, int32_t index_system, int32_t res,
                            const struct ArrowDeviceArray* x, const struct ArrowDeviceArray* y,
                            const struct ArrowDeviceArray* point_id, int64_t capacity, int64_t* out_n_pairs,
                            int64_t* out_point_id, int32_t* out_polygon_id, void* stream, mgpu_stats* stats) {
  if (!ctx) return fail(MGPU_E_INVALID_ARG, "ctx is NULL");
  if (int32_t st = set_device(ctx->device)) return st;
  hipStream_t s = (hipStream_t)stream;
  const void *xd, *yd, *pd = nullptr;
  const uint8_t *xv, *yv, *pv = nullptr;
  int64_t xo, yo, po = 0;
  if (int32_t st = arrow_column(ctx, x, 8, &xd, &xv, &xo, "x")) return st;
  if (int32_t st = arrow_column(ctx, y, 8, &yd, &yv, &yo, "y")) return st;
  const int64_t n = x->array.length;
  if (y->array.length != n) return fail(MGPU_E_INVALID_ARG, "x and y differ in length");
  if (point_id) {
    if (int32_t st = arrow_column(ctx, point_id, 8, &pd, &pv, &po, "point_id")) return st;
    if (point_id->array.length != n) return fail(MGPU_E_INVALID_ARG, "point_id and x differ in length");
    if (pv) return fail(MGPU_E_INVALID_ARG, "point_id has nulls");
  }
  const uint8_t* valid = nullptr;
  int64_t voff = 0;
  if (xv && yv) {
    if (int32_t st = ensure_scratch(ctx, (size_t)(n + 7) / 8 + 1)) return st;
    HIP_TRY(mgpu::launch_valid_and(xv, xo, yv, yo, n, (uint8_t*)ctx->scratch, s));
    valid = (const uint8_t*)ctx->scratch;
  } else if (xv || yv) {
    valid = xv ? xv : yv;
    voff = xv ? xo : yo;
  }
  return pip_join_sync(ctx, chips, index_system, res, (const double*)xd, (const double*)yd, (const int64_t*)pd,
                       point_id ? 0 : x->array.offset, n, capacity, out_n_pairs, out_point_id, out_polygon_id, stream, stats, valid,
                       voff);
}

int32_t mgpu_test_parse_number(const char* s, int32_t len, double* out) {
  return mgpu::dec::parse_number(s, len, out);
}

int32_t mgpu_test_h3_elementary_host(int32_t fn, const double* a, const double* b, int64_t n, double* out) {
  namespace X = mgpu::exact;
  for (int64_t i = 0; i < n; ++i) {
    const double x = a[i], y = b ? b[i] : 0.0;
    double r = 0.0;
    switch (fn) {
      case 0: r = X::cr_sin(x); break;
      case 1: r = X::cr_cos(x); break;
      case 2: r = X::cr_tan(x); break;
      case 3: r = X::cr_acos(x); break;
      case 4: r = X::cr_atan2(x, y); break;
      // the integer emulation the device runs (not the host's x87 unit)
      case 5: r = X::x80_to_double(X::x80_add(X::x80_from_double(x), X::kX2Pi)); break;
      case 6: r = X::x80_to_double(X::x80_add(X::x80_from_double(x), X::x80_neg(X::kX2Pi))); break;
      case 7: r = X::x80_to_double(X::x80_mul(X::x80_from_double(x), X::kXSqrt7)); break;
      case 8: r = X::x80_to_double(X::x80_div(X::x80_from_double(x), X::kXSin60)); break;
      case 9: r = X::x80_to_double(X::x80_add(X::x80_from_double(x), X::x80_neg(X::kXAp7Rot))); break;
      case 10: r = X::x80_to_double(X::x80_div(X::x80_from_double(x), X::kXSqrt7)); break;
      case 11: r = X::x80_to_double(X::x80_add(X::x80_from_double(x), X::kXAp7Rot)); break;
      case 12: r = X::x80_cmp(X::x80_from_double(x), X::kXEpsilon) < 0 ? 1.0 : 0.0; break;
      case 13: r = X::x80_cmp(X::x80_from_double(x), X::kX2Pi) >= 0 ? 1.0 : 0.0; break;
      // the cell-geometry route's additions (no oracle code: checked against asinl / atanl)
      case 14: r = X::cr_asin(x); break;
      case 15: r = X::cr_atan(x); break;
      default: return MGPU_E_INVALID_ARG;
    }
    out[i] = r;
  }
  return MGPU_OK;
}

int32_t mgpu_test_h3_route_host(const double* lon, const double* lat, int64_t n, int32_t res, int64_t* out_cell) {
  if (res < 0 || res > 15) return MGPU_E_RESOLUTION;
  mgpu::parallel_for(n, 4096, [&](int64_t b, int64_t e, int) {
    for (int64_t i = b; i < e; ++i) {
      bool tie;
      out_cell[i] = (int64_t)mgpu::h3::point_to_cell(lon[i], lat[i], res, &tie);
    }
  });
  return MGPU_OK;
}

int32_t mgpu_test_h3_glibc_host(const double* lon, const double* lat, int64_t n, int32_t res, int64_t* out_cell) {
  if (res < 0 || res > 15) return MGPU_E_RESOLUTION;
  mgpu::parallel_for(n, 4096, [&](int64_t b, int64_t e, int) {
    for (int64_t i = b; i < e; ++i) out_cell[i] = (int64_t)mgpu::h3glibc::point_to_cell(lon[i], lat[i], res);
  });
  return MGPU_OK;
}

int32_t mgpu_test_decode_point(int32_t format, const uint8_t* data, int64_t len, double* x, double* y) {
  switch (format) {
    case MGPU_GEOM_WKB: return mgpu::geom::wkb_centroid(data, len, x, y);
    case MGPU_GEOM_WKT: return mgpu::geom::wkt_centroid((const char*)data, len, x, y);
    case MGPU_GEOM_HEX: return mgpu::geom::hex_centroid((const char*)data, len, x, y);
    case MGPU_GEOM_GEOJSON: return mgpu::geom::json_centroid((const char*)data, len, x, y);
  }
  return mgpu::geom::kDecUnsupported;
}

int32_t mgpu_test_join_counters(mgpu_ctx* ctx, uint64_t* out16) {
  if (!ctx || !out16) return fail(MGPU_E_INVALID_ARG, "bad arguments");
  memset(out16, 0, 16 * 8);
  if (!ctx->ws) return MGPU_OK;
  if (int32_t st = set_device(ctx->device)) return st;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out16, ctx->ws, 16 * 8, hipMemcpyDeviceToHost));
  return MGPU_OK;
}

int32_t mgpu_test_fine_table(const mgpu_chips* chips, int64_t* dims, double* geom, uint16_t* out_classes,
                             uint8_t* out_fine) {
  if (!chips || !dims) return fail(MGPU_E_INVALID_ARG, "bad arguments");
  if (int32_t st = set_device(chips->device)) return st;
  const mgpu::ChipTableView& v = chips->view;
  const bool lonlat = v.raster_mode == mgpu::kRasterLonLat;
  const int64_t d[7] = {lonlat ? v.raster_nx : 0, lonlat ? v.raster_ny : 0, v.fine_sx, v.fine_sy, v.fine_bnx, v.fine_bny,
                        v.raster_fine ? 1 : 0};
  memcpy(dims, d, sizeof d);
  if (geom) {
    const double g[8] = {v.raster_x0, v.raster_y0, v.raster_inv_dx, v.raster_inv_dy, v.bbox[0], v.bbox[1], v.bbox[2], v.bbox[3]};
    memcpy(geom, g, sizeof g);
  }
  if (out_classes && d[0] * d[1])
    HIP_TRY(hipMemcpy(out_classes, v.raster, (size_t)(d[0] * d[1]) * 2, hipMemcpyDeviceToHost));
  if (out_fine && v.raster_fine)
    HIP_TRY(hipMemcpy(out_fine, v.raster_fine, (size_t)(d[4] * d[5]), hipMemcpyDeviceToHost));
  return MGPU_OK;
}

int32_t mgpu_test_internal_centroid(int64_t n, const int32_t* type_id, const int64_t* row_part, const int64_t* part_ring,
                                    const int64_t* ring_off, const double* xy, double* x, double* y, int32_t* status) {
  for (int64_t i = 0; i < n; i++)
    status[i] = mgpu::geom::internal_centroid(type_id[i], row_part[i], row_part[i + 1], part_ring, ring_off, xy, &x[i], &y[i]);
  return MGPU_OK;
}

}  // extern "C"

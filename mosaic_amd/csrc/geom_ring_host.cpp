// grid_geometrykring, the host side (geom_ring.h has the definition): the argument checks of
// both entries, the figures of the last call, and the kernels' host twin,
// mgpu_test_geometry_kring_host -- per geometry the records of geom_ring.h from the ring code of
// h3_ring.h / bng_core.h, a sort, and the ids whose lowest key kept member 1.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <iterator>
#include <vector>

#include "../../include/mosaic_gpu.h"
#include "bng_core.h"
#include "error.h"
#include "geom_ring.h"
#include "h3_ring.h"

namespace mgpu {
namespace geomring {

namespace {

thread_local int64_t g_last[8] = {0, 0, 0, 0, 0, 0, 0, 0};

// H3Core.kRing(h, k) as a set: the spiral, or H3's _kRingInternal where it meets a pentagon
bool h3_ring_set(uint64_t h, int k, std::vector<int64_t>* out) {
  const int64_t m = h3ring::max_kring(k);
  out->assign((size_t)m, 0);
  const int64_t n = h3ring::kring(h, k, out->data());
  if (n >= 0) {
    out->resize((size_t)n);
    return true;
  }
  std::vector<uint64_t> tab((size_t)m), stk((size_t)k + 2);
  std::vector<int32_t> dist((size_t)m);
  std::vector<int8_t> nxt((size_t)k + 2);
  if (!h3ring::kring_hash(h, k, tab.data(), dist.data(), stk.data(), nxt.data())) return false;
  out->clear();
  for (uint64_t c : tab)
    if (c) out->push_back((int64_t)c);
  return true;
}

// one cell's kRing / kLoop (any order); 0, or the status of a cell the index system does not have
int32_t cell_list(const char* what, int is, int64_t id, int k, bool loop, std::vector<int64_t>* out) {
  out->clear();
  if (is == MGPU_H3) {
    const uint64_t h = (uint64_t)id;
    if (!h3ring::valid_cell(h)) return set_error(MGPU_E_INVALID_ARG, "%s: %lld is not an H3 cell id", what, (long long)id);
    bool ok = true;
    if (!loop) {
      ok = h3_ring_set(h, k, out);
    } else {
      out->assign((size_t)std::max(1, 6 * k), 0);
      const int64_t n = h3ring::hex_ring(h, k, out->data());
      if (n >= 0) {
        out->resize((size_t)n);
      } else {  // Mosaic's kLoop where hexRing throws: kRing(k).toSet diff kRing(k - 1).toSet
        std::vector<int64_t> a, b;
        ok = h3_ring_set(h, k, &a) && h3_ring_set(h, k - 1, &b);
        std::sort(a.begin(), a.end());
        std::sort(b.begin(), b.end());
        out->clear();
        std::set_difference(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(*out));
        out->erase(std::unique(out->begin(), out->end()), out->end());
      }
    }
    if (!ok) return set_error(MGPU_E_INTERNAL, "%s: a pentagon walk overflowed its hash set (inconsistent tables)", what);
    return MGPU_OK;
  }
  // BNGIndexSystem.kRing / kLoop (BNGIndexSystem.scala:221-252): the cell, then loops 1..k;
  // a loop = pointToIndex of the 8j corners around the cell, kept when isValid
  int r, xl, yl;
  int32_t e, x, y;
  bool bad = !bng::cell_corner(id, &r, &e, &x, &y, &xl, &yl);
  if (!bad && !loop) out->push_back(id);
  for (int j = loop ? k : 1; j <= k && !bad; j++)
    for (int c = 0; c < 8 * j && !bad; c++) {
      int32_t px, py;
      bng::kloop_xy(x, y, e, j, c, &px, &py);
      int64_t nb = 0;
      bng::point_to_cell((double)px, (double)py, r, &nb);
      const int v = bng::valid_state(nb);
      bad = v < 0;
      if (v > 0) out->push_back(nb);
    }
  if (bad)
    return set_error(MGPU_E_INVALID_ARG, "%s: %lld is not a BNG cell or reaches ids BNGIndexSystem.isValid cannot parse", what,
                     (long long)id);
  return MGPU_OK;
}

}  // namespace

void note_last(const int64_t v[8]) {
  for (int i = 0; i < 8; i++) g_last[i] = v[i];
}

int32_t check_args(const char* what, int32_t index_system, int64_t n_geoms, const void* row_off, const void* cell,
                   const void* is_core, int32_t k, int32_t loop_only, const void* out_cells, int64_t capacity,
                   const void* out_offsets, const void* out_total) {
  (void)cell, (void)is_core;  // (either may be NULL when there are no rows: checked once row_off is read)
  if (index_system != MGPU_H3 && index_system != MGPU_BNG)
    return set_error(MGPU_E_INVALID_ARG, "%s: unknown index system %d (0 = H3, 1 = BNG)", what, index_system);
  if (n_geoms < 0 || !row_off) return set_error(MGPU_E_INVALID_ARG, "%s: bad geometry offsets", what);
  if (loop_only != 0 && loop_only != 1) return set_error(MGPU_E_INVALID_ARG, "%s: loop_only must be 0 or 1", what);
  if (k < (loop_only ? 1 : 0) || k > kMaxK)
    return set_error(MGPU_E_INVALID_ARG, "%s: k must be in [%d, %d]", what, loop_only ? 1 : 0, kMaxK);
  if (!out_offsets || !out_total || capacity < 0 || (capacity > 0 && !out_cells))
    return set_error(MGPU_E_INVALID_ARG, "%s: bad output buffers", what);
  return MGPU_OK;
}

}  // namespace geomring
}  // namespace mgpu

extern "C" {

int32_t mgpu_test_geometry_kring_host(int32_t index_system, int64_t n_geoms, const int64_t* row_off, const int64_t* cell,
                                      const uint8_t* is_core, int32_t k, int32_t loop_only, int64_t* out_cells,
                                      int64_t capacity, int64_t* out_offsets, int64_t* out_total) {
  namespace GR = mgpu::geomring;
  const char* what = "geometry_kring_host";
  if (int32_t st = GR::check_args(what, index_system, n_geoms, row_off, cell, is_core, k, loop_only, out_cells, capacity,
                                  out_offsets, out_total))
    return st;
  for (int64_t g = 0; g < n_geoms; g++)
    if (row_off[g] < 0 || row_off[g + 1] < row_off[g])
      return mgpu::set_error(MGPU_E_INVALID_ARG, "%s: row_off must start at or above 0 and not decrease", what);
  if (n_geoms && row_off[n_geoms] > row_off[0] && (!cell || !is_core))
    return mgpu::set_error(MGPU_E_INVALID_ARG, "%s: cell / is_core is NULL", what);
  int64_t last[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<unsigned long long> keys;
  std::vector<int64_t> list;
  int64_t total = 0;
  out_offsets[0] = 0;
  *out_total = 0;
  for (int64_t g = 0; g < n_geoms; g++) {
    keys.clear();
    for (int64_t r = row_off[g]; r < row_off[g + 1]; r++) {
      const int64_t id = cell[r];
      if (is_core[r]) {
        if (id < 0 || id >= GR::kIdLimit)
          return mgpu::set_error(MGPU_E_INVALID_ARG, "%s: core row %lld holds %lld, no cell id", what, (long long)r, (long long)id);
        keys.push_back(((unsigned long long)id << 1) | (loop_only ? 0ull : 1ull));
        continue;
      }
      last[GR::kLastBorder]++;
      if (int32_t st = GR::cell_list(what, index_system, id, k, loop_only != 0, &list)) return st;
      for (int64_t c : list) keys.push_back(((unsigned long long)c << 1) | 1ull);
      if (loop_only) {
        if (int32_t st = GR::cell_list(what, index_system, id, k - 1, false, &list)) return st;
        for (int64_t c : list) keys.push_back((unsigned long long)c << 1);
      }
    }
    last[GR::kLastGenerated] += (int64_t)keys.size();
    std::sort(keys.begin(), keys.end());
    for (size_t i = 0; i < keys.size(); i++) {
      if (i > 0 && (keys[i] >> 1) == (keys[i - 1] >> 1)) continue;
      if (!(keys[i] & 1ull)) continue;
      if (total < capacity) out_cells[total] = (int64_t)(keys[i] >> 1);
      total++;
    }
    out_offsets[g + 1] = total;
  }
  last[GR::kLastReturned] = total;
  GR::note_last(last);
  *out_total = total;
  if (total > capacity)
    return mgpu::set_error(MGPU_E_CAPACITY, "%s: %lld cells needed, %lld given", what, (long long)total, (long long)capacity);
  return MGPU_OK;
}

int32_t mgpu_test_geometry_kring_last(int64_t* out8) {
  if (!out8) return mgpu::set_error(MGPU_E_INVALID_ARG, "geometry_kring_last: out8 is NULL");
  for (int i = 0; i < 8; i++) out8[i] = mgpu::geomring::g_last[i];
  return MGPU_OK;
}

}  // extern "C"

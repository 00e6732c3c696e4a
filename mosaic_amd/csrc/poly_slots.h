// The polygon slots of a chip table (mgpu_pip_join_count): the distinct polygon ids of
// chip_poly sorted ascending -- slot k holds ids[k] -- and each chip row's slot.  Host
// only; the ids are arbitrary int32 values (negative ones and INT32_MIN included).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace mgpu {

struct PolySlots {
  std::vector<int32_t> ids;           // ascending, distinct
  std::vector<uint32_t> slot_of_row;  // [n]: ids[slot_of_row[i]] == polygon_id[i]
};

inline PolySlots poly_slots(const int32_t* polygon_id, int64_t n) {
  PolySlots s;
  if (n <= 0) return s;
  s.ids.assign(polygon_id, polygon_id + n);
  std::sort(s.ids.begin(), s.ids.end());
  s.ids.erase(std::unique(s.ids.begin(), s.ids.end()), s.ids.end());
  s.slot_of_row.resize((size_t)n);
  for (int64_t i = 0; i < n; i++)
    s.slot_of_row[(size_t)i] =
        (uint32_t)(std::lower_bound(s.ids.begin(), s.ids.end(), polygon_id[i]) - s.ids.begin());
  return s;
}

// The dense id -> slot table over [min id, max id] is used when it is at most this many
// entries and at most 16 entries per polygon: 2^22 u32 = 16 MiB, a small fraction of the
// chip tables it serves, and sparse enough ids (ids scaled by 1000, INT32_MIN) fall back
// to the binary search of the sorted ids.
constexpr int64_t kDenseSlotMax = (int64_t)1 << 22;
inline bool poly_slots_dense(const std::vector<int32_t>& ids) {
  if (ids.empty()) return false;
  const int64_t range = (int64_t)ids.back() - (int64_t)ids.front() + 1;
  return range <= kDenseSlotMax && range <= 16 * (int64_t)ids.size() + 1024;
}

}  // namespace mgpu

// grid_geometrykring / grid_geometrykloop: the ring cells of a geometry --
// Mosaic.geometryKRing / geometryKLoop (core/Mosaic.scala:123-156, getCellSets :226-238):
//   (core, border) = the geometry's chips split by is_core, as sets of cell ids
//   geometryKRing(k) = core  u  U_{b in border} kRing(b, k)
//   geometryKLoop(k) = U_{b in border} kLoop(b, k)  -  (core  u  U_{b in border} kRing(b, k - 1))
// with the kRing / kLoop of mgpu_grid_kring.  What the kernels of geom_ring.hip and the host
// twin (mgpu_test_geometry_kring_host, geom_ring_host.cpp) share: the record of a cell, the
// bound of one cell's list, the argument checks and the counters of the last call.
//
// A record is one 64-bit key, (cell id << 1) | member: member = 1 for a cell of the union that is
// asked for, 0 for a cell of the set that is taken away (loop only: core and the (k - 1)-rings).
// Per geometry the keys are made distinct by id keeping the LOWEST key, so a cell with any
// member-0 record ends with member 0; the output is the ids whose key kept member 1, ascending.
// Cell ids are in [0, 2^62): H3 ids are below 2^60 and BNG ids below 2^53.
#pragma once
#include <stdint.h>

#include "../../include/mosaic_gpu.h"

namespace mgpu {
namespace geomring {

constexpr int kMaxK = 1024;
constexpr int64_t kIdLimit = (int64_t)1 << 62;
constexpr unsigned long long kEmpty = ~0ull;  // an unused slot of a set (no key: ids are below 2^62)
constexpr uint32_t kLdsSlots = 16384;         // the LDS set: 128 KiB of keys, one workgroup per CU
constexpr uint32_t kLdsSlotsMin = 64;
constexpr int kBlock = 512;                   // lanes of the workgroup that owns a geometry
constexpr int64_t kSlabRecords = (int64_t)1 << 24;  // ring ids of a slab held in scratch (128 MiB per list)

// mgpu_test_geometry_kring_last's figures
enum { kLastLds = 0, kLastHbm = 1, kLastSlabs = 2, kLastBorder = 3, kLastGenerated = 4, kLastReturned = 5,
       kLastKernelUs = 6, kLastFallback = 7 };

// the most ids one cell's kRing / kLoop can hold
inline int64_t list_bound(int is, int k, int loop_only) {
  if (loop_only) return k == 0 ? 1 : (is == MGPU_BNG ? 8 : 6) * (int64_t)k;
  return is == MGPU_BNG ? (2 * (int64_t)k + 1) * (2 * (int64_t)k + 1) : 3 * (int64_t)k * (k + 1) + 1;
}

// the checks both entries make before they read an array
int32_t check_args(const char* what, int32_t index_system, int64_t n_geoms, const void* row_off, const void* cell,
                   const void* is_core, int32_t k, int32_t loop_only, const void* out_cells, int64_t capacity,
                   const void* out_offsets, const void* out_total);
void note_last(const int64_t v[8]);

}  // namespace geomring
}  // namespace mgpu

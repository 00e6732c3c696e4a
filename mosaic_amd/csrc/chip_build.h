// The chip-table builder's interface (chip_build.cpp: host only, no HIP call, no mgpu_ctx):
// the blob's format, the build itself and the pieces it hands to a sink.  capi.cpp stages
// the blob to the device through these.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include <functional>
#include <vector>
#ifdef MGPU_BLOB_TIMING
#include <chrono>
#include <cstdio>
#endif

#include "../../include/mosaic_gpu.h"
#include "chip_table.h"

namespace mgpu {

// The chip-table blob is self-describing: a header at offset 0 records the array
// offsets, so a byte copy of the blob on another GPU (RCCL broadcast) is a
// complete chip table there.
constexpr uint64_t kBlobMagic = 0x4d4f534149434850ULL;  // "MOSAICHP"
constexpr int kBlobArrays = 29;
constexpr uint32_t kBlobVersion = 13;  // 12: BNG cell answer grids; 13: palette-compressed second level
struct BlobHeader {
  uint64_t magic;
  uint32_t version, hash_mask, max_probe, n_chips, n_cells;
  int32_t index_system;  // MGPU_H3 / MGPU_BNG: the system the chip cells belong to
  int64_t n_vertices;
  uint64_t off[kBlobArrays];
  int32_t probe_mode, res;
  uint32_t face_mask, pad2;
  double bbox[4];
  double k_res;
  DenseFace dense[20];
  uint32_t bng_edge, pad3;
  double bng_inv_edge;
  int32_t raster_mode;
  uint32_t raster_nx, raster_ny, raster_pix;
  int32_t raster_px0, raster_py0;
  double raster_x0, raster_y0, raster_inv_dx, raster_inv_dy;
  uint64_t blob_bytes;  // the whole blob (header included)
  uint32_t max_cell_chips, pad4;
  uint32_t raster_pc[4];
  uint32_t raster_sub_n, raster_sub_w;
  uint32_t raster_bshift, raster_bnx, raster_bny, raster_ncls;
  uint32_t raster_band_shift, raster_nband;
  uint32_t cell_ans_g, cell_ans_sw;
  uint32_t raster_pal, pad5;  // 1: the second level is palette-compressed
};
constexpr size_t kBlobHeaderBytes = 1024;
static_assert(sizeof(BlobHeader) <= kBlobHeaderBytes, "header too large");

// The blob's arrays, in blob order (BlobHeader::off is indexed by these; a new array goes
// before kArrCount and bumps kBlobVersion)
enum BlobArray : int {
  kArrSlots,          // HashSlot: the cell hash
  kArrChipPoly,       // int32 per sorted chip
  kArrChipFlags,      // uint8
  kArrChipPart,       // uint32, n_chips + 1
  kArrChipEnv,        // double x 4
  kArrChipRow,        // int64: the input row
  kArrPartRing,       // uint32
  kArrRingVtx,        // uint32
  kArrRingEnv,        // double x 4
  kArrVtx,            // double x 2
  kArrRowToChip,      // uint32 per input row
  kArrChipStrip,      // uint32, n_chips + 1
  kArrChipSy,         // double x 2
  kArrStripEdge,      // uint32
  kArrEdges,          // double
  kArrEdgeRing,       // uint8
  kArrChipHdr,        // ChipHdr
  kArrGrid,           // uint64: the dense probe grid
  kArrRaster,         // uint16: the pixel index
  kArrRasterCls,      // uint64
  kArrRasterRank,     // RankWord
  kArrRasterSub,      // uint16
  kArrRasterBlk,      // uint16
  kArrRasterClsPoly,  // int32
  kArrRasterBand,     // uint32
  kArrCellAnsRow,     // uint32: BNG cell answer grids
  kArrCellAns,        // uint16
  kArrRasterPal,      // uint64
  kArrRasterIdx2,     // uint8
  kArrCount
};
static_assert(kArrCount == kBlobArrays, "BlobArray names every array of the header");

// The table a blob at `base` (host or device memory) describes.
ChipTableView view_from_header(const BlobHeader& h, uint8_t* base);
// A blob header read back from memory: magic, version, sizes and array offsets checked.
int32_t check_header(const BlobHeader& hdr, int64_t bytes);

// The host blob: malloc'd and filled without a zero pass (build_blob writes every byte)
struct HostBlob {
  uint8_t* p = nullptr;
  size_t n = 0;
  HostBlob() = default;
  HostBlob(const HostBlob&) = delete;
  HostBlob& operator=(const HostBlob&) = delete;
  ~HostBlob() { free(p); }
  bool alloc(size_t bytes) {
    free(p);
    p = (uint8_t*)malloc(bytes);
    n = p ? bytes : 0;
    return p != nullptr;
  }
  uint8_t* data() const { return p; }
  size_t size() const { return n; }
  uint8_t* release() {
    uint8_t* q = p;
    p = nullptr;
    n = 0;
    return q;
  }
};

// The blob as pieces of its byte stream: [off, off + bytes) from src, then `zero` zero
// bytes.  build_blob hands them to a sink (the upload stages them straight into pinned
// buffers: no whole host blob) or assembles the host blob from them.
struct BlobPiece {
  size_t off;
  const uint8_t* src;
  size_t bytes, zero;
};
using BlobSink = std::function<int32_t(size_t total, const std::vector<BlobPiece>& pieces)>;

// bytes [off, off + n) of the stream the (ascending, contiguous) pieces make, to dst
void fill_from_pieces(const std::vector<BlobPiece>& pieces, uint8_t* dst, size_t off, size_t n);

// The whole chip table as one host blob (header + arrays, chip_table.h), or -- with a sink
// -- as pieces handed to it (`host` stays empty).  `bo` is taken as valid.
int32_t build_blob(int32_t index_system, int64_t n_chips, const int64_t* cell, const int32_t* polygon_id,
                   const uint8_t* is_core, const int64_t* wkb_offsets, const uint8_t* wkb, HostBlob& host,
                   BlobHeader& hdr_out, const mgpu_build_opts& bo, const BlobSink* sink = nullptr);

}  // namespace mgpu

// Phase timing of the build on stderr (-DMGPU_BLOB_TIMING: compile both chip_build.cpp and
// capi.cpp with it; tools/variants.sh "all:").  *_T0 starts a clock in the scope, *_MARK
// prints the time since the last mark.
#ifdef MGPU_BLOB_TIMING
#define BLOB_T0() auto blob_t = std::chrono::steady_clock::now()
#define SIDE_T0() auto side_t = std::chrono::steady_clock::now()
#define SIDE_MARK(what)                                                                                   \
  do {                                                                                                    \
    const auto now = std::chrono::steady_clock::now();                                                    \
    fprintf(stderr, "[blob]   side:%-8s %.3f s\n", what, std::chrono::duration<double>(now - side_t).count()); \
    side_t = now;                                                                                         \
  } while (0)
#define BLOB_MARK(what)                                                                                   \
  do {                                                                                                    \
    const auto now = std::chrono::steady_clock::now();                                                    \
    fprintf(stderr, "[blob] %-10s %.3f s\n", what, std::chrono::duration<double>(now - blob_t).count()); \
    blob_t = now;                                                                                         \
  } while (0)
#else
#define BLOB_T0() \
  do {            \
  } while (0)
#define BLOB_MARK(what) \
  do {                  \
  } while (0)
#define SIDE_T0() \
  do {            \
  } while (0)
#define SIDE_MARK(what) \
  do {                  \
  } while (0)
#endif

/*
 * mosaic_gpu.h -- C ABI of the MI355X grid-indexed point-in-polygon join.
 *
 * The drop-in boundary for the reference's hot path (tiems90/mosaic 0.4.3):
 *   points -> cell id        grid_pointascellid / grid_longlatascellid
 *   polygons -> chips        grid_tessellateexplode rows (is_core, index_id, wkb)
 *   join + filter            cell == index_id AND (is_core OR st_contains(wkb, pt))
 * behind the reference's IndexSystem plugin interface
 *   src/main/scala/com/databricks/labs/mosaic/core/index/IndexSystem.scala:15-318
 * Each entry point below names the reference interface it replaces.  A JVM host
 * binds them through a thin JNI shim; this repository's Python
 * host (mosaic_amd/) binds them with ctypes.
 *
 * Conventions
 *  - Plain C types only.  Status codes: 0 = ok, negative = error class; the
 *    message of the calling thread's last error is mgpu_last_error().
 *  - "device" pointers are HBM allocations on the context's GPU (hipMalloc /
 *    torch tensors); "host" pointers are ordinary memory.  `stream` is a
 *    hipStream_t (NULL = the legacy default stream).
 *  - Functions are thread-safe for distinct contexts; one context must not be used
 *    concurrently from several threads (one context per executor thread/GPU).
 *  - index_system: MGPU_H3 (H3IndexSystem) or MGPU_BNG (BNGIndexSystem);
 *    resolutions are validated like IndexSystem.getResolution
 *    (H3IndexSystem.scala:45-60: 0..15; BNGIndexSystem.scala:349-360: +-1..+-6).
 */
#ifndef MOSAIC_GPU_H
#define MOSAIC_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGPU_OK 0
#define MGPU_E_INVALID_ARG -1       /* IllegalArgumentException (bad argument, NaN H3 coordinate) */
#define MGPU_E_RESOLUTION -2        /* IllegalStateException (resolution not supported) */
#define MGPU_E_NAN -3               /* IllegalStateException (BNG: "NaN coordinates are not supported.") */
#define MGPU_E_WKB -4               /* JTS ParseException / unsupported chip geometry */
#define MGPU_E_CAPACITY -5          /* output arrays too small; the required count is returned */
#define MGPU_E_DEVICE -6            /* HIP runtime error */
#define MGPU_E_INTERNAL -7          /* kernel protocol failure (look-back timeout) */
#define MGPU_E_UNSUPPORTED -8       /* input outside what the device path builds (geometry types, huge polygons) */
#define MGPU_E_EMPTY -9             /* IllegalStateException (JTS: getX / getY of an empty Point) */

#define MGPU_H3 0
#define MGPU_BNG 1

typedef struct mgpu_ctx mgpu_ctx;
typedef struct mgpu_chips mgpu_chips;

/* Per-call statistics (optional out-parameter). */
typedef struct mgpu_stats {
    int64_t n_points;       /* points processed */
    int64_t n_pairs;        /* (point, polygon) pairs produced */
    int64_t n_near_ties;    /* H3 points whose hex2d coordinate is within 2^-40 (relative)
                               of a cell edge: the only points where an ulp-level libm
                               difference could change the cell */
    int64_t n_candidates;   /* (point, border chip) PIP evaluations */
    float kernel_ms;        /* device time of the whole call's launches (HIP events) */
    float stream_kernel_ms; /* of which the streaming kernel over all points (pip_join_kernel,
                               classify_kernel in the split pipeline, pip_binned_kernel in
                               the binned one) */
    float mixed_kernel_ms;  /* split pipeline: pip_mixed_kernel + pip_mixed_fix_kernel;
                               binned pipeline: the binning (rank, scan, scatter) */
    float emit_kernel_ms;   /* split pipeline: tile_scan_kernel + split_emit_kernel;
                               binned pipeline: fix, count, scan and emit */
    int32_t pipeline;       /* MGPU_PIPELINE_FUSED, _SPLIT or _BINNED */
    int32_t libm_overrides; /* near-tie cells the reference's libm placed differently from the
                               device's correctly rounded route (the call was then completed
                               with the reference's cells; h3_libm option) */
} mgpu_stats;
/* the join's three pipelines: one fused kernel per tile of points; for a chip
 * table with a pixel index, classify all points, resolve the mixed ones, emit; for a chip
 * table far larger than the caches, bin the points spatially (counting sort), join the
 * binned points, gather the answers back in input order */
#define MGPU_PIPELINE_AUTO (-1)
#define MGPU_PIPELINE_FUSED 0
#define MGPU_PIPELINE_SPLIT 1
#define MGPU_PIPELINE_BINNED 2

/* H3 near-tie points (the few whose cell an ulp of libm can move): the reference's
 * arithmetic -- H3-Java's JNI library on the host: platform glibc sin/cos/tan/acos/atan2,
 * x87 long double -- or the device's correctly rounded route. */
#define MGPU_LIBM_REFERENCE 0
#define MGPU_LIBM_CORRECTLY_ROUNDED 1

const char* mgpu_last_error(void);
const char* mgpu_version(void);
/* Points per tile of mgpu_pip_join (its per-tile workspace and statistics; no
 * reference counterpart). */
int32_t mgpu_join_tile_points(void);

/* One context per GPU/executor: owns the stream-ordered workspace (and, after
 * mgpu_comm_init, the RCCL communicator; destroyed with the context). */
int32_t mgpu_ctx_create(int32_t device_id, mgpu_ctx** out);
int32_t mgpu_ctx_destroy(mgpu_ctx* ctx);

/* Per-context options (no reference counterpart: the reference's planner is Spark's).
 * Nothing is read from the process environment; a JVM host sets these per context.
 *   "h3_libm"         MGPU_LIBM_REFERENCE (default) / MGPU_LIBM_CORRECTLY_ROUNDED
 *   "pipeline"        MGPU_PIPELINE_AUTO (default), or force _FUSED, _SPLIT (tables with a
 *                     pixel index), _BINNED (whenever it applies, at any size)
 *   "bin_count"       bins of the binned pipeline, 1..512 (default 64)
 *   "bin_min_mb"      the planner bins for chip tables of at least this size (256)
 *   "bin_min_points"  ... and batches of at least this many points (2^21)
 *   "bin_xcd"         1 (default): binned tiles dealt to the 8 XCDs in contiguous runs
 *   "bin_keys"        1: H3 binned joins over a dense grid take each point's grid entry from
 *                     the binning pass (which projects the point); 0 (default): the join
 *                     projects (C3: binning +1.4 ms, join -0.16 ms per 1.25e8 points)
 *   "ring_batch"      ring joins hold at most this many candidate pairs in scratch at a time
 *                     (landmarks in batches; default 2^26)
 *   "spin_us"         synchronous calls poll their stream (yielding the core between polls)
 *                     at most this long, then block in hipStreamSynchronize (default 2000;
 *                     0 = block at once)
 *   "bng_split"       1 / 0 (default): a BNG table on a dense grid without a pixel index
 *                     joins through the split pipeline with the grid entry as the code (a
 *                     cell of core chips, or an answer-grid square, answers its points; the
 *                     rest go to the mixed tiles) / through the fused pipeline
 *   "cfy_fine"        1 (default) / 0, read by each join: the split pipeline's classify pass
 *                     answers from the table's finer byte-coded block table (derived at upload
 *                     for H3 tables with a block table, row bands and a second level, when a
 *                     shape finer than 8 x 8 pixels fits the LDS) / from the 8 x 8 block table,
 *                     as for a table without one.  The pairs are the same either way
 *   "count_lds_slots" mgpu_pip_join_count keeps per-workgroup LDS histograms for chip tables
 *                     of at most this many polygons (default and maximum 4096: 48 KiB of
 *                     counts and sums per workgroup, two workgroups per CU); larger tables go through a
 *                     per-workgroup LDS hash table in front of global atomics; 0: every
 *                     addition is a global atomic
 *   "count_groups"    0 (default): mgpu_pip_join_count's aggregation kernel runs on its
 *                     resident grid; 1..65536: on at most this many workgroups (a test hook:
 *                     a small value makes every workgroup take many chunks or tiles)
 *   "cellagg_groups"  0 (default): the mgpu_cell_agg_add_* accumulation runs on its resident
 *                     grid; 1..65536: on at most this many workgroups (a test hook: one
 *                     workgroup then carries its LDS table over many chunks)
 *   "cellagg_lds"     1 (default): each workgroup of that accumulation keeps an LDS hash
 *                     table in front of the global one; 0: every addition goes to the
 *                     global table
 *   "cellagg_bin_min" a column of at least this many cells (default 2^22; one without a validity
 *                     bitmap) that holds more distinct cells than an LDS table is first dealt
 *                     into 512 bins by hash (a counting sort in context scratch, 8 or 16 B per
 *                     cell), so that each workgroup's table holds the cells it meets; 0: never
 *   "kring_batch"     0 (default): mgpu_grid_kring's H3 pentagon fallback takes as many cells
 *                     per launch as fit its 256 MB of scratch; 1..2^31-1: at most this many
 *                     (and still at most what fits; a test hook: a small value makes the
 *                     fallback run in many batches)
 *   "polyfill_slab"   mgpu_grid_polyfill processes its lattice samples in slabs of at most this
 *                     many (default 2^24, 256..2^28), whose matches wait in context scratch for
 *                     the gather; a slab boundary does not change the output
 *   "geomring_slab"   mgpu_geometry_kring expands the border cells of its geometries in slabs of at
 *                     most this many (default 2^16, 1..2^24; and at most what keeps a slab's ring
 *                     lists within 2^24 ids each), whose lists wait in context scratch; a slab
 *                     boundary, also one inside a geometry, does not change the output
 *   "geomring_lds_slots"
 *                     0 (default): a geometry's LDS set has up to 16384 slots (128 KiB); >= 64: up
 *                     to the largest power of two not above the value, capped at the default (a
 *                     test hook: a small value sends geometries down the HBM path)
 *   "raster", "raster_bng", "raster_sub", "raster_milli"
 *                     the chip-table builder of mgpu_chips_upload on this context
 *                     (mgpu_build_opts below)
 * MGPU_E_INVALID_ARG for an unknown key or a value out of range. */
int32_t mgpu_ctx_set_option(mgpu_ctx* ctx, const char* key, int64_t value);
int32_t mgpu_ctx_get_option(const mgpu_ctx* ctx, const char* key, int64_t* value);

/* Chip-table builder options (mgpu_chips_host_blob_ex; mgpu_chips_upload takes its
 * context's).  raster: 1 = build the pixel index where it pays (H3 res >= 5), 0 = never;
 * raster_bng: 1 = build it for BNG tables too (default 0: measured slower on C4);
 * raster_sub: sub-pixels per mixed pixel edge (2..16, 0 = no second level; default 16);
 * raster_milli: pixel edge / mean cell edge x 1000 (10..1000, default 250). */
typedef struct mgpu_build_opts {
    int32_t raster, raster_bng, raster_sub, raster_milli;
} mgpu_build_opts;
void mgpu_build_opts_default(mgpu_build_opts* opts);

/* IndexSystem.getResolution for an integer resolution (H3IndexSystem.scala:45-60,
 * BNGIndexSystem.scala:349-360).  Returns MGPU_OK or MGPU_E_RESOLUTION. */
int32_t mgpu_check_resolution(int32_t index_system, int32_t res);

/* IndexSystem.pointToIndex(x, y, res) over a batch (IndexSystem.scala:237;
 * H3IndexSystem.scala:168-170 = H3Core.geoToH3(lat, lon, res);
 * BNGIndexSystem.scala:284-298).  x = lon / eastings, y = lat / northings.
 * Device pointers, asynchronous on `stream`; `stats` (optional) is filled after
 * a stream synchronisation. */
int32_t mgpu_points_to_cells(mgpu_ctx* ctx, int32_t index_system, int32_t res,
                             const double* x, const double* y, int64_t n,
                             int64_t* out_cell, void* stream, mgpu_stats* stats);

/* grid_pointascellid on a geometry column (PointIndexGeom.scala:33-47: GeometryAPI.geometry
 * (GeometryAPI.scala:81-89) decodes BinaryType as WKB, StringType as WKT, HexType as
 * hex WKB, JSONType as GeoJSON, then getCentroid -- JTS Centroid: area-weighted for
 * polygons, length-weighted for lines, the mean of points -- then pointToIndex).  Rows
 * are data[offsets[i] .. offsets[i + 1]) (the Arrow binary / utf8 layout).  WKB / HEX:
 * every geometry type (big- or little-endian, EWKB / ISO Z, M, nested collections; the
 * rings and one-point lines JTS's non-strict WKBReader repairs are repaired); WKT (Java
 * Double.parseDouble rounding; WKTReader) and GeoJSON (GeoJsonReader): every type, Z / M
 * ignored, collections nested up to 8 deep, strict rings.  Malformed rows MGPU_E_WKB (JTS
 * ParseException / IllegalArgumentException), empty
 * geometries MGPU_E_EMPTY.  `valid` (optional Arrow bitmap, bit offset valid_offset): null rows are
 * null out -- out_cell 0 and a 0 bit in out_valid ((n + 7) / 8 bytes, optional).
 * mgpu_points_from_geometry stops at the point (x, y; NaN for null rows).  Device
 * pointers; synchronises `stream`. */
#define MGPU_GEOM_WKB 0
#define MGPU_GEOM_WKT 1
#define MGPU_GEOM_HEX 2     /* HexType: WKB as hex text (WKBReader.hexToBytes) */
#define MGPU_GEOM_GEOJSON 3 /* JSONType: GeoJSON text (GeoJsonReader) */
int32_t mgpu_points_from_geometry(mgpu_ctx* ctx, int32_t format, const uint8_t* data, const int64_t* offsets,
                                  const uint8_t* valid, int64_t valid_offset, int64_t n, double* out_x, double* out_y,
                                  void* stream);
int32_t mgpu_geometry_to_cells(mgpu_ctx* ctx, int32_t index_system, int32_t res, int32_t format, const uint8_t* data,
                               const int64_t* offsets, const uint8_t* valid, int64_t valid_offset, int64_t n,
                               int64_t* out_cell, uint8_t* out_valid, void* stream, mgpu_stats* stats);

/* grid_pointascellid on Mosaic's InternalGeometryType column (InternalGeometry.scala:
 * typeId, boundaries, holes; MosaicGeometryJTS.fromInternal, MosaicGeometryJTS.scala:343-357)
 * flattened as nested lists: row i's parts [row_part[i], row_part[i + 1]), part q's
 * rings [part_ring[q], part_ring[q + 1]) (the boundary, then its holes), ring k's points
 * xy[2 ring_off[k] .. 2 ring_off[k + 1]) -- the Arrow layout of list<list<list<x, y>>>.
 * type_id: POINT 1, MULTIPOINT 2, LINESTRING 3, MULTILINESTRING 4, POLYGON 5,
 * MULTIPOLYGON 6 (GeometryTypeEnum); others MGPU_E_UNSUPPORTED.  Centroid, validity and
 * errors as mgpu_geometry_to_cells.  Device pointers; synchronises `stream`. */
int32_t mgpu_internal_geometry_to_cells(mgpu_ctx* ctx, int32_t index_system, int32_t res, int64_t n,
                                        const int32_t* type_id, const int64_t* row_part, const int64_t* part_ring,
                                        const int64_t* ring_off, const double* xy, const uint8_t* valid,
                                        int64_t valid_offset, int64_t* out_cell, uint8_t* out_valid, void* stream,
                                        mgpu_stats* stats);

/* Host-pointer convenience form (copies over PCIe). */
int32_t mgpu_points_to_cells_host(mgpu_ctx* ctx, int32_t index_system, int32_t res,
                                  const double* x, const double* y, int64_t n, int64_t* out_cell);

/* BNGIndexSystem.format / parse (BNGIndexSystem.scala:119-134, 440-442; parse at
 * the `parse` method) -- the StringType cell id (default for BNG).  `out` receives
 * concatenated ASCII ids, out_offsets[n + 1] their boundaries; out_bytes is the
 * capacity of `out` (ids are at most 16 chars). Host pointers. */
int32_t mgpu_bng_format(const int64_t* cells, int64_t n, char* out, int64_t out_bytes, int64_t* out_offsets);
int32_t mgpu_bng_parse(const char* ids, const int64_t* offsets, int64_t n, int64_t* out_cells);
/* StringType cell ids on the device (IndexSystem.serializeCellId, IndexSystem.scala:61-70):
 * BNG = BNGIndexSystem.format as above, H3 = h3ToString (lowercase hex, H3IndexSystem
 * format).  Device pointers, out_offsets[n + 1] device int64.  Synchronises `stream`;
 * *out_total = bytes the ids need.  MGPU_E_INVALID_ARG if an id has no string form
 * (the reference throws), MGPU_E_CAPACITY if out_bytes is too small (only the ids
 * that fit are written).  mgpu_bng_format_device = index_system MGPU_BNG. */
int32_t mgpu_format_cells_device(mgpu_ctx* ctx, int32_t index_system, const int64_t* cells, int64_t n, char* out,
                                 int64_t out_bytes, int64_t* out_offsets, int64_t* out_total, void* stream);
int32_t mgpu_bng_format_device(mgpu_ctx* ctx, const int64_t* cells, int64_t n, char* out, int64_t out_bytes,
                               int64_t* out_offsets, int64_t* out_total, void* stream);

/* IndexSystem.kRing / kLoop over a device column of cells (grid_cellkring /
 * grid_cellkloop: expressions/index/CellKRing.scala:68, CellKLoop.scala:63) --
 * BNGIndexSystem.kRing / kLoop, BNGIndexSystem.scala:221-252 (the cell, then loops
 * 1..k; a loop = pointToIndex of the 8k corners around the cell, kept when isValid),
 * in the reference's order.  H3: H3IndexSystem.kRing / kLoop, H3IndexSystem.scala:
 * 182-205 (H3 v3.7 kRing spiral / hexRing order; a walk that meets a pentagon takes H3's
 * _kRingInternal hash-set order, and kLoop Mosaic's kRing(k) diff kRing(k - 1) in Scala
 * HashSet order, any k).  Cell i's list
 * is out_cells[out_offsets[i] .. out_offsets[i + 1]); device pointers; *out_total =
 * entries needed (MGPU_E_CAPACITY when above `capacity`).  0 <= k <= 1024. */
int32_t mgpu_grid_kring(mgpu_ctx* ctx, int32_t index_system, const int64_t* cells, int64_t n, int32_t k,
                        int32_t loop_only, int64_t* out_cells, int64_t capacity, int64_t* out_offsets,
                        int64_t* out_total, void* stream);

/* Mosaic.geometryKRing / geometryKLoop (core/Mosaic.scala:123-156, getCellSets :226-238) over a
 * batch of geometries given as chip rows -- grid_geometrykring / grid_geometrykloop and their
 * explode forms (expressions/index/GeometryKRing.scala, GeometryKLoop.scala).  Geometry g owns the
 * rows [row_off[g], row_off[g + 1]) of `cell` / `is_core` (the tessellator's index_id and is_core,
 * keep_core_geometries = false).  With core = its rows with is_core != 0 and border the others, as
 * sets of cell ids,
 *   loop_only = 0:  core  u  U_{b in border} kRing(b, k)                                  0 <= k <= 1024
 *   loop_only = 1:  U_{b in border} kLoop(b, k)  -  (core  u  U_{b in border} kRing(b, k - 1))   1 <= k <= 1024
 * where kRing / kLoop are mgpu_grid_kring's (H3: the pentagon fallbacks; BNG: invalid cells dropped,
 * quadrant resolutions).  The definition is computed as it stands: every border cell's lists are
 * expanded and the sets formed, no metric shortcut.
 * Output: geometry g's cells are out_cells[out_offsets[g] .. out_offsets[g + 1]), every cell once,
 * ASCENDING by id (the reference returns an unordered Set; ascending is this library's documented
 * order: two runs, and the host twin, give the same bytes).  A geometry without rows gives an empty
 * list, and so does, with loop_only, one with core rows only.  *out_total = the entries needed,
 * MGPU_E_CAPACITY when above `capacity` (out_offsets is still written in full; the entries that fit
 * are written); out_cells = NULL with capacity 0 asks for the size.
 * MGPU_E_INVALID_ARG: k outside its range (the reference's kRing(b, -1) for a loop of k = 0 has no
 * meaning), a border row that is not a cell id of the index system (mgpu_grid_kring's verdict), a
 * core row outside [0, 2^62) (no cell id of either system), row_off decreasing or negative.
 * MGPU_E_UNSUPPORTED: one geometry with 2^31 or more ring ids within a slab that did not fit its
 * LDS set (lower "geomring_slab").
 * All pointers are device pointers; the call synchronises `stream` (several times: it reads the
 * geometries' sizes and each slab's verdicts back).  Options "geomring_slab", "geomring_lds_slots". */
int32_t mgpu_geometry_kring(mgpu_ctx* ctx, int32_t index_system, int64_t n_geoms, const int64_t* row_off, const int64_t* cell,
                            const uint8_t* is_core, int32_t k, int32_t loop_only, int64_t* out_cells, int64_t capacity,
                            int64_t* out_offsets, int64_t* out_total, void* stream);

/* Cell id -> geometry over a device column of cells: what grid_boundaryaswkb /
 * grid_boundary (expressions/index/IndexGeometry.scala:65-75) and grid_cellarea
 * (expressions/index/CellArea.scala) compute per row.  Device pointers throughout; `valid`
 * an optional Arrow validity bitmap read from bit valid_offset (as mgpu_geometry_to_cells),
 * out_valid (optional) its copy at bit offset 0.  A null row gets 0 vertices, an empty WKB
 * row, NaN centre and area.  A non-null row that is not a cell id fails the whole call with
 * MGPU_E_INVALID_ARG before anything is written (the reference throws there or returns
 * garbage) -- H3: mode != 1, base cell >= 122, a digit 7 at or before the resolution or
 * another digit after it, a pentagon's deleted subsequence; BNG: the ids whose digits
 * BNGIndexSystem.getResolution / getX / getY cannot decode.  Every entry reads that verdict
 * back first (one small kernel and a wait on `stream`).
 * H3 coordinates are H3 v3.7's h3ToGeoBoundary / h3ToGeo with correctly rounded sin, cos,
 * asin, atan, atan2 (the reference's come from glibc's, which are not: DESIGN 3.8 has the
 * measured gap, below 1e-12 degrees); mgpu_test_cell_geometry_host is the same code on
 * the host, equal bit for bit.  BNG is integer arithmetic and exact.
 *
 * mgpu_cells_to_centers: IndexSystem.indexToCenter (IndexSystem.scala:239-241;
 * H3IndexSystem.scala:230-233: h3ToGeo), out_x = lng, out_y = lat, degrees.  H3 only:
 * MGPU_E_UNSUPPORTED for BNG (BNGIndexSystem.scala:518-520 throws NotImplementedError).
 * The centres are queued on `stream`; the call does not wait for them. */
int32_t mgpu_cells_to_centers(mgpu_ctx* ctx, int32_t index_system, const int64_t* cells, const uint8_t* valid,
                              int64_t valid_offset, int64_t n, double* out_x, double* out_y, uint8_t* out_valid,
                              void* stream);
/* IndexSystem.indexToBoundary (IndexSystem.scala:243-245; H3IndexSystem.scala:235-237:
 * h3ToGeoBoundary, not closed, 5 to 10 vertices with the distortion vertices of Class III
 * cells on icosahedron edges) and the corners of BNGIndexSystem.indexToGeometry
 * (BNGIndexSystem.scala:418-431: (x, y), (x + e, y), (x + e, y + e), (x, y + e)).  Row i:
 * out_nverts[i] (x, y) pairs at out_xy[20 i ..] (16-byte aligned; the pairs beyond are
 * left as they were).  The boundaries are queued on `stream`; the call does not wait for them. */
int32_t mgpu_cells_to_boundaries(mgpu_ctx* ctx, int32_t index_system, const int64_t* cells, const uint8_t* valid,
                                 int64_t valid_offset, int64_t n, double* out_xy, int32_t* out_nverts,
                                 uint8_t* out_valid, void* stream);
/* IndexSystem.indexToGeometry as WKB (H3IndexSystem.scala:103-112, BNGIndexSystem.scala:
 * 418-431; IndexGeometry.scala:65-75): row i at out[out_offsets[i] .. out_offsets[i + 1]),
 * big-endian 2-D, the bytes the tessellator's chips carry for a whole cell: a Polygon of one
 * ring, the boundary closed with its first vertex; an H3 cell holding a pole as
 * makePoleGeometry's cap (:361-384), one across the antimeridian cut in two (:386-410) --
 * those few rows are shaped on the host from the device's boundaries.  out_offsets[n + 1]
 * device int64.  Synchronises `stream`; *out_total = the bytes needed, MGPU_E_CAPACITY when
 * out_bytes is below that (the rows that fit are written). */
int32_t mgpu_cells_boundary_wkb(mgpu_ctx* ctx, int32_t index_system, const int64_t* cells, const uint8_t* valid,
                                int64_t valid_offset, int64_t n, uint8_t* out, int64_t out_bytes, int64_t* out_offsets,
                                int64_t* out_total, uint8_t* out_valid, void* stream);
/* IndexSystem.area in km^2 (IndexSystem.scala:248-289: haversine sides and the spherical
 * excess of the centre-vertex triangles, r = 6371.0088, operation for operation on the
 * coordinates above; BNGIndexSystem.scala:510-516: (edge / 1000)^2).  Queued on `stream`. */
int32_t mgpu_cells_area(mgpu_ctx* ctx, int32_t index_system, const int64_t* cells, const uint8_t* valid,
                        int64_t valid_offset, int64_t n, double* out_area_km2, uint8_t* out_valid, void* stream);

/* IndexSystem.polyfill (IndexSystem.scala:166; H3IndexSystem.scala:134-154; BNGIndexSystem.scala:185-209),
 * grid_polyfill (expressions/index/Polyfill.scala) over a polygon set: for polygon p, every cell at
 * `res` whose centre lies in p's interior (the documented definition; docs/source/api/
 * spatial-indexing.rst:191-220).  H3: the centre is h3ToGeo in degrees on the correctly rounded
 * route of mgpu_cells_to_centers; BNG: JTS Centroid of the ring of indexToGeometry's corners.
 * Containment is planar JTS PointLocator (RayCrossingCounter per ring: inside the shell and
 * outside every hole of some part; a centre on the boundary is not contained).  Two documented
 * differences from the reference: it returns the full set (the reference's flood fill / BFS can
 * miss a matching cell that no chain of matching neighbours joins to a seed), and the H3 centres
 * are the correctly rounded ones (within 1e-12 degrees of glibc's).
 * Geometry: host pointers, the layout of mgpu_tessellate (rings closed, at least 4 points).
 * Output: device pointers; polygon p's cells are out_cells[out_offsets[p] .. out_offsets[p+1]),
 * in the order of the lattice the call lays over p's bounding box (row by row from the south-west;
 * deterministic, not the reference's hash-set order); no cell twice; a polygon without parts
 * gives an empty list.  *out_total = cells needed, MGPU_E_CAPACITY when above `capacity`
 * (offsets are still written).  Synchronises `stream`.
 * MGPU_E_RESOLUTION as mgpu_check_resolution; MGPU_E_INVALID_ARG: non-finite coordinates, H3
 * coordinates outside [-180, 180] x [-90, 90], a ring of fewer than 4 points or not closed, a
 * polygon whose lattice would exceed 2^31 - 1 samples; MGPU_E_UNSUPPORTED: an H3 polygon whose
 * bounding box spans 180 degrees of longitude or more; MGPU_E_INTERNAL: the H3 lattice's
 * certificate failed at every spacing tried.
 * Option "polyfill_slab" (context): the samples whose matches are held in scratch at a time. */
int32_t mgpu_grid_polyfill(mgpu_ctx* ctx, int32_t index_system, int32_t res, int64_t n_polys,
                           const int64_t* poly_part_off, const int64_t* part_ring_off, const int64_t* ring_off,
                           const double* xy, int64_t* out_cells, int64_t capacity, int64_t* out_offsets,
                           int64_t* out_total, void* stream);

/* Upload a chip table (the rows of grid_tessellateexplode, MosaicExplode.scala:70-83,
 * ChipType.scala:17-29): cell id, owning polygon id, is_core, and the chip WKB
 * (big- or little-endian, Polygon / MultiPolygon / GeometryCollection of those;
 * a NULL geometry is wkb_offsets[i] == wkb_offsets[i+1]).  Host pointers.  The WKB
 * is parsed once here (the reference re-parses it per candidate row).  For H3 the
 * cell hash is keyed by lattice position (see mosaic_amd/csrc/chip_table.h). */
int32_t mgpu_chips_upload(mgpu_ctx* ctx, int32_t index_system, int64_t n_chips, const int64_t* cell,
                          const int32_t* polygon_id, const uint8_t* is_core, const int64_t* wkb_offsets,
                          const uint8_t* wkb, mgpu_chips** out);
int32_t mgpu_chips_destroy(mgpu_chips* chips);
/* The chip table is one device allocation: expose it for replication (RCCL
 * broadcast of `bytes` at `device_ptr`), and rebuild a handle on another GPU from
 * a received copy (the received buffer is copied into a new allocation). */
int32_t mgpu_chips_device_blob(const mgpu_chips* chips, void** device_ptr, int64_t* bytes);
int32_t mgpu_chips_from_device_blob(mgpu_ctx* ctx, const void* device_ptr, int64_t bytes, mgpu_chips** out);
int32_t mgpu_chips_info(const mgpu_chips* chips, int64_t* n_chips, int64_t* n_cells, int64_t* n_vertices);
/* The table's pixel index (no reference counterpart; read-only): *mode = 0 when it has
 * none, *n_classes = the pixel classes of an H3 table's index, class 0 (empty) included
 * (else 0).  Either may be NULL. */
int32_t mgpu_chips_raster_info(const mgpu_chips* chips, int64_t* mode, int64_t* n_classes);
/* The distinct polygon ids of the table, ascending, into out_ids[cap] (host); *out_n =
 * their number P.  These are the slots of mgpu_pip_join_count: slot k is out_ids[k].
 * MGPU_E_CAPACITY with *out_n set if cap is short (cap 0 / out_ids NULL asks for P).  The
 * id -> slot table is built at the first call (or the first mgpu_pip_join_count) from the
 * table's polygon column and kept on the handle, outside the blob. */
int32_t mgpu_chips_polygons(const mgpu_chips* chips, int32_t* out_ids, int64_t cap, int64_t* out_n);

/* The chip table as one self-describing host blob (what mgpu_chips_upload uploads): a
 * JVM driver can build it once and ship the bytes to its executors, which upload them
 * with mgpu_chips_upload_blob.  Free with mgpu_host_free.  mgpu_host_blob_info checks a
 * received blob (magic, version, size, offsets) and reports its contents.  Host only. */
int32_t mgpu_chips_host_blob(int32_t index_system, int64_t n_chips, const int64_t* cell, const int32_t* polygon_id,
                             const uint8_t* is_core, const int64_t* wkb_offsets, const uint8_t* wkb, uint8_t** out,
                             int64_t* bytes);
int32_t mgpu_chips_host_blob_ex(int32_t index_system, int64_t n_chips, const int64_t* cell, const int32_t* polygon_id,
                                const uint8_t* is_core, const int64_t* wkb_offsets, const uint8_t* wkb,
                                const mgpu_build_opts* opts, uint8_t** out, int64_t* bytes);
int32_t mgpu_host_free(void* p);
int32_t mgpu_host_blob_info(const void* host_blob, int64_t bytes, int32_t* index_system, int64_t* n_chips,
                            int64_t* n_cells, int64_t* n_vertices);
int32_t mgpu_chips_upload_blob(mgpu_ctx* ctx, const void* host_blob, int64_t bytes, mgpu_chips** out);

/* Multi-GPU (one process per GPU): points are sharded by contiguous id range,
 * the chip table is replicated.  The reference's scale-out is Spark's broadcast of the
 * chip side to every executor (BroadcastHashJoin in the plan of notebooks/examples/python/
 * Quickstart/QuickstartNotebook.ipynb:1835); here each GPU's context owns an RCCL
 * communicator:
 *   mgpu_comm_unique_id  one rank creates the id (ncclGetUniqueId) and ships its
 *                        MGPU_COMM_ID_BYTES to every rank out of band (the JVM driver's
 *                        broadcast; torch.distributed's store in mosaic_amd/dist.py);
 *   mgpu_comm_init       every rank joins (ncclCommInitRank; blocks until all have);
 *   mgpu_chips_broadcast the root's chip table is replicated into a new allocation on
 *                        every other rank by one RCCL broadcast of the blob (plus one of
 *                        its 1 KiB header to size it); *out = the replica (NULL on root);
 *   mgpu_pair_offsets    RCCL all-gather of the per-rank pair counts: this rank's offset
 *                        in the globally ordered output, the total, and (optionally)
 *                        out_counts[world].
 * The collectives are enqueued on `stream` and complete before the calls return. */
#define MGPU_COMM_ID_BYTES 128
int32_t mgpu_comm_unique_id(uint8_t* out_id);
int32_t mgpu_comm_init(mgpu_ctx* ctx, const uint8_t* unique_id, int32_t rank, int32_t world);
int32_t mgpu_comm_info(mgpu_ctx* ctx, int32_t* rank, int32_t* world);
int32_t mgpu_comm_destroy(mgpu_ctx* ctx);
int32_t mgpu_chips_broadcast(mgpu_ctx* ctx, const mgpu_chips* chips, int32_t root, mgpu_chips** out, void* stream);
int32_t mgpu_pair_offsets(mgpu_ctx* ctx, int64_t local_pairs, int64_t* out_offset, int64_t* out_total,
                          int64_t* out_counts, void* stream);
/* TEST ONLY: a receiving rank's side of mgpu_chips_broadcast without RCCL -- the header
 * read from the device buffer dev_blob, the receiving allocation (fail_alloc != 0 forces
 * it to fail), the blob copied in, the table adopted -- so a corrupt header or a failed
 * allocation can be shown to return an error (it does not wait on anything). */
int32_t mgpu_test_receive_blob(mgpu_ctx* ctx, const void* dev_blob, int32_t fail_alloc, mgpu_chips** out);

/* The grid-ring neighbour join of SpatialKNN for point landmarks and point candidates, one
 * iteration (models/knn/GridRingNeighbours.scala: transform :121 and resultTransform;
 * SpatialKNN.scala's per-iteration filter): each landmark's cells -- kRing(cell, k)
 * (loop_only = 0: iteration 1's grid_geometrykringexplode) or kLoop(cell, k) (loop_only =
 * 1: iteration k's grid_geometrykloopexplode) of pointToIndex(landmark) -- joined with the
 * candidates' cells (grid_tessellateexplode of a point: its one chip); every (landmark,
 * candidate) sharing a cell is a pair once, self matches (identical coordinates) dropped,
 * distance = st_distance (JTS Coordinate.distance: Math.hypot), pairs with distance <=
 * max_distance (< 0: no threshold), per landmark ordered by (distance, candidate index)
 * and cut to the first max_per_left (0: all; SpatialKNN's neighbour_number <= k).  Output:
 * out_left = left_id_base + landmark index, out_right = candidate index, out_dist; landmarks
 * in order.  Device pointers; synchronises `stream`; MGPU_E_CAPACITY with *out_n when the
 * pairs exceed `capacity`. */
int32_t mgpu_ring_join(mgpu_ctx* ctx, int32_t index_system, int32_t res, int32_t k, int32_t loop_only,
                       const double* left_x, const double* left_y, int64_t n_left, const double* right_x,
                       const double* right_y, int64_t n_right, int64_t left_id_base, int32_t max_per_left,
                       double max_distance, int64_t capacity, int64_t* out_n, int64_t* out_left, int64_t* out_right,
                       double* out_dist, void* stream);
/* mgpu_ring_join with flags.  MGPU_RING_LEFT_OUTER: the join is left_outer
 * (GridRingNeighbours.scala:128) and resultTransform keeps the null group
 * (coalesce(intersects, true), :151): a landmark with a ring cell that holds no candidate
 * gets one row (left, -1, NaN) before its pairs -- Spark orders the null distance first in
 * the ascending window -- not counted by max_per_left nor filtered by max_distance.
 * Self matches: dropped when the coordinates are bit-identical; the reference compares
 * hash() of the geometry column (:154), so two rows holding the same point in different
 * text or WKB (or -0.0 vs 0.0) are distinct there but one here. */
#define MGPU_RING_LEFT_OUTER 1
int32_t mgpu_ring_join_ex(mgpu_ctx* ctx, int32_t index_system, int32_t res, int32_t k, int32_t loop_only,
                          const double* left_x, const double* left_y, int64_t n_left, const double* right_x,
                          const double* right_y, int64_t n_right, int64_t left_id_base, int32_t max_per_left,
                          double max_distance, int32_t flags, int64_t capacity, int64_t* out_n, int64_t* out_left,
                          int64_t* out_right, double* out_dist, void* stream);
/* SpatialKNN's exactness iteration (GridRingNeighbours.leftTransform, iterationID = -1,
 * GridRingNeighbours.scala:82-90; SpatialKNN.resultTransform): per landmark i, the cells of
 * grid_tessellate(st_buffer(landmark, radius[i]), res) -- JTS's 32-gon circle, mosaicFill's
 * cells (mgpu_tessellate) -- minus grid_geometrykring(landmark, res, k_iterated[i])
 * (array_except), joined with the candidates as mgpu_ring_join_ex does.  radius[i] (the
 * landmark's k-th match distance) NaN or <= 0 gives the landmark no cells.  radius and
 * k_iterated are HOST arrays; the points are device pointers.  Synchronises `stream`. */
int32_t mgpu_ring_join_final(mgpu_ctx* ctx, int32_t index_system, int32_t res, const double* left_x,
                             const double* left_y, const double* radius, const int32_t* k_iterated, int64_t n_left,
                             const double* right_x, const double* right_y, int64_t n_right, int64_t left_id_base,
                             int32_t max_per_left, double max_distance, int32_t flags, int64_t capacity,
                             int64_t* out_n, int64_t* out_left, int64_t* out_right, double* out_dist, void* stream);

/* st_contains(chip.wkb, point) for explicit (chip row, point) pairs
 * (ST_Contains.scala:21-44 -> MosaicGeometryJTS.contains, MosaicGeometryJTS.scala:197).
 * out[i] = 1 / 0, or -1 when the chip's geometry is NULL.  Device pointers.
 * Synchronises `stream`: a chip row outside [0, n_chips) fails the call with
 * MGPU_E_INVALID_ARG (its out[i] is -2). */
int32_t mgpu_st_contains(mgpu_ctx* ctx, const mgpu_chips* chips, const int64_t* chip_row,
                         const double* x, const double* y, int64_t n, int8_t* out, void* stream);

/* The hot path: cell id per point, equi-join against the chip table's
 * cell ids, `is_core OR st_contains` filter (one of three pipelines, chosen per call:
 * split for pixel-indexed tables, binned for tables beyond the caches, else fused --
 * mgpu_stats.pipeline); emits (point_id, polygon_id) pairs
 * ordered by input position then polygon id (sorted by point_id when point ids
 * ascend, e.g. contiguous id shards).  point_id may be NULL: ids are
 * point_id_base + index.  Device pointers.  Synchronises `stream` to return the
 * pair count in *out_n_pairs; if it exceeds `capacity` only the first `capacity`
 * pairs are written and MGPU_E_CAPACITY is returned.
 * H3 cells are the reference's bit for bit: the device decides every point outside a
 * 2^-40 tie band around the cell boundaries; the few inside it (mgpu_stats.n_near_ties)
 * are recomputed on the host with the reference's libm (option h3_libm), and when that
 * moves a cell the join is rerun with the corrected cells (mgpu_stats.libm_overrides). */
int32_t mgpu_pip_join(mgpu_ctx* ctx, const mgpu_chips* chips, int32_t index_system, int32_t res,
                      const double* x, const double* y, const int64_t* point_id, int64_t point_id_base,
                      int64_t n, int64_t capacity, int64_t* out_n_pairs, int64_t* out_point_id,
                      int32_t* out_polygon_id, void* stream, mgpu_stats* stats);

/* After mgpu_pip_join returned MGPU_E_CAPACITY (*out_n_pairs = the count): write all
 * pairs of that join into larger output arrays without redoing it -- the join's pair
 * records stay in the context until its next call.  (Only when the workspace's overflow
 * pool had to drop records -- tiles with more pairs than points beyond the capacity --
 * is the join redone, from the same, unchanged, input arrays.)  Synchronises `stream`;
 * MGPU_E_INVALID_ARG if no join was kept, MGPU_E_CAPACITY if capacity is still short. */
int32_t mgpu_pip_join_fetch(mgpu_ctx* ctx, int64_t capacity, int64_t* out_n_pairs, int64_t* out_point_id,
                            int32_t* out_polygon_id, void* stream);

/* The join aggregated per polygon, without the pair output: what a host does with the
 * joined rows is most often a count (the Quickstart's joined_df.count(),
 * docs/source/usage/quickstart.ipynb:692) or a groupBy(polygon).agg(count, sum).  For the
 * table's distinct polygon ids ascending (mgpu_chips_polygons), count[k] = the number of
 * pairs (point, ids[k]) mgpu_pip_join emits for the same inputs -- cell == index_id AND
 * (is_core OR st_contains(wkb, point)), ST_Contains.scala:21-44 -- and sum[k] = the sum
 * of weight[p] over those pairs (two's complement wrap).  A point in several overlapping
 * polygons adds to each; polygons without points get 0.  Integer arithmetic: the results
 * are exact and do not depend on scheduling.
 * count / sum: device int64[n_slots]; weight: device int64[n] or NULL (then sum must be
 * NULL, and a weight needs a sum); accumulate != 0 adds to the arrays' contents instead of
 * overwriting them (streaming batches).  n_slots != P -> MGPU_E_INVALID_ARG.
 * The cells are the reference's as in mgpu_pip_join (near-tie queue, host libm pass, the
 * override rerun when a cell moves); invalid coordinates raise the same errors.  count /
 * sum are written only after the join has settled: a failing call leaves them untouched.
 * Synchronises `stream`; stats as mgpu_pip_join (n_pairs = the sum of the counts added;
 * kernel_ms includes the aggregation, emit_kernel_ms is the aggregation's time).  The
 * join's records stay in the context: mgpu_pip_join_fetch after this call writes the
 * pairs mgpu_pip_join would have. */
int32_t mgpu_pip_join_count(mgpu_ctx* ctx, const mgpu_chips* chips, int32_t index_system, int32_t res,
                            const double* x, const double* y, const int64_t* weight, int64_t n, int64_t n_slots,
                            int64_t* count, int64_t* sum, int32_t accumulate, void* stream, mgpu_stats* stats);

/* The join as a per-point column, in input order: "which zone is this trip in?" -- the
 * Quickstart's join (notebooks/examples/python/Quickstart/QuickstartNotebook.ipynb:1835)
 * taken as a left join of the points with the chips and first(polygon) per point, over the predicate
 * of ST_Contains.scala:21-44.  For input position i:
 *   out_polygon[i]  the polygon id of the first pair mgpu_pip_join emits for point i on the
 *                   same inputs -- the lowest matching id -- or null_id when it has none;
 *   out_matches[i]  the number of pairs mgpu_pip_join emits for point i (0: none; more than
 *                   1: overlapping polygons).  May be NULL: then it is not written.  With it
 *                   a host builds a validity bitmap whatever null_id is.
 * Both are device int32[n]; every element of [0, n) is written exactly once by a successful
 * call (no pre-fill needed), and only after the join has settled (near-tie queue, host libm
 * pass, override rerun, as mgpu_pip_join): a failing call -- invalid coordinates raise the
 * same errors as mgpu_pip_join -- leaves them untouched.  n == 0 is MGPU_OK and writes
 * nothing; out_polygon == NULL with n > 0 is MGPU_E_INVALID_ARG.  No pairs are written and
 * no output offsets computed: 4 or 8 bytes per point instead of 12 per pair.
 * Synchronises `stream`; stats as mgpu_pip_join (n_pairs = the sum of the match counts;
 * kernel_ms includes the lookup launch, emit_kernel_ms is its time).  The join's records
 * stay in the context: mgpu_pip_join_fetch after this call writes the pairs mgpu_pip_join
 * would have. */
int32_t mgpu_pip_join_lookup(mgpu_ctx* ctx, const mgpu_chips* chips, int32_t index_system, int32_t res,
                             const double* x, const double* y, int64_t n, int32_t null_id,
                             int32_t* out_polygon, int32_t* out_matches, void* stream, mgpu_stats* stats);

/* CellAggregate: counts and sums per cell of a stream of points -- what a grid user does
 * with a cell column before any polygon exists: with_postcodes.groupBy("index_id").count()
 * (notebooks/examples/python/TransformBNG/transform_join_bng.ipynb:5321), count and sum per
 * index_id in the gridded-EO notebooks (notebooks/examples/python/EOGriddedSTAC/03. Gridded
 * EO Data.ipynb:3194-3233), over the cells of IndexSystem.pointToIndex
 * (IndexSystem.scala:237).  A hash aggregation in LDS and device memory instead of a sort
 * of the 8 B/point cell column.  The handle lives across batches (and contexts of its
 * device); all arithmetic is integer, so the results are exact and do not depend on
 * scheduling, batch boundaries or table growth.  Every call synchronises `stream`; n == 0 is
 * MGPU_OK and adds nothing; a NULL ctx or handle is MGPU_E_INVALID_ARG before the device is
 * touched.  All column pointers are device pointers; n_cells / out_n are host pointers.
 *
 * create: an aggregate for (index_system, res) -- checked as mgpu_check_resolution does,
 *   before anything else -- with a sum column iff with_sum != 0.  Memory: one open-addressing
 *   table of 16 B (24 B with a sum) per entry, kept at most half full; it never grows with
 *   the number of points, only with the number of distinct cells D: the table holds at most
 *   4 entries per distinct cell (96 B with a sum) above a floor of 1024 entries, and 6 per
 *   cell for the duration of a growth step (old and new table).  initial_cells sizes it at
 *   create (entries = the power of two >= 2 * initial_cells, at least the floor), so an
 *   aggregate created for D cells takes D cells without growing.
 * add_points: adds the cells mgpu_points_to_cells writes for the same inputs and context
 *   options -- the fast path, the near-tie queue, the host glibc pass under h3_libm =
 *   reference -- one count each and weight[i] to the sum.  Invalid coordinates raise the
 *   same errors.  The aggregate is touched only after the cells have settled: a failing call
 *   leaves counts and sums untouched.  The cell column goes to context scratch (8 B/point,
 *   and as much again, twice with a weight, for a column that is binned: option
 *   "cellagg_bin_min") and is never returned.  stats as mgpu_points_to_cells fills it; emit_kernel_ms is the
 *   aggregation's time (kernel_ms includes it).
 * add_cells: adds a cell column, e.g. mgpu_geometry_to_cells' output.  Any int64 is a key: 0,
 *   -1, INT64_MIN and INT64_MAX included (the table's free-slot marker is -1; the aggregate of
 *   the key -1 is kept in a side record, so no key is lost to it).  valid: optional Arrow
 *   bitmap at bit offset valid_offset; null rows add nothing.
 * weight (both): device int64[n], accepted only on a with_sum aggregate, and with_sum
 *   requires it: otherwise MGPU_E_INVALID_ARG.  Sums wrap in two's complement.
 * add_counted: adds (cell, count, sum) records, count[i] >= 0; a record of count 0 adds
 *   nothing (and creates no cell).  sum is given exactly on a with_sum aggregate.  Reloads a
 *   fetched result, merges another rank's or another aggregate's, and is the table's own
 *   rehash on growth.
 * size: *n_cells = the number of distinct cells with count > 0.
 * fetch: those cells ascending as signed int64 with their counts and sums into device
 *   int64[capacity] columns (compaction and a radix sort on the device); out_sum is NULL
 *   exactly when the aggregate has no sum.  *out_n is always the exact number of cells, on
 *   MGPU_OK and on MGPU_E_CAPACITY (capacity < *out_n: nothing is written).  Non-destructive
 *   and repeatable; adding may continue afterwards.
 * clear: empties the aggregate and keeps its memory.
 * Context options: "cellagg_groups", "cellagg_lds", "cellagg_bin_min" (mgpu_ctx_set_option). */
typedef struct mgpu_cell_agg mgpu_cell_agg;
int32_t mgpu_cell_agg_create(mgpu_ctx* ctx, int32_t index_system, int32_t res, int32_t with_sum,
                             int64_t initial_cells, mgpu_cell_agg** out);
int32_t mgpu_cell_agg_add_points(mgpu_ctx* ctx, mgpu_cell_agg* agg, const double* x, const double* y,
                                 const int64_t* weight, int64_t n, void* stream, mgpu_stats* stats);
int32_t mgpu_cell_agg_add_cells(mgpu_ctx* ctx, mgpu_cell_agg* agg, const int64_t* cells, const uint8_t* valid,
                                int64_t valid_offset, const int64_t* weight, int64_t n, void* stream);
int32_t mgpu_cell_agg_add_counted(mgpu_ctx* ctx, mgpu_cell_agg* agg, const int64_t* cells, const int64_t* count,
                                  const int64_t* sum, int64_t n, void* stream);
int32_t mgpu_cell_agg_size(mgpu_ctx* ctx, const mgpu_cell_agg* agg, int64_t* n_cells, void* stream);
int32_t mgpu_cell_agg_fetch(mgpu_ctx* ctx, const mgpu_cell_agg* agg, int64_t capacity, int64_t* out_cell,
                            int64_t* out_count, int64_t* out_sum, int64_t* out_n, void* stream);
int32_t mgpu_cell_agg_clear(mgpu_ctx* ctx, mgpu_cell_agg* agg, void* stream);
int32_t mgpu_cell_agg_destroy(mgpu_cell_agg* agg);

/* Asynchronous form, in two calls.  mgpu_pip_join_async enqueues the join on `stream`
 * and returns at once: the pair count is left in device memory (*d_n_pairs, one int64)
 * -- graph-capturable once mgpu_ctx_reserve has sized the workspace and one call of the
 * same size has grown the split / binned pipeline's buffers.  As in the synchronous
 * call, H3 points inside the fast path's tie band are joined with the fast cell and
 * queued; mgpu_pip_join_finish (same context, no other call on it in between) waits
 * for the stream, recomputes the queued points with the reference's libm (option
 * h3_libm; H3IndexSystem.scala:168-170 -> H3-Java's glibc) and, only when that moves a
 * cell, reruns the join into the same output arrays and *d_n_pairs.  The pairs equal
 * mgpu_pip_join's once mgpu_pip_join_finish has returned MGPU_OK (or MGPU_E_CAPACITY,
 * with *out_n_pairs the count: mgpu_pip_join_fetch then writes them all); before it, a
 * batch with near-ties may hold the fast cell at those points.  BNG joins and the
 * correctly rounded mode have no host step, but the call is still required.
 * mgpu_pip_join_finish: MGPU_E_INVALID_ARG when no asynchronous join is pending (another
 * call on the context ended it).
 * Graph replays are NOT settled: finish pairs with the host-side mgpu_pip_join_async call
 * that queued the work, so a captured join replayed from a graph keeps the fast cell at
 * the points of its tie band (H3, reference libm) and finish after a replay returns
 * MGPU_E_INVALID_ARG.  A caller replaying graphs either sets h3_libm to
 * MGPU_LIBM_CORRECTLY_ROUNDED (the device decides every point, no host step) or reads the
 * replay's queued positions with mgpu_last_near_ties and reruns those batches with
 * mgpu_pip_join. */
int32_t mgpu_pip_join_async(mgpu_ctx* ctx, const mgpu_chips* chips, int32_t index_system, int32_t res,
                            const double* x, const double* y, const int64_t* point_id, int64_t point_id_base,
                            int64_t n, int64_t capacity, int64_t* d_n_pairs, int64_t* out_point_id,
                            int32_t* out_polygon_id, void* stream);
int32_t mgpu_pip_join_finish(mgpu_ctx* ctx, int64_t* out_n_pairs, mgpu_stats* stats);
int32_t mgpu_ctx_reserve(mgpu_ctx* ctx, int64_t max_points);

/* Parity audit (no reference counterpart): the input positions of the H3 near-tie
 * points of the last call on `ctx` (mgpu_pip_join, mgpu_points_to_cells, the geometry
 * entries) -- the points the device's route resolved inside its tie band
 * (mgpu_stats.n_near_ties), the only ones whose cell an ulp of libm can move; the
 * synchronous calls gave each of them the reference's cell.  Ascending.  Synchronises
 * the device.  MGPU_E_CAPACITY (with *out_n set) if cap is too small; MGPU_E_INTERNAL
 * if an asynchronous join found more than the queue holds. */
int32_t mgpu_last_near_ties(mgpu_ctx* ctx, int64_t* out_index, int64_t cap, int64_t* out_n);

/* Host-pointer convenience form of mgpu_pip_join (copies points in, pairs out). */
int32_t mgpu_pip_join_host(mgpu_ctx* ctx, const mgpu_chips* chips, int32_t index_system, int32_t res,
                           const double* x, const double* y, const int64_t* point_id, int64_t n,
                           int64_t capacity, int64_t* out_n_pairs, int64_t* out_point_id,
                           int32_t* out_polygon_id);

/* grid_tessellateexplode for a polygon set (Mosaic.getChips / mosaicFill,
 * core/Mosaic.scala:22-99; IndexSystem.getCoreChips/getBorderChips,
 * IndexSystem.scala:178-213).  Polygons are given as flat rings:
 *   polygon p has parts [poly_part_off[p], poly_part_off[p+1]),
 *   part q has rings [part_ring_off[q], part_ring_off[q+1]) (first = shell),
 *   ring r has vertices xy[2*ring_off[r] .. 2*ring_off[r+1]) (closed rings).
 * Output rows are returned through an opaque result read with
 * mgpu_tess_result_*; chip WKB is big-endian (JTS WKBWriter).  Host only. */
typedef struct mgpu_tess mgpu_tess;
int32_t mgpu_tessellate(int32_t index_system, int32_t res, int64_t n_polys, const int32_t* polygon_id,
                        const int64_t* poly_part_off, const int64_t* part_ring_off, const int64_t* ring_off,
                        const double* xy, int32_t keep_core_geometries, mgpu_tess** out);
/* The is_core rule (mgpu_tessellate uses MGPU_CORE_MOSAICFILL):
 *   MGPU_CORE_MOSAICFILL  the reference's: core iff the cell is in polyfill(buffer(-r))
 *                         (Mosaic.scala:71-93, getCoreChips IndexSystem.scala:208-213: its
 *                         centre inside the polygon at distance >= r = getBufferRadius from
 *                         the boundary); a border-set cell is never core -- getBorderChips'
 *                         equalsExact (IndexSystem.scala:186-188) compares JTS overlay's
 *                         clockwise shell with indexToGeometry's counter-clockwise cell --
 *                         so a cell the polygon holds whole but outside the core set is a
 *                         border chip whose geometry is the whole cell; chip cells beyond
 *                         the border band are dropped (never visited by the reference);
 *                         Near r the sets are decided as JTS 1.20's BufferOp builds them
 *                         (8 quadrant segments: fillets of chords, input simplification,
 *                         depth >= 1 of the raw offset curves -- mosaic_amd/csrc/jts_buffer.h);
 *   MGPU_CORE_CLIP        every cell the polygon holds whole is core;
 *   MGPU_CORE_DISTANCE    round 4's form of MOSAICFILL: the sets decided by the centre's
 *                         exact distance to the boundary (arcs, no simplification).
 * mgpu_tess_result_stats: out6 = {rows, core rows, whole cells flagged border (demoted),
 * partly covered cells flagged core (promoted), dropped, rows the restatement leaves
 * undecided (ambiguous: a centre within 1e-9 r of a buffer curve, or band membership
 * within the band simplification's 0.01 r; MGPU_CORE_DISTANCE: rows within the JTS
 * tolerance bands)}. */
#define MGPU_CORE_MOSAICFILL 0
#define MGPU_CORE_CLIP 1
#define MGPU_CORE_DISTANCE 2
int32_t mgpu_tessellate_ex(int32_t index_system, int32_t res, int64_t n_polys, const int32_t* polygon_id,
                           const int64_t* poly_part_off, const int64_t* part_ring_off, const int64_t* ring_off,
                           const double* xy, int32_t keep_core_geometries, int32_t core_rule, mgpu_tess** out);
/* mgpu_tessellate_geom: mgpu_tessellate_ex with the input geometries' types and the way
 * border chips are cut.  poly_type[n_polys] (NULL: MULTIPOLYGON iff several parts) holds
 * each geometry's WKB type, 3 = POLYGON or 6 = MULTIPOLYGON: coerceChipGeometry
 * (IndexSystem.scala:293-303) re-nodes a chip whose type differs from its polygon's.
 * chip_geometry: MGPU_CHIPS_OVERLAY (default) -- `polygon INTERSECTION cell` as JTS
 * OverlayNG computes it (RobustLineIntersector nodes, minimal result rings, separate pieces;
 * mosaic_amd/csrc/jts_overlay.h); MGPU_CHIPS_SUTHERLAND_HODGMAN -- rounds 1-5's ring clip
 * (its own crossing arithmetic, pieces bridged along the cell boundary), kept to count what
 * the overlay changes. */
#define MGPU_CHIPS_OVERLAY 0
#define MGPU_CHIPS_SUTHERLAND_HODGMAN 1
int32_t mgpu_tessellate_geom(int32_t index_system, int32_t res, int64_t n_polys, const int32_t* polygon_id,
                             const int64_t* poly_part_off, const int64_t* part_ring_off, const int64_t* ring_off,
                             const double* xy, const uint8_t* poly_type, int32_t keep_core_geometries,
                             int32_t core_rule, int32_t chip_geometry, mgpu_tess** out);
int32_t mgpu_tess_result_stats(const mgpu_tess* t, int64_t* out6);
/* mgpu_tess_result_core_stats: the first n of {rows, core rows, demoted, promoted,
 * dropped, ambiguous, carved tests, band tests, core rows whose centre is < r deep,
 * border rows whose centre is >= r deep, chip cells outside the band (dropped),
 * DP-sensitive rows, unresolved rows, polygons with an empty buffer(-r), border chips cut
 * by the overlay, ... of several pieces, ... re-noded by coerceChipGeometry, nodes that
 * re-noding added, ... whose overlay also gave lines / points}. */
int32_t mgpu_tess_result_core_stats(const mgpu_tess* t, int64_t* out, int32_t n);
int32_t mgpu_tess_result_sizes(const mgpu_tess* t, int64_t* n_chips, int64_t* wkb_bytes);
int32_t mgpu_tess_result_copy(const mgpu_tess* t, int64_t* cell, int32_t* polygon_id, uint8_t* is_core,
                              int64_t* wkb_offsets, uint8_t* wkb);
/* The rows the core rule left undecided (core_stats' ambiguous): n, their WKB bytes, and
 * when cell != NULL per row its cell, polygon, {kind (1 DP-sensitive band membership, 2 a
 * centre on a buffer curve), kept (the table holds the row), core}, and its chip -- the
 * one the table holds, or the one a dropped row would carry -- to count the pairs at stake. */
int32_t mgpu_tess_result_undecided(const mgpu_tess* t, int64_t* n, int64_t* wkb_bytes, int64_t* cell, int32_t* poly,
                                   uint8_t* kind_kept_core, int64_t* wkb_offsets, uint8_t* wkb);
/* frees the result (its memory returns on a helper thread, joined by the next
 * mgpu_tessellate* call and at unload: at most one result is in release at a time) */
int32_t mgpu_tess_destroy(mgpu_tess* t);

/* TEST ONLY -- not an interface of the reference.  Builds the chip table on the host
 * and evaluates st_contains(chip row, point) for n pairs by the join's path (the
 * classification grid + strip index of the device chip table) and by the sequential
 * JTS PointLocator; out_* = 1 / 0, -1 for a NULL geometry.  Host pointers; no GPU. */
int32_t mgpu_test_chip_contains_host(int32_t index_system, int64_t n_chips, const int64_t* cell,
                                     const int32_t* polygon_id, const uint8_t* is_core, const int64_t* wkb_offsets,
                                     const uint8_t* wkb, int64_t n, const int64_t* chip_row, const double* x,
                                     const double* y, int8_t* out_join_path, int8_t* out_point_locator);

/* TEST ONLY -- while on, every border chip the overlay's one-crossing-chain shortcut cuts
 * (jts_overlay.h Clipper::one_crossing_chain) is cut again by the general noded graph and
 * the two compared; out2 = {cells so checked, cells that differed} since it was turned on
 * (on = 1 resets the counts; on = 0 reads them and stops). */
int32_t mgpu_test_overlay_verify(int32_t on, int64_t* out2);

/* TEST ONLY -- the decimal parser of the WKT path (Double.parseDouble semantics) on one
 * string: characters consumed (0: not a number) and the value.  Host only. */
int32_t mgpu_test_parse_number(const char* s, int32_t len, double* out);
/* TEST ONLY -- the WKB / WKT point decoder on one host row: status 0 ok, 1 malformed,
 * 2 unsupported type, 3 empty. */
/* Test hooks of the exact H3 route (h3_exact.h), host-side: the route's elementary
 * operations (fn codes as oracle/oracle.h orc_h3_elementary: correctly rounded libm and
 * emulated x87 long-double expressions; 14 and 15: the correctly rounded asin and atan of
 * the cell-geometry route), and point -> cell by the route alone. */
int32_t mgpu_test_h3_elementary_host(int32_t fn, const double* a, const double* b, int64_t n, double* out);
int32_t mgpu_test_h3_route_host(const double* lon, const double* lat, int64_t n, int32_t res, int64_t* out_cell);
/* The near-tie resolver of the synchronous calls (h3_glibc.cpp: the reference's libm and
 * x87 arithmetic) on n host points. */
int32_t mgpu_test_h3_glibc_host(const double* lon, const double* lat, int64_t n, int32_t res, int64_t* out_cell);
/* H3 cell geometry as the builder computes it (h3ToGeoBoundary / h3ToGeo, degrees):
 * out_lonlat[20 n] (up to 10 vertices per cell), out_nverts[n], out_center[2 n]. */
int32_t mgpu_test_h3_boundary_host(const int64_t* cells, int64_t n, double* out_lonlat, int32_t* out_nverts,
                                   double* out_center);
/* The cell-geometry kernels' host twin: the code of mgpu_cells_to_boundaries / _centers /
 * _area compiled for the host (no GPU).  Host pointers: out_xy[20 n], out_nverts[n],
 * out_center[2 n] (optional; NaN for BNG), out_area[n] (optional). */
int32_t mgpu_test_cell_geometry_host(int32_t index_system, const int64_t* cells, int64_t n, double* out_xy,
                                     int32_t* out_nverts, double* out_center, double* out_area);
/* TEST ONLY: mgpu_grid_polyfill's host twin -- the same plan walked by the same code on the
 * host (no GPU), host pointers throughout; the same lists in the same order. */
int32_t mgpu_test_grid_polyfill_host(int32_t index_system, int32_t res, int64_t n_polys, const int64_t* poly_part_off,
                                     const int64_t* part_ring_off, const int64_t* ring_off, const double* xy,
                                     int64_t* out_cells, int64_t capacity, int64_t* out_offsets, int64_t* out_total);
/* TEST ONLY (and tools/polyfill_time.py): figures of the last mgpu_grid_polyfill or
 * mgpu_test_grid_polyfill_host call made on the CALLING THREAD (thread-local state, overwritten
 * by either entry; zeros before the first call): out8 = lattice samples, tiles, certificate
 * failures over all attempts, attempts (1 = the first spacing held), device microseconds of the
 * last attempt's launches between two events on its stream (the host twin: 0), 0, 0, 0. */
int32_t mgpu_test_grid_polyfill_last(int64_t* out8);
/* TEST ONLY: mgpu_geometry_kring's host twin -- the same contract on host arrays (no GPU), from
 * the ring code the kernels run compiled for the host (h3_ring.h, bng_core.h); the same bytes. */
int32_t mgpu_test_geometry_kring_host(int32_t index_system, int64_t n_geoms, const int64_t* row_off, const int64_t* cell,
                                      const uint8_t* is_core, int32_t k, int32_t loop_only, int64_t* out_cells,
                                      int64_t capacity, int64_t* out_offsets, int64_t* out_total);
/* TEST ONLY (and tools/geomring_time.py): figures of the last mgpu_geometry_kring or
 * mgpu_test_geometry_kring_host call made on the CALLING THREAD (thread-local, overwritten by
 * either entry; zeros before the first call): out8 = geometries finished on the LDS path,
 * geometries finished on the HBM path, slabs run, border cells, ids generated (the lists' ids plus
 * one per row), ids returned, microseconds between the first and last launch on the stream (host
 * waits in between included; the twin: 0), border cells that took an H3 pentagon fallback. */
int32_t mgpu_test_geometry_kring_last(int64_t* out8);
/* TEST ONLY: an H3 cell's geometry as a core chip of it carries it (indexToGeometry,
 * H3IndexSystem.scala:103-112: the polar caps of makePoleGeometry, antimeridian cells
 * cut) as WKB into out[cap]; *out_len = its size (MGPU_E_CAPACITY when it exceeds cap). */
int32_t mgpu_test_h3_cell_wkb_host(int64_t cell, uint8_t* out, int64_t cap, int64_t* out_len);
int32_t mgpu_test_decode_point(int32_t format, const uint8_t* data, int64_t len, double* x, double* y);
/* TEST ONLY (profiling): the last join's 16 workspace counters (pairs, near-ties, invalid
 * points, candidates, ...; builds with -DMGPU_STAMPS add per-phase clock ticks of the
 * join tiles at [10..14]).  Waits for the device. */
int32_t mgpu_test_join_counters(mgpu_ctx* ctx, uint64_t* out16);
/* TEST ONLY: the classify kernels' finer block table of an uploaded table (derived on the
 * device when the table is adopted).  dims[7] = raster_nx, raster_ny, the block shifts sx
 * and sy, the table's columns and rows, and 1 when the table has one (else the four before
 * it are 0).  geom[8] (or NULL) = the pixel grid's origin x0, y0 and scales 1 / dx, 1 / dy
 * (pixel = ((lon - x0) / dx, (lat - y0) / dy) truncated, clamped to the last one) and the
 * table's box lon_min, lat_min, lon_max, lat_max.  out_classes (or NULL): the raster_ny *
 * raster_nx 16-bit pixel classes the table was derived from; out_fine (or NULL): its rows *
 * columns bytes -- both host arrays, row-major. */
int32_t mgpu_test_fine_table(const mgpu_chips* chips, int64_t* dims, double* geom, uint16_t* out_classes,
                             uint8_t* out_fine);
/* TEST ONLY: the host part of mgpu_chips_polygons (poly_slots.h) -- the distinct values
 * of polygon_id[n] ascending into out_ids (room for n), *out_n their number, and
 * out_slot_of_row[i] = the slot of polygon_id[i]. */
int32_t mgpu_test_poly_slots_host(const int32_t* polygon_id, int64_t n, int32_t* out_ids, int64_t* out_n,
                                  uint32_t* out_slot_of_row);

/* TEST ONLY: the centroids of n InternalGeometryType rows (layout of
 * mgpu_internal_geometry_to_cells) on the host; status[i] 0 ok, 1 malformed, 2 unsupported,
 * 3 empty. */
int32_t mgpu_test_internal_centroid(int64_t n, const int32_t* type_id, const int64_t* row_part, const int64_t* part_ring,
                                    const int64_t* ring_off, const double* xy, double* x, double* y, int32_t* status);

/* TEST ONLY -- st_contains(chip row, point) evaluated on a HOST blob (the join's
 * classification grid + strip path), to check on the CPU that a shipped blob is a
 * complete chip table.  out = 1 / 0, -1 NULL geometry.  Host pointers; no GPU. */
int32_t mgpu_test_blob_contains_host(const void* host_blob, int64_t bytes, int64_t n, const int64_t* chip_row,
                                     const double* x, const double* y, int8_t* out);

/* TEST ONLY -- not an interface of the reference.  Builds the chip table on the host and
 * looks n points up in its pixel index (the pre-resolved answers of the streaming join,
 * chip_table.h): out_kind 0 = no match, 1 = pure pixel (matches = sorted chips
 * out_first + j for the bits j of out_mask), 2 = full path, 3 = invalid coordinate,
 * 4 = no pixel index for this table/resolution; out_chip_poly[n_chips] = polygon id of
 * each sorted chip.  Host pointers; no GPU. */
int32_t mgpu_test_raster_host(int32_t index_system, int32_t res, int64_t n_chips, const int64_t* cell,
                              const int32_t* polygon_id, const uint8_t* is_core, const int64_t* wkb_offsets,
                              const uint8_t* wkb, int64_t n, const double* x, const double* y, int8_t* out_kind,
                              uint32_t* out_first, uint32_t* out_mask, int32_t* out_chip_poly);

/* TEST ONLY -- as mgpu_test_raster_host, for the BNG per-cell answer grids the fused
 * join's phase 1 reads (chip_table.h cell_ans): out_kind 0 / 1 = answered, 2 = not
 * answered (candidates' path), 3 = invalid coordinate, 4 = the table has none.
 * MGPU_E_INVALID_ARG for H3.  Host pointers; no GPU. */
int32_t mgpu_test_cell_answers_host(int32_t index_system, int32_t res, int64_t n_chips, const int64_t* cell,
                                    const int32_t* polygon_id, const uint8_t* is_core, const int64_t* wkb_offsets,
                                    const uint8_t* wkb, int64_t n, const double* x, const double* y, int8_t* out_kind,
                                    uint32_t* out_first, uint32_t* out_mask, int32_t* out_chip_poly);

/* TEST ONLY -- as mgpu_test_raster_host, for the H3 whole-cell shortcut of the streaming
 * joins (a one-chip cell whose chip is its own hexagon, a point deep inside the cell):
 * out_kind 1 = answered (chip out_first), 2 = not answered, 3 = invalid coordinate,
 * 4 = no dense H3 probe.  MGPU_E_INVALID_ARG for BNG.  Host pointers; no GPU. */
int32_t mgpu_test_whole_cells_host(int32_t index_system, int32_t res, int64_t n_chips, const int64_t* cell,
                                   const int32_t* polygon_id, const uint8_t* is_core, const int64_t* wkb_offsets,
                                   const uint8_t* wkb, int64_t n, const double* x, const double* y, int8_t* out_kind,
                                   uint32_t* out_first, uint32_t* out_mask, int32_t* out_chip_poly);

#ifdef __cplusplus
}
#endif

#endif /* MOSAIC_GPU_H */

"""mosaic_amd -- MI355X-native grid-indexed point-in-polygon join.

A drop-in for the hot path of Databricks Labs Mosaic 0.4.3 (tiems90/mosaic):
grid_pointascellid / grid_longlatascellid, grid_tessellateexplode chips with
is_core, st_contains on chip WKB, and their join -- behind the IndexSystem
plugin boundary (H3IndexSystem, BNGIndexSystem).  Compute runs in hand-written
gfx950 HIP kernels (mosaic_amd/csrc, C ABI in include/mosaic_gpu.h); there is
no CPU fallback on the data path.
"""
from ._native import (CapacityError, IllegalArgumentException, IllegalStateException, MosaicGpuError,
                      EXPORTS, LIB_PATH)
from .chips import ChipTable, DeviceChips, Polygons, tessellate
from .context import GpuContext, MosaicContext, default_context
from .functions import (AsyncJoin, CellAggregate, CellCounts, CountResult, GeometryColumn, GeometryRings, InternalGeometryColumn, JoinResult, LookupResult, grid_boundary, grid_boundaryaswkb, grid_cellarea, grid_cellcount, grid_cellkloop, grid_cellkring, grid_geometrykloop, grid_geometrykloopexplode, grid_geometrykring, grid_geometrykringexplode, grid_longlatascellid, grid_pointascellid, grid_polyfill,
                        grid_ring_join, grid_ring_join_final, grid_tessellateexplode, pip_join, pip_join_async, pip_join_count, pip_join_lookup, points_from_geometry, st_contains)
from .index_system import BNGIndexSystem, H3IndexSystem, IndexSystem, get_index_system

__version__ = "0.1.0"

__all__ = [
    "AsyncJoin", "BNGIndexSystem", "CapacityError", "CellAggregate", "CellCounts", "ChipTable", "CountResult", "DeviceChips", "EXPORTS", "GeometryColumn", "GeometryRings", "GpuContext", "InternalGeometryColumn", "H3IndexSystem",
    "IllegalArgumentException", "IllegalStateException", "IndexSystem", "JoinResult", "LIB_PATH", "LookupResult",
    "MosaicContext", "MosaicGpuError", "Polygons", "default_context", "get_index_system", "grid_boundary", "grid_boundaryaswkb", "grid_cellarea", "grid_cellcount", "grid_cellkloop",
    "grid_cellkring", "grid_geometrykloop", "grid_geometrykloopexplode", "grid_geometrykring", "grid_geometrykringexplode", "grid_longlatascellid", "grid_polyfill",
    "grid_pointascellid", "grid_ring_join", "grid_ring_join_final", "grid_tessellateexplode", "pip_join", "pip_join_async", "pip_join_count", "pip_join_lookup", "points_from_geometry", "st_contains", "tessellate",
]

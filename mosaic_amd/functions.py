"""The hot-path function surface, as the reference registers it.

  grid_longlatascellid(lon, lat, res)   MosaicContext.scala:429-432 -> PointIndexLonLat.scala:44-51
  grid_pointascellid(point, res)        MosaicContext.scala:453-457 -> PointIndexGeom.scala:33-47
  grid_tessellateexplode(geom, res)     MosaicContext.scala:400-408 -> MosaicExplode.scala:70-79
  st_contains(chip.wkb, point)          MosaicContext.scala:166     -> ST_Contains.scala:21-44
  pip_join(points, chips, res)          the user-level join of the Quickstart notebooks
                                        (QuickstartNotebook.ipynb:1835): cell == index_id
                                        AND (is_core OR st_contains(wkb, point))

Column arguments are float64 device tensors (structure of arrays); results stay in HBM.
"""
import numpy as np

from . import _native as N
from .chips import ChipTable, DeviceChips, tessellate
from .index_system import H3IndexSystem, _check_points

_H3 = H3IndexSystem()


def grid_longlatascellid(lon, lat, resolution, index_system=None, ctx=None, stream=None, stats=False,
                         cell_id_type="long"):
    """Cell id of every (lon, lat) -- (eastings, northings) for BNG.

    cell_id_type "long": an int64 tensor (LongType).  "string": the StringType ids
    (IndexSystem.serializeCellId -- BNG's default cell id type, BNGIndexSystem.scala:30),
    formatted on the device: (chars uint8 tensor, offsets int64 tensor of n + 1)."""
    isys = index_system or _H3
    out = isys.points_to_index(lon, lat, resolution, ctx=ctx, stream=stream, stats=stats)
    if cell_id_type == "long":
        return out
    if cell_id_type != "string":
        raise N.IllegalArgumentException(N.MGPU_E_INVALID_ARG, "cell_id_type must be 'long' or 'string'")
    cells, st = out if stats else (out, None)
    strs = isys.format_device(cells, ctx=ctx, stream=stream)
    return (strs, st) if stats else strs


class GeometryColumn:
    """A geometry column in device memory as Arrow lays out binary / utf8: one byte buffer,
    int64 offsets (n + 1), optional validity bitmap (LSB first, 1 = present).  Format:
    MGPU_GEOM_WKB (BinaryType), _WKT (StringType), _HEX (HexType: hex WKB text) or
    _GEOJSON (JSONType), GeometryAPI.geometry's input types (GeometryAPI.scala:81-89)."""

    FORMATS = {"wkb": N.MGPU_GEOM_WKB, "wkt": N.MGPU_GEOM_WKT, "hex": N.MGPU_GEOM_HEX, "geojson": N.MGPU_GEOM_GEOJSON}

    def __init__(self, fmt, data, offsets, valid=None, valid_offset=0):
        """``valid_offset``: the bit of row 0 in ``valid`` (a sliced column: ``offsets`` a
        view of the parent's from that row on, the bitmap the parent's)."""
        self.format, self.data, self.offsets, self.valid = fmt, data, offsets, valid
        self.valid_offset = int(valid_offset)

    def __len__(self):
        return self.offsets.numel() - 1

    @staticmethod
    def from_rows(rows, device="cuda", fmt=None):
        """Python rows (bytes: WKB, str: WKT unless `fmt` says "hex" / "geojson", None:
        null) -> device column."""
        import torch
        kinds = {type(r) for r in rows if r is not None}
        if len(kinds) > 1:
            raise N.IllegalArgumentException(N.MGPU_E_INVALID_ARG, "mixed binary and text rows")
        code = GeometryColumn.FORMATS[fmt] if fmt else (N.MGPU_GEOM_WKT if kinds == {str} else N.MGPU_GEOM_WKB)
        bs = [b"" if r is None else (r.encode() if isinstance(r, str) else bytes(r)) for r in rows]
        off = np.zeros(len(bs) + 1, np.int64)
        off[1:] = np.cumsum([len(b) for b in bs])
        data = np.frombuffer(b"".join(bs) or b"\0", np.uint8)
        valid = None
        if any(r is None for r in rows):
            valid = np.packbits(np.array([r is not None for r in rows], bool), bitorder="little")
            valid = torch.from_numpy(valid).to(device)
        return GeometryColumn(code, torch.from_numpy(data.copy()).to(device), torch.from_numpy(off).to(device), valid)


class InternalGeometryColumn:
    """Mosaic's InternalGeometryType column (InternalGeometry.scala: typeId, boundaries,
    holes) flattened as nested lists in device memory (mgpu_internal_geometry_to_cells):
    type_id[n]; row_part[n + 1]; part_ring[P + 1] (each part's boundary, then its holes);
    ring_off[R + 1]; xy[2 V].  ``valid``: optional validity bitmap (LSB first, 1 = present),
    row 0's bit at ``valid_offset`` (a sliced column: type_id / row_part views of the
    parent's from that row on)."""

    def __init__(self, type_id, row_part, part_ring, ring_off, xy, valid=None, valid_offset=0):
        self.type_id, self.row_part, self.part_ring, self.ring_off, self.xy = type_id, row_part, part_ring, ring_off, xy
        self.valid, self.valid_offset = valid, int(valid_offset)

    def __len__(self):
        return self.type_id.numel()

    @staticmethod
    def from_rows(rows, device="cuda"):
        """rows: (type_id, parts), parts = [[ring, ring, ...], ...] (boundary first), a
        ring a list of (x, y)."""
        import torch
        tid, rp, pr, ro, xy = [], [0], [0], [0], []
        for t, parts in rows:
            tid.append(t)
            for part in parts:
                for ring in part:
                    xy.extend(ring)
                    ro.append(len(xy))
                pr.append(len(ro) - 1)
            rp.append(len(pr) - 1)
        T = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(device)
        return InternalGeometryColumn(T(tid, np.int32), T(rp, np.int64), T(pr, np.int64), T(ro, np.int64),
                                      T(np.array(xy, np.float64).reshape(-1, 2) if xy else np.zeros((1, 2)), np.float64))


def _valid_buffer(out_valid, n, dev):
    """The output bitmap of a geometry call: the caller's buffer (checked), or a fresh one."""
    import torch
    if out_valid is None:
        return torch.empty((n + 7) // 8 + 1, dtype=torch.uint8, device=dev)
    if out_valid.dtype != torch.uint8 or out_valid.device != dev or not out_valid.is_contiguous() \
            or out_valid.numel() < (n + 7) // 8:
        raise N.IllegalArgumentException(N.MGPU_E_INVALID_ARG, "out_valid must be a contiguous uint8 tensor of at "
                                         "least (n + 7) // 8 bytes on the column's device")
    return out_valid


def grid_pointascellid(points, resolution, index_system=None, ctx=None, stream=None, stats=False, out_valid=None):
    """grid_pointascellid (PointIndexGeom.scala:33-47): the cell of each row's centroid.

    ``points``: a GeometryColumn (WKB / HEX rows of any type, WKT / GeoJSON POINT or
    MULTIPOINT rows, decoded on the GPU and reduced to JTS's centroid; null rows give
    cell 0 -- returned with the validity bitmap as (cells, valid)), an
    InternalGeometryColumn (the same with a bitmap), an (n, 2) float64 tensor, or an (x, y)
    pair (a point's centroid is the point itself, MosaicGeometryJTS.scala:60-64).  Types a
    format does not build raise MGPU_E_UNSUPPORTED, an empty geometry IllegalStateException
    (JTS getX on an empty point).  ``out_valid``: a caller-owned uint8 device buffer of at
    least (n + 7) // 8 bytes for the returned bitmap (geometry columns; returned whole)."""
    if isinstance(points, (InternalGeometryColumn, GeometryColumn)):
        import ctypes
        import torch
        from .context import default_context
        isys = index_system or _H3
        res = isys.get_resolution(resolution)
        internal = isinstance(points, InternalGeometryColumn)
        dev = points.type_id.device if internal else points.offsets.device
        ctx = ctx or default_context(dev)
        n = len(points)
        cells = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        valid = _valid_buffer(out_valid, n, dev) if (points.valid is not None or out_valid is not None) else None
        in_valid = None if points.valid is None else points.valid.data_ptr()
        out_ptr = None if valid is None else valid.data_ptr()
        st = N.MgpuStats()
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        if internal:
            N.check(N.lib().mgpu_internal_geometry_to_cells(ctx.handle, isys.code, res, n, points.type_id.data_ptr(),
                                                            points.row_part.data_ptr(), points.part_ring.data_ptr(),
                                                            points.ring_off.data_ptr(), points.xy.data_ptr(), in_valid,
                                                            points.valid_offset, cells.data_ptr(), out_ptr, s,
                                                            ctypes.byref(st)))
        else:
            N.check(N.lib().mgpu_geometry_to_cells(ctx.handle, isys.code, res, points.format, points.data.data_ptr(),
                                                   points.offsets.data_ptr(), in_valid, points.valid_offset, n,
                                                   cells.data_ptr(), out_ptr, s, ctypes.byref(st)))
        if valid is None:
            out = cells[:n]
        else:
            out = (cells[:n], valid if out_valid is not None else valid[:(n + 7) // 8])
        return (out, st.as_dict()) if stats else out
    if isinstance(points, (tuple, list)):
        x, y = points
    else:
        x, y = points[:, 0].contiguous(), points[:, 1].contiguous()
    return grid_longlatascellid(x, y, resolution, index_system=index_system, ctx=ctx, stream=stream, stats=stats)


def points_from_geometry(col, ctx=None, stream=None):
    """mgpu_points_from_geometry: the centroid of every row of a GeometryColumn as two
    float64 device tensors (x, y); a null row gives NaN in both."""
    import torch
    from .context import default_context
    dev = col.offsets.device
    ctx = ctx or default_context(dev)
    n = len(col)
    x = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
    y = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
    s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
    N.check(N.lib().mgpu_points_from_geometry(ctx.handle, col.format, col.data.data_ptr(), col.offsets.data_ptr(),
                                              None if col.valid is None else col.valid.data_ptr(), col.valid_offset,
                                              n, x.data_ptr(), y.data_ptr(), s))
    return x[:n], y[:n]


def grid_cellkring(cells, k, index_system, loop_only=False, ctx=None, stream=None):
    """grid_cellkring / grid_cellkloop (CellKRing.scala:68, CellKLoop.scala:63 ->
    IndexSystem.kRing / kLoop) over a device int64 column, on the GPU (BNG and H3; H3
    pentagon neighbourhoods in the reference's fallback order), for k in [0, 1024], else
    IllegalArgumentException (MGPU_E_INVALID_ARG).  Returns
    (ids int64 tensor, offsets int64 tensor of n + 1): cell i's list is
    ids[offsets[i]:offsets[i + 1]], in the reference's order."""
    import ctypes
    import torch
    from .context import default_context
    if cells.dtype != torch.int64 or not cells.is_cuda:
        raise N.IllegalArgumentException(N.MGPU_E_INVALID_ARG, "cells must be an int64 device tensor")
    cells = cells.contiguous()
    ctx = ctx or default_context(cells.device)
    n = cells.numel()
    k = int(k)
    per = max(8 * k, 1) if loop_only else 1 + 4 * k * (k + 1)  # H3 hexRing(0) = [cell]
    cap = max(n * per, 1)
    out = torch.empty(cap, dtype=torch.int64, device=cells.device)
    off = torch.empty(n + 1, dtype=torch.int64, device=cells.device)
    tot = ctypes.c_int64()
    s = stream if stream is not None else torch.cuda.current_stream(cells.device).cuda_stream
    N.check(N.lib().mgpu_grid_kring(ctx.handle, index_system.code, cells.data_ptr(), n, k, 1 if loop_only else 0,
                                    out.data_ptr(), cap, off.data_ptr(), ctypes.byref(tot), s),
            required=tot.value)
    return out[:tot.value], off


def grid_cellkloop(cells, k, index_system, ctx=None, stream=None):
    """grid_cellkloop (CellKLoop.scala:63 -> IndexSystem.kLoop) on the GPU (BNG, H3)."""
    return grid_cellkring(cells, k, index_system, loop_only=True, ctx=ctx, stream=stream)


_POLYFILL_FIRST_CAPACITY = 1 << 24  # cells (128 MiB): beyond it the reported total sizes the second call


def _polyfill_capacity(polygons, index_system, res):
    """A first output capacity for grid_polyfill: the rings' areas over the index system's
    cell area, so that the usual set fits at the first call (a short buffer costs a second
    pass); at most _POLYFILL_FIRST_CAPACITY -- a larger set is sized by the total the first call
    reports, as grid_cellkring's buffer is."""
    xy, ro = polygons.xy, polygons.ring_off
    if len(xy) < 2 or len(ro) < 2:
        return 1024
    cross = xy[:-1, 0] * xy[1:, 1] - xy[1:, 0] * xy[:-1, 1]
    csum = np.concatenate([[0.0], np.cumsum(cross)])
    # (ring r's edges are the cross products ro[r] .. ro[r + 1] - 2: the one joining two rings is left out)
    last = np.maximum(ro[1:] - 1, ro[:-1])
    area = 0.5 * np.abs(csum[last] - csum[ro[:-1]])
    cells = float(np.sum(area / index_system.cell_area_estimate(res, xy[np.minimum(ro[:-1], len(xy) - 1), 1])))
    if not np.isfinite(cells):
        cells = 0.0
    return int(min(max(1.25 * cells + 64 * len(polygons), 1024), _POLYFILL_FIRST_CAPACITY))


def grid_polyfill(polygons, resolution, index_system=None, ctx=None, stream=None):
    """grid_polyfill(geometry, resolution) (expressions/index/Polyfill.scala -> IndexSystem.polyfill)
    over a polygon set (``Polygons``), on the GPU (H3, BNG): for each polygon the cells whose
    centre lies in its interior.  Returns (cells int64 device tensor, offsets int64 device
    tensor of n + 1): polygon p's cells are cells[offsets[p]:offsets[p + 1]], in the order of
    the lattice laid over its bounding box (deterministic; not the reference's hash-set order),
    no cell twice.  The full set: the reference's flood fill / BFS can miss a matching cell that
    no chain of matching neighbours joins to a seed."""
    import ctypes
    import torch
    from .context import default_context
    from .index_system import H3IndexSystem
    index_system = index_system or H3IndexSystem()
    res = index_system.get_resolution(resolution)
    ctx = ctx or default_context()
    dev = ctx.device
    n = len(polygons)
    off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    tot = ctypes.c_int64()
    s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
    cap = _polyfill_capacity(polygons, index_system, res)  # grown to the reported size when the set needs more
    while True:
        out = torch.empty(cap, dtype=torch.int64, device=dev)
        st = N.lib().mgpu_grid_polyfill(ctx.handle, index_system.code, res, n, polygons.poly_part_off.ctypes.data,
                                        polygons.part_ring_off.ctypes.data, polygons.ring_off.ctypes.data,
                                        polygons.xy.ctypes.data, out.data_ptr(), cap, off.data_ptr(), ctypes.byref(tot), s)
        if st != N.MGPU_E_CAPACITY or tot.value <= cap:
            break
        cap = tot.value
    N.check(st, required=tot.value)
    return out[:tot.value], off


class GeometryRings:
    """grid_geometrykring / grid_geometrykloop of a batch: ``ids`` (int32 numpy array: the
    geometries' polygon ids, ascending, as ``DeviceChips.polygons()`` orders them; 0 .. n - 1 for
    geometries without ids), ``cells`` (int64 device tensor) and ``offsets`` (int64 device tensor of
    len(ids) + 1): geometry ids[g]'s cells are cells[offsets[g]:offsets[g + 1]], ascending."""

    def __init__(self, ids, cells, offsets):
        self.ids, self.cells, self.offsets = ids, cells, offsets

    def __len__(self):
        return len(self.ids)

    def lists(self):
        """The lists on the host: one int64 numpy array per geometry."""
        c, o = self.cells.cpu().numpy(), self.offsets.cpu().numpy()
        return [c[o[g]:o[g + 1]] for g in range(len(self.ids))]

    def explode(self):
        """(row, cell) device columns, one row per (geometry, cell): row g repeated for each of
        its cells -- the explode forms' output."""
        import torch
        n = self.offsets[1:] - self.offsets[:-1]
        row = torch.repeat_interleave(torch.arange(len(self.ids), dtype=torch.int64, device=self.cells.device), n)
        return row, self.cells


def _geometry_rows(geoms, index_system, resolution, ctx, stream):
    """(ids, row_off, cell, is_core, n_rows) of grid_geometrykring's ``geoms``, the three columns on the device."""
    import torch
    from .chips import Polygons
    dev = ctx.device
    if isinstance(geoms, Polygons):
        if resolution is None:
            raise N.IllegalArgumentException(N.MGPU_E_INVALID_ARG, "a Polygons set needs a resolution")
        geoms = tessellate(geoms, index_system, resolution, keep_core_geometries=False)  # (as Mosaic.getCellSets)
    if isinstance(geoms, ChipTable):
        if geoms.index_system != index_system.code:
            raise N.IllegalArgumentException(N.MGPU_E_INVALID_ARG, "the chip table belongs to another index system")
        order = np.argsort(geoms.polygon_id, kind="stable")
        pid = geoms.polygon_id[order]
        ids = np.unique(pid).astype(np.int32)
        row_off = np.append(np.searchsorted(pid, ids, side="left"), len(pid)).astype(np.int64)
        return (ids, torch.from_numpy(row_off).to(dev), torch.from_numpy(geoms.cell[order]).to(dev),
                torch.from_numpy(geoms.is_core[order]).to(dev), len(pid))
    if isinstance(geoms, (tuple, list)) and len(geoms) == 3:
        row_off, cell, is_core = geoms
        if (row_off.dtype != torch.int64 or cell.dtype != torch.int64 or is_core.dtype not in (torch.uint8, torch.bool)
                or not (row_off.is_cuda and cell.is_cuda and is_core.is_cuda) or row_off.numel() < 1
                or cell.numel() != is_core.numel()):
            raise N.IllegalArgumentException(N.MGPU_E_INVALID_ARG, "(row_off int64, cell int64, is_core uint8) device tensors expected")
        is_core = is_core.contiguous()
        if is_core.dtype == torch.bool:
            is_core = is_core.view(torch.uint8)
        n = row_off.numel() - 1
        return np.arange(n, dtype=np.int32), row_off.contiguous(), cell.contiguous(), is_core, cell.numel()
    if isinstance(geoms, (tuple, list)) and len(geoms) == 2:
        if resolution is None:
            raise N.IllegalArgumentException(N.MGPU_E_INVALID_ARG, "point columns need a resolution")
        x, y = geoms
        cell = grid_longlatascellid(x, y, resolution, index_system, ctx=ctx, stream=stream)  # (Mosaic.pointChip: one border chip)
        n = cell.numel()
        return (np.arange(n, dtype=np.int32), torch.arange(n + 1, dtype=torch.int64, device=dev), cell,
                torch.zeros(n, dtype=torch.uint8, device=dev), n)
    raise N.IllegalArgumentException(N.MGPU_E_INVALID_ARG, "geoms: a ChipTable, a Polygons set, (row_off, cell, is_core) or (x, y)")


def _geometry_rings(geoms, k, index_system, resolution, loop_only, ctx, stream):
    import ctypes
    import torch
    from .context import default_context
    if ctx is None:
        t = geoms[0] if isinstance(geoms, (tuple, list)) else None
        ctx = default_context(t.device) if t is not None and getattr(t, "is_cuda", False) else default_context()
    dev = ctx.device
    k = int(k)
    s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
    ids, row_off, cell, is_core, n_rows = _geometry_rows(geoms, index_system, resolution, ctx, s if stream is not None else None)
    n = len(ids)
    off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    tot = ctypes.c_int64()
    # a first capacity: per row its own cell and the cells a border row adds along a border line,
    # per geometry one whole list; grown once to the reported total when the sets need more
    one = 8 * max(k, 1) if loop_only else 1 + 4 * k * (k + 1)
    cap = int(min(n_rows * one, n_rows * (2 * k + 2) + n * one) + 1024)
    while True:
        out = torch.empty(cap, dtype=torch.int64, device=dev)
        st = N.lib().mgpu_geometry_kring(ctx.handle, index_system.code, n, row_off.data_ptr(), cell.data_ptr(),
                                         is_core.data_ptr(), k, 1 if loop_only else 0, out.data_ptr(), cap, off.data_ptr(),
                                         ctypes.byref(tot), s)
        if st != N.MGPU_E_CAPACITY or tot.value <= cap:
            break
        cap = tot.value
    N.check(st, required=tot.value)
    return GeometryRings(ids, out[:tot.value], off)


def grid_geometrykring(geoms, k, index_system, resolution=None, ctx=None, stream=None):
    """grid_geometrykring(geometry, resolution, k) (expressions/index/GeometryKRing.scala ->
    Mosaic.geometryKRing, core/Mosaic.scala:123-137) over a batch, on the GPU (H3, BNG): per
    geometry, its core cells and the k-rings of its border cells, every cell once, ascending.
    ``geoms``: a ``ChipTable`` (rows grouped by polygon id), a ``(row_off, cell, is_core)`` triple
    of device tensors (geometry g owns rows row_off[g]:row_off[g + 1]), a ``Polygons`` set with
    ``resolution`` (tessellated without core geometries, as the reference does), or an ``(x, y)``
    pair of float64 device columns with ``resolution`` (each point one border chip).  Returns a
    ``GeometryRings``.  k in [0, 1024]."""
    return _geometry_rings(geoms, k, index_system, resolution, False, ctx, stream)


def grid_geometrykloop(geoms, k, index_system, resolution=None, ctx=None, stream=None):
    """grid_geometrykloop (GeometryKLoop.scala -> Mosaic.geometryKLoop, core/Mosaic.scala:139-156):
    the k-loops of the border cells without the core cells and the border cells' (k - 1)-rings;
    arguments and result as grid_geometrykring.  k in [1, 1024]."""
    return _geometry_rings(geoms, k, index_system, resolution, True, ctx, stream)


def grid_geometrykringexplode(geoms, k, index_system, resolution=None, ctx=None, stream=None):
    """grid_geometrykringexplode: grid_geometrykring as (row, cell) device columns, one row per cell."""
    return grid_geometrykring(geoms, k, index_system, resolution, ctx, stream).explode()


def grid_geometrykloopexplode(geoms, k, index_system, resolution=None, ctx=None, stream=None):
    """grid_geometrykloopexplode: grid_geometrykloop as (row, cell) device columns, one row per cell."""
    return grid_geometrykloop(geoms, k, index_system, resolution, ctx, stream).explode()


def grid_boundaryaswkb(cells, index_system, valid=None, valid_offset=0, ctx=None, stream=None):
    """grid_boundaryaswkb (IndexGeometry.scala:65-75 -> IndexSystem.indexToGeometry, as WKB)
    over a device int64 column, on the GPU (H3, BNG).  Returns (bytes uint8 tensor, offsets
    int64 tensor of n + 1) like IndexSystem.format_device: row i is
    bytes[offsets[i]:offsets[i + 1]] -- a Polygon of the cell's closed boundary; an H3 cell
    holding a pole is the reference's polar cap, one across the antimeridian its two parts.
    ``valid``: an optional Arrow validity bitmap (uint8 device tensor) read from bit
    ``valid_offset``; null rows are empty, and the rows' bitmap (bit offset 0) comes back as
    a third element.  A non-null row that is not a cell id raises IllegalArgumentException."""
    return index_system.cells_boundary_wkb(cells, valid=valid, valid_offset=valid_offset, ctx=ctx, stream=stream)


def grid_boundary(cells, fmt, index_system, valid=None, valid_offset=0, ctx=None, stream=None):
    """grid_boundary(cell, format) (IndexGeometry.scala:65-75).  The device path writes WKB
    only: "WKT", "GEOJSON" and "COORDS" need Java's Double.toString and raise
    IllegalArgumentException."""
    if str(fmt).upper() != "WKB":
        raise N.IllegalArgumentException(N.MGPU_E_INVALID_ARG, "grid_boundary: format %r is not on the device path "
                                         "(WKB only)" % (fmt,))
    return grid_boundaryaswkb(cells, index_system, valid=valid, valid_offset=valid_offset, ctx=ctx, stream=stream)


def grid_cellarea(cells, index_system, valid=None, valid_offset=0, ctx=None, stream=None):
    """grid_cellarea (CellArea.scala -> IndexSystem.area) over a device int64 column, on the
    GPU: km^2 as a float64 device tensor (NaN in null rows; with ``valid`` the rows' bitmap
    as a second element)."""
    return index_system.cells_area(cells, valid=valid, valid_offset=valid_offset, ctx=ctx, stream=stream)


def grid_tessellateexplode(polygons, resolution, keep_core_geometries=True, index_system=None):
    """Chip rows (is_core, index_id, wkb) of every polygon -> ChipTable (host columns)."""
    return tessellate(polygons, index_system or _H3, resolution, keep_core_geometries)


def st_contains(chips, chip_rows, x, y, stream=None):
    """st_contains(chip.wkb, point) for explicit pairs: int8 tensor of 1 / 0, -1 where the
    chip geometry is NULL (SQL null)."""
    import torch
    if isinstance(chips, ChipTable):
        chips = chips.upload()
    _check_points(x, y)
    rows = chip_rows.to(device=x.device, dtype=torch.int64).contiguous()
    if rows.numel() != x.numel():
        raise N.IllegalArgumentException(N.MGPU_E_INVALID_ARG, "chip_rows and points differ in length")
    out = torch.empty(x.numel(), dtype=torch.int8, device=x.device)
    s = stream if stream is not None else torch.cuda.current_stream(x.device).cuda_stream
    N.check(N.lib().mgpu_st_contains(chips.ctx.handle, chips.handle, rows.data_ptr(), x.data_ptr(), y.data_ptr(),
                                     x.numel(), out.data_ptr(), s))
    return out


class JoinResult:
    def __init__(self, point_id, polygon_id, stats):
        self.point_id = point_id
        self.polygon_id = polygon_id
        self.stats = stats

    def __len__(self):
        return self.point_id.numel()

    def numpy(self):
        return self.point_id.cpu().numpy(), self.polygon_id.cpu().numpy()


def pip_join(x, y, chips, resolution, index_system=None, point_id=None, point_id_base=0, capacity=None,
             out=None, stream=None):
    """The grid-indexed point-in-polygon join (fused, one kernel).

    Returns a JoinResult with int64 point ids and int32 polygon ids ordered by input
    position then polygon id.  ``capacity`` bounds the output (default: n + 1/8 n
    headroom; when the pairs do not fit, arrays of the exact count are allocated and
    filled from the join's kept records by mgpu_pip_join_fetch -- the join is not redone).
    ``out`` = (point ids, polygon ids) preallocated: with ``capacity`` None, pairs that do
    not fit them go to fresh arrays of the exact count the same way; an explicit
    ``capacity`` is a hard bound (CapacityError, with the count)."""
    import torch
    isys = index_system or _H3
    res = isys.get_resolution(resolution)
    if isinstance(chips, ChipTable):
        if chips.index_system != isys.code:
            raise N.IllegalArgumentException(N.MGPU_E_INVALID_ARG, "chip table built for another index system")
        chips = chips.upload()
    _check_points(x, y)
    n = x.numel()
    if chips.ctx.device != x.device:
        raise N.IllegalArgumentException(N.MGPU_E_INVALID_ARG, "chip table on %s, points on %s" % (chips.ctx.device, x.device))
    pid_ptr = None
    if point_id is not None:
        if point_id.dtype != torch.int64 or point_id.numel() != n or point_id.device != x.device:
            raise N.IllegalArgumentException(N.MGPU_E_INVALID_ARG, "point_id must be int64 on the points' device")
        point_id = point_id.contiguous()  # kept alive (bound here) until the call returns
        pid_ptr = point_id.data_ptr()
    s = stream if stream is not None else torch.cuda.current_stream(x.device).cuda_stream
    import ctypes
    if out is not None:
        op, oq = out
        cap = min(op.numel(), oq.numel())
    else:
        cap = int(capacity if capacity is not None else max(16, n + n // 8))
        op = torch.empty(cap, dtype=torch.int64, device=x.device)
        oq = torch.empty(cap, dtype=torch.int32, device=x.device)
    cnt = ctypes.c_int64()
    st = N.MgpuStats()
    status = N.lib().mgpu_pip_join(chips.ctx.handle, chips.handle, isys.code, res, x.data_ptr(), y.data_ptr(),
                                   pid_ptr, int(point_id_base), n, cap, ctypes.byref(cnt), op.data_ptr(),
                                   oq.data_ptr(), s, st)
    if status == N.MGPU_E_CAPACITY and capacity is None:
        # the join's records are kept: write them into arrays of the exact size
        cap = int(cnt.value)
        op = torch.empty(cap, dtype=torch.int64, device=x.device)
        oq = torch.empty(cap, dtype=torch.int32, device=x.device)
        status = N.lib().mgpu_pip_join_fetch(chips.ctx.handle, cap, ctypes.byref(cnt), op.data_ptr(), oq.data_ptr(), s)
    N.check(status, required=cnt.value)
    m = int(cnt.value)
    return JoinResult(op[:m], oq[:m], st.as_dict())


class CountResult:
    """pip_join_count's result: ``polygon_id`` (int32 tensor, the table's distinct ids
    ascending), ``count`` (int64 tensor, pairs per polygon), ``sum`` (int64 tensor, the
    weights summed per polygon, or None without a weight) and the stats dict."""

    def __init__(self, polygon_id, count, sum, stats):
        self.polygon_id = polygon_id
        self.count = count
        self.sum = sum
        self.stats = stats

    def __len__(self):
        return self.polygon_id.numel()


def pip_join_count(x, y, chips, resolution, index_system=None, weight=None, out=None, accumulate=False, stream=None):
    """The join aggregated per polygon (mgpu_pip_join_count): for the table's distinct
    polygon ids ascending, the number of pairs pip_join emits for the same inputs and --
    with ``weight``, an int64 device column of one value per point -- the sum of the
    weights over those pairs (two's complement wrap).  No pairs are written.

    ``out`` = (count, sum) preallocated int64 device tensors of one element per polygon
    (sum None without a weight); ``accumulate`` adds to their contents instead of
    overwriting them, so a stream of batches is one call each into the same arrays.  A
    call that raises leaves them untouched."""
    import ctypes
    import torch
    isys = index_system or _H3
    res = isys.get_resolution(resolution)
    if isinstance(chips, ChipTable):
        if chips.index_system != isys.code:
            raise N.IllegalArgumentException(N.MGPU_E_INVALID_ARG, "chip table built for another index system")
        chips = chips.upload()
    _check_points(x, y)
    n = x.numel()
    if chips.ctx.device != x.device:
        raise N.IllegalArgumentException(N.MGPU_E_INVALID_ARG, "chip table on %s, points on %s" % (chips.ctx.device, x.device))
    w_ptr = None
    if weight is not None:
        if weight.dtype != torch.int64 or weight.numel() != n or weight.device != x.device:
            raise N.IllegalArgumentException(N.MGPU_E_INVALID_ARG, "weight must be int64 on the points' device, one value per point")
        weight = weight.contiguous()  # kept alive (bound here) until the call returns
        w_ptr = weight.data_ptr()
    ids = chips.polygons()
    if out is not None:
        cnt, sm = out
        for t, what in ((cnt, "count"), (sm, "sum")):
            if t is not None and (t.dtype != torch.int64 or t.device != x.device or not t.is_contiguous()):
                raise N.IllegalArgumentException(N.MGPU_E_INVALID_ARG, "out %s must be a contiguous int64 tensor on the points' device" % what)
        if cnt is None or (sm is None) != (weight is None):
            raise N.IllegalArgumentException(N.MGPU_E_INVALID_ARG, "out must be (count, sum), sum None exactly when weight is None")
        if sm is not None and sm.numel() != cnt.numel():
            raise N.IllegalArgumentException(N.MGPU_E_INVALID_ARG, "out count and sum differ in length")
        n_slots = cnt.numel()
    else:
        if accumulate:
            raise N.IllegalArgumentException(N.MGPU_E_INVALID_ARG, "accumulate needs out=(count, sum) to add to")
        n_slots = len(ids)
        cnt = torch.empty(n_slots, dtype=torch.int64, device=x.device)
        sm = torch.empty(n_slots, dtype=torch.int64, device=x.device) if weight is not None else None
    s = stream if stream is not None else torch.cuda.current_stream(x.device).cuda_stream
    st = N.MgpuStats()
    N.check(N.lib().mgpu_pip_join_count(chips.ctx.handle, chips.handle, isys.code, res, x.data_ptr(), y.data_ptr(),
                                        w_ptr, n, n_slots, cnt.data_ptr(), None if sm is None else sm.data_ptr(),
                                        1 if accumulate else 0, s, ctypes.byref(st)))
    return CountResult(chips.polygons_device(), cnt, sm, st.as_dict())


class LookupResult:
    """pip_join_lookup's result: ``polygon_id`` (int32 tensor, one per input point: its
    lowest matching polygon id, ``null_id`` without a match), ``matches`` (int32 tensor,
    the point's number of matches, or None when not asked for) and the stats dict."""

    def __init__(self, polygon_id, matches, stats):
        self.polygon_id = polygon_id
        self.matches = matches
        self.stats = stats

    def __len__(self):
        return self.polygon_id.numel()


def pip_join_lookup(x, y, chips, resolution, index_system=None, null_id=-1, matches=True, out=None, stream=None):
    """The join as a per-point column in input order (mgpu_pip_join_lookup): for point i,
    the polygon id of the first pair pip_join emits for it on the same inputs -- the lowest
    matching id -- or ``null_id`` when it has none, and (``matches``) the number of pairs
    pip_join emits for it.  No pairs are written.

    ``out`` = (polygon_id, matches) preallocated contiguous int32 device tensors of one
    element per point (matches None exactly when ``matches`` is False); they are written in
    place and returned.  Every element is written; a call that raises leaves them
    untouched."""
    import ctypes
    import torch
    isys = index_system or _H3
    res = isys.get_resolution(resolution)
    if isinstance(chips, ChipTable):
        if chips.index_system != isys.code:
            raise N.IllegalArgumentException(N.MGPU_E_INVALID_ARG, "chip table built for another index system")
        chips = chips.upload()
    _check_points(x, y)
    n = x.numel()
    if chips.ctx.device != x.device:
        raise N.IllegalArgumentException(N.MGPU_E_INVALID_ARG, "chip table on %s, points on %s" % (chips.ctx.device, x.device))
    null_id = int(null_id)
    if not -2 ** 31 <= null_id < 2 ** 31:
        raise N.IllegalArgumentException(N.MGPU_E_INVALID_ARG, "null_id must fit an int32")
    if out is not None:
        op, om = out
        for t, what in ((op, "polygon_id"), (om, "matches")):
            if t is not None and (t.dtype != torch.int32 or t.device != x.device or not t.is_contiguous()
                                  or t.numel() != n):
                raise N.IllegalArgumentException(
                    N.MGPU_E_INVALID_ARG, "out %s must be a contiguous int32 tensor on the points' device, one element per point" % what)
        if op is None or (om is None) != (not matches):
            raise N.IllegalArgumentException(N.MGPU_E_INVALID_ARG, "out must be (polygon_id, matches), matches None exactly when matches=False")
    else:
        op = torch.empty(n, dtype=torch.int32, device=x.device)
        om = torch.empty(n, dtype=torch.int32, device=x.device) if matches else None
    s = stream if stream is not None else torch.cuda.current_stream(x.device).cuda_stream
    st = N.MgpuStats()
    N.check(N.lib().mgpu_pip_join_lookup(chips.ctx.handle, chips.handle, isys.code, res, x.data_ptr(), y.data_ptr(), n,
                                         null_id, op.data_ptr(), None if om is None else om.data_ptr(), s,
                                         ctypes.byref(st)))
    return LookupResult(op, om, st.as_dict())


class CellCounts:
    """CellAggregate.result(): ``cell`` (int64 tensor, the distinct cells ascending),
    ``count`` (int64 tensor, rows per cell) and ``sum`` (int64 tensor, the weights summed
    per cell, or None on an aggregate without a sum)."""

    def __init__(self, cell, count, sum):
        self.cell = cell
        self.count = count
        self.sum = sum

    def __len__(self):
        return self.cell.numel()


def _i64_column(t, what, n=None, device=None):
    import torch
    if t.dtype != torch.int64 or not t.is_cuda or (device is not None and t.device != device) or (
            n is not None and t.numel() != n):
        raise N.IllegalArgumentException(N.MGPU_E_INVALID_ARG,
                                         "%s must be an int64 device tensor on the aggregate's device, one value per row" % what)
    return t.contiguous()


class CellAggregate:
    """Counts (and, ``with_sum``, int64 sums of a weight) per cell of a stream of batches
    (mgpu_cell_agg_*): ``df.groupBy("index_id").count()`` / ``.agg(count, sum)`` over
    grid_longlatascellid's cells, without the cell column and without a sort.  Integer
    arithmetic: the result is exact and does not depend on how the stream was cut into
    batches.  ``initial_cells`` sizes the table for that many distinct cells; it grows on
    demand."""

    def __init__(self, index_system, resolution, with_sum=False, initial_cells=0, ctx=None):
        import ctypes
        from .context import default_context
        self.index_system = index_system or _H3
        self.resolution = self.index_system.get_resolution(resolution)
        self.with_sum = bool(with_sum)
        self.ctx = ctx or default_context()
        self.handle = None
        h = ctypes.c_void_p()
        N.check(N.lib().mgpu_cell_agg_create(self.ctx.handle, self.index_system.code, self.resolution,
                                             1 if self.with_sum else 0, int(initial_cells), ctypes.byref(h)))
        self.handle = h

    def _stream(self, stream):
        import torch
        return stream if stream is not None else torch.cuda.current_stream(self.ctx.device).cuda_stream

    def add_points(self, x, y, weight=None, stream=None, stats=False):
        """One count per point at its cell (grid_longlatascellid's), ``weight`` (int64, one
        per point; exactly on a with_sum aggregate) to the cell's sum.  A call that raises
        -- invalid coordinates, as grid_longlatascellid -- leaves the aggregate unchanged."""
        import ctypes
        _check_points(x, y)
        n = x.numel()
        if weight is not None:
            weight = _i64_column(weight, "weight", n, x.device)  # (bound here: alive until the call returns)
        st = N.MgpuStats()
        N.check(N.lib().mgpu_cell_agg_add_points(self.ctx.handle, self.handle, x.data_ptr(), y.data_ptr(),
                                                 None if weight is None else weight.data_ptr(), n,
                                                 self._stream(stream), ctypes.byref(st)))
        return st.as_dict() if stats else None

    def add_cells(self, cells, weight=None, valid=None, valid_offset=0, stream=None):
        """A cell column (any int64 values); ``valid``: optional Arrow validity bitmap (uint8
        device tensor) read from bit ``valid_offset``: null rows add nothing."""
        import torch
        cells = _i64_column(cells, "cells")
        n = cells.numel()
        if weight is not None:
            weight = _i64_column(weight, "weight", n, cells.device)
        if valid is not None:
            if valid.dtype != torch.uint8 or valid.device != cells.device or valid_offset < 0 or \
                    valid.numel() * 8 < valid_offset + n:
                raise N.IllegalArgumentException(N.MGPU_E_INVALID_ARG, "valid must be a uint8 device bitmap covering valid_offset + n bits")
            valid = valid.contiguous()
        N.check(N.lib().mgpu_cell_agg_add_cells(self.ctx.handle, self.handle, cells.data_ptr(),
                                                None if valid is None else valid.data_ptr(), int(valid_offset),
                                                None if weight is None else weight.data_ptr(), n, self._stream(stream)))

    def add_counted(self, cells, count, sum=None, stream=None):
        """(cell, count, sum) records -- a fetched result reloaded, another rank's or another
        aggregate's result merged.  count >= 0; a record of count 0 adds nothing."""
        cells = _i64_column(cells, "cells")
        n = cells.numel()
        count = _i64_column(count, "count", n, cells.device)
        if sum is not None:
            sum = _i64_column(sum, "sum", n, cells.device)
        N.check(N.lib().mgpu_cell_agg_add_counted(self.ctx.handle, self.handle, cells.data_ptr(), count.data_ptr(),
                                                  None if sum is None else sum.data_ptr(), n, self._stream(stream)))

    def __len__(self):
        import ctypes
        n = ctypes.c_int64()
        N.check(N.lib().mgpu_cell_agg_size(self.ctx.handle, self.handle, ctypes.byref(n), self._stream(None)))
        return int(n.value)

    def result(self, stream=None):
        """The distinct cells ascending with their counts and sums (device tensors).  The
        aggregate is unchanged: adding may continue."""
        import ctypes
        import torch
        n = len(self)
        dev = self.ctx.device
        cell = torch.empty(n, dtype=torch.int64, device=dev)
        cnt = torch.empty(n, dtype=torch.int64, device=dev)
        sm = torch.empty(n, dtype=torch.int64, device=dev) if self.with_sum else None
        got = ctypes.c_int64()
        st = N.lib().mgpu_cell_agg_fetch(self.ctx.handle, self.handle, n, cell.data_ptr(), cnt.data_ptr(),
                                         None if sm is None else sm.data_ptr(), ctypes.byref(got), self._stream(stream))
        N.check(st, required=got.value)
        return CellCounts(cell, cnt, sm)

    def clear(self, stream=None):
        """Empty the aggregate; its memory is kept."""
        N.check(N.lib().mgpu_cell_agg_clear(self.ctx.handle, self.handle, self._stream(stream)))

    def close(self):
        if self.handle:
            N.lib().mgpu_cell_agg_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def grid_cellcount(lon, lat, resolution, index_system=None, weight=None, ctx=None, stream=None):
    """``groupBy(grid_longlatascellid(lon, lat, res)).count()`` (with ``weight``: and
    ``sum(weight)``) in one call: CellCounts of the distinct cells ascending."""
    from .context import default_context
    # (sized for up to 2^20 distinct cells at once: 32 MiB; more cells grow the table)
    agg = CellAggregate(index_system, resolution, with_sum=weight is not None,
                        initial_cells=min(lon.numel(), 1 << 20), ctx=ctx or default_context(lon.device))
    try:
        agg.add_points(lon, lat, weight=weight, stream=stream)
        return agg.result(stream=stream)
    finally:
        agg.close()


class AsyncJoin:
    """A join enqueued by pip_join_async: ``finish()`` settles it (mgpu_pip_join_finish:
    the stream's wait, the H3 near-ties recomputed with the reference's libm, a rerun only
    when a cell moves) and returns the JoinResult.  ``count`` is the device-side pair
    count (one int64 tensor) the enqueued work leaves before finish."""

    def __init__(self, ctx, op, oq, count, keep):
        self._ctx, self._op, self._oq, self.count, self._keep = ctx, op, oq, count, keep
        self._done = None

    def finish(self):
        import ctypes
        if self._done is not None:
            return self._done
        cnt = ctypes.c_int64()
        st = N.MgpuStats()
        status = N.lib().mgpu_pip_join_finish(self._ctx.handle, ctypes.byref(cnt), st)
        N.check(status, required=cnt.value)
        m = int(cnt.value)
        self._done = JoinResult(self._op[:m], self._oq[:m], st.as_dict())
        return self._done


def pip_join_async(x, y, chips, resolution, index_system=None, point_id=None, point_id_base=0, capacity=None,
                   stream=None):
    """mgpu_pip_join_async: enqueue the join on the stream (nothing waits); the pairs
    equal pip_join's after ``finish()`` (include/mosaic_gpu.h).  ``capacity`` is a hard
    bound here (CapacityError from finish, with the count)."""
    import torch
    isys = index_system or _H3
    res = isys.get_resolution(resolution)
    if isinstance(chips, ChipTable):
        chips = chips.upload()
    _check_points(x, y)
    n = x.numel()
    pid_ptr = None
    if point_id is not None:
        point_id = point_id.contiguous()
        pid_ptr = point_id.data_ptr()
    s = stream if stream is not None else torch.cuda.current_stream(x.device).cuda_stream
    cap = int(capacity if capacity is not None else max(16, n + n // 8))
    op = torch.empty(cap, dtype=torch.int64, device=x.device)
    oq = torch.empty(cap, dtype=torch.int32, device=x.device)
    count = torch.zeros(1, dtype=torch.int64, device=x.device)
    N.check(N.lib().mgpu_pip_join_async(chips.ctx.handle, chips.handle, isys.code, res, x.data_ptr(), y.data_ptr(),
                                        pid_ptr, int(point_id_base), n, cap, count.data_ptr(), op.data_ptr(),
                                        oq.data_ptr(), s))
    return AsyncJoin(chips.ctx, op, oq, count, (x, y, point_id, chips))


def _ring_call(call, left_x, max_per_left):
    """Run a ring-join entry with an output sized up front, once more at the reported size."""
    import ctypes
    import torch
    n = ctypes.c_int64()
    cap = max(16, left_x.numel() * (max_per_left + 1 if max_per_left > 0 else 8))
    for _ in range(2):
        ol = torch.empty(cap, dtype=torch.int64, device=left_x.device)
        orr = torch.empty(cap, dtype=torch.int64, device=left_x.device)
        od = torch.empty(cap, dtype=torch.float64, device=left_x.device)
        st = call(cap, ctypes.byref(n), ol.data_ptr(), orr.data_ptr(), od.data_ptr())
        if st == N.MGPU_E_CAPACITY:
            cap = int(n.value)
            continue
        N.check(st)
        m = int(n.value)
        return ol[:m], orr[:m], od[:m]
    N.check(st, required=n.value)


def grid_ring_join(left_x, left_y, right_x, right_y, resolution, k=1, index_system=None, loop_only=False,
                   max_per_left=0, max_distance=-1.0, left_id_base=0, left_outer=False, stream=None):
    """One iteration of SpatialKNN's grid-ring neighbour join for point landmarks (left) and
    point candidates (right) -- GridRingNeighbours.transform (models/knn/
    GridRingNeighbours.scala:121) with its resultTransform (mgpu_ring_join_ex): the pairs whose
    cells meet in kRing(cell(landmark), k) (``loop_only``: kLoop, iterations > 1), self
    matches dropped, ``distance <= max_distance`` (< 0: none), per landmark by (distance,
    candidate index), at most ``max_per_left`` (0: all).  ``left_outer``: the left_outer
    join's null row (right -1, distance NaN) first for a landmark with a cell holding no
    candidate.  Returns (left ids, right indices, distances) on the points' device."""
    import torch
    from .context import default_context
    isys = index_system or _H3
    res = isys.get_resolution(resolution)
    _check_points(left_x, left_y)
    _check_points(right_x, right_y)
    ctx = default_context(left_x.device)
    s = stream if stream is not None else torch.cuda.current_stream(left_x.device).cuda_stream
    flags = N.MGPU_RING_LEFT_OUTER if left_outer else 0
    return _ring_call(lambda cap, n, ol, orr, od: N.lib().mgpu_ring_join_ex(
        ctx.handle, isys.code, res, int(k), 1 if loop_only else 0, left_x.data_ptr(), left_y.data_ptr(),
        left_x.numel(), right_x.data_ptr(), right_y.data_ptr(), right_x.numel(), int(left_id_base),
        int(max_per_left), float(max_distance), flags, cap, n, ol, orr, od, s), left_x, max_per_left)


def grid_ring_join_final(left_x, left_y, radius, k_iterated, right_x, right_y, resolution, index_system=None,
                         max_per_left=0, max_distance=-1.0, left_id_base=0, left_outer=False, stream=None):
    """SpatialKNN's exactness iteration (GridRingNeighbours.leftTransform with iterationID
    -1, GridRingNeighbours.scala:82-90; mgpu_ring_join_final): per landmark, the cells of
    grid_tessellate(st_buffer(landmark, radius[i])) not in kRing(cell, k_iterated[i]),
    joined with the candidates as grid_ring_join does.  ``radius`` / ``k_iterated``: host
    arrays (the landmarks' k-th match distance and their last iteration)."""
    import numpy as np
    import torch
    from .context import default_context
    isys = index_system or _H3
    res = isys.get_resolution(resolution)
    _check_points(left_x, left_y)
    _check_points(right_x, right_y)
    rad = np.ascontiguousarray(radius, dtype=np.float64)
    kit = np.ascontiguousarray(k_iterated, dtype=np.int32)
    assert rad.shape == kit.shape == (left_x.numel(),)
    ctx = default_context(left_x.device)
    s = stream if stream is not None else torch.cuda.current_stream(left_x.device).cuda_stream
    flags = N.MGPU_RING_LEFT_OUTER if left_outer else 0
    return _ring_call(lambda cap, n, ol, orr, od: N.lib().mgpu_ring_join_final(
        ctx.handle, isys.code, res, left_x.data_ptr(), left_y.data_ptr(), rad.ctypes.data, kit.ctypes.data,
        left_x.numel(), right_x.data_ptr(), right_y.data_ptr(), right_x.numel(), int(left_id_base),
        int(max_per_left), float(max_distance), flags, cap, n, ol, orr, od, s), left_x, max_per_left)

"""The IndexSystem plugin boundary, MI355X-backed.

Mirrors the reference's abstract class
  src/main/scala/com/databricks/labs/mosaic/core/index/IndexSystem.scala:15-318
and its two grid implementations used on the point-in-polygon path,
  H3IndexSystem  (H3IndexSystem.scala:24-412)  and
  BNGIndexSystem (BNGIndexSystem.scala:30-555),
selected by name like IndexSystemFactory.getIndexSystem
(IndexSystemFactory.scala:15-63).  Same method names (snake_case), same argument
meaning, same exception classes.  The per-row methods of the reference become
batch methods over device tensors; the scalar forms are kept for API parity and
run as a batch of one.
"""
import numpy as np

from . import _native as N
from ._native import IllegalArgumentException, IllegalStateException


class IndexSystem:
    """Abstract index system (IndexSystem.scala:15)."""

    code = None
    name = None
    crs_id = None
    cell_id_type = "long"  # IndexSystem(cellIdType); LongType for H3, StringType for BNG

    def __init__(self):
        self._cell_id_type = self.cell_id_type

    # -- resolution -------------------------------------------------------
    @property
    def resolutions(self):
        raise NotImplementedError

    def get_resolution(self, res):
        raise NotImplementedError

    # -- cell ids ---------------------------------------------------------
    def get_cell_id_data_type(self):
        return self._cell_id_type

    def set_cell_id_data_type(self, dt):
        """IndexSystem.setCellIdDataType (IndexSystem.scala:43-45); "long" or "string"."""
        if dt not in ("long", "string"):
            raise IllegalArgumentException(N.MGPU_E_INVALID_ARG, "Cell ID data type not supported.")
        self._cell_id_type = dt

    def format(self, cell_id):
        raise NotImplementedError

    def parse(self, cell_id):
        raise NotImplementedError

    def format_cell_id(self, cell_id, dt=None):
        """IndexSystem.formatCellId (IndexSystem.scala:48-57)."""
        dt = dt or self._cell_id_type
        if dt == "long":
            return self.parse(cell_id) if isinstance(cell_id, str) else int(cell_id)
        if dt == "string":
            return cell_id if isinstance(cell_id, str) else self.format(int(cell_id))
        raise IllegalArgumentException(N.MGPU_E_INVALID_ARG, "Cell ID data type not supported.")

    serialize_cell_id = format_cell_id  # IndexSystem.serializeCellId (IndexSystem.scala:61-70)

    # -- point -> cell ----------------------------------------------------
    def points_to_index(self, x, y, resolution, out=None, ctx=None, stream=None, stats=False):
        """Batch IndexSystem.pointToIndex over device tensors (float64 SoA).

        Returns an int64 device tensor of cell ids (and the stats dict if asked)."""
        import torch
        from .context import default_context
        res = self.get_resolution(resolution)
        ctx = ctx or default_context(x.device)
        _check_points(x, y)
        n = x.numel()
        if out is None:
            out = torch.empty(n, dtype=torch.int64, device=x.device)
        st = N.MgpuStats()
        s = stream if stream is not None else torch.cuda.current_stream(x.device).cuda_stream
        N.check(N.lib().mgpu_points_to_cells(ctx.handle, self.code, res, x.data_ptr(), y.data_ptr(), n,
                                             out.data_ptr(), s, st))
        return (out, st.as_dict()) if stats else out

    def point_to_index(self, lon, lat, resolution):
        """Scalar IndexSystem.pointToIndex(lon, lat, res) (IndexSystem.scala:237)."""
        import torch
        from .context import default_context
        ctx = default_context()
        dev = ctx.device
        x = torch.tensor([float(lon)], dtype=torch.float64, device=dev)
        y = torch.tensor([float(lat)], dtype=torch.float64, device=dev)
        return int(self.points_to_index(x, y, resolution, ctx=ctx)[0].item())

    def format_device(self, cells, ctx=None, stream=None):
        """StringType cell ids of a device int64 column (IndexSystem.serializeCellId,
        IndexSystem.scala:61-70; mgpu_format_cells_device, HIP): BNG format / H3 hex.
        Returns (chars: uint8 tensor of the concatenated ids, offsets: int64 tensor of n + 1)."""
        import ctypes
        import torch
        from .context import default_context
        if cells.dtype != torch.int64 or not cells.is_cuda:
            raise IllegalArgumentException(N.MGPU_E_INVALID_ARG, "cells must be an int64 device tensor")
        cells = cells.contiguous()
        ctx = ctx or default_context(cells.device)
        n = cells.numel()
        off = torch.empty(n + 1, dtype=torch.int64, device=cells.device)
        cap = max(16 * n, 1)  # an id is at most 16 chars
        out = torch.empty(cap, dtype=torch.uint8, device=cells.device)
        tot = ctypes.c_int64()
        s = stream if stream is not None else torch.cuda.current_stream(cells.device).cuda_stream
        st = N.lib().mgpu_format_cells_device(ctx.handle, self.code, cells.data_ptr(), n, out.data_ptr(), cap,
                                              off.data_ptr(), ctypes.byref(tot), s)
        N.check(st, "cell id has no string form")
        return out[:tot.value], off

    def k_ring(self, index, n):
        """IndexSystem.kRing(index, n) (H3IndexSystem.scala:182-184, BNGIndexSystem.scala:
        221-226): the list of ids, in the reference's order, on the device."""
        import torch
        from .context import default_context
        from .functions import grid_cellkring
        ctx = default_context()
        ids, _ = grid_cellkring(torch.tensor([int(index)], dtype=torch.int64, device=ctx.device), n, self, ctx=ctx)
        return [int(v) for v in ids.cpu().tolist()]

    def k_loop(self, index, n):
        """IndexSystem.kLoop(index, n) (H3IndexSystem.scala:194-205, BNGIndexSystem.scala:
        239-252) on the device."""
        import torch
        from .context import default_context
        from .functions import grid_cellkring
        ctx = default_context()
        ids, _ = grid_cellkring(torch.tensor([int(index)], dtype=torch.int64, device=ctx.device), n, self,
                                loop_only=True, ctx=ctx)
        return [int(v) for v in ids.cpu().tolist()]


    # -- cell -> geometry (mgpu_cells_*, HIP) ------------------------------
    def _cell_column(self, cells, valid, valid_offset, ctx, stream):
        import torch
        from .context import default_context
        if cells.dtype != torch.int64 or not cells.is_cuda or cells.dim() != 1:
            raise IllegalArgumentException(N.MGPU_E_INVALID_ARG, "cells must be a 1-D int64 device tensor")
        cells = cells.contiguous()
        n = cells.numel()
        if valid is not None and (valid.dtype != torch.uint8 or valid.device != cells.device or not valid.is_contiguous()
                                  or valid_offset < 0 or valid.numel() * 8 < valid_offset + n):
            raise IllegalArgumentException(N.MGPU_E_INVALID_ARG, "valid must be a contiguous uint8 bitmap of at least "
                                           "valid_offset + n bits on the cells' device")
        ctx = ctx or default_context(cells.device)
        s = stream if stream is not None else torch.cuda.current_stream(cells.device).cuda_stream
        out_valid = None if valid is None else torch.empty((n + 7) // 8 + 1, dtype=torch.uint8, device=cells.device)
        return cells, n, ctx, s, (None if valid is None else valid.data_ptr()), out_valid

    def cells_to_centers(self, cells, valid=None, valid_offset=0, ctx=None, stream=None):
        """Batch IndexSystem.indexToCenter (IndexSystem.scala:239) over a device int64 column:
        (lng, lat) float64 device tensors, NaN in null rows; with ``valid`` (an Arrow bitmap
        read from bit ``valid_offset``) also the rows' bitmap at bit offset 0."""
        import torch
        cells, n, ctx, s, vp, ov = self._cell_column(cells, valid, valid_offset, ctx, stream)
        x = torch.empty(max(n, 1), dtype=torch.float64, device=cells.device)
        y = torch.empty(max(n, 1), dtype=torch.float64, device=cells.device)
        N.check(N.lib().mgpu_cells_to_centers(ctx.handle, self.code, cells.data_ptr(), vp, valid_offset, n, x.data_ptr(),
                                              y.data_ptr(), None if ov is None else ov.data_ptr(), s))
        return (x[:n], y[:n]) if ov is None else (x[:n], y[:n], ov[:(n + 7) // 8])

    def cells_to_boundaries(self, cells, valid=None, valid_offset=0, ctx=None, stream=None):
        """Batch IndexSystem.indexToBoundary (IndexSystem.scala:243; BNG: the corners of
        indexToGeometry): (xy float64 (n, 10, 2), nverts int32 (n)) device tensors -- row i's
        boundary is xy[i, :nverts[i]], (x, y) = (lng, lat) for H3, not closed; a null row has
        0 vertices.  With ``valid`` also the rows' bitmap."""
        import torch
        cells, n, ctx, s, vp, ov = self._cell_column(cells, valid, valid_offset, ctx, stream)
        xy = torch.zeros((max(n, 1), 10, 2), dtype=torch.float64, device=cells.device)
        nv = torch.empty(max(n, 1), dtype=torch.int32, device=cells.device)
        N.check(N.lib().mgpu_cells_to_boundaries(ctx.handle, self.code, cells.data_ptr(), vp, valid_offset, n,
                                                 xy.data_ptr(), nv.data_ptr(), None if ov is None else ov.data_ptr(), s))
        return (xy[:n], nv[:n]) if ov is None else (xy[:n], nv[:n], ov[:(n + 7) // 8])

    def cells_boundary_wkb(self, cells, valid=None, valid_offset=0, ctx=None, stream=None):
        """Batch IndexSystem.indexToGeometry as WKB (IndexGeometry.scala:65-75): (bytes uint8
        tensor, offsets int64 tensor of n + 1), row i = bytes[offsets[i]:offsets[i + 1]]
        (empty for a null row).  With ``valid`` also the rows' bitmap."""
        import ctypes
        import torch
        cells, n, ctx, s, vp, ov = self._cell_column(cells, valid, valid_offset, ctx, stream)
        off = torch.empty(n + 1, dtype=torch.int64, device=cells.device)
        cap = 125 * n + 1024  # a hexagon's row; grown to the reported size when the column needs more
        tot = ctypes.c_int64()
        while True:
            out = torch.empty(cap, dtype=torch.uint8, device=cells.device)
            st = N.lib().mgpu_cells_boundary_wkb(ctx.handle, self.code, cells.data_ptr(), vp, valid_offset, n,
                                                 out.data_ptr(), cap, off.data_ptr(), ctypes.byref(tot),
                                                 None if ov is None else ov.data_ptr(), s)
            if st != N.MGPU_E_CAPACITY or tot.value <= cap:
                break
            cap = tot.value
        N.check(st, required=tot.value)
        return (out[:tot.value], off) if ov is None else (out[:tot.value], off, ov[:(n + 7) // 8])

    def cells_area(self, cells, valid=None, valid_offset=0, ctx=None, stream=None):
        """Batch IndexSystem.area (IndexSystem.scala:248-289, BNGIndexSystem.scala:510-516):
        km^2 as a float64 device tensor, NaN in null rows.  With ``valid`` also the rows' bitmap."""
        import torch
        cells, n, ctx, s, vp, ov = self._cell_column(cells, valid, valid_offset, ctx, stream)
        a = torch.empty(max(n, 1), dtype=torch.float64, device=cells.device)
        N.check(N.lib().mgpu_cells_area(ctx.handle, self.code, cells.data_ptr(), vp, valid_offset, n, a.data_ptr(),
                                        None if ov is None else ov.data_ptr(), s))
        return a[:n] if ov is None else (a[:n], ov[:(n + 7) // 8])

    def polyfill(self, geometry, resolution, ctx=None, stream=None):
        """IndexSystem.polyfill(geometry, resolution, geometryAPI): Seq[Long] (IndexSystem.scala:166)
        on the device (mgpu_grid_polyfill): the cells whose centre lies in the geometry.  One
        geometry -- a list of parts, each a list of closed rings [(x, y), ...], the shell first --
        gives a Python list of ids; a ``Polygons`` set gives functions.grid_polyfill's (cells,
        offsets) device tensors."""
        from .chips import Polygons
        from .functions import grid_polyfill
        if isinstance(geometry, Polygons):
            return grid_polyfill(geometry, resolution, self, ctx=ctx, stream=stream)
        cells, _ = grid_polyfill(Polygons.from_lists([(0, geometry)]), resolution, self, ctx=ctx, stream=stream)
        return [int(v) for v in cells.cpu().tolist()]

    def geometry_k_ring(self, geometry, resolution, k, ctx=None, stream=None):
        """Mosaic.geometryKRing(geometry, resolution, k, indexSystem, geometryAPI) (core/Mosaic.scala:
        123-137) for one geometry (parts of closed rings, as ``polyfill`` takes them) on the device
        (mgpu_geometry_kring, a batch of one): the Python list of its cell ids, ascending."""
        return self._geometry_k(geometry, resolution, k, False, ctx, stream)

    def geometry_k_loop(self, geometry, resolution, k, ctx=None, stream=None):
        """Mosaic.geometryKLoop (core/Mosaic.scala:139-156) for one geometry; as geometry_k_ring."""
        return self._geometry_k(geometry, resolution, k, True, ctx, stream)

    def _geometry_k(self, geometry, resolution, k, loop_only, ctx, stream):
        from .chips import Polygons
        from .functions import grid_geometrykloop, grid_geometrykring
        fn = grid_geometrykloop if loop_only else grid_geometrykring
        polys = geometry if isinstance(geometry, Polygons) else Polygons.from_lists([(0, geometry)])
        res = fn(polys, k, self, resolution=resolution, ctx=ctx, stream=stream)
        if isinstance(geometry, Polygons):
            return res
        return [int(v) for v in res.cells.cpu().tolist()]

    def _one_cell(self, index):
        import torch
        from .context import default_context
        ctx = default_context()
        cell = self.parse(index) if isinstance(index, str) else int(index)
        return torch.tensor([cell], dtype=torch.int64, device=ctx.device), ctx

    def index_to_center(self, index):
        """IndexSystem.indexToCenter(index) (IndexSystem.scala:239-241): (lat, lng), as the
        reference's Coordinates; a string id goes through parse."""
        cells, ctx = self._one_cell(index)
        x, y = self.cells_to_centers(cells, ctx=ctx)
        return (float(y[0].item()), float(x[0].item()))

    def index_to_boundary(self, index):
        """IndexSystem.indexToBoundary(index) (IndexSystem.scala:243-245): the list of
        (lat, lng) Coordinates, not closed."""
        cells, ctx = self._one_cell(index)
        xy, nv = self.cells_to_boundaries(cells, ctx=ctx)
        return [(float(p[1]), float(p[0])) for p in xy[0, :int(nv[0].item())].cpu().tolist()]

    def index_to_geometry(self, index):
        """IndexSystem.indexToGeometry(index) (IndexSystem.scala:223) as WKB bytes."""
        cells, ctx = self._one_cell(index)
        w, _ = self.cells_boundary_wkb(cells, ctx=ctx)
        return bytes(w.cpu().numpy().tobytes())

    def area(self, index):
        """IndexSystem.area(index) (IndexSystem.scala:248-291), km^2."""
        cells, ctx = self._one_cell(index)
        return float(self.cells_area(cells, ctx=ctx)[0].item())


def _check_points(x, y):
    if x.dtype != y.dtype or str(x.dtype) != "torch.float64":
        raise IllegalArgumentException(N.MGPU_E_INVALID_ARG, "coordinates must be float64 tensors")
    if x.shape != y.shape or x.dim() != 1 or not x.is_contiguous() or not y.is_contiguous():
        raise IllegalArgumentException(N.MGPU_E_INVALID_ARG, "coordinates must be 1-D contiguous tensors")
    if x.device.type != "cuda" or y.device != x.device:
        raise IllegalArgumentException(N.MGPU_E_INVALID_ARG, "coordinates must live on the context's GPU")


class H3IndexSystem(IndexSystem):
    """H3IndexSystem (H3IndexSystem.scala:24): H3 v3.7, resolutions 0..15, LongType ids."""

    code = N.MGPU_H3
    name = "H3"
    crs_id = 4326
    cell_id_type = "long"

    @property
    def resolutions(self):
        return set(range(16))

    def get_resolution(self, res):
        """H3IndexSystem.getResolution (H3IndexSystem.scala:45-60)."""
        if isinstance(res, bool):
            raise IllegalArgumentException(N.MGPU_E_INVALID_ARG, "Resolution must be an Int or String.")
        if isinstance(res, (int, np.integer)):
            r = int(res)
        elif isinstance(res, str):
            try:
                r = int(res)
            except ValueError:
                raise IllegalArgumentException(N.MGPU_E_INVALID_ARG, "Resolution must be an Int or String.")
        else:
            raise IllegalArgumentException(N.MGPU_E_INVALID_ARG, "Resolution must be an Int or String.")
        if r < 0 or r > 15:
            raise IllegalStateException(N.MGPU_E_RESOLUTION, "H3 resolution has to be between 0 and 15; found %d" % r)
        return r

    def cell_area_estimate(self, resolution, lat):
        """A lower estimate of a cell's area in square degrees at latitude(s) ``lat``, for sizing
        buffers (grid_polyfill): H3's mean hexagon area is 4,250,547 km^2 / 7^res, its smallest
        cells (around the pentagons) about half of that; a degree is 111.32 km."""
        km2 = 0.5 * 4250546.848 / 7.0 ** resolution
        return km2 / (111.32 ** 2 * np.cos(np.radians(np.clip(lat, -89.0, 89.0))))

    def format(self, cell_id):
        """H3 string form (the 15-hex-digit address)."""
        return "%x" % int(cell_id)

    def parse(self, cell_id):
        return int(cell_id, 16)

    def get_resolution_str(self, resolution):
        return str(resolution)


class BNGIndexSystem(IndexSystem):
    """BNGIndexSystem (BNGIndexSystem.scala:30): British National Grid, EPSG:27700, StringType ids."""

    code = N.MGPU_BNG
    name = "BNG"
    crs_id = 27700
    cell_id_type = "string"
    # BNGIndexSystem.resolutionMap (BNGIndexSystem.scala:46-60)
    resolution_map = {"500km": -1, "100km": 1, "50km": -2, "10km": 2, "5km": -3, "1km": 3, "500m": -4,
                      "100m": 4, "50m": -5, "10m": 5, "5m": -6, "1m": 6}

    @property
    def resolutions(self):
        return {1, -1, 2, -2, 3, -3, 4, -4, 5, -5, 6, -6}

    def get_resolution(self, res):
        """BNGIndexSystem.getResolution (BNGIndexSystem.scala:349-360)."""
        if isinstance(res, (int, np.integer)) and not isinstance(res, bool) and int(res) in self.resolutions:
            return int(res)
        if isinstance(res, str) and res in self.resolution_map:
            return self.resolution_map[res]
        raise IllegalStateException(N.MGPU_E_RESOLUTION, "BNG resolution not supported; found %s" % (res,))

    def edge_size(self, resolution):
        """BNGIndexSystem.getEdgeSize (BNGIndexSystem.scala:163-170): metres; a quadrant
        resolution (negative) has half the edge of the grid above it."""
        r = self.get_resolution(resolution)
        return 10 ** (6 - r) if r > 0 else 5 * 10 ** (6 + r)

    def cell_area_estimate(self, resolution, lat=None):
        """A cell's area in square metres, for sizing buffers (grid_polyfill)."""
        return float(self.edge_size(resolution)) ** 2

    def get_resolution_str(self, resolution):
        for k, v in self.resolution_map.items():
            if v == resolution:
                return k
        return ""

    def format_many(self, cells):
        """BNGIndexSystem.format over an int64 array (host)."""
        c = np.ascontiguousarray(np.asarray(cells, dtype=np.int64))
        n = c.shape[0]
        buf = np.zeros(max(24 * n, 1), dtype=np.uint8)
        off = np.zeros(n + 1, dtype=np.int64)
        st = N.lib().mgpu_bng_format(c.ctypes.data, n, buf.ctypes.data, buf.shape[0], off.ctypes.data)
        N.check(st, "BNG cell id has no string form")
        raw = buf.tobytes()
        return [raw[off[i]:off[i + 1]].decode() for i in range(n)]

    def parse_many(self, ids):
        enc = [s.encode() for s in ids]
        off = np.zeros(len(enc) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(e) for e in enc])
        buf = np.frombuffer(b"".join(enc) or b"\0", dtype=np.uint8).copy()
        out = np.zeros(len(enc), dtype=np.int64)
        N.check(N.lib().mgpu_bng_parse(buf.ctypes.data, off.ctypes.data, len(enc), out.ctypes.data),
                "not a BNG cell id")
        return out

    def index_to_center(self, index):
        """BNGIndexSystem.indexToCenter (BNGIndexSystem.scala:518-520) throws NotImplementedError."""
        raise NotImplementedError

    def index_to_boundary(self, index):
        """BNGIndexSystem.indexToBoundary (BNGIndexSystem.scala:522-524) throws NotImplementedError."""
        raise NotImplementedError

    def format(self, cell_id):
        return self.format_many([cell_id])[0]

    def parse(self, cell_id):
        return int(self.parse_many([cell_id])[0])


def get_index_system(name):
    """IndexSystemFactory.getIndexSystem(name) (IndexSystemFactory.scala:31-63)."""
    n = str(name).upper()
    if n == "H3":
        return H3IndexSystem()
    if n == "BNG":
        return BNGIndexSystem()
    raise IllegalArgumentException(N.MGPU_E_INVALID_ARG,
                                   "Index system %s not supported by the MI355X path (H3, BNG)" % name)

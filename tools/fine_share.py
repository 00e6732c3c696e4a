#!/usr/bin/env python3
"""Host only: what a block table of each shape answers on a bench config's table.

For the config's chip table (built as a host blob, no GPU) and a sample of the config's own
points: the share of points whose block of 8x8, 8x4, 4x8 and 4x4 pixels is uniform -- and, for
the byte-coded table (chip_table.h raster_fine), uniform with a class below 255 -- and the
bytes of each table plus the row bands, i.e. the LDS a classify workgroup holds.  The pixel of
a point is computed as raster.h raster_index computes it.  One JSON line per config.

  python3 tools/fine_share.py --configs c2,c5 [--points 20000000]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

U32, I32, U64, I64, F64 = ctypes.c_uint32, ctypes.c_int32, ctypes.c_uint64, ctypes.c_int64, ctypes.c_double
ARR_RASTER = 18  # chip_build.h BlobArray kArrRaster


class DenseFace(ctypes.Structure):
    _fields_ = [("a0", I32), ("b0", I32), ("w", U32), ("h", U32), ("base", U32)]


class BlobHeader(ctypes.Structure):  # chip_build.h BlobHeader
    _fields_ = [("magic", U64), ("version", U32), ("hash_mask", U32), ("max_probe", U32), ("n_chips", U32),
                ("n_cells", U32), ("index_system", I32), ("n_vertices", I64), ("off", U64 * 29), ("probe_mode", I32),
                ("res", I32), ("face_mask", U32), ("pad2", U32), ("bbox", F64 * 4), ("k_res", F64),
                ("dense", DenseFace * 20), ("bng_edge", U32), ("pad3", U32), ("bng_inv_edge", F64),
                ("raster_mode", I32), ("raster_nx", U32), ("raster_ny", U32), ("raster_pix", U32), ("raster_px0", I32),
                ("raster_py0", I32), ("raster_x0", F64), ("raster_y0", F64), ("raster_inv_dx", F64),
                ("raster_inv_dy", F64), ("blob_bytes", U64), ("max_cell_chips", U32), ("pad4", U32),
                ("raster_pc", U32 * 4), ("raster_sub_n", U32), ("raster_sub_w", U32), ("raster_bshift", U32),
                ("raster_bnx", U32), ("raster_bny", U32), ("raster_ncls", U32), ("raster_band_shift", U32),
                ("raster_nband", U32)]


def block_codes(cls, sx, sy):
    """(uniform, class) per block of 2^sx x 2^sy pixels, clipped at the raster's edges."""
    ny, nx = cls.shape
    by, bx = -(-ny // (1 << sy)), -(-nx // (1 << sx))
    pad = np.pad(cls, ((0, (by << sy) - ny), (0, (bx << sx) - nx)), mode="edge")
    blocks = pad.reshape(by, 1 << sy, bx, 1 << sx)
    first = blocks[:, 0, :, 0]
    return (blocks == first[:, None, :, None]).all(axis=(1, 3)), first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c5")
    ap.add_argument("--points", type=int, default=20_000_000)
    a = ap.parse_args()
    import bench as B
    import bench_workloads as W
    import mosaic_amd as M
    from mosaic_amd import dist as D
    for c in a.configs.split(","):
        ns = argparse.Namespace(config=c, res=None, seed=0x20250314, points=None)
        wl = B.workload(ns, W, M)
        blob = D.host_blob(M.tessellate(wl["polygons"], wl["isys"], ns.res))
        h = BlobHeader.from_buffer_copy(blob[:ctypes.sizeof(BlobHeader)])
        assert h.blob_bytes == len(blob) and h.raster_mode == 1, "not a lon/lat pixel index"
        nx, ny = h.raster_nx, h.raster_ny
        cls = np.frombuffer(blob, np.uint16, nx * ny, h.off[ARR_RASTER]).reshape(ny, nx)
        x, y = wl["points_np"](a.points, ns.seed)
        inside = (x >= h.bbox[0]) & (x <= h.bbox[2]) & (y >= h.bbox[1]) & (y <= h.bbox[3])
        ix = np.minimum(((x[inside] - h.raster_x0) * h.raster_inv_dx).astype(np.uint32), nx - 1)
        iy = np.minimum(((y[inside] - h.raster_y0) * h.raster_inv_dy).astype(np.uint32), ny - 1)
        out = {"config": c, "res": ns.res, "raster": [int(nx), int(ny)], "classes": int(h.raster_ncls),
               "row_band_bytes": 4 * int(h.raster_nband), "points": int(a.points),
               "outside_box": float(1 - inside.mean()), "shapes": {}}
        n = float(len(x))
        for name, sx, sy in (("8x8", 3, 3), ("8x4", 3, 2), ("4x8", 2, 3), ("4x4", 2, 2)):
            uni, first = block_codes(cls, sx, sy)
            u = uni[iy >> sy, ix >> sx]
            f = first[iy >> sy, ix >> sx]
            out["shapes"][name] = {
                "blocks": int(uni.size), "lds_bytes_u16": 2 * int(uni.size) + out["row_band_bytes"],
                "lds_bytes_u8": (int(uni.size) + 3) // 4 * 4 + out["row_band_bytes"],
                "uniform": float(u.sum() / n), "uniform_below_255": float((u & (f < 255)).sum() / n),
                "uniform_class_255_up": float((u & (f >= 255) & (f < 0x8000)).sum() / n)}
        # (a point in no uniform block takes a pixel gather; of those, the refined pixels a second one)
        px = cls[iy, ix]
        out["refined_pixel"] = float(((px >= 0x8000) & (px != 0xFFFF)).sum() / n)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

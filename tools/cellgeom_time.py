#!/usr/bin/env python3
"""Cell id -> geometry timed: 1e6 distinct cells each of H3 r9, H3 r10 and BNG r4 through
  boundaries   IndexSystem.cells_to_boundaries (mgpu_cells_to_boundaries)
  wkb          grid_boundaryaswkb (mgpu_cells_boundary_wkb)
  area         grid_cellarea (mgpu_cells_area)
-- HIP events around each whole call, the three alternating step by step, in --series series
of --steps timed steps each; a step time is the median of the series' medians, a spread
(max - min) / median over them (as tools/cellagg_time.py) -- and beside them, for H3, the
host route the device replaces (mgpu_test_h3_boundary_host, one thread, timed once over the
same cells).  One JSON line per config, with the share of special WKB rows (pole cells, cells
across the antimeridian: shaped on the host).  Recorded, not gated."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from count_time import series  # noqa: E402

CONFIGS = {"h3_r9": ("H3", 9), "h3_r10": ("H3", 10), "bng_r4": ("BNG", 4)}


def distinct_cells(M, isys, res, n, dev, seed):
    """n distinct cells of uniform points (the globe / the BNG extent), ascending."""
    rng = np.random.default_rng(seed)
    out = torch.empty(0, dtype=torch.int64, device=dev)
    while out.numel() < n:
        m = n + n // 4
        if isys.name == "H3":
            x, y = rng.uniform(-180.0, 180.0, m), np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, m)))
        else:
            x, y = rng.uniform(0.0, 700000.0, m), rng.uniform(0.0, 1300000.0, m)
        c = M.grid_longlatascellid(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), res, index_system=isys)
        out = torch.unique(torch.cat([out, c]))
    return out[torch.randperm(out.numel(), device=dev, generator=torch.Generator(dev).manual_seed(seed))[:n]].sort().values


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="h3_r9,h3_r10,bng_r4")
    ap.add_argument("--cells", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--series", type=int, default=3)
    ap.add_argument("--baseline-cells", type=int, default=None, help="cells of the host baseline (default: all)")
    a = ap.parse_args()
    import mosaic_amd as M
    from mosaic_amd import _native as N
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    for c in a.configs.split(","):
        name, res = CONFIGS[c]
        isys = M.get_index_system(name)
        cells = distinct_cells(M, isys, res, a.cells, dev, 20250314 + res)
        n = cells.numel()
        fns = {"boundaries": lambda: isys.cells_to_boundaries(cells),
               "wkb": lambda: M.grid_boundaryaswkb(cells, isys),
               "area": lambda: M.grid_cellarea(cells, isys)}
        runs = [series(fns, a.steps, a.warmup if i == 0 else 1) for i in range(a.series)]
        med = {k: [r[k][0] for r in runs] for k in fns}
        mid = {k: float(np.median(v)) for k, v in med.items()}
        (xy, nv), (w, off) = runs[-1]["boundaries"][1], runs[-1]["wkb"][1]
        special = int((off[1:] - off[:-1] != 13 + 16 * (nv.to(torch.int64) + 1)).sum().item())
        out = {"config": c, "index_system": name, "res": res, "cells": n, "series": a.series, "steps": a.steps,
               "wkb_bytes": int(w.numel()), "special_rows": special, "special_share": special / n}
        for k in fns:
            out[k + "_ms"], out[k + "_ms_runs"] = mid[k], med[k]
            out[k + "_spread"] = (max(med[k]) - min(med[k])) / mid[k]
            out[k + "_cells_per_s"] = n / (mid[k] * 1e-3)
        if name == "H3":
            nb = min(n, a.baseline_cells or n)
            hc = np.ascontiguousarray(cells[:nb].cpu().numpy())
            hxy, hnv, hc2 = np.zeros((nb, 20)), np.zeros(nb, np.int32), np.zeros((nb, 2))
            t0 = time.perf_counter()
            N.check(N.lib().mgpu_test_h3_boundary_host(ctypes.c_void_p(hc.ctypes.data), nb, ctypes.c_void_p(hxy.ctypes.data),
                                                       ctypes.c_void_p(hnv.ctypes.data), ctypes.c_void_p(hc2.ctypes.data)))
            host_ms = (time.perf_counter() - t0) * 1e3 * (n / nb)
            out.update({"host_route_ms": host_ms, "host_route_cells": nb, "host_over_boundaries": host_ms / mid["boundaries"],
                        "nverts_equal_host": bool(np.array_equal(hnv, nv[:nb].cpu().numpy()))})
        print(json.dumps(out), flush=True)
        del cells, runs, xy, nv, w, off
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

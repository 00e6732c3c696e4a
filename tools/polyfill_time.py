#!/usr/bin/env python3
"""grid_polyfill timed on the device (mgpu_grid_polyfill through functions.grid_polyfill):
  nyc_r9, nyc_r10   the 263 NYC taxi zones at H3 res 9 and 10
  tracts_r10        bench_workloads.tract_polygons() at H3 res 10
-- HIP events around each whole call (the host's plan, the uploads, the kernels and the
readback of the total), --series series of --steps calls after a warm-up; the time is the
median of the series' medians, the spread (max - min) / median over them.  kernels_ms is the
median over the timed calls of the entry's own event pair around its launches
(mgpu_test_grid_polyfill_last), host_ms the call's time less that.  Beside it, timed
once, the only route a caller had before: the host tessellate() of the same polygons.  That
route also cuts the chips, so the ratio is what a caller saves who wants the cells alone, not a
like-for-like comparison of two kernels.  One JSON line per config.  Recorded, not gated."""
import argparse
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

CONFIGS = {"nyc_r9": ("nyc", 9), "nyc_r10": ("nyc", 10), "tracts_r10": ("tracts", 10)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="nyc_r9,nyc_r10,tracts_r10")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--series", type=int, default=3)
    ap.add_argument("--tracts", type=int, default=None, help="tract polygons (default: the workload's)")
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    import mosaic_amd as M
    from mosaic_amd import _native as N
    import bench_workloads as W
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    h3 = M.H3IndexSystem()
    for c in a.configs.split(","):
        what, res = CONFIGS[c]
        polys = W.nyc_zones() if what == "nyc" else (W.tract_polygons(a.tracts) if a.tracts else W.tract_polygons())
        kernel_us = []

        def call():
            out = M.grid_polyfill(polys, res, h3)
            N.check(N.lib().mgpu_test_grid_polyfill_last(last.ctypes.data))
            kernel_us.append(int(last[4]))
            return out

        last = np.zeros(8, np.int64)
        fns = {"polyfill": call}
        runs = [series(fns, a.steps, a.warmup if i == 0 else 1) for i in range(a.series)]
        med = [r["polyfill"][0] for r in runs]
        mid = float(np.median(med))
        cells, off = runs[-1]["polyfill"][1]
        kernel_ms = float(np.median(kernel_us[-a.steps * a.series:])) * 1e-3
        out = {"config": c, "res": res, "polygons": len(polys), "vertices": int(polys.xy.shape[0]), "cells": int(cells.numel()),
               "samples": int(last[0]), "tiles": int(last[1]), "certificate_failures": int(last[2]), "attempts": int(last[3]),
               "series": a.series, "steps": a.steps, "polyfill_ms": mid, "polyfill_ms_runs": med,
               "polyfill_spread": (max(med) - min(med)) / mid, "cells_per_s": int(cells.numel()) / (mid * 1e-3),
               "samples_per_s": int(last[0]) / (mid * 1e-3), "kernels_ms": kernel_ms, "host_ms": mid - kernel_ms,
               "kernel_samples_per_s": int(last[0]) / max(kernel_ms * 1e-3, 1e-9), "samples_per_cell": int(last[0]) / max(int(cells.numel()), 1)}
        if not a.no_baseline:
            t0 = time.perf_counter()
            chips = M.tessellate(polys, h3, res)
            host_ms = (time.perf_counter() - t0) * 1e3
            out.update({"host_tessellate_ms": host_ms, "host_tessellate_chips": len(chips),
                        "host_tessellate_over_polyfill": host_ms / mid,
                        "note": "tessellate() also cuts the chips: the ratio is what a caller of the cells alone saves"})
        print(json.dumps(out), flush=True)
        del cells, off, runs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

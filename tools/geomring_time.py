#!/usr/bin/env python3
"""grid_geometrykring / grid_geometrykloop timed on the device against what a caller had before.

  new        mgpu_geometry_kring through functions.grid_geometrykring / grid_geometrykloop on the
             chip rows as device columns; the result stays on the device (new_ms), or is also
             copied to the host as lists (new_lists_ms)
  composed   the parts that existed: grid_cellkring (and, for the loop, grid_cellkloop) over the
             border cells on the device, the lists copied to the host, np.unique per polygon with
             its core cells (the loop: np.setdiff1d against core and the (k - 1)-rings)

Configs: the 263 NYC taxi zones at H3 res 9 with k = 1, 2, 3, the London districts at BNG res 4
with k = 1, ring and loop each.  Both ways get the same prepared input (rows grouped by polygon,
uploaded) and are checked equal once.  Every call is timed by a host clock around the call and a
device synchronise; the two ways alternate call by call; --series series of --steps calls after a
warm-up; the time is the median of the series' medians, the spread (max - min) / median over them.
ids_generated / ids_returned is the duplication the sets remove.  One JSON line per config.
Recorded, not gated."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [("nyc_r9", 1), ("nyc_r9", 2), ("nyc_r9", 3), ("london_bng4", 1)]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def series(fns, steps, warmup):
    """{name: (median ms, last result)}: `steps` rounds in which every variant runs once."""
    last = {}
    for _ in range(warmup):
        for k, fn in fns.items():
            last[k] = fn()
    ms = {k: [] for k in fns}
    for _ in range(steps):
        for k, fn in fns.items():
            t, last[k] = timed(fn)
            ms[k].append(t)
    return {k: (float(np.median(v)), last[k]) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--series", type=int, default=3)
    ap.add_argument("--only", default=None, help="nyc_r9 or london_bng4")
    a = ap.parse_args()
    import mosaic_amd as M
    from mosaic_amd import _native as N
    import bench_workloads as W
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    tables = {}
    for name, k in CONFIGS:
        if a.only and name != a.only:
            continue
        if name not in tables:
            isys = M.H3IndexSystem() if name == "nyc_r9" else M.BNGIndexSystem()
            polys = W.nyc_zones() if name == "nyc_r9" else W.london_districts()
            chips = M.tessellate(polys, isys, 9 if name == "nyc_r9" else 4, keep_core_geometries=False)
            order = np.argsort(chips.polygon_id, kind="stable")
            pid, cell, core = chips.polygon_id[order], chips.cell[order], chips.is_core[order]
            ids = np.unique(pid)
            row_off = np.append(np.searchsorted(pid, ids), len(pid)).astype(np.int64)
            bstart = np.concatenate([[0], np.cumsum(core == 0)])[row_off]  # the polygons' starts among the border rows
            core_lists = [cell[row_off[g]:row_off[g + 1]][core[row_off[g]:row_off[g + 1]] != 0] for g in range(len(ids))]
            dev_cols = (torch.from_numpy(row_off).to(dev), torch.from_numpy(cell).to(dev), torch.from_numpy(core).to(dev))
            tables[name] = (isys, len(ids), bstart, core_lists, dev_cols)
        isys, n, bstart, core_lists, dev_cols = tables[name]
        for loop in (False, True):
            last = np.zeros(8, np.int64)
            fn = M.grid_geometrykloop if loop else M.grid_geometrykring

            def new():
                r = fn(dev_cols, k, isys)
                N.check(N.lib().mgpu_test_geometry_kring_last(last.ctypes.data))
                return r

            def new_lists():
                return fn(dev_cols, k, isys).lists()

            def composed():
                border = dev_cols[1][dev_cols[2] == 0]
                ring, off = M.grid_cellkring(border, k, isys, loop_only=loop)
                ring, off = ring.cpu().numpy(), off.cpu().numpy()
                if loop:
                    inner, ioff = M.grid_cellkring(border, k - 1, isys)
                    inner, ioff = inner.cpu().numpy(), ioff.cpu().numpy()
                out = []
                for g in range(n):
                    b0, b1 = bstart[g], bstart[g + 1]
                    mine = ring[off[b0]:off[b1]]
                    if loop:
                        out.append(np.setdiff1d(mine, np.concatenate([core_lists[g], inner[ioff[b0]:ioff[b1]]])))
                    else:
                        out.append(np.unique(np.concatenate([core_lists[g], mine])))
                return out

            fns = {"new": new, "new_lists": new_lists, "composed": composed}
            runs = [series(fns, a.steps, a.warmup if i == 0 else 1) for i in range(a.series)]
            got, want = runs[-1]["new_lists"][1], runs[-1]["composed"][1]
            equal = len(got) == len(want) and all(np.array_equal(x, y) for x, y in zip(got, want))
            out = {"config": name, "k": k, "loop": loop, "geometries": n, "rows": int(dev_cols[1].numel()),
                   "border_cells": int(last[3]), "ids_generated": int(last[4]), "ids_returned": int(last[5]),
                   "duplication": float(last[4]) / max(int(last[5]), 1), "lds_geometries": int(last[0]),
                   "hbm_geometries": int(last[1]), "slabs": int(last[2]), "stream_us": int(last[6]),
                   "equal_to_composed": bool(equal), "series": a.series, "steps": a.steps}
            for key in fns:
                med = [r[key][0] for r in runs]
                mid = float(np.median(med))
                out[key + "_ms"] = mid
                out[key + "_ms_runs"] = med
                out[key + "_spread"] = (max(med) - min(med)) / mid
            out["cells_per_s"] = int(last[5]) / (out["new_ms"] * 1e-3)
            out["composed_over_new"] = out["composed_ms"] / out["new_ms"]
            out["composed_over_new_lists"] = out["composed_ms"] / out["new_lists_ms"]
            print(json.dumps(out), flush=True)
            del runs, got, want
    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

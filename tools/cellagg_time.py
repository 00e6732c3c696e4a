#!/usr/bin/env python3
"""grid_cellcount against the cell column sorted by torch.unique, on the bench configs'
point sets at bench size and resolution (C2: H3 r9, C4: BNG r4): one JSON line per config
with the step times (HIP events around the whole call) of
  unique       grid_longlatascellid, then torch.unique(return_counts=True): the caller's way
               without the aggregate
  cells        grid_longlatascellid alone
  cellcount    grid_cellcount
  cellcount_w  grid_cellcount with a weight column
-- the four alternate step by step, in --series series of --steps timed steps each; a step
time is the median of the series' medians, a spread (max - min) / median over them -- and
cellcount / unique, cellcount - cells (the aggregation's own cost) and that cost in cells
per second."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from count_time import series  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c4")
    ap.add_argument("--points", type=int, default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--series", type=int, default=3)
    ap.add_argument("--option", action="append", default=[], metavar="KEY=VALUE")
    a = ap.parse_args()
    import mosaic_amd as M
    import bench as B
    import bench_workloads as W
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = M.default_context(dev)
    for kv in a.option:
        k, v = kv.split("=")
        ctx.set_option(k, int(v))
    for c in a.configs.split(","):
        ns = argparse.Namespace(config=c, res=None, seed=0x20250314, points=a.points)
        wl = B.workload(ns, W, M)
        n, isys, res = ns.points, wl["isys"], ns.res
        x, y = wl["points"](n, 0, dev)
        w = torch.arange(n, dtype=torch.int64, device=dev) * 3 - 7
        cells = lambda: M.grid_longlatascellid(x, y, res, index_system=isys)
        fns = {"unique": lambda: torch.unique(cells(), return_counts=True),
               "cells": cells,
               "cellcount": lambda: M.grid_cellcount(x, y, res, index_system=isys),
               "cellcount_w": lambda: M.grid_cellcount(x, y, res, index_system=isys, weight=w)}
        runs = [series(fns, a.steps, a.warmup if i == 0 else 1) for i in range(a.series)]
        med = {k: [r[k][0] for r in runs] for k in fns}
        mid = {k: float(np.median(v)) for k, v in med.items()}
        spread = {k: (max(v) - min(v)) / mid[k] for k, v in med.items()}
        (u, ucnt), r, rw = runs[-1]["unique"][1], runs[-1]["cellcount"][1], runs[-1]["cellcount_w"][1]
        agg_ms = mid["cellcount"] - mid["cells"]
        margin = max(spread["unique"], spread["cellcount"])
        out = {"config": c, "points": n, "index_system": isys.name, "res": res, "cells": len(r),
               "series": a.series, "steps": a.steps}
        for k in fns:
            out[k + "_ms"], out[k + "_ms_runs"], out[k + "_spread"] = mid[k], med[k], spread[k]
        out.update({
            "equals_unique": bool(torch.equal(u, r.cell) and torch.equal(ucnt, r.count)
                                  and torch.equal(rw.cell, r.cell) and torch.equal(rw.count, r.count)),
            "cellcount_over_unique": mid["cellcount"] / mid["unique"],
            "aggregation_ms": agg_ms,
            "aggregation_cells_per_s": n / (agg_ms * 1e-3) if agg_ms > 0 else None,
            "aggregation_weight_ms": mid["cellcount_w"] - mid["cells"],
            "accepted": bool(mid["cellcount"] < mid["unique"] * (1 - margin)),
        })
        print(json.dumps(out), flush=True)
        del x, y, w, u, ucnt, r, rw, runs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""pip_join against pip_join_lookup on the bench configs, at bench sizes: one JSON line per
config with the step times (HIP events around the whole call) of pip_join and of
pip_join_lookup with and without the match counts -- the three alternate step by step, in
--series series of --steps timed steps each; a step time is the median of the series'
medians, a spread (max - min) / median over them -- the lookup kernel's own time (stats
emit_kernel_ms of the lookup call) and its achieved bytes per second over its algorithmic
traffic (split: the code, 2 B H3 / 4 B BNG; binned: 8 B answer + 4 B perm; fused: 8 B per
record; plus the 4 or 8 B written per point).  pip_join is the yardstick: the same build,
the same run.  "accept": the lookup with matches is not slower than pip_join by more than
the larger of the two spreads."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from count_time import series  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c3,c4")
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
        n = ns.points
        ctx.reserve(n)
        table = M.tessellate(wl["polygons"], wl["isys"], ns.res, keep_core_geometries=wl.get("keep_core", True))
        chips = table.upload(ctx)
        x, y = wl["points"](n, 0, dev)
        cap = int(n * wl["pairs_per_point"]) + 1024
        op = torch.empty(cap, dtype=torch.int64, device=dev)
        oq = torch.empty(cap, dtype=torch.int32, device=dev)
        lp = torch.empty(n, dtype=torch.int32, device=dev)
        lm = torch.empty(n, dtype=torch.int32, device=dev)
        lp1 = torch.empty(n, dtype=torch.int32, device=dev)
        join = lambda: M.pip_join(x, y, chips, ns.res, out=(op, oq), capacity=cap, index_system=wl["isys"])
        look = lambda: M.pip_join_lookup(x, y, chips, ns.res, index_system=wl["isys"], out=(lp, lm))
        look1 = lambda: M.pip_join_lookup(x, y, chips, ns.res, index_system=wl["isys"], matches=False, out=(lp1, None))
        fns = {"join": join, "lookup": look, "lookup_no_matches": look1}
        runs = [series(fns, a.steps, a.warmup if i == 0 else 1) for i in range(a.series)]
        med = {k: [r[k][0] for r in runs] for k in fns}
        mid = {k: float(np.median(v)) for k, v in med.items()}
        spread = {k: (max(v) - min(v)) / mid[k] for k, v in med.items()}
        rj, rl, r1 = (runs[-1][k][1] for k in ("join", "lookup", "lookup_no_matches"))
        # the column against the ordered pairs of the same build
        m = len(rj)
        pid = rj.point_id
        cnt = torch.bincount(pid, minlength=n).to(torch.int32)
        head = torch.ones(m, dtype=torch.bool, device=dev)
        head[1:] = pid[1:] != pid[:-1]
        first = torch.full((n,), -1, dtype=torch.int32, device=dev)
        first[pid[head]] = rj.polygon_id[head]
        equal = bool(torch.equal(lm, cnt)) and bool(torch.equal(lp, first)) and bool(torch.equal(lp1, first))
        pipeline = rl.stats["pipeline"]
        read = {1: 2 if wl["isys"].code == 0 else 4, 2: 12}.get(pipeline)
        read_bytes = n * read if read else 8 * m
        gbs = lambda st, w: (read_bytes + w * n) / (st["emit_kernel_ms"] * 1e-3) / 1e9 if st["emit_kernel_ms"] > 0 else None
        slack = max(spread["join"], spread["lookup"]) * mid["join"]
        print(json.dumps({
            "config": c, "points": n, "pairs": m, "pipeline": pipeline, "series": a.series, "steps": a.steps,
            "join_ms": mid["join"], "join_ms_runs": med["join"], "join_spread": spread["join"],
            "lookup_ms": mid["lookup"], "lookup_ms_runs": med["lookup"], "lookup_spread": spread["lookup"],
            "lookup_no_matches_ms": mid["lookup_no_matches"], "lookup_no_matches_ms_runs": med["lookup_no_matches"],
            "lookup_no_matches_spread": spread["lookup_no_matches"],
            "join_emit_kernel_ms": rj.stats["emit_kernel_ms"], "join_kernel_ms": rj.stats["kernel_ms"],
            "lookup_kernel_ms": rl.stats["emit_kernel_ms"], "lookup_total_kernel_ms": rl.stats["kernel_ms"],
            "lookup_no_matches_kernel_ms": r1.stats["emit_kernel_ms"],
            "lookup_kernel_gbs": gbs(rl.stats, 8), "lookup_no_matches_kernel_gbs": gbs(r1.stats, 4),
            "lookup_equals_join": equal,
            "lookup_over_join": mid["lookup"] / mid["join"],
            "lookup_no_matches_over_join": mid["lookup_no_matches"] / mid["join"],
            "accept": bool(mid["lookup"] <= mid["join"] + slack),
        }), flush=True)
        del x, y, op, oq, lp, lm, lp1, chips, table, cnt, first, head, pid, rj, rl, r1, runs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

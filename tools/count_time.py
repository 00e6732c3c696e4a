#!/usr/bin/env python3
"""pip_join against pip_join_count on the bench configs, at bench sizes: one JSON line per
config with the step times (HIP events around the whole call) of pip_join and of
pip_join_count without and with a weight column -- the three alternate step by step, in
--series series of --steps timed steps each; a step time is the median of the series'
medians, a spread (max - min) / median over them -- and the aggregation kernel's own time
(stats emit_kernel_ms of the count call)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def series(fns, steps, warmup):
    """`steps` rounds in which every variant of `fns` runs once, each call timed by HIP
    events, after `warmup` untimed rounds: {name: (median ms, last result)}.  The variants
    alternate step by step, so a drift of the clocks falls on all of them alike."""
    last = {}
    for _ in range(warmup):
        for k, fn in fns.items():
            last[k] = fn()
    ms = {k: [] for k in fns}
    for _ in range(steps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            last[k] = fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: (float(np.median(v)), last[k]) for k, v in ms.items()}


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
        w = torch.arange(n, dtype=torch.int64, device=dev) * 3 - 7
        cap = int(n * wl["pairs_per_point"]) + 1024
        op = torch.empty(cap, dtype=torch.int64, device=dev)
        oq = torch.empty(cap, dtype=torch.int32, device=dev)
        P = len(chips.polygons())
        cnt = torch.zeros(P, dtype=torch.int64, device=dev)
        sm = torch.zeros(P, dtype=torch.int64, device=dev)
        join = lambda: M.pip_join(x, y, chips, ns.res, out=(op, oq), capacity=cap, index_system=wl["isys"])
        count = lambda: M.pip_join_count(x, y, chips, ns.res, index_system=wl["isys"], out=(cnt, None))
        countw = lambda: M.pip_join_count(x, y, chips, ns.res, index_system=wl["isys"], weight=w, out=(cnt, sm))
        fns = {"join": join, "count": count, "count_weight": countw}
        runs = [series(fns, a.steps, a.warmup if i == 0 else 1) for i in range(a.series)]
        med = {k: [r[k][0] for r in runs] for k in fns}
        mid = {k: float(np.median(v)) for k, v in med.items()}
        spread = {k: (max(v) - min(v)) / mid[k] for k, v in med.items()}
        rj, rw = runs[-1]["join"][1], runs[-1]["count_weight"][1]
        rc = count()  # (the unweighted counts last: cnt is checked below)
        # the counts against the pairs of the same build
        m = len(rj)
        ids = rc.polygon_id.to(torch.int64)
        ref = torch.bincount(torch.searchsorted(ids, rj.polygon_id.to(torch.int64)), minlength=P)
        print(json.dumps({
            "config": c, "points": n, "polygons": P, "pairs": m, "pipeline": rc.stats["pipeline"],
            "series": a.series, "steps": a.steps,
            "join_ms": mid["join"], "join_ms_runs": med["join"], "join_spread": spread["join"],
            "count_ms": mid["count"], "count_ms_runs": med["count"], "count_spread": spread["count"],
            "count_weight_ms": mid["count_weight"], "count_weight_ms_runs": med["count_weight"],
            "count_weight_spread": spread["count_weight"],
            "join_emit_kernel_ms": rj.stats["emit_kernel_ms"], "join_kernel_ms": rj.stats["kernel_ms"],
            "count_agg_kernel_ms": rc.stats["emit_kernel_ms"], "count_kernel_ms": rc.stats["kernel_ms"],
            "count_weight_agg_kernel_ms": rw.stats["emit_kernel_ms"],
            "count_equals_join": bool(torch.equal(ref, cnt)) and int(cnt.sum()) == m,
            "count_over_join": mid["count"] / mid["join"],
            "count_weight_over_join": mid["count_weight"] / mid["join"],
        }), flush=True)
        del x, y, w, op, oq, chips, table, cnt, sm
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

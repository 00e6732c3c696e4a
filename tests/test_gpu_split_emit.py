"""split_emit_kernel's two per-item forms, against the oracle, pair for pair and in order.

A wave of the emit takes the branch-free fast form when each of its 1,024 points is empty,
a one-match class answered from the LDS class table, or a mixed point whose staged answer
has at most one match; any other item (a multi-match class, a class past the staged table,
a mixed rank past the kEmitMres = 512 staged answers, a mixed answer over several chips)
sends its whole wave through the general loop.  Both forms fill the same LDS window (2,048
pairs), which the workgroup then writes out; a chunk whose pairs fit one window skips the
per-item window test.  Every case forces the split pipeline, is at most three chunks of
4,096 points, and shows from the oracle (or the pixel index's host lookup) that its input
has the property it is named for.
"""
import os
import struct
import sys

import numpy as np
import pytest
import torch

import mosaic_amd as M
import oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from geom_util import NYC_BBOX, nyc_points  # noqa: E402
from test_raster_host import raster_lookup  # noqa: E402

pytestmark = pytest.mark.gpu

CHUNK = 4096      # kChunk: points per emit workgroup
ITEMS = 16        # kClsItems: codes per emit thread
WAVE = 64 * ITEMS  # points of one emit wave
STAGED = 512      # kEmitMres: mixed answers of a chunk staged in LDS
WINDOW = 2048     # kEmitWin: pairs staged at a time
MIXED = 2         # mgpu_test_raster_host's kind of a point left to the mixed tiles
INT32_MIN = -2 ** 31


def T(a, dev, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def oracle_join(c, x, y, res=9):
    return O.pip_join(c.index_system, res, x, y, c.cell, c.polygon_id, c.is_core, c.wkb_offsets, c.wkb)


def split_join(gpu, c, x, y, res=9, **kw):
    ctx = M.default_context(gpu)
    with ctx.options(pipeline=1):
        r = M.pip_join(T(x, gpu), T(y, gpu), c, res, **kw)
    assert r.stats["pipeline"] == 1  # the split pipeline (classify / mixed / emit)
    return r


def assert_pairs_equal(got, want):
    assert len(got[0]) == len(want[0]), "%d pairs, the oracle has %d" % (len(got[0]), len(want[0]))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def pairs_per_point(op, n):
    return np.bincount(op, minlength=n)


def chip_edge_points(c, n, seed, eps=1e-7):
    """Chip vertices and edge midpoints (as test_gpu_parity's adversarial_points), each
    moved by a seeded jitter of at most eps degrees in x and y: points on either side of,
    and a few exactly on, chip edges.  The first n of a seeded shuffle."""
    xs, ys = [], []
    for r in range(0, len(c), 3):
        blob = bytes(c.wkb[c.wkb_offsets[r]:c.wkb_offsets[r + 1]])
        if not blob or blob[4] != 3:
            continue
        (npts,) = struct.unpack(">I", blob[9:13])
        pts = [struct.unpack(">dd", blob[13 + 16 * i:29 + 16 * i]) for i in range(npts)]
        for i in range(npts - 1):
            xs += [pts[i][0], 0.5 * (pts[i][0] + pts[i + 1][0])]
            ys += [pts[i][1], 0.5 * (pts[i][1] + pts[i + 1][1])]
    x, y = np.array(xs), np.array(ys)
    rng = np.random.default_rng(seed)
    sel = rng.permutation(len(x))[:n]
    assert len(sel) == n
    jx, jy = rng.uniform(-eps, eps, n), rng.uniform(-eps, eps, n)
    keep = rng.random(n) < 0.05  # (a few stay exactly on their vertex or midpoint)
    jx[keep], jy[keep] = 0.0, 0.0
    return x[sel] + jx, y[sel] + jy


def overlap_chips(nyc_zones):
    """The NYC zones and one rectangle over the middle quarter of their bbox, tessellated
    together at res 9: consecutive uniform points fall into one-match classes (outside the
    rectangle, or inside it on water) and two-match classes (inside it on a zone)."""
    x0, y0, x1, y1 = NYC_BBOX
    xa, xb = x0 + 0.25 * (x1 - x0), x0 + 0.75 * (x1 - x0)
    ya, yb = y0 + 0.25 * (y1 - y0), y0 + 0.75 * (y1 - y0)
    rect = [(xa, ya), (xb, ya), (xb, yb), (xa, yb), (xa, ya)]
    new_id = int(nyc_zones.poly_id.max()) + 1000
    polys = M.Polygons.from_lists(_lists(nyc_zones) + [(new_id, [[rect]])])
    return M.tessellate(polys, M.H3IndexSystem(), 9), new_id


@pytest.fixture(scope="module")
def nyc_overlap_chips(nyc_zones):
    return overlap_chips(nyc_zones)


def _lists(P):
    out = []
    for p in range(len(P)):
        parts = []
        for q in range(P.poly_part_off[p], P.poly_part_off[p + 1]):
            parts.append([[tuple(v) for v in P.xy[P.ring_off[r]:P.ring_off[r + 1]]]
                          for r in range(P.part_ring_off[q], P.part_ring_off[q + 1])])
        out.append((int(P.poly_id[p]), parts))
    return out


# ------------------------------------------------------------ 1. sizes and tails

@pytest.fixture(scope="module")
def uniform_8205(nyc_chips_r9):
    x, y = nyc_points(8205, 84)  # (its first point lies in a zone: n = 1 gives a pair)
    return x, y, oracle_join(nyc_chips_r9, x, y)


@pytest.mark.parametrize("n", [1, 15, 16, 4095, 4096, 4097, 8205])
def test_sizes_and_tails(gpu, nyc_chips_r9, uniform_8205, n):
    """Uniform points, zones that do not overlap: the partial last thread and chunk,
    threads without a pair, one window per chunk, the fast form throughout (a pure point
    has at most one match; the few mixed points are far fewer than the staged 512)."""
    x, y, (op, oq) = uniform_8205
    keep = op < n  # (the join of a prefix is the prefix of the join: pairs are in point order)
    want = (op[keep], oq[keep])
    assert len(want[0]) > 0, "a non-empty result"
    ppp = pairs_per_point(want[0], n)
    assert ppp.max() == 1
    # per thread of the launched workgroups (the codes past the last point are empty)
    per_thread = np.pad(ppp, (0, -n % CHUNK)).reshape(-1, ITEMS).sum(1)
    assert n in (CHUNK - 1, CHUNK) or (per_thread == 0).any(), "threads with no pair"
    if n >= CHUNK - 1:
        assert per_thread.max() > 1, "threads with several pairs"
        assert np.add.reduceat(ppp, np.arange(0, n, CHUNK)).max() <= WINDOW
    r = split_join(gpu, nyc_chips_r9, x[:n], y[:n])
    assert_pairs_equal(r.numpy(), want)
    assert r.stats["n_pairs"] == len(want[0])


# ------------------------------------------------------------ 2. more than one window

def test_two_windows_fast_form(gpu, nyc_chips_r9):
    """4,196 points inside one large zone: one pair per point, 4,096 pairs in the first
    chunk -- two windows, so the fast form runs with its per-item window test."""
    x, y = nyc_points(60_000, 90)
    op, oq = oracle_join(nyc_chips_r9, x, y)
    big = np.bincount(oq - oq.min()).argmax() + oq.min()
    inside = op[oq == big]  # (uniform points in that zone's bounding box, then those it holds)
    rng = np.random.default_rng(91)
    x = rng.uniform(x[inside].min(), x[inside].max(), 40_000)
    y = rng.uniform(y[inside].min(), y[inside].max(), 40_000)
    op, oq = oracle_join(nyc_chips_r9, x, y)
    sel = op[oq == big][:CHUNK + 100]
    assert len(sel) == CHUNK + 100
    x, y = np.ascontiguousarray(x[sel]), np.ascontiguousarray(y[sel])
    want = oracle_join(nyc_chips_r9, x, y)
    assert np.array_equal(want[0], np.arange(len(x))) and (want[1] == big).all(), "exactly one pair per point"
    assert_pairs_equal(split_join(gpu, nyc_chips_r9, x, y).numpy(), want)


# ------------------------------------------------------------ 3. general form everywhere

SQ0 = 10.0  # the squares' common corner, in degrees of longitude and latitude


def nested_squares(res):
    sq = [(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0), (0.0, 0.0)]
    polys = [(pid, [[[(SQ0 + x * (1 + 0.01 * pid), SQ0 + y * (1 + 0.01 * pid)) for x, y in sq]]])
             for pid in (5, 3, 9, 1, 7)]
    return M.tessellate(M.Polygons.from_lists(polys), M.H3IndexSystem(), res)


def test_five_matches_per_point_general_form(gpu):
    """Five nested squares (test_pip_join_default_capacity_grows's, H3 res 5), 4,196 points
    inside the innermost: every point gives five pairs -- classes past raster_pc[3], ten
    windows in the first chunk, every wave in the general form.  That test's squares have
    their corner at (0, 0), where the table gets no pixel index at any resolution from 3 to
    9 (so no split pipeline); here the same squares stand at (10, 10), where it gets one at
    res 5 -- shown below with the host lookup."""
    c = nested_squares(5)
    rng = np.random.default_rng(85)
    n = CHUNK + 100
    x, y = SQ0 + rng.uniform(0.05, 0.95, n), SQ0 + rng.uniform(0.05, 0.95, n)
    kind, _, mask, _ = raster_lookup(c, 5, x, y)
    assert not (kind == 4).any(), "the table has a pixel index at res 5"
    pure = kind == 1
    assert pure.mean() > 0.5 and all(bin(int(m)).count("1") == 5 for m in mask[pure]), "five-match classes"
    want = oracle_join(c, x, y, res=5)
    assert (pairs_per_point(want[0], n) == 5).all()
    r = split_join(gpu, c, x, y, res=5, capacity=5 * n)
    assert_pairs_equal(r.numpy(), want)


# ------------------------------------------------------------ 4. both forms' lanes in one wave

def test_one_and_two_match_classes_in_one_wave(gpu, nyc_overlap_chips):
    """The zones plus a rectangle over a quarter of the bbox: one- and two-match classes
    (and none) side by side in every wave, so lanes the fast form could answer go through
    the general form with their wave, beside waves of other chunks that stay fast."""
    c, new_id = nyc_overlap_chips
    x, y = nyc_points(8205, 86)
    want = oracle_join(c, x, y)
    ppp = pairs_per_point(want[0], len(x))
    assert (ppp[:64] == 1).any() and (ppp[:64] == 2).any(), "both pair counts among the first 64 points"
    for w in range(0, len(x), WAVE):
        assert (ppp[w:w + WAVE] == 2).any() and (ppp[w:w + WAVE] == 1).any()
    assert (want[1] == new_id).any() and (want[1] != new_id).any()
    assert_pairs_equal(split_join(gpu, c, x, y).numpy(), want)


# ------------------------------------------------------------ 5. mixed answers past the staged 512

def check_chip_edge_points(gpu, c, seed, multi):
    n = 3500
    x, y = chip_edge_points(c, n, seed)
    kind, _, _, _ = raster_lookup(c, 9, x, y)
    assert (kind == MIXED).sum() > 2 * STAGED, "far more mixed points in the chunk than the staged %d" % STAGED
    want = oracle_join(c, x, y)
    ppp = pairs_per_point(want[0], n)[kind == MIXED]
    assert (ppp == 0).any() and (ppp == 1).any(), "0- and 1-match mixed answers"
    assert not multi or (ppp == 2).sum() > 100, "many 2-match mixed answers"
    r = split_join(gpu, c, x, y)
    assert r.stats["n_candidates"] > STAGED
    assert_pairs_equal(r.numpy(), want)


def test_mixed_answers_past_the_staged_count(gpu, nyc_chips_r9):
    """3,500 points within 1e-7 degrees of chip edges, one chunk: mixed ranks below and past
    the 512 staged in LDS, with no match and with one."""
    check_chip_edge_points(gpu, nyc_chips_r9, 87, multi=False)


def test_multi_chip_mixed_answers(gpu, nyc_overlap_chips):
    """The same on the overlapping table: mixed answers with two matches, over two chips."""
    check_chip_edge_points(gpu, nyc_overlap_chips[0], 88, multi=True)


# ------------------------------------------------------------ 6. ids and bounds

def test_ids_and_bounds(gpu, nyc_chips_r9):
    """Negative polygon ids with INT32_MIN, an explicit point_id column, a point_id_base, a
    capacity below the pair count, and a preallocated output of the exact size."""
    c0 = nyc_chips_r9
    pid = -c0.polygon_id.astype(np.int64) * 1000
    x, y = nyc_points(CHUNK + 205, 89)
    _, q0 = oracle_join(c0, x, y)
    pid[c0.polygon_id == np.bincount(q0).argmax()] = INT32_MIN
    c = M.ChipTable(c0.cell, pid.astype(np.int32), c0.is_core, c0.wkb_offsets, c0.wkb)
    op, oq = oracle_join(c, x, y)
    assert (oq < 0).all() and (oq == INT32_MIN).any() and len(op) > 1000
    d = c.upload()
    ids = np.arange(len(x), dtype=np.int64) * 7 + 11
    r = split_join(gpu, d, x, y, point_id=T(ids, gpu, np.int64))
    assert_pairs_equal(r.numpy(), (ids[op], oq))
    r = split_join(gpu, d, x, y, point_id_base=10 ** 12)
    assert_pairs_equal(r.numpy(), (op + 10 ** 12, oq))
    ctx = M.default_context(gpu)
    with ctx.options(pipeline=1), pytest.raises(M.CapacityError) as ei:
        M.pip_join(T(x, gpu), T(y, gpu), d, 9, capacity=len(op) - 1)
    assert ei.value.required == len(op)
    out = (torch.full((len(op),), -5, dtype=torch.int64, device=gpu),
           torch.full((len(op),), 5, dtype=torch.int32, device=gpu))
    r = split_join(gpu, d, x, y, out=out, capacity=len(op))
    assert_pairs_equal(r.numpy(), (op, oq))
    assert np.array_equal(out[0].cpu().numpy(), op) and np.array_equal(out[1].cpu().numpy(), oq)

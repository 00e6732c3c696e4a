"""Shared by tests/test_cellgeom_host.py and tests/test_gpu_cellgeom.py: the fixed H3 cell
set, the host twin's binding, and Python restatements of the reference's cell geometry
(IndexSystem.area, BNGIndexSystem getX / getY / getEdgeSize, H3IndexSystem.indexToGeometry's
ring shapes, the WKB layout)."""
import ctypes
import functools
import os
import struct

import numpy as np

import oracle as O
from mosaic_amd import _native

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PENTAGON_BASE_CELLS = (4, 14, 24, 38, 49, 58, 63, 72, 83, 97, 107, 117)
DOC_AREA_CELL, DOC_AREA_KM2 = 613177664827555839, 0.78595419  # docs/source/api/spatial-indexing.rst:642-648


def _P(a):
    return ctypes.c_void_p(a.ctypes.data)


def h3_cell(res, base_cell, digits=()):
    """The H3 id of (resolution, base cell, digits 1..res); the digits beyond are 7."""
    h = (1 << 59) | (res << 52) | (base_cell << 45)
    for r in range(1, 16):
        d = digits[r - 1] if r <= res else 7
        h |= d << (3 * (15 - r))
    return h


def pentagons(res):
    return [h3_cell(res, bc, (0,) * res) for bc in PENTAGON_BASE_CELLS]


def uniform_points(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-180.0, 180.0, n), np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, n)))


@functools.lru_cache(maxsize=None)
def fixed_h3_cells():
    """The issue's cell set (distinct, ascending): res 0 and 1 whole, the pentagons and pole
    cells of every resolution, cells across the antimeridian at res 0-5, cells on
    icosahedron edges at res 5, 9, 15 (distortion vertices), 300 uniform cells per res 2-15."""
    cells = [h3_cell(0, bc) for bc in range(122)]
    cells += [h3_cell(1, bc, (d,)) for bc in range(122) for d in range(7) if not (bc in PENTAGON_BASE_CELLS and d == 1)]
    for r in range(16):
        cells += pentagons(r)
        cells += O.h3_points_to_cells(np.zeros(2), np.array([90.0, -90.0]), r).tolist()
    lat = np.linspace(-80.0, 80.0, 33)
    for r in range(6):
        for lon in (179.9999, -179.9999):
            cells += O.h3_points_to_cells(np.full(len(lat), lon), lat, r).tolist()
    z = np.load(os.path.join(GOLDEN, "h3_edge_points.npz"))
    for r in (5, 9, 15):
        cells += O.h3_points_to_cells(z["lon"][:2000].copy(), z["lat"][:2000].copy(), r).tolist()
    for r in range(2, 16):
        x, y = uniform_points(300, 8800 + r)
        cells += O.h3_points_to_cells(x, y, r).tolist()
    out = np.unique(np.array(cells, dtype=np.int64))
    out.setflags(write=False)
    return out


def twin(index_system, cells):
    """mgpu_test_cell_geometry_host: (xy (n, 10, 2), nverts, centre (n, 2), area) on the host."""
    cells = np.ascontiguousarray(cells, dtype=np.int64)
    n = len(cells)
    xy = np.zeros((max(n, 1), 20))
    nv = np.zeros(max(n, 1), np.int32)
    c = np.zeros((max(n, 1), 2))
    a = np.zeros(max(n, 1))
    _native.check(_native.lib().mgpu_test_cell_geometry_host(index_system, _P(cells), n, _P(xy), _P(nv), _P(c), _P(a)))
    return xy[:n].reshape(n, 10, 2), nv[:n], c[:n], a[:n]


@functools.lru_cache(maxsize=None)
def fixed_h3_twin():
    out = twin(0, fixed_h3_cells())
    for a in out:
        a.setflags(write=False)
    return out


def glibc_route(cells):
    """mgpu_test_h3_boundary_host: today's host route (the host's libm)."""
    cells = np.ascontiguousarray(cells, dtype=np.int64)
    n = len(cells)
    xy = np.zeros((n, 20))
    nv = np.zeros(n, np.int32)
    c = np.zeros((n, 2))
    _native.check(_native.lib().mgpu_test_h3_boundary_host(_P(cells), n, _P(xy), _P(nv), _P(c)))
    return xy.reshape(n, 10, 2), nv, c


# ---------------------------------------------------------------- IndexSystem.area (IndexSystem.scala:248-289)

def _haversine(lat1, lng1, lat2, lng2):
    c = np.pi / 180
    th1, th2, dph = c * lat1, c * lat2, c * (lng1 - lng2)
    dz = np.sin(th1) - np.sin(th2)
    dx = np.cos(dph) * np.cos(th1) - np.cos(th2)
    dy = np.sin(dph) * np.cos(th1)
    return np.arcsin(np.sqrt(dx * dx + dy * dy + dz * dz) / 2) * 2


def np_area(xy, nv, centre):
    """IndexSystem.area restated with numpy over boundaries (n, 10, 2) of (lng, lat) and
    centres (n, 2): the triangles (centre, b_k, b_k+1) of the closed boundary, in order."""
    out = np.zeros(len(nv))
    for k in range(10):
        m = nv > k
        if not m.any():
            break
        b0 = xy[m, k]
        b1 = xy[m, np.where(k + 1 < nv[m], k + 1, 0)]
        clng, clat = centre[m, 0], centre[m, 1]
        a = _haversine(clat, clng, b0[:, 1], b0[:, 0])
        b = _haversine(b0[:, 1], b0[:, 0], b1[:, 1], b1[:, 0])
        c = _haversine(b1[:, 1], b1[:, 0], clat, clng)
        s = (a + b + c) / 2
        t = np.sqrt(np.tan(s / 2) * np.tan((s - a) / 2) * np.tan((s - b) / 2) * np.tan((s - c) / 2))
        out[m] += 4 * np.arctan(t) * 6371.0088 * 6371.0088
    return out


# ---------------------------------------------------------------- BNG (BNGIndexSystem.scala:163-170, 451-516)

BNG_RESOLUTIONS = (1, -1, 2, -2, 3, -3, 4, -4, 5, -5, 6, -6)
_BNG_EDGE = {1: 100000, -1: 500000, 2: 10000, -2: 50000, 3: 1000, -3: 5000, 4: 100, -4: 500, 5: 10, -5: 50, 6: 1, -6: 5}


def bng_cell_geometry(cell):
    """(corners [(x, y)] * 4, area km^2) from the id's decimal digits, as getResolution,
    getEdgeSize, getX, getY, indexToGeometry and area do it."""
    digits = [int(ch) for ch in str(int(cell))]
    n = len(digits)
    if n < 6:
        res = -1
    else:
        k = (n - 6) // 2
        res = -(k + 2) if digits[-1] > 0 else k + 1
    edge = _BNG_EDGE[res]
    k = (n - 6) // 2 if n >= 6 else -1  # (n - 6) / 2 of a JVM Int truncates towards zero
    k = max(k, 0)
    q = digits[-1]
    adj = 2 * edge if q > 0 else edge
    x = int("".join(map(str, digits[1:3] + digits[5:5 + k]))) * adj + (edge if q in (3, 4) else 0)
    y = int("".join(map(str, digits[3:5] + digits[5 + k:5 + 2 * k]))) * adj + (edge if q in (2, 3) else 0)
    corners = [(float(x), float(y)), (float(x + edge), float(y)), (float(x + edge), float(y + edge)), (float(x), float(y + edge))]
    return corners, (edge / 1000.0) ** 2


# ---------------------------------------------------------------- H3IndexSystem.indexToGeometry's shapes

def jts_intersection(p1, p2, q1, q2):
    """JTS 1.20 Intersection.intersection, in its operation order (tests/test_tessellate_host.py)."""
    midx = (max(min(p1[0], p2[0]), min(q1[0], q2[0])) + min(max(p1[0], p2[0]), max(q1[0], q2[0]))) / 2.0
    midy = (max(min(p1[1], p2[1]), min(q1[1], q2[1])) + min(max(p1[1], p2[1]), max(q1[1], q2[1]))) / 2.0
    p1x, p1y, p2x, p2y = p1[0] - midx, p1[1] - midy, p2[0] - midx, p2[1] - midy
    q1x, q1y, q2x, q2y = q1[0] - midx, q1[1] - midy, q2[0] - midx, q2[1] - midy
    px, py, pw = p1y - p2y, p2x - p1x, p1x * p2y - p2x * p1y
    qx, qy, qw = q1y - q2y, q2x - q1x, q1x * q2y - q2x * q1y
    x, y, w = py * qw - qy * pw, qx * pw - px * qw, px * qy - qx * py
    return (x / w + midx, y / w + midy)


def make_pole_geometry(boundary, north):
    """makePoleGeometry (H3IndexSystem.scala:361-380), as tests/test_tessellate_host.py
    restates it: one ring, counter-clockwise at the north pole, clockwise at the south."""
    pl = 90.0 if north else -90.0
    v = sorted(((x + 360.0 if x < 0 else x, y) for x, y in boundary), key=lambda p: p[0])
    k = next(i for i, p in enumerate(v) if p[0] > 180.0)
    cut = jts_intersection(v[k - 1], v[k], (180.0, 90.0), (180.0, -90.0))
    west = v[:k] + [cut]
    east = [(cut[0] - 360.0, cut[1])] + [(x - 360.0, y) for x, y in v[k:]]
    return west + [(180.0, pl), (-180.0, pl)] + east + [west[0]]


def _ring_area(r):
    return 0.5 * sum(r[i][0] * r[i + 1][1] - r[i + 1][0] * r[i][1] for i in range(len(r) - 1))


def _clip_ring(ring, clip):
    """Sutherland-Hodgman of a closed ring against a convex ccw box (closed): a closed ring or None."""
    cur = ring[:-1]
    for e in range(len(clip) - 1):
        if not cur:
            break
        a, b = clip[e], clip[e + 1]
        side = lambda p: (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])  # noqa: E731
        out = []
        prev = cur[-1]
        sp = side(prev)
        for p in cur:
            sc = side(p)
            if sc >= 0:
                if sp < 0:
                    t = sp / (sp - sc)
                    out.append((prev[0] + t * (p[0] - prev[0]), prev[1] + t * (p[1] - prev[1])))
                out.append(p)
            elif sp >= 0:
                t = sp / (sp - sc)
                out.append((prev[0] + t * (p[0] - prev[0]), prev[1] + t * (p[1] - prev[1])))
            prev, sp = p, sc
        cur = out
    return cur + [cur[0]] if len(cur) >= 3 else None


def crosses_antimeridian(boundary):
    lo, hi = min(p[0] for p in boundary), max(p[0] for p in boundary)
    return lo < 0 <= hi and hi - lo > 180.0


def antimeridian_parts(boundary):
    """makeSafeGeometry (H3IndexSystem.scala:386-410) for a cell across the antimeridian:
    the western longitudes shifted east, the ring cut at 180 into its western part and its
    eastern part (shifted back), each a counter-clockwise ring."""
    b = [(x + 360.0 if x < 0 else x, y) for x, y in boundary]
    b.append(b[0])
    if _ring_area(b) < 0:
        b.reverse()
    parts = []
    w = _clip_ring(b, [(0.0, -90.0), (180.0, -90.0), (180.0, 90.0), (0.0, 90.0), (0.0, -90.0)])
    if w and abs(_ring_area(w)) > 0:
        parts.append(w)
    e = _clip_ring(b, [(180.0, -90.0), (360.0, -90.0), (360.0, 90.0), (180.0, 90.0), (180.0, -90.0)])
    if e and abs(_ring_area(e)) > 0:
        parts.append([(x - 360.0, y) for x, y in e])
    return parts


def pack_wkb(rings):
    """Big-endian 2-D WKB of one-ring polygons: a Polygon, or a MultiPolygon of several."""
    def polygon(r):
        return struct.pack(">BII", 0, 3, 1) + struct.pack(">I", len(r)) + b"".join(struct.pack(">dd", x, y) for x, y in r)
    if len(rings) == 1:
        return polygon(rings[0])
    return struct.pack(">BII", 0, 6, len(rings)) + b"".join(polygon(r) for r in rings)


def h3_expected_wkb(cell, boundary, poles):
    """The WKB of an H3 cell from its boundary [(lng, lat)] (not closed): the pole caps,
    the antimeridian split, or the closed ring.  poles: {cell: north?} of its resolution."""
    if cell in poles:
        return pack_wkb([make_pole_geometry(boundary, poles[cell])])
    if crosses_antimeridian(boundary):
        return pack_wkb(antimeridian_parts(boundary))
    return pack_wkb([boundary + [boundary[0]]])


@functools.lru_cache(maxsize=None)
def pole_cells():
    """{cell: is the north pole's} over every resolution."""
    out = {}
    for r in range(16):
        n, s = O.h3_points_to_cells(np.zeros(2), np.array([90.0, -90.0]), r).tolist()
        out[n], out[s] = True, False
    return out

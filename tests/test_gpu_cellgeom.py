"""Cell id -> geometry on the device (mgpu_cells_to_centers / _boundaries / _boundary_wkb /
_area and their hosts) on the MI355X.

The device runs the code of the host twin (mgpu_test_cell_geometry_host; h3_boundary.h under
its correctly rounded policy), so boundaries, centres and areas are compared with it bit for
bit, no tolerance; tests/test_cellgeom_host.py pins the twin against today's glibc route and a
numpy restatement of IndexSystem.area.  Independently of the twin, every centre and every
vertex nudged towards the centre maps back to its cell under the oracle's geoToH3.  WKB rows
are compared with rings packed in Python from the device's own boundaries: the closed ring,
makePoleGeometry's cap, the antimeridian split.  BNG is exact against a Python restatement of
getX / getY / getEdgeSize.
"""
import ctypes
import os

import numpy as np
import pytest

import cellgeom_util as U
import mosaic_amd as M
import oracle as O
from mosaic_amd import _native as N

pytestmark = pytest.mark.gpu

H3, BNG = M.H3IndexSystem(), M.BNGIndexSystem()
_CACHE = {}


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.array(a)).to(gpu)  # (a copy: the fixed set is read-only)


def _device_geometry(gpu):
    """The fixed H3 set through the four batch forms, once: numpy (xy, nverts, centre, area,
    wkb bytes, wkb offsets)."""
    if "h3" not in _CACHE:
        cells = _dev(U.fixed_h3_cells(), gpu)
        xy, nv = H3.cells_to_boundaries(cells)
        cx, cy = H3.cells_to_centers(cells)
        area = H3.cells_area(cells)
        w, off = H3.cells_boundary_wkb(cells)
        _CACHE["h3"] = (xy.cpu().numpy(), nv.cpu().numpy(), np.stack([cx.cpu().numpy(), cy.cpu().numpy()], 1),
                        area.cpu().numpy(), w.cpu().numpy().tobytes(), off.cpu().numpy())
    return _CACHE["h3"]


def _assert_equals_twin(got, want, what=""):
    xy, nv, centre, area = got
    txy, tnv, tcentre, tarea = want
    assert np.array_equal(nv, tnv), what
    m = np.broadcast_to(np.arange(10)[None, :, None] < tnv[:, None, None], txy.shape)
    assert np.array_equal(xy[m].view(np.int64), txy[m].view(np.int64)), what
    assert np.array_equal(centre.view(np.int64), tcentre.view(np.int64)), what
    assert np.array_equal(area.view(np.int64), tarea.view(np.int64)), what


def test_device_equals_twin_bit_for_bit(gpu):
    xy, nv, centre, area, _, _ = _device_geometry(gpu)
    _assert_equals_twin((xy, nv, centre, area), U.fixed_h3_twin())
    assert set(np.unique(nv).tolist()) == {5, 6, 7, 8, 10}  # pentagons, distortion vertices, Class III pentagons


@pytest.mark.parametrize("n", [1, 7, 9, 65])
def test_device_equals_twin_tails_and_misaligned_column(gpu, n):
    """Group (8 lanes per cell) and wave tails, and a column that starts 8 bytes past a
    16-byte boundary.  The cells: spread over the fixed set, a Class III pentagon first."""
    import torch
    all_cells = U.fixed_h3_cells()
    pick = np.r_[np.flatnonzero(U.fixed_h3_twin()[1] == 10)[:1], np.linspace(0, len(all_cells) - 1, n).astype(np.int64)][:n]
    want = tuple(a[pick] for a in U.fixed_h3_twin())
    buf = torch.zeros(n + 2, dtype=torch.int64, device=gpu)
    col = buf[1 - (buf.data_ptr() // 8) % 2:][:n]
    assert col.data_ptr() % 16 == 8
    col.copy_(_dev(all_cells[pick], gpu))
    xy, nv = H3.cells_to_boundaries(col)
    cx, cy = H3.cells_to_centers(col)
    area = H3.cells_area(col)
    got = (xy.cpu().numpy(), nv.cpu().numpy(), np.stack([cx.cpu().numpy(), cy.cpu().numpy()], 1), area.cpu().numpy())
    _assert_equals_twin(got, want, n)


def _nudge(v, c, pole, frac):
    """The point `frac` of the way from vertex v to centre c ((lng, lat) degrees) along the
    chord; for pole cells in the azimuthal plane about their pole (unit vectors lose the
    colatitude there)."""
    lo, la, clo, cla = np.radians(v[:, 0]), np.radians(v[:, 1]), np.radians(c[:, 0]), np.radians(c[:, 1])
    a = np.stack([np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)], -1)
    b = np.stack([np.cos(cla) * np.cos(clo), np.cos(cla) * np.sin(clo), np.sin(cla)], -1)
    u = a + frac[:, None] * (b - a)
    x, y = np.degrees(np.arctan2(u[:, 1], u[:, 0])), np.degrees(np.arctan2(u[:, 2], np.hypot(u[:, 0], u[:, 1])))
    s = np.sign(c[:, 1])
    r0, r1 = 90 - s * v[:, 1], 90 - s * c[:, 1]
    px = r0 * np.cos(lo) + frac * (r1 * np.cos(clo) - r0 * np.cos(lo))
    py = r0 * np.sin(lo) + frac * (r1 * np.sin(clo) - r0 * np.sin(lo))
    return np.where(pole, np.degrees(np.arctan2(py, px)), x), np.where(pole, s * (90 - np.hypot(px, py)), y)


def test_oracle_anchor(gpu):
    """Independent of the twin: every device centre maps back to its cell under the oracle's
    geoToH3, and so does every device vertex moved 1e-3 of the way to the centre.  The pole
    cells of resolutions 14 and 15 are moved 0.1 of the way: H3's asin(sinlat) leaves a
    vertex at colatitude p with an error of 2^-53 / p, which for a pole cell (p about the
    edge e) is 2^-53 / e^2 of the edge -- 2.5e-3 at resolution 14 (e = 2.1e-7 rad), 1.7e-2
    at 15, 3.5e-4 at 13.  The reference's vertices carry the same error."""
    cells = U.fixed_h3_cells()
    xy, nv, centre, _, _, _ = _device_geometry(gpu)
    res = (cells >> 52) & 15
    pole = np.array([h in U.pole_cells() for h in cells.tolist()])
    frac = np.where(pole & (res >= 14), 0.1, 1e-3)
    for r in range(16):
        m = res == r
        assert np.array_equal(O.h3_points_to_cells(centre[m, 0].copy(), centre[m, 1].copy(), r), cells[m]), r
        for k in range(10):
            mk = m & (nv > k)
            if mk.any():
                x, y = _nudge(xy[mk, k], centre[mk], pole[mk], frac[mk])
                assert np.array_equal(O.h3_points_to_cells(x, y, r), cells[mk]), (r, k)


def _check_h3_wkb(cells, xy, nv, w, off, valid=None):
    assert off[0] == 0 and np.all(np.diff(off) >= 0) and off[-1] == len(w)
    special = 0
    for i, h in enumerate(cells.tolist()):
        row = w[off[i]:off[i + 1]]
        if valid is not None and not valid[i]:
            assert row == b""
            continue
        b = [tuple(p) for p in xy[i, :nv[i]].tolist()]
        assert row == U.h3_expected_wkb(h, b, U.pole_cells()), hex(h)
        special += h in U.pole_cells() or U.crosses_antimeridian(b)
    return special


def test_wkb_rows(gpu):
    cells = U.fixed_h3_cells()
    xy, nv, _, _, w, off = _device_geometry(gpu)
    special = _check_h3_wkb(cells, xy, nv, w, off)
    assert special >= 32 + 12  # every resolution's two pole cells, cells across the antimeridian


def test_wkb_capacity_and_empty_column(gpu):
    import torch
    cells = _dev(U.fixed_h3_cells()[::40], gpu)
    n = cells.numel()
    ctx = M.default_context(gpu)
    s = torch.cuda.current_stream(gpu).cuda_stream
    w, off = H3.cells_boundary_wkb(cells)
    need = w.numel()
    out = torch.zeros(need, dtype=torch.uint8, device=gpu)
    o2 = torch.zeros(n + 1, dtype=torch.int64, device=gpu)
    tot = ctypes.c_int64()
    call = lambda cap: N.lib().mgpu_cells_boundary_wkb(ctx.handle, 0, cells.data_ptr(), None, 0, n, out.data_ptr(), cap,  # noqa: E731
                                                       o2.data_ptr(), ctypes.byref(tot), None, s)
    assert call(need - 1) == N.MGPU_E_CAPACITY and tot.value == need
    assert call(need) == N.MGPU_OK and tot.value == need
    assert torch.equal(out, w) and torch.equal(o2, off)
    e, eo = H3.cells_boundary_wkb(cells[:0])
    assert e.numel() == 0 and eo.cpu().tolist() == [0]
    assert H3.cells_area(cells[:0]).numel() == 0 and H3.cells_to_boundaries(cells[:0])[1].numel() == 0


def test_nulls(gpu):
    """A validity bitmap read from bit 3, and an all-null column: null rows have 0 vertices,
    an empty WKB row, a 0 bit in the returned bitmap, NaN centre and area."""
    cells = U.fixed_h3_cells()[::23]
    n = len(cells)
    rng = np.random.default_rng(11)
    for keep in (rng.random(n) < 0.6, np.zeros(n, bool)):
        bits = np.zeros(3 + n + 16, np.uint8)
        bits[:3] = 1  # (the bits before the offset belong to other rows)
        bits[3:3 + n] = keep
        col = np.where(keep, cells, -1)  # null rows hold no cell id
        dc, dv = _dev(col, gpu), _dev(np.packbits(bits, bitorder="little"), gpu)
        want = tuple(a[::23] for a in U.fixed_h3_twin())
        xy, nv, ov = H3.cells_to_boundaries(dc, valid=dv, valid_offset=3)
        cx, cy, ov2 = H3.cells_to_centers(dc, valid=dv, valid_offset=3)
        area, ov3 = H3.cells_area(dc, valid=dv, valid_offset=3)
        w, off, ov4 = H3.cells_boundary_wkb(dc, valid=dv, valid_offset=3)
        for o in (ov, ov2, ov3, ov4):
            assert np.array_equal(np.unpackbits(o.cpu().numpy(), bitorder="little")[:n].astype(bool), keep)
        xy, nv, area = xy.cpu().numpy(), nv.cpu().numpy(), area.cpu().numpy()
        centre = np.stack([cx.cpu().numpy(), cy.cpu().numpy()], 1)
        assert (nv[~keep] == 0).all() and np.isnan(area[~keep]).all() and np.isnan(centre[~keep]).all()
        _assert_equals_twin((xy[keep], nv[keep], centre[keep], area[keep]), tuple(a[keep] for a in want))
        _check_h3_wkb(col, xy, nv, w.cpu().numpy().tobytes(), off.cpu().numpy(), valid=keep)


def test_invalid_ids(gpu):
    """Each kind of invalid id alone in an otherwise valid column fails the call; so does BNG
    where BNGIndexSystem's digit decode fails; BNG centres are unsupported."""
    import torch
    good = U.fixed_h3_cells()[::97]
    ok = U.h3_cell(3, 20, (1, 2, 3))
    bad_h3 = [ok & ~(15 << 59) | (2 << 59),        # mode 2
              U.h3_cell(3, 122, (1, 2, 3)),         # base cell 122
              U.h3_cell(3, 20, (1, 7, 3)),          # a digit 7 at or before the resolution
              ok & ~(7 << 33),                      # a digit other than 7 after it
              U.h3_cell(3, 4, (0, 1, 2))]           # a pentagon's deleted subsequence
    for bad in bad_h3:
        col = good.copy()
        col[len(col) // 2] = bad
        for call in (H3.cells_to_centers, H3.cells_to_boundaries, H3.cells_boundary_wkb, H3.cells_area):
            with pytest.raises(M.IllegalArgumentException):
                call(_dev(col, gpu))
    x, y = np.array([530000.0, 1000.0]), np.array([180000.0, 999000.0])
    bng = O.bng_points_to_cells(x, y, 4)
    for bad in (0, -5, 123, 1 << 53):
        col = np.r_[bng, bad, bng]
        for call in (BNG.cells_to_boundaries, BNG.cells_boundary_wkb, BNG.cells_area):
            with pytest.raises(M.IllegalArgumentException):
                call(_dev(col, gpu))
    ctx = M.default_context(gpu)
    d = _dev(bng, gpu)
    out = torch.zeros(4, dtype=torch.float64, device=gpu)
    st = N.lib().mgpu_cells_to_centers(ctx.handle, 1, d.data_ptr(), None, 0, 2, out.data_ptr(), out[2:].data_ptr(), None,
                                       torch.cuda.current_stream(gpu).cuda_stream)
    assert st == N.MGPU_E_UNSUPPORTED
    with pytest.raises(NotImplementedError):
        BNG.index_to_center(int(bng[0]))
    with pytest.raises(NotImplementedError):
        BNG.index_to_boundary(int(bng[0]))


def test_bng_exact(gpu):
    """Boundaries, WKB and areas of the oracle's cells of 500 London points at each of the 12
    resolutions, exact against the Python restatement of getX / getY / getEdgeSize."""
    z = np.load(os.path.join(U.GOLDEN, "london_postcode_zones.npz"))
    pts = z["xy"][:500]
    cells = np.concatenate([O.bng_points_to_cells(pts[:, 0].copy(), pts[:, 1].copy(), r) for r in U.BNG_RESOLUTIONS])
    d = _dev(cells, gpu)
    xy, nv = BNG.cells_to_boundaries(d)
    area = BNG.cells_area(d).cpu().numpy()
    w, off = BNG.cells_boundary_wkb(d)
    xy, nv, w, off = xy.cpu().numpy(), nv.cpu().numpy(), w.cpu().numpy().tobytes(), off.cpu().numpy()
    assert (nv == 4).all() and off[0] == 0 and off[-1] == len(w) == 93 * len(cells)
    known = {}
    for i, c in enumerate(cells.tolist()):
        if c not in known:
            corners, a = U.bng_cell_geometry(c)
            known[c] = (corners, a, U.pack_wkb([corners + [corners[0]]]))
        corners, a, wkb = known[c]
        assert xy[i, :4].tolist() == [list(p) for p in corners] and area[i] == a
        assert w[off[i]:off[i + 1]] == wkb
    txy, tnv, _, tarea = U.twin(1, cells)
    assert np.array_equal(txy[:, :4], xy[:, :4]) and np.array_equal(tarea, area)


def test_hosts(gpu):
    """The scalar IndexSystem forms agree with the batch forms; grid_boundary takes WKB only;
    a CellAggregate's cell column goes through grid_boundaryaswkb."""
    import torch
    cells = U.fixed_h3_cells()
    xy, nv, centre, area, w, off = _device_geometry(gpu)
    for i in (0, 500, len(cells) - 1, int(np.flatnonzero(nv == 10)[0])):
        h = int(cells[i])
        assert H3.index_to_center(h) == (centre[i, 1], centre[i, 0])
        assert H3.index_to_boundary(H3.format(h)) == [(p[1], p[0]) for p in xy[i, :nv[i]].tolist()]
        assert H3.index_to_geometry(h) == w[off[i]:off[i + 1]]
        assert H3.area(h) == area[i]
    bng = int(O.bng_points_to_cells(np.array([530000.0]), np.array([180000.0]), -4)[0])
    corners, a = U.bng_cell_geometry(bng)
    assert BNG.area(BNG.format(bng)) == a and BNG.index_to_geometry(bng) == U.pack_wkb([corners + [corners[0]]])
    d = _dev(cells[:100], gpu)
    for fmt in ("WKT", "GEOJSON", "COORDS"):
        with pytest.raises(M.IllegalArgumentException, match="not on the device path"):
            M.grid_boundary(d, fmt, H3)
    gw, go = M.grid_boundary(d, "wkb", H3)
    assert gw.cpu().numpy().tobytes() == w[:off[100]] and np.array_equal(go.cpu().numpy(), off[:101])
    assert np.array_equal(M.grid_cellarea(d, H3).cpu().numpy(), area[:100])
    # groupBy("index_id").count(), then the cells drawn
    x, y = U.uniform_points(20_000, 77)
    agg = M.CellAggregate(H3, 3, ctx=M.default_context(gpu))
    agg.add_points(_dev(x, gpu), _dev(y, gpu))
    col = agg.result().cell
    assert col.numel() > 1000
    cw, co = M.grid_boundaryaswkb(col, H3)
    cxy, cnv = H3.cells_to_boundaries(col)
    _check_h3_wkb(col.cpu().numpy(), cxy.cpu().numpy(), cnv.cpu().numpy(), cw.cpu().numpy().tobytes(), co.cpu().numpy())
    torch.cuda.synchronize(gpu)

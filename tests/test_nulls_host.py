"""The expectations of test_gpu_nulls.py, tested where they can be without a GPU: the
input-building helpers and the expected bitmap (tests/nulls_util.py) against bit-by-bit
Python loops on CPU tensors, and the ArrowArray fields the column builders produce."""
import ctypes

import numpy as np
import pytest
import torch

import mosaic_amd as M
import nulls_util as U
from mosaic_amd import arrow as A

JOIN_OFFSETS = [(0, 0), (2, 2), (8, 8), (123, 123), (6, 13), (64, 1), (5, 5)]
JOIN_SIZES = [1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097, 12289]
GEO_SIZES = (1, 8, 9, 255, 256, 257, 2049)
GEO_OFFSETS = (0, 3, 8, 61)


def bit(buf, i):
    return (int(buf[i >> 3]) >> (i & 7)) & 1


def buffer_bytes(col, k, nbytes):
    return np.frombuffer(ctypes.string_at(col.struct.array.buffers[k], nbytes), np.uint8)


@pytest.mark.parametrize("name", U.PATTERNS)
def test_patterns_row_by_row(name):
    n = 9000
    p = U.present_pattern(name, n, 5)
    assert p.dtype == bool and p.shape == (n,)
    for i in range(n):
        want = {"even_null": i % 2 == 1, "odd_null": i % 2 == 0, "runs64": (i // 64) % 2 == 0,
                "runs4096": (i // 4096) % 2 == 0, "all_null": False, "all_valid": True}.get(name)
        if want is not None:
            assert p[i] == want, (name, i)
    if name == "random30":
        assert 0.25 < 1 - p.mean() < 0.35 and np.array_equal(p, U.present_pattern(name, n, 5))
        assert not np.array_equal(p, U.present_pattern(name, n, 6))
    if name == "runs4096":  # a whole chunk of the split pipeline (rows 4096 .. 8191) is null
        assert not p[4096:8192].any() and p[:4096].all() and p[8192:].all()


@pytest.mark.parametrize("n", GEO_SIZES + (7, 63, 64, 4097))
@pytest.mark.parametrize("off", GEO_OFFSETS + (2, 13, 123))
def test_expected_bitmap_bit_by_bit(n, off):
    rng = np.random.default_rng(n * 131 + off)
    present = rng.random(off + n + 40) >= 0.3
    present[:off] = True
    present[off + n:] = True
    got = U.expected_bitmap(present, off, n)
    assert got.dtype == np.uint8 and len(got) == (n + 7) // 8
    for i in range(8 * len(got)):
        assert bit(got, i) == (int(present[off + i]) if i < n else 0), i
    # ... and the input side: the bitmap a column carries holds row r at bit r
    full = A.bitmap(present, "cpu").numpy()
    assert len(full) == (len(present) + 7) // 8
    for r in range(len(present)):
        assert bit(full, r) == int(present[r])


def _case(n, x_off, y_off, which, payloads=U.PAYLOADS, seed=0):
    rng = np.random.default_rng(1000 + n + seed)
    x, y = rng.uniform(1.0, 2.0, n), rng.uniform(3.0, 4.0, n)
    fx, fy = rng.uniform(10.0, 11.0, 300), rng.uniform(12.0, 13.0, 300)
    xp = U.present_pattern("random30", n, 1) if which in ("x", "both") else None
    yp = U.present_pattern("odd_null", n) if which in ("y", "both") else None
    rows = U.null_rows(x, y, xp, yp, payloads)
    return x, y, fx, fy, xp, yp, rows, U.embed(rows, x_off, y_off, fx, fy)


@pytest.mark.parametrize("which", ["x", "y", "both"])
@pytest.mark.parametrize("payloads", [U.PAYLOADS, U.BNG_PAYLOADS])
@pytest.mark.parametrize("n,offs", [(n, JOIN_OFFSETS[i % len(JOIN_OFFSETS)]) for i, n in enumerate(JOIN_SIZES)] +
                         [(1000, o) for o in JOIN_OFFSETS])
def test_join_case_row_by_row(n, offs, which, payloads):
    x_off, y_off = offs
    x, y, fx, fy, xp, yp, rows, case = _case(n, x_off, y_off, which, payloads)
    assert case.n == n and len(case.x) == x_off + n + U.TAIL and len(case.y) == y_off + n + U.TAIL
    sel, kept, turn = [], [], 0
    for i in range(n):
        xv = True if xp is None else bool(xp[i])
        yv = True if yp is None else bool(yp[i])
        if xv and yv:
            sel.append(i)
            assert case.x[x_off + i] == x[i] and case.y[y_off + i] == y[i]
            continue
        pay = payloads[turn % len(payloads)]
        turn += 1
        if isinstance(pay, str):
            kept.append(i)
            assert case.x[x_off + i] == x[i] and case.y[y_off + i] == y[i]
            continue
        for v, orig, ok in ((case.x[x_off + i], x[i], xv), (case.y[y_off + i], y[i], yv)):
            if ok:  # a present slot of a null row keeps its value
                assert v == orig
            else:
                assert (np.isnan(v) and np.isnan(pay)) or v == pay
    assert rows.sel.tolist() == sel and rows.kept.tolist() == kept
    assert np.array_equal(rows.both, np.isin(np.arange(n), sel))
    # outside the slice: the fill points, the same for both tails, every bit set
    assert np.array_equal(case.x[:x_off], fx[:x_off]) and np.array_equal(case.y[:y_off], fy[:y_off])
    assert np.array_equal(case.x[x_off + n:], fx[U.HEAD:U.HEAD + U.TAIL])
    assert np.array_equal(case.y[y_off + n:], fy[U.HEAD:U.HEAD + U.TAIL])
    for present, full, off in ((xp, case.x_present, x_off), (yp, case.y_present, y_off)):
        if present is None:
            assert full is None
            continue
        assert len(full) == off + n + U.TAIL
        for r in range(len(full)):
            assert full[r] == (present[r - off] if off <= r < off + n else True)


def test_join_case_keep_rows():
    n = 400
    x, y = np.arange(n) + 0.5, np.arange(n) + 0.25
    xp = U.present_pattern("even_null", n)
    keep = [0, 2, 10, 11]  # (11 is present: not a null row, so not kept)
    rows = U.null_rows(x, y, xp, None, keep_rows=keep)
    assert {0, 2, 10} <= set(rows.kept.tolist()) and 11 not in rows.kept and 11 in rows.sel
    for i in (0, 2, 10):
        assert rows.x[i] == x[i] and rows.y[i] == y[i]
    assert np.array_equal(rows.y, y)  # y has no nulls: never poisoned
    assert not np.array_equal(rows.x[::2], x[::2])


@pytest.mark.parametrize("n,offs", [(1, (0, 0)), (9, (6, 13)), (257, (64, 1)), (4097, (123, 123)), (12289, (2, 2))])
def test_float64_column_fields(n, offs):
    x_off, y_off = offs
    *_, xp, yp, rows, case = _case(n, x_off, y_off, "both")
    xc, yc = U.columns(case, "cpu")
    for col, off, present, full, vals in ((xc, x_off, xp, case.x_present, case.x), (yc, y_off, yp, case.y_present, case.y)):
        a = col.struct.array
        assert (a.length, a.offset, a.n_buffers) == (n, off, 2)
        assert a.null_count == sum(1 for i in range(n) if not present[i])  # the slice's rows only
        bm = buffer_bytes(col, 0, (len(full) + 7) // 8)
        for r in range(len(full)):
            assert bit(bm, r) == int(full[r])
        assert np.array_equal(np.frombuffer(ctypes.string_at(a.buffers[1], 8 * len(vals)), np.float64), vals, equal_nan=True)
    assert U.classify_kernel(xc, yc) in ("pair", "wave")
    if x_off % 2 or y_off % 2:  # (tensor storage is at least 16-byte aligned)
        assert U.classify_kernel(xc, yc) == "wave"
    # the defaults, and the forced counts
    t = torch.arange(10, dtype=torch.float64)
    a = A.float64_column(t).struct.array
    assert (a.length, a.offset, a.null_count) == (10, 0, 0) and not a.buffers[0]
    a = A.float64_column(t, offset=3).struct.array
    assert (a.length, a.offset, a.null_count) == (7, 3, 0)
    p = np.array([0, 1, 1, 0, 1, 1, 1, 0, 1, 0], bool)
    a = A.float64_column(t, p, offset=3).struct.array
    assert (a.length, a.offset, a.null_count) == (7, 3, 3)
    a = A.float64_column(t, p, offset=1, length=2).struct.array
    assert (a.length, a.offset, a.null_count) == (2, 1, 0) and a.buffers[0]
    a = A.float64_column(t, p, offset=3, length=4, null_count=-1).struct.array
    assert (a.length, a.offset, a.null_count) == (4, 3, -1)
    a = A.float64_column(t, np.zeros(10, bool), null_count=0).struct.array
    assert (a.length, a.offset, a.null_count) == (10, 0, 0) and a.buffers[0]


@pytest.mark.parametrize("large", [False, True])
def test_geometry_column_fields(large):
    rows = ["POINT (%d %d)" % (i, i + 1) for i in range(40)]
    col = M.GeometryColumn.from_rows(rows, "cpu")
    assert col.valid is None and col.valid_offset == 0
    arr, schema = A.geometry_column(col, large)
    a = arr.struct.array
    assert (a.length, a.offset, a.null_count, a.n_buffers) == (40, 0, 0, 3) and schema.format == (b"U" if large else b"u")
    present = np.random.default_rng(3).random(40) >= 0.3
    with_nulls = M.GeometryColumn(col.format, col.data, col.offsets, valid=A.bitmap(present, "cpu"))
    for off, n in ((0, 40), (3, 9), (8, 32), (13, 1), (39, 1), (40, 0)):
        arr, schema = A.geometry_column(with_nulls, large, offset=off, length=n)
        a = arr.struct.array
        assert (a.length, a.offset) == (n, off)
        assert a.null_count == sum(1 for i in range(off, off + n) if not present[i])
        # the buffers are the whole column's: ArrowArray.offset slices
        width = 8 if large else 4
        offs = np.frombuffer(ctypes.string_at(a.buffers[1], width * 41), np.int64 if large else np.int32)
        assert np.array_equal(offs, col.offsets.numpy())
        assert a.buffers[2] == col.data.data_ptr() and a.buffers[0] == with_nulls.valid.data_ptr()
        text = bytes(col.data.numpy())
        for i in range(n):
            assert text[offs[off + i]:offs[off + i + 1]].decode() == rows[off + i]
    arr, _ = A.geometry_column(with_nulls, large, offset=5)
    assert (arr.struct.array.length, arr.struct.array.offset) == (35, 5)
    with pytest.raises(M.IllegalArgumentException):
        A.geometry_column(with_nulls, large, offset=5, length=36)
    sliced = M.GeometryColumn(col.format, col.data, col.offsets[5:], valid=with_nulls.valid, valid_offset=5)
    assert len(sliced) == 35 and sliced.valid_offset == 5
    with pytest.raises(M.IllegalArgumentException):  # one ArrowArray.offset for offsets and bitmap alike
        A.geometry_column(sliced, large)


def test_internal_geometry_column_carries_a_bitmap():
    rows = [(1, [[[(float(i), 2.0)]]]) for i in range(20)]
    ic = M.InternalGeometryColumn.from_rows(rows, "cpu")
    assert ic.valid is None and ic.valid_offset == 0 and len(ic) == 20
    bm = A.bitmap(np.arange(20) % 3 != 0, "cpu")
    s = M.InternalGeometryColumn(ic.type_id[4:13], ic.row_part[4:14], ic.part_ring, ic.ring_off, ic.xy, valid=bm,
                                 valid_offset=4)
    assert len(s) == 9 and s.valid is bm and s.valid_offset == 4
    assert s.row_part.data_ptr() == ic.row_part.data_ptr() + 4 * 8 and s.type_id.data_ptr() == ic.type_id.data_ptr() + 4 * 4

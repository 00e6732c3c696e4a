"""The three entries that produce variable-length lists -- StringType cell ids
(mgpu_format_cells_device), kRing / kLoop (mgpu_grid_kring) and SpatialKNN's ring join
(mgpu_ring_join_ex) -- past one 4096-cell chunk of input: the carries between chunks and
slices, more than 1024 chunk sums (the scans' carry loops), the pentagon fallback in every
chunk and in batches (option kring_batch), rows of different lengths at every byte
alignment, short capacities, distance ties, the Shell sort with a cut, empty sides.

References: the CPU oracle (oracle.py) and plain Python / numpy, compared bit for bit.
Every precondition is asserted from the reference side only.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import jts_centroid as JC
import mosaic_amd as M
import oracle as O
from geom_util import nyc_points
from mosaic_amd import _native as N

pytestmark = pytest.mark.gpu

CHUNK = 4096                      # kFmtChunk: ids per workgroup of the count / write kernels
N_BIG = 1024 * CHUNK + 4097       # more than 1024 chunk sums: scan_sums_kernel's carry loop
SENT = -0x0123456789ABCDEF        # never a cell id (negative)
H3, BNG = M.H3IndexSystem(), M.BNGIndexSystem()


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def TI(a, dev):
    return torch.from_numpy(np.array(a, dtype=np.int64)).to(dev)   # (a copy: the shared columns are read-only)


# ---------------------------------------------------------------- kRing / kLoop: columns and references

@functools.lru_cache(maxsize=None)
def h3_col():
    """12,000 res-1 cells of points uniform on the sphere, duplicates kept, input order
    (842 cells at res 1: every pentagon neighbourhood many times in every chunk)."""
    rng = np.random.default_rng(6)
    lon = rng.uniform(-180, 180, 12_000)
    lat = np.degrees(np.arcsin(rng.uniform(-1, 1, 12_000)))
    c = O.h3_points_to_cells(lon, lat, 1).astype(np.int64)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def bng_col(res):
    """Cells all over the extent (its four corners included) whose kRing(2) the reference
    computes without throwing: more than two chunks of them."""
    rng = np.random.default_rng(500 + abs(res) + (res < 0))
    e = np.concatenate([[0.5, 699_999.0, 350_000.0, 1.0], rng.uniform(0, 700_000, 8_996)])
    nn = np.concatenate([[0.5, 1_299_999.0, 0.5, 1_299_999.0], rng.uniform(0, 1_300_000, 8_996)])
    cells = O.bng_points_to_cells(e, nn, res).astype(np.int64)
    ring2 = {}
    for u in np.unique(cells).tolist():
        try:
            ring2[u] = O.bng_k_ring(u, 2)
        except ValueError:  # the reference throws (NumberFormatException)
            pass
    c = cells[np.isin(cells, np.fromiter(ring2, np.int64, len(ring2)))]
    c.setflags(write=False)
    _BNG_RING2[res] = ring2
    return c


_BNG_RING2 = {}   # res -> {cell: O.bng_k_ring(cell, 2)}, kept from bng_col's filter


@functools.lru_cache(maxsize=None)
def oracle_lists(system, k, loop, res=0):
    """(unique cells, their oracle lists as int64 arrays): one oracle call per unique cell."""
    col = h3_col() if system == "h3" else bng_col(res)
    fn = {("h3", False): O.h3_k_ring, ("h3", True): O.h3_k_loop,
          ("bng", False): O.bng_k_ring, ("bng", True): O.bng_k_loop}[(system, loop)]
    uniq = np.unique(col)
    if (system, k, loop) == ("bng", 2, False):
        fn = lambda c, k: _BNG_RING2[res][c]  # noqa: E731  (computed once, by bng_col)
    return uniq, [np.array(fn(int(c), k), dtype=np.uint64).view(np.int64) for c in uniq]


def expected_lists(system, k, loop, cells, res=0):
    """(ids, offsets) the entry must return for `cells` (rows of the system's column)."""
    uniq, lists = oracle_lists(system, k, loop, res)
    inv = np.searchsorted(uniq, cells)
    assert np.array_equal(uniq[inv], cells)
    lens = np.array([len(v) for v in lists], np.int64)
    off = np.concatenate([[0], np.cumsum(lens[inv])]).astype(np.int64)
    ids = np.concatenate([lists[j] for j in inv] + [np.zeros(0, np.int64)])
    return ids, off


def run_kring(gpu, isys, cells, k, loop):
    ids, off = M.grid_cellkring(TI(cells, gpu), k, isys, loop_only=loop)
    return ids.cpu().numpy(), off.cpu().numpy()


def assert_lists_equal(got, want, tag):
    (gi, go), (wi, wo) = got, want
    assert np.array_equal(go, wo), ("offsets", tag, int(np.argmax(go != wo)) if len(go) == len(wo) else (len(go), len(wo)))
    assert len(gi) == len(wi), ("ids length", tag)
    if not np.array_equal(gi, wi):
        q = int(np.argmax(gi != wi))
        raise AssertionError(("ids", tag, "first difference at id", q, "of cell", int(np.searchsorted(wo, q, "right") - 1)))


@functools.lru_cache(maxsize=None)
def h3_fallback_mask(k):
    """Rows of h3_col() whose cell's hexRing(c, j) throws for some j <= k (the walks that
    meet a pentagon: the device's fallback cells), from the oracle."""
    uniq = np.unique(h3_col())
    bad = np.zeros(len(uniq), bool)
    for q, c in enumerate(uniq):
        for j in range(1, k + 1):
            try:
                O.h3_hex_ring(int(c), j)
            except O.PentagonEncountered:
                bad[q] = True
                break
    return bad[np.searchsorted(uniq, h3_col())]


# ---------------------------------------------------------------- kRing / kLoop across chunks

@pytest.mark.parametrize("loop", [False, True])
@pytest.mark.parametrize("k", [1, 3])
def test_h3_kring_fallbacks_in_every_chunk(gpu, k, loop):
    """Three chunks (12,000 cells), each with at least 150 pentagon-fallback cells: every
    list and every offset == the oracle (chunk_off of blocks 1 and 2, the fallback's
    additions into chunk_tot[1] and [2], fb_idx filled by three workgroups)."""
    col, fb = h3_col(), h3_fallback_mask(k)
    per_chunk = [int(fb[c0:c0 + CHUNK].sum()) for c0 in range(0, len(col), CHUNK)]
    assert len(per_chunk) == 3 and min(per_chunk) >= 150, per_chunk
    assert_lists_equal(run_kring(gpu, H3, col, k, loop), expected_lists("h3", k, loop, col), (k, loop))


@pytest.mark.parametrize("loop", [False, True])
@pytest.mark.parametrize("n", [255, 256, 257, 4095, 4096, 4097, 8192, 8193])
def test_h3_kring_boundary_sizes(gpu, n, loop):
    """Prefixes that end just before, at and just after a slice (256) and a chunk (4096)."""
    col = h3_col()[:n]
    assert_lists_equal(run_kring(gpu, H3, col, 2, loop), expected_lists("h3", 2, loop, col), (n, loop))


@pytest.mark.parametrize("loop", [False, True])
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("res", [3, -3])
def test_bng_kring_across_chunks(gpu, res, k, loop):
    col = bng_col(res)
    assert len(col) > 2 * CHUNK + 1
    ids, off = expected_lists("bng", k, loop, col, res)
    assert len(np.unique(np.diff(off))) > 1   # (the extent's edges: lists of different lengths)
    assert_lists_equal(run_kring(gpu, BNG, col, k, loop), (ids, off), (res, k, loop))


@pytest.mark.parametrize("system", ["h3", "bng"])
def test_kring_bad_ids_across_chunks(gpu, system):
    """Five ids that are no cells, in the first, second and third chunk (at the chunks'
    first and last rows): all five are counted."""
    if system == "h3":
        isys, col, bad = H3, h3_col().copy(), [0, -1, 1051200030000, 12345, 1 << 62]
    else:
        isys, col, bad = BNG, np.resize(bng_col(3), 12_000), [-5, 0, 7, 99, -(1 << 40)]
    col[[0, 4095, 4096, 8191, 11_999]] = bad
    for loop in (False, True):
        with pytest.raises(M.IllegalArgumentException) as ei:
            M.grid_cellkring(TI(col, gpu), 1, isys, loop_only=loop)
        assert str(ei.value).startswith("5 cells"), str(ei.value)


def test_kring_batch_option_range(gpu):
    ctx = M.default_context(gpu)
    assert ctx.get_option("kring_batch") == 0
    for bad in (-1, -(1 << 40), 1 << 31):
        with pytest.raises(M.IllegalArgumentException):
            ctx.set_option("kring_batch", bad)
        assert N.lib().mgpu_ctx_set_option(ctx.handle, b"kring_batch", bad) == N.MGPU_E_INVALID_ARG
    assert ctx.get_option("kring_batch") == 0
    for v in (1, 65, (1 << 31) - 1):
        with ctx.options(kring_batch=v):
            assert ctx.get_option("kring_batch") == v
    assert ctx.get_option("kring_batch") == 0


@pytest.mark.parametrize("loop", [False, True])
@pytest.mark.parametrize("batch,n", [(1000, 12_000), (64, 12_000), (65, 12_000), (1, 4097)])
def test_h3_kring_fallback_batches(gpu, batch, n, loop):
    """The pentagon fallback in many launches (j0 > 0 in kring_fallback_kernel; batches of
    one wave exactly, one wave and a lane, one cell): == the oracle and == the default
    batch's result."""
    col = h3_col()[:n]
    n_fb = int(h3_fallback_mask(3)[:n].sum())
    assert n_fb > 3 * batch and n_fb > 1000, n_fb
    ctx = M.default_context(gpu)
    default = run_kring(gpu, H3, col, 3, loop)
    with ctx.options(kring_batch=batch):
        got = run_kring(gpu, H3, col, 3, loop)
    assert ctx.get_option("kring_batch") == 0
    assert_lists_equal(got, expected_lists("h3", 3, loop, col), (batch, loop))
    assert_lists_equal(got, default, ("default", batch, loop))


@pytest.mark.parametrize("system,loop", [("h3", False), ("h3", True), ("bng", False)])
def test_kring_k0_more_than_1024_chunks(gpu, system, loop):
    """k = 0 over 1024 * 4096 + 4097 cells: every list is the cell itself, so the ids are
    the column and the offsets 0 .. n (1026 chunk sums: the scan's second round and its
    carry)."""
    col = h3_col() if system == "h3" else bng_col(3)
    cells = TI(np.tile(col, N_BIG // len(col) + 1)[:N_BIG], gpu)
    ids, off = M.grid_cellkring(cells, 0, H3 if system == "h3" else BNG, loop_only=loop)
    assert off.numel() == N_BIG + 1 and ids.numel() == N_BIG
    assert bool(torch.equal(off, torch.arange(N_BIG + 1, dtype=torch.int64, device=gpu)))
    assert bool(torch.equal(ids, cells))


def test_h3_kloop_more_than_1024_chunks(gpu):
    """k = 1 loops (pentagon fallbacks in every chunk) over 1026 chunks: all offsets == the
    cumulative oracle lengths; the ids of the first and the last 5000 cells == the oracle."""
    col = h3_col()
    uniq, lists = oracle_lists("h3", 1, True)
    lens = np.array([len(v) for v in lists], np.int64)
    reps = N_BIG // len(col) + 1
    want_off = np.concatenate([[0], np.cumsum(np.tile(lens[np.searchsorted(uniq, col)], reps)[:N_BIG])])
    cells = np.tile(col, reps)[:N_BIG]
    ids, off = M.grid_cellkring(TI(cells, gpu), 1, H3, loop_only=True)
    assert bool(torch.equal(off, torch.from_numpy(want_off).to(gpu)))
    assert ids.numel() == want_off[-1]
    head = ids[:int(want_off[5000])].cpu().numpy()
    tail = ids[int(want_off[N_BIG - 5000]):].cpu().numpy()
    assert np.array_equal(head, expected_lists("h3", 1, True, cells[:5000])[0])
    assert np.array_equal(tail, expected_lists("h3", 1, True, cells[N_BIG - 5000:])[0])


def raw_kring(gpu, isys, cells, k, loop, out, capacity, off):
    tot = ctypes.c_int64(-1)
    st = N.lib().mgpu_grid_kring(M.default_context(gpu).handle, isys.code, cells.data_ptr(), cells.numel(), k,
                                 1 if loop else 0, None if out is None else out.data_ptr(), capacity, off.data_ptr(),
                                 ctypes.byref(tot), torch.cuda.current_stream(gpu).cuda_stream)
    return st, tot.value


@pytest.mark.parametrize("system,k,loop", [("h3", 3, False), ("h3", 3, True), ("bng", 2, False)])
def test_kring_short_capacity(gpu, system, k, loop):
    """mgpu_grid_kring with half the capacity: MGPU_E_CAPACITY, the exact total, complete
    offsets, every list that fits == the oracle, nothing written at or past `capacity`;
    the sizing call (capacity 0, no output array) reports the same total."""
    isys, col = (H3, h3_col()) if system == "h3" else (BNG, bng_col(3))
    want_ids, want_off = expected_lists(system, k, loop, col, 0 if system == "h3" else 3)
    total = int(want_off[-1])
    cap = total // 2
    fit = int(np.searchsorted(want_off, cap, "right")) - 1   # lists 0 .. fit - 1 end at or before cap
    assert CHUNK < fit < len(col) - CHUNK and 0 < want_off[fit] <= cap   # (the cut: inside the second chunk)
    if system == "h3":
        fb = h3_fallback_mask(k)
        assert fb[:fit].sum() > 100 and fb[fit:].sum() > 100   # fallback lists on both sides of the cut
    cells = TI(col, gpu)
    out = torch.full((total + 4096,), SENT, dtype=torch.int64, device=gpu)
    off = torch.full((len(col) + 1,), SENT, dtype=torch.int64, device=gpu)
    st, tot = raw_kring(gpu, isys, cells, k, loop, out, cap, off)
    assert st == N.MGPU_E_CAPACITY and tot == total
    assert np.array_equal(off.cpu().numpy(), want_off)
    got = out.cpu().numpy()
    assert np.array_equal(got[:want_off[fit]], want_ids[:want_off[fit]])
    assert (got[cap:] == SENT).all()
    off.fill_(SENT)
    st, tot = raw_kring(gpu, isys, cells, k, loop, None, 0, off)
    assert st == N.MGPU_E_CAPACITY and tot == total
    assert np.array_equal(off.cpu().numpy(), want_off)
    st, tot = raw_kring(gpu, isys, cells, k, loop, out, total, off)   # the exact capacity fits
    assert st == N.MGPU_OK and tot == total
    got = out.cpu().numpy()
    assert np.array_equal(got[:total], want_ids) and (got[total:] == SENT).all()


# ---------------------------------------------------------------- string ids

@functools.lru_cache(maxsize=None)
def hex_col():
    """20,000 int64 whose top set bit is uniform over 0 .. 63 (hex lengths 1 .. 16), with
    0, -1, INT64_MIN and small values first; (values, their Long.toHexString)."""
    rng = np.random.default_rng(64)
    top = rng.integers(0, 64, 20_000)
    low = rng.integers(0, 1 << 63, 20_000, dtype=np.uint64)
    v = (np.uint64(1) << top.astype(np.uint64)) | (low & ((np.uint64(1) << top.astype(np.uint64)) - np.uint64(1)))
    v = v.view(np.int64).copy()
    v[:12] = [0, -1, -(1 << 63), 1, 2, 9, 10, 15, 16, 255, 256, (1 << 63) - 1]
    strs = ["%x" % (int(x) & (2 ** 64 - 1)) for x in v]
    assert {len(s) for s in strs} == set(range(1, 17))
    v.setflags(write=False)
    return v, strs


@functools.lru_cache(maxsize=None)
def bng_mixed_col():
    """20,000 BNG cells, the 12 resolutions interleaved row by row; (cells, format_many)."""
    rng = np.random.default_rng(65)
    e, nn = rng.uniform(0, 700_000, 20_000), rng.uniform(0, 1_300_000, 20_000)
    cells = np.zeros(20_000, np.int64)
    for q, res in enumerate((1, 2, 3, 4, 5, 6, -1, -2, -3, -4, -5, -6)):
        cells[q::12] = O.bng_points_to_cells(e[q::12], nn[q::12], res)
    strs = BNG.format_many(cells)
    assert len({len(s) for s in strs}) >= 6
    cells.setflags(write=False)
    return cells, strs


def expected_strings(strs):
    off = np.concatenate([[0], np.cumsum([len(s) for s in strs])]).astype(np.int64)
    return np.frombuffer("".join(strs).encode(), np.uint8), off


def assert_strings_equal(gpu, isys, cells, strs, tag):
    chars, off = isys.format_device(TI(cells, gpu))
    want_c, want_o = expected_strings(strs)
    go, gc = off.cpu().numpy(), chars.cpu().numpy()
    assert np.array_equal(go, want_o), ("offsets", tag)
    assert len(gc) == len(want_c), ("length", tag)
    if not np.array_equal(gc, want_c):
        q = int(np.argmax(gc != want_c))
        raise AssertionError(("chars", tag, "first difference at byte", q, "of row", int(np.searchsorted(want_o, q, "right") - 1)))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4095, 4096, 4097, 20_000])
def test_h3_hex_of_arbitrary_int64(gpu, n):
    """H3 string ids of arbitrary int64 (Long.toHexString: 1 to 16 characters), rows of
    every length starting at every byte alignment: every character and offset."""
    v, strs = hex_col()
    assert_strings_equal(gpu, H3, v[:n], strs[:n], n)


def test_bng_strings_mixed_resolutions(gpu):
    cells, strs = bng_mixed_col()
    assert_strings_equal(gpu, BNG, cells, strs, "bng mixed")


def test_bng_strings_bad_ids_across_chunks(gpu):
    cells = bng_mixed_col()[0].copy()
    cells[[0, 4096, len(cells) - 1]] = [-5, 0, -(1 << 40)]
    with pytest.raises(M.IllegalArgumentException) as ei:
        BNG.format_device(TI(cells, gpu))
    assert "3 BNG cell ids" in str(ei.value)


def test_h3_strings_more_than_1024_chunks(gpu):
    """The mixed-length column tiled to 1024 * 4096 + 4097 rows: all offsets == the
    cumulative reference lengths, all characters == the block's characters tiled."""
    v, strs = hex_col()
    reps, rem = divmod(N_BIG, len(v))
    lens = np.array([len(s) for s in strs], np.int64)
    want_off = np.concatenate([[0], np.cumsum(np.tile(lens, reps + 1)[:N_BIG])])
    block, _ = expected_strings(strs)
    want_chars = np.concatenate([np.tile(block, reps), block[:lens[:rem].sum()]])
    chars, off = H3.format_device(TI(np.tile(v, reps + 1)[:N_BIG], gpu))
    assert bool(torch.equal(off, torch.from_numpy(want_off).to(gpu)))
    assert chars.numel() == len(want_chars)
    assert bool(torch.equal(chars, torch.from_numpy(want_chars).to(gpu)))


@pytest.mark.parametrize("system", ["h3", "bng"])
def test_strings_short_out_bytes(gpu, system):
    """mgpu_format_cells_device with out_bytes short by one, by half, at 3 and at 0:
    MGPU_E_CAPACITY, the exact total, the reference's prefix in [0, out_bytes), nothing
    written at or past out_bytes, complete offsets."""
    isys, (cells, strs) = (H3, hex_col()) if system == "h3" else (BNG, bng_mixed_col())
    want_c, want_o = expected_strings(strs)
    total = len(want_c)
    dc = TI(cells, gpu)
    for out_bytes in (total - 1, total // 2 + 1, 3, 0, total):
        out = torch.full((total + 64,), 0xEE, dtype=torch.uint8, device=gpu)
        off = torch.full((len(cells) + 1,), SENT, dtype=torch.int64, device=gpu)
        tot = ctypes.c_int64(-1)
        st = N.lib().mgpu_format_cells_device(M.default_context(gpu).handle, isys.code, dc.data_ptr(), len(cells),
                                              out.data_ptr(), out_bytes, off.data_ptr(), ctypes.byref(tot),
                                              torch.cuda.current_stream(gpu).cuda_stream)
        assert st == (N.MGPU_OK if out_bytes == total else N.MGPU_E_CAPACITY), out_bytes
        assert tot.value == total, out_bytes
        got = out.cpu().numpy()
        assert np.array_equal(got[:out_bytes], want_c[:out_bytes]), out_bytes
        assert (got[out_bytes:] == 0xEE).all(), out_bytes
        assert np.array_equal(off.cpu().numpy(), want_o), out_bytes


# ---------------------------------------------------------------- ring join

def run_join(gpu, lx, ly, rx, ry, res, k, **kw):
    got = M.grid_ring_join(T(lx, gpu), T(ly, gpu), T(rx, gpu), T(ry, gpu), res, k, **kw)
    return tuple(v.cpu().numpy() for v in got)


def assert_rows_equal(got, want, tag):
    (gl, gr, gd), (ol, orr, od) = got, want
    assert len(gl) == len(ol), (tag, len(gl), len(ol))
    assert np.array_equal(gl, ol), tag
    assert np.array_equal(gr, orr), (tag, int(np.argmax(gr != orr)))
    assert np.array_equal(gd.view(np.int64), od.view(np.int64)), tag


@functools.lru_cache(maxsize=None)
def shell_inputs():
    lx, ly = nyc_points(300, 81)
    rx, ry = nyc_points(30_000, 82)
    full = O.ring_join(0, 8, 1, lx, ly, rx, ry)
    return lx, ly, rx, ry, np.bincount(full[0], minlength=300)


@pytest.mark.parametrize("left_outer", [False, True])
@pytest.mark.parametrize("keep", [33, 40, 64])
def test_ring_join_shell_sort_then_cut(gpu, keep, left_outer):
    """max_per_left above 32 and below the segment length: the whole segment Shell-sorted,
    then cut (at most 32 is the selection path)."""
    lx, ly, rx, ry, per = shell_inputs()
    assert (per > 64).sum() >= 100, int((per > 64).sum())
    want = O.ring_join(0, 8, 1, lx, ly, rx, ry, max_per_left=keep, left_outer=left_outer)
    got = run_join(gpu, lx, ly, rx, ry, 8, 1, index_system=H3, max_per_left=keep, left_outer=left_outer)
    assert_rows_equal(got, want, (keep, left_outer))


OFFSETS_5 = [(3, 4), (3, -4), (-3, 4), (-3, -4), (4, 3), (4, -3), (-4, 3), (-4, -3), (5, 0), (-5, 0), (0, 5), (0, -5)]


@functools.lru_cache(maxsize=None)
def tie_inputs():
    """400 landmarks at integer coordinates inside London; around each, candidates at the
    12 lattice offsets of length exactly 5, three of them twice more (identical
    coordinates), and the same 12 offsets doubled (length exactly 10) four times each, so
    that a cut at 40 falls inside a tie group too; 2000 random candidates; shuffled."""
    rng = np.random.default_rng(55)
    lx = rng.integers(505_000, 559_000, 400).astype(np.float64)
    ly = rng.integers(157_000, 199_000, 400).astype(np.float64)
    offs = OFFSETS_5 + 2 * [OFFSETS_5[1], OFFSETS_5[6], OFFSETS_5[8]] + 4 * [(2 * a, 2 * b) for a, b in OFFSETS_5]
    dx, dy = np.array(offs, np.float64).T
    rx = np.concatenate([(lx[:, None] + dx[None, :]).ravel(), rng.uniform(503_000, 561_000, 2000)])
    ry = np.concatenate([(ly[:, None] + dy[None, :]).ravel(), rng.uniform(155_000, 201_000, 2000)])
    p = np.random.default_rng(56).permutation(len(rx))
    rx, ry = rx[p], ry[p]
    full = O.ring_join(1, 3, 1, lx, ly, rx, ry)
    return lx, ly, rx, ry, full


@pytest.mark.parametrize("keep", [0, 5, 13, 40])
def test_ring_join_ties_and_duplicates(gpu, keep):
    """Exact distance ties and duplicate candidates: the order inside a tie is the
    candidate index, on the selection path (5, 13: the cut inside the 18 pairs at distance
    5), the Shell sort (0) and the Shell sort with the cut inside the pairs at distance 10
    (40)."""
    lx, ly, rx, ry, (fl, fr, fd) = tie_inputs()
    assert JC.hypot(3.0, 4.0) == 5.0 and JC.hypot(-8.0, 6.0) == 10.0
    for i in range(len(lx)):
        d = fd[fl == i]
        assert (d == 5.0).sum() >= 18 and (d[:18] == 5.0).all(), i
        assert d[4] == d[5] and d[12] == d[13] and d[39] == d[40] == 10.0, i
    want = O.ring_join(1, 3, 1, lx, ly, rx, ry, max_per_left=keep)
    got = run_join(gpu, lx, ly, rx, ry, 3, 1, index_system=BNG, max_per_left=keep)
    assert_rows_equal(got, want, keep)


QNAN = np.array([0x7FF8000000000000], np.int64)


@pytest.mark.parametrize("system", ["h3", "bng"])
def test_ring_join_empty_sides(gpu, system):
    """No candidates: no rows, or with left_outer exactly one (left, -1, NaN) row per
    landmark in landmark order; no landmarks: no rows."""
    if system == "h3":
        isys, res, (lx, ly) = H3, 9, nyc_points(700, 83)
    else:
        rng = np.random.default_rng(84)
        isys, res, lx, ly = BNG, 3, rng.uniform(520_000, 540_000, 700), rng.uniform(170_000, 190_000, 700)
    none = np.zeros(0)
    for k, loop in ((1, False), (2, True)):
        gl, gr, gd = run_join(gpu, lx, ly, none, none, res, k, index_system=isys, loop_only=loop, left_id_base=11)
        assert len(gl) == len(gr) == len(gd) == 0
        gl, gr, gd = run_join(gpu, lx, ly, none, none, res, k, index_system=isys, loop_only=loop, left_id_base=11,
                              left_outer=True, max_per_left=3)
        assert np.array_equal(gl, 11 + np.arange(len(lx))) and (gr == -1).all() and len(gr) == len(lx)
        assert (gd.view(np.int64) == QNAN[0]).all()
        for lo in (False, True):
            got = run_join(gpu, none, none, lx, ly, res, k, index_system=isys, loop_only=loop, left_outer=lo)
            assert all(len(v) == 0 for v in got)


@pytest.mark.parametrize("loop", [False, True])
@pytest.mark.parametrize("system", ["h3", "bng"])
def test_ring_join_k0(gpu, system, loop):
    """k = 0: kRing(c, 0) = [c]; kLoop(c, 0) is H3's hexRing(c, 0) = [c] and BNG's empty
    loop (no cells: no rows at all) == the oracle, left_outer on and off."""
    if system == "h3":
        isys, code, res, (lx, ly), (rx, ry) = H3, 0, 9, nyc_points(2000, 85), nyc_points(6000, 86)
    else:
        rng = np.random.default_rng(87)
        isys, code, res = BNG, 1, 3
        lx, ly = rng.uniform(520_000, 540_000, 2000), rng.uniform(170_000, 190_000, 2000)
        rx, ry = rng.uniform(518_000, 542_000, 900), rng.uniform(168_000, 192_000, 900)
    for lo in (False, True):
        want = O.ring_join(code, res, 0, lx, ly, rx, ry, loop_only=loop, left_outer=lo)
        if not (system == "bng" and loop):
            assert (want[1] >= 0).sum() > 200 and (not lo or (want[1] == -1).sum() > 200)
        else:
            assert len(want[0]) == 0
        got = run_join(gpu, lx, ly, rx, ry, res, 0, index_system=isys, loop_only=loop, left_outer=lo)
        assert_rows_equal(got, want, (system, loop, lo))


@functools.lru_cache(maxsize=None)
def big_join():
    """1024 * 1024 + 1500 landmarks x 300 candidates, BNG res 3, k = 0, restated in numpy:
    a landmark pairs with the candidates of its own cell, ordered by (distance, index); a
    landmark whose cell holds no candidate has a null row.  Returns the inputs, the pairs
    (left, right, distance) in output order and the null-row flags."""
    rng = np.random.default_rng(3)
    n_left = 1024 * 1024 + 1500
    lx, ly = rng.uniform(500_000, 540_000, n_left), rng.uniform(160_000, 200_000, n_left)
    rx, ry = rng.uniform(500_000, 540_000, 300), rng.uniform(160_000, 200_000, 300)
    lc, rc = O.bng_points_to_cells(lx, ly, 3), O.bng_points_to_cells(rx, ry, 3)
    order = np.argsort(rc, kind="stable")
    src = rc[order]
    lo, hi = np.searchsorted(src, lc, "left"), np.searchsorted(src, lc, "right")
    cnt = hi - lo
    left = np.repeat(np.arange(n_left), cnt)
    right = order[np.repeat(lo, cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))]
    same = (lx[left].view(np.int64) == rx[right].view(np.int64)) & (ly[left].view(np.int64) == ry[right].view(np.int64))
    assert not same.any()   # (no self matches to drop)
    dist = np.array([JC.hypot(float(a), float(b)) for a, b in zip(lx[left] - rx[right], ly[left] - ry[right])])
    o = np.lexsort((right, dist, left))
    return lx, ly, rx, ry, left[o], right[o].astype(np.int64), dist[o], cnt == 0


@pytest.mark.parametrize("left_outer", [False, True])
def test_ring_join_more_than_1024_scan_blocks(gpu, left_outer):
    """More than 1024 * 1024 landmarks: rj_scan_sums_kernel's second round and its carry;
    all rows == the numpy restatement."""
    lx, ly, rx, ry, pl, pr, pd, null = big_join()
    assert len(pl) > 150_000 and null.sum() > 800_000
    if left_outer:
        nl = np.nonzero(null)[0]
        rank = np.concatenate([np.zeros(len(nl), np.int8), np.ones(len(pl), np.int8)])
        wl = np.concatenate([nl, pl])
        o = np.lexsort((np.arange(len(wl)), rank, wl))   # per landmark: the null row, then its pairs in order
        wl = wl[o]
        wr = np.concatenate([np.full(len(nl), -1, np.int64), pr])[o]
        wd = np.concatenate([np.full(len(nl), np.nan), pd]).view(np.int64)
        wd[:len(nl)] = QNAN[0]
        wd = wd[o].view(np.float64)
    else:
        wl, wr, wd = pl, pr, pd
    got = M.grid_ring_join(T(lx, gpu), T(ly, gpu), T(rx, gpu), T(ry, gpu), 3, 0, index_system=BNG,
                           left_outer=left_outer)
    for g, w, what in zip(got, (wl, wr, wd.view(np.int64)), ("left", "right", "distance")):
        g = g.view(torch.int64) if what == "distance" else g
        assert g.numel() == len(w), what
        assert bool(torch.equal(g, torch.from_numpy(np.ascontiguousarray(w)).to(gpu))), what

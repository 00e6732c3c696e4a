"""Inputs and expectations of the null / sliced-column tests (test_gpu_nulls.py, checked
themselves on CPU tensors by test_nulls_host.py).

A join case is built in two steps.  null_rows() takes the logical rows (x, y and one
validity pattern per column) and overwrites the null slots with payloads a kernel must
never look at -- Arrow leaves a null slot's bytes undefined.  embed() then places each
column in a longer array at its own offset; the rows before and after the slice hold
points known to lie in a polygon, with their validity bits set, so a kernel that mis-bases
the data or the bitmap, or runs past the slice's end, produces pairs the oracle lacks.
"""
import types

import numpy as np

KEEP = "keep"  # a null slot that keeps its (in-range, often in-polygon) coordinates
PAYLOADS = (np.nan, np.inf, 1e300, KEEP)
BNG_PAYLOADS = (np.nan, -250000.5, np.inf, 1e300, KEEP)
PATTERNS = ("random30", "even_null", "odd_null", "runs64", "runs4096", "all_null", "all_valid")
HEAD = 128  # the fill rows kept for the columns' heads (>= every offset used); tails come after
TAIL = 77   # rows after the slice (odd: the arrays end off every unit)


def present_pattern(name, n, seed=0):
    """bool[n], True = present.  runs4096: rows [4096, 8192), [12288, ...) ... are null --
    whole chunks of the split pipeline (4096 points each, counted from the slice's start)."""
    i = np.arange(n)
    if name == "random30":
        return np.random.default_rng(seed).random(n) >= 0.3
    if name == "even_null":
        return (i & 1) == 1
    if name == "odd_null":
        return (i & 1) == 0
    if name == "runs64":
        return ((i >> 6) & 1) == 0
    if name == "runs4096":
        return ((i >> 12) & 1) == 0
    if name == "all_null":
        return np.zeros(n, bool)
    if name == "all_valid":
        return np.ones(n, bool)
    raise ValueError(name)


def null_rows(x, y, x_present, y_present, payloads=PAYLOADS, keep_rows=()):
    """The logical rows with their null slots poisoned.  x_present / y_present: bool[n], or
    None for a column without a bitmap.  The null rows (either bit 0) take the payloads in
    turn; a payload goes into the slot of each column that is null there, KEEP leaves the
    row as it is.  keep_rows: null rows that keep their coordinates whatever their turn.
    -> namespace: x, y (poisoned), x_present, y_present, both, sel (the valid rows) and
    kept (the null rows that kept their coordinates)."""
    n = len(x)
    xp = np.ones(n, bool) if x_present is None else np.asarray(x_present, bool)
    yp = np.ones(n, bool) if y_present is None else np.asarray(y_present, bool)
    both = xp & yp
    nulls = np.nonzero(~both)[0]
    turn = np.arange(len(nulls)) % len(payloads)
    forced = np.isin(nulls, np.asarray(keep_rows, np.int64))
    lx = np.array(x, np.float64)
    ly = np.array(y, np.float64)
    kept = [nulls[forced]]
    for k, pay in enumerate(payloads):
        rows = nulls[(turn == k) & ~forced]
        if isinstance(pay, str):
            kept.append(rows)
            continue
        lx[rows[~xp[rows]]] = pay
        ly[rows[~yp[rows]]] = pay
    return types.SimpleNamespace(n=n, x=lx, y=ly, x_present=x_present, y_present=y_present, both=both,
                                 sel=np.nonzero(both)[0], kept=np.sort(np.concatenate(kept)))


def embed(rows, x_off, y_off, fill_x, fill_y, tail=TAIL):
    """Place the logical rows at x_off / y_off of longer arrays.  fill_x / fill_y: points
    inside a polygon, at least HEAD + tail of them; a column's head is the first `offset`
    of them, both tails are the same `tail` points.  The bits outside the slice are 1.
    -> namespace: x, y (float64 arrays), x_present, y_present (bool arrays of the same
    lengths, or None), x_off, y_off, n."""
    assert max(x_off, y_off) <= HEAD and len(fill_x) >= HEAD + tail and len(fill_y) >= HEAD + tail

    def col(v, off, fill, present):
        full = np.concatenate([fill[:off], v, fill[HEAD:HEAD + tail]])
        if present is None:
            return full, None
        return full, np.concatenate([np.ones(off, bool), np.asarray(present, bool), np.ones(tail, bool)])

    xf, xpf = col(rows.x, x_off, fill_x, rows.x_present)
    yf, ypf = col(rows.y, y_off, fill_y, rows.y_present)
    return types.SimpleNamespace(x=xf, y=yf, x_present=xpf, y_present=ypf, x_off=x_off, y_off=y_off, n=rows.n)


def expected_bitmap(present, offset, n):
    """The bitmap a call over rows [offset, offset + n) of `present` returns: bit i of the
    result is row offset + i; the bits at or above n in the last byte are 0."""
    return np.packbits(np.asarray(present, bool)[offset:offset + n], bitorder="little")


def columns(case, device, x_null_count=None, y_null_count=None):
    """The embedded case as two Arrow float64 columns on `device` -> (x column, y column)."""
    import torch
    from mosaic_amd import arrow as A
    xt = torch.from_numpy(np.ascontiguousarray(case.x)).to(device)
    yt = torch.from_numpy(np.ascontiguousarray(case.y)).to(device)
    return (A.float64_column(xt, case.x_present, offset=case.x_off, length=case.n, null_count=x_null_count),
            A.float64_column(yt, case.y_present, offset=case.y_off, length=case.n, null_count=y_null_count))


def classify_kernel(x_col, y_col):
    """Which classify kernel the split pipeline takes for these columns: the one reading
    two points per lane needs the first x and the first y of the slice 16-byte aligned
    (kernels.hip launch_split_t)."""
    ax, ay = x_col.struct.array, y_col.struct.array
    px = x_col._keep[-1].data_ptr() + 8 * ax.offset
    py = y_col._keep[-1].data_ptr() + 8 * ay.offset
    return "pair" if ((px | py) & 15) == 0 else "wave"

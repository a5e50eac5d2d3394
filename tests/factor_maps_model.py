"""TEST INFRASTRUCTURE: the exact integer model of the strand-bias grid and the space-scale histogram -- the yardstick
for the device kernels (nolzss_amd/csrc/factor_maps.hip), written independently of them.

Strand grid: with unit D = x_bins * y_bins and t = (x - start) * D every crossing of a cell edge is an integer t; a
cell holds the total t-length of the parts of its strand's segments inside it (Python integers: no width limit).
`exact_grid` is the general form (breakpoints collected and sorted, the cell of a part found from twice its midpoint);
`exact_grid_fast` takes the factors whose two ends lie in one cell with numpy int64 / object arithmetic and hands the
rest to the general form, so that 10^7 factors take seconds.  Histogram: numpy.histogram2d itself.
"""
import numpy as np

RC_MASK = 1 << 63


def kept_factors(records, min_factor_length=1, sentinel_indices=()):
    """records: (z, 3) uint64-like (start, length, raw ref) -> [(start, length, ref, is_rc)] arrays of the kept ones"""
    rec = np.asarray(records, dtype=np.uint64).reshape(-1, 3)
    keep = rec[:, 1] >= np.uint64(max(int(min_factor_length), 0))
    if len(sentinel_indices):
        keep[np.asarray(list(sentinel_indices), dtype=np.int64)] = True
    rec = rec[keep]
    is_rc = (rec[:, 2] >> np.uint64(63)).astype(bool)
    ref = rec[:, 2] & np.uint64(RC_MASK - 1)
    return rec[:, 0], rec[:, 1], ref, is_rc


def extents(s, l, r, total_length=None):
    if total_length is not None:
        return int(total_length), int(total_length)
    return max(int(a) + int(b) for a, b in zip(s.tolist(), l.tolist())), \
        max(int(a) + int(b) for a, b in zip(r.tolist(), l.tolist()))


def _add_general(fw, rc, s, l, r, is_rc, xb, yb, xmax, ymax):
    D = xb * yb
    bps = {0, l * D}
    k = (s * xb) // xmax
    while True:
        t = k * xmax * yb - s * D
        if t >= l * D or k > xb:
            break
        if t > 0:
            bps.add(t)
        k += 1
    step = ymax * xb                             # y edges j * ymax / yb: those strictly inside (r, r + l)
    j = (r * D) // step + 1
    while j <= yb and j * step < (r + l) * D:
        bps.add((r + l) * D - j * step if is_rc else j * step - r * D)
        j += 1
    bl = sorted(bps)
    for a, b in zip(bl[:-1], bl[1:]):
        m2 = a + b
        xi = ((2 * s * D + m2) * xb) // (2 * D * xmax)
        yn = 2 * (r + l) * D - m2 if is_rc else 2 * r * D + m2
        yi = (yn * yb) // (2 * D * ymax)
        if 0 <= xi < xb and 0 <= yi < yb:
            cell = (yi, xi)
            g = rc if is_rc else fw
            g[cell] = g.get(cell, 0) + (b - a)


def exact_grid(factors, xb, yb, total_length=None):
    """factors: iterable of (start, length, ref, is_rc) Python ints -> (forward dict, rc dict, unit): sparse
    {(yi, xi): units}"""
    factors = list(factors)
    xmax = total_length if total_length is not None else max(s + l for s, l, *_ in factors)
    ymax = total_length if total_length is not None else max(r + l for _, l, r, *_ in factors)
    fw, rc = {}, {}
    for s, l, r, is_rc in factors:
        _add_general(fw, rc, int(s), int(l), int(r), bool(is_rc), xb, yb, xmax, ymax)
    return fw, rc, xb * yb


def dense(sparse, xb, yb):
    out = np.zeros((yb, xb), dtype=np.uint64)
    for (yi, xi), v in sparse.items():
        out[yi, xi] = v
    return out


def exact_grid_fast(s, l, r, is_rc, xb, yb, total_length=None):
    """arrays of the kept factors -> (forward_units, rc_units) dense uint64 (yb, xb).  Coordinates below 2^40."""
    xmax, ymax = extents(s, l, r, total_length)
    D = xb * yb
    s64, l64, r64 = (np.asarray(a).astype(np.int64) for a in (s, l, r))
    is_rc = np.asarray(is_rc, dtype=bool)
    # nothing of a factor with start >= x_max or ref >= y_max is inside the extents (either strand: y > ref)
    pos = (l64 > 0) & (s64 < xmax) & (r64 < ymax)
    # single cell: first and last base of the segment in the same column and the same row, inside the extents
    x0 = (s64 * xb) // xmax
    x1 = ((s64 + l64) * xb - 1) // xmax          # column of the last point before the end: ceil(e * xb / xmax) - 1
    # rows that the open y interval (r, r + l) meets, on either strand: floor(r * yb / ymax) .. ceil(.) - 1
    yf0, yf1 = (r64 * yb) // ymax, ((r64 + l64) * yb - 1) // ymax
    single = pos & (x0 == x1) & (yf0 == yf1) & (x1 < xb) & (yf1 < yb)
    fw = np.zeros(xb * yb, dtype=np.uint64)
    rc = np.zeros(xb * yb, dtype=np.uint64)
    cell = yf0 * xb + x0
    for grid, sel in ((fw, single & ~is_rc), (rc, single & is_rc)):
        if sel.any():
            # per-cell sums of lengths stay below 2^53 per bincount weight only if done in integers: use add.at
            np.add.at(grid, cell[sel], l64[sel].astype(np.uint64))
    fw *= np.uint64(D)
    rc *= np.uint64(D)
    fws, rcs = {}, {}
    rest = np.flatnonzero(pos & ~single)
    for i in rest.tolist():
        _add_general(fws, rcs, int(s64[i]), int(l64[i]), int(r64[i]), bool(is_rc[i]), xb, yb, xmax, ymax)
    fw = fw.reshape(yb, xb)
    rc = rc.reshape(yb, xb)
    for sparse, grid in ((fws, fw), (rcs, rc)):
        for (yi, xi), v in sparse.items():
            grid[yi, xi] += np.uint64(v)
    return fw, rc, xmax, ymax


def units_to_float(units, unit):
    units = np.asarray(units, dtype=np.uint64)
    return (units // np.uint64(unit)).astype(np.float64) + (units % np.uint64(unit)).astype(np.float64) / float(unit)


def histogram(s, l, is_rc, length_edges, position_edges):
    """numpy.histogram2d(lengths, starts) per strand as uint64 counts [length_bin][position_bin]"""
    out = []
    for sel in (~is_rc, is_rc):
        h, _, _ = np.histogram2d(np.asarray(l)[sel].astype(np.float64), np.asarray(s)[sel].astype(np.float64),
                                 bins=[np.asarray(length_edges, dtype=np.float64),
                                       np.asarray(position_edges, dtype=np.float64)])
        out.append(h.astype(np.uint64))
    return out

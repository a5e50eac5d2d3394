"""The self dot-plot rasters as their definition states them, base pair by base pair, in numpy -- the model the
device rasteriser (nolzss_amd/csrc/dotplot.hip) is compared with.  Nothing here walks pixel columns or clips
segments: every base pair of every kept factor is enumerated.

Kept: length >= min_factor_length or a sentinel factor (by factor index), and len_lo <= length <= len_hi (len_hi = 0:
no upper bound).  Base pair t of (start, length, ref) lies at x = start + t, y = ref + t (forward) or
ref + length - 1 - t (reverse complement); in view when x in [x_lo, x_hi) and y in [y_lo, y_hi); its pixel is
px = (x - x_lo) * W // (x_hi - x_lo), py = (y - y_lo) * H // (y_hi - y_lo).
"""
import numpy as np

RC_BIT = np.uint64(1 << 63)
BATCH_BASE_PAIRS = 1 << 22


def split(recs):
    recs = np.asarray(recs, dtype=np.uint64).reshape(-1, 3)
    is_rc = (recs[:, 2] & RC_BIT) != 0
    return (recs[:, 0].astype(np.int64), recs[:, 1].astype(np.int64), (recs[:, 2] & ~RC_BIT).astype(np.int64), is_rc)


def kept_mask(length, min_factor_length=1, sentinels=(), length_range=None):
    keep = length >= min_factor_length
    sent = np.asarray(sorted(sentinels), dtype=np.int64)
    keep[sent[sent < len(length)]] = True
    lo, hi = (0, 0) if length_range is None else length_range
    keep &= length >= lo
    if hi:
        keep &= length <= hi
    return keep


def render(recs, x_range, y_range, width, height, min_factor_length=1, sentinels=(), length_range=None, hover_bins=0,
           counts=False):
    """-> dict with the keys of DotPlot.render: max_forward, max_rc, count_forward, count_rc (None without counts),
    visible_forward, visible_rc, hover_start, hover_length, hover_ref (None without hover_bins)"""
    start, length, ref, is_rc = split(recs)
    (x_lo, x_hi), (y_lo, y_hi) = x_range, y_range
    W, H = width, height
    assert x_hi - x_lo >= W >= 1 and y_hi - y_lo >= H >= 1
    keep = kept_mask(length, min_factor_length, sentinels, length_range)
    maxp = np.zeros((2, H * W), dtype=np.uint32)
    cnt = np.zeros((2, H * W), dtype=np.uint32)
    visible = np.zeros(len(start), dtype=bool)
    ids = np.flatnonzero(keep & (length > 0))
    at = 0
    while at < len(ids):
        # a batch of whole factors of about BATCH_BASE_PAIRS base pairs
        csum = np.cumsum(length[ids[at:]])
        take = max(1, int(np.searchsorted(csum, BATCH_BASE_PAIRS, side="right")))
        b = ids[at:at + take]
        at += take
        owner = np.repeat(b, length[b])
        t = np.arange(len(owner), dtype=np.int64) - np.repeat(np.cumsum(length[b]) - length[b], length[b])
        x = start[owner] + t
        y = np.where(is_rc[owner], ref[owner] + length[owner] - 1 - t, ref[owner] + t)
        inside = (x >= x_lo) & (x < x_hi) & (y >= y_lo) & (y < y_hi)
        owner, x, y = owner[inside], x[inside], y[inside]
        px = (x - x_lo) * W // (x_hi - x_lo)
        py = (y - y_lo) * H // (y_hi - y_lo)
        once = np.unique(owner * (W * H) + py * W + px)  # a factor once per pixel
        f, pixel = once // (W * H), once % (W * H)
        visible[f] = True
        strand = is_rc[f].astype(np.int64)
        np.maximum.at(maxp, (strand, pixel), length[f].astype(np.uint32))
        np.add.at(cnt, (strand, pixel), np.uint32(1))
    out = {"max_forward": maxp[0].reshape(H, W), "max_rc": maxp[1].reshape(H, W),
           "count_forward": cnt[0].reshape(H, W) if counts else None,
           "count_rc": cnt[1].reshape(H, W) if counts else None,
           "visible_forward": int((visible & ~is_rc).sum()), "visible_rc": int((visible & is_rc).sum()),
           "hover_start": None, "hover_length": None, "hover_ref": None}
    if hover_bins:
        out.update(hover(recs, visible, x_lo, x_hi, hover_bins))
    return out


def hover(recs, visible, x_lo, x_hi, B):
    """per column floor((2 * start + length - 2 * x_lo) * B / (2 * (x_hi - x_lo))) of the visible kept factors with
    2 * x_lo <= 2 * start + length < 2 * x_hi: the greatest length, ties to the smallest factor index"""
    recs = np.asarray(recs, dtype=np.uint64).reshape(-1, 3)
    best = [None] * B
    for i in np.flatnonzero(visible).tolist():
        s, l = int(recs[i, 0]), int(recs[i, 1])
        mid2 = 2 * s + l
        if not 2 * x_lo <= mid2 < 2 * x_hi:
            continue
        c = (mid2 - 2 * x_lo) * B // (2 * (x_hi - x_lo))
        if best[c] is None or l > int(recs[best[c], 1]):  # (ascending i: an equal length does not replace)
            best[c] = i
    table = np.zeros((3, B), dtype=np.uint64)
    for c, i in enumerate(best):
        if i is not None:
            table[:, c] = recs[i]
    return {"hover_start": table[0], "hover_length": table[1], "hover_ref": table[2]}


def assert_equal(got, exp, what=""):
    for k, e in exp.items():
        g = got[k]
        if e is None:
            assert g is None, (what, k)
        elif isinstance(e, np.ndarray):
            assert g is not None and g.dtype == e.dtype and g.shape == e.shape, (what, k)
            assert np.array_equal(g, e), (what, k, int((g != e).sum()))
        else:
            assert g == e, (what, k, g, e)

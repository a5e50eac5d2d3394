"""Inputs for the one-trip form of the window rounds of group_sort.hpp (a scanning member asks for the words of its scan and
of its window at once and cuts the window from registers; places counted with one position per thread; queue items taken
from a counter) -- TEST INFRASTRUCTURE ONLY.  The expectation is tests/group_sort_model.py, unchanged; this file only builds
texts and lists for it.  Used by tests/test_gpu_group_sort_trips.py (GPU) and tests/test_group_sort_trips_host.py (CPU).

Every text is 2-bit DNA of at most 2^16 symbols.  A FAMILY is k members that share a random string S: member i is
S[:q_i], then the symbol S[q_i] with its lowest code bit flipped (A <-> C, G <-> T), then a few random symbols; q_i is where
the member first differs from S.  With h0 = 14 the first round's window covers symbols [14, 78); a family whose q are all
>= 78 is not split by it, so the second round SCANS from d0 = 78: word 0 is [78, 110), the last symbol of word 7 is 333,
and 334 = d0 + 8 words is the scan's stop.
"""
import functools
from collections import namedtuple

import numpy as np

import group_sort_model as M

H0 = 14
PER = 32                      # symbols per 64-bit word at 2 bits
D0 = H0 + 2 * PER             # 78: depth of a family after a first round that did not split it
STOP = D0 + M.SCAN_WORDS * PER  # 334
FLIP = {65: 67, 67: 65, 71: 84, 84: 71}
Built = namedtuple("Built", "text listed")


def _rand(rng, length):
    return M._rand(rng, M.A2, length)


def family(rng, qs, s_len=None, junk=True):
    """-> (bytes, member offsets): one member per q in qs (None: S itself, whole)"""
    s_len = s_len or max(q for q in qs if q is not None) + 70
    s = _rand(rng, s_len)
    out, starts = b"", []
    for q in qs:
        if junk:
            out += _rand(rng, int(rng.integers(1, 4)))
        starts.append(len(out))
        out += s if q is None else s[:q] + bytes([FLIP[s[q]]]) + _rand(rng, 6)
    return out, starts


def spread(first, second, k):
    """q of k members: the earliest difference, the second one, the rest from there on every few symbols"""
    return [None, first, second] + [second + 1 + (7 * i) % 90 for i in range(k - 3)]


def build(parts, h0=H0, order="shuffle", tail=M.A2, gap=1):
    """parts: (bytes, member offsets) -> one text, one group per part"""
    data, groups = b"", []
    for chunk, starts in parts:
        groups.append(np.array(starts, dtype=np.int64) + len(data))
        data += chunk
    text = M.Text(data + tail)
    assert text.bits == 2 and text.n <= 1 << 16, (text.bits, text.n)
    return Built(text, M.lay_out(text, h0, groups, order, gap, seed=len(data)))


# ---- group sizes ---------------------------------------------------------------------------------------------------------
SIZES = (65, 127, 128, 129, 255, 256, 257, 1024)


@functools.lru_cache(maxsize=None)
def sizes_text():
    """copies_text families of every size of the ladder and a few small ones; groups by their first h0 symbols"""
    text = M.Text(M.copies_text(7, 2, [(k, H0 + 3) for k in SIZES + (2, 3, 40, 64, 5, 2)]))
    assert text.n <= 1 << 16
    return text


@functools.lru_cache(maxsize=None)
def sizes_case(size, with_small, order="shuffle"):
    """the group of `size` members alone, or between small groups in one list"""
    text = sizes_text()
    pool = [g for g in text.groups(H0) if g.size >= 2]
    big = next(g for g in pool if g.size == size)
    small = [next(g for g in pool if g.size == s) for s in (2, 40, 64, 3, 5)] if with_small else []
    groups = small[:3] + [big] + small[3:]
    return Built(text, M.lay_out(text, H0, groups, order, 1, seed=size))


@functools.lru_cache(maxsize=None)
def ladder_case(order="shuffle"):
    """every size of the ladder in one list, small groups between them (the pivot and the marked runs)"""
    text = sizes_text()
    pool = [g for g in text.groups(H0) if g.size >= 2]
    groups = []
    for s in SIZES:
        groups.append(next(g for g in pool if g.size == s))
        groups.append(next(g for g in pool if g.size == (2 if s % 2 else 40) and not any(g is x for x in groups)))
    return Built(text, M.lay_out(text, H0, groups, order, 1, seed=3))


def mark_of(built):
    """the equalising round's filter: every other group counts as compared already"""
    mark = np.arange(built.text.n, dtype=np.uint32) % 7
    heads = np.unique(built.listed.grp)
    mark[heads[0::2] + 1] = M.PENDING
    mark[heads[1::2] + 1] = M.COMPARED
    mark.setflags(write=False)
    return mark


# ---- where the first differences lie ----------------------------------------------------------------------------------------
FIRST = {"word0": D0 + 5, "word7_last_bit": STOP - 1, "word8_stop": STOP}
SECOND = (63, 64, 65)  # symbols into the window that starts at the first difference


@functools.lru_cache(maxsize=None)
def diff_case(first, second, k):
    """one family of k members (3: tiles; 66: one thread per position, 128 threads; 130: 256 threads): the earliest
    difference at FIRST[first], the next one `second` symbols behind it"""
    rng = np.random.default_rng(100 + 7 * second + k + len(first))
    q1 = FIRST[first]
    return build([family(rng, spread(q1, q1 + second, k))])


# ---- ends inside the round ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ends_case(k):
    """a family in a segmented text (terminators: bytes that occur once).  Members end at 178 (inside the scanned words), two at
    138 with different terminators, one at 128 (inside the window that starts at 98) -- and the text itself ends 98 symbols
    into the last member: its scan from 78 would run 236 symbols past the end of the text, the segment's depth becomes 98
    and that member's terminator stands on the window's first symbol."""
    rng = np.random.default_rng(200 + k)
    s = _rand(rng, 520)
    t = iter(M.TERM_BYTES)
    term = lambda: bytes([next(t)])  # noqa: E731
    members = [s[:178] + term(), s[:138] + term(), s + term(), s[:138] + term(), s[:128] + term()]
    for i in range(k - 6):
        q = 140 + (11 * i) % 300
        members.append(s[:q] + bytes([FLIP[s[q]]]) + _rand(rng, 5) + (term() if i % 9 == 0 else b""))
    members.append(s[:98])  # (the end of the text is its terminator)
    data, starts = b"", []
    for mem in members:
        data += _rand(rng, int(rng.integers(1, 4)))
        starts.append(len(data))
        data += mem
    text = M.Text(data)
    assert text.segmented and text.bits == 2 and text.n <= 1 << 16 and text.lim[starts[-1]] == 98
    return Built(text, M.lay_out(text, H0, [np.array(starts)], "shuffle", 1, seed=k))


# ---- groups that give up ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def equal_case(k):
    """exact copies back to back: the groups stay tied as deep as anybody looks; three of them in one list"""
    text = M.Text(M.periodic_text(300 + k, k, 9000 // k))
    groups = [g for g in text.groups(H0) if g.size == k][:3]
    assert len(groups) == 3
    return Built(text, M.lay_out(text, H0, groups, "shuffle", 1, seed=k))


# ---- more queue items in a shard than workgroups of the shard ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def many_items_case():
    """65 copies of one head of 314 symbols: the suffixes at every offset of the head are a group of 65 -- 301 groups and more in
    one list of about 19 600 entries, 77 workgroups of group_dir_kernel, two workgroups of the queue kernel per shard"""
    text = M.Text(M.copies_text(401, 2, [(65, H0 + 300)]))
    groups = [g for g in text.groups(H0) if g.size == 65]
    assert len(groups) >= 300 and text.n <= 1 << 16
    return Built(text, M.lay_out(text, H0, groups, "shuffle", 0, seed=1))

"""Sequential model of the relative-LZ archive (nolzss_rlz_archive_*, include/nolzss_hip.h): the text behind the block
from absolute records, ranges by slicing, and the refusal rules of open and extract as (rule, index).

Records are (start, length, ref) rows or a FACTOR_DTYPE array in the layout of genomics.rlz.absolute_records: ref carries
RC_MASK, a literal has ref == start."""
import functools

import numpy as np

RC_MASK = 1 << 63
_COMP = {65: 84, 84: 65, 67: 71, 71: 67}  # A<->T, C<->G

TILING, LITERAL_LENGTH, SOURCE_IN_BLOCK, TARGET_BOUNDARY, LITERAL_COUNT = (
    "tiling", "literal length", "source inside the block", "target boundary", "literal count")
BAD_TARGET, LO_ABOVE_HI, HI_BEYOND, TOO_MANY_BYTES, CAPACITY = "target", "lo exceeds hi", "hi exceeds the length", "2^32 bytes", "d_out_capacity"


def rows(records):
    if isinstance(records, np.ndarray) and records.dtype.names:
        return list(zip(records["start"].tolist(), records["length"].tolist(), records["ref"].tolist()))
    return [tuple(int(x) for x in r) for r in records]


def expand(block, records, literals, faults=None):
    """-> the bytes behind the block.  A reverse-complement copy of a byte that is not A/C/G/T raises ValueError, or,
    with a list given as `faults`, leaves a zero byte and appends its position behind the block to the list."""
    block, literals = bytes(block), bytes(literals)
    out, lit = bytearray(), 0
    for start, length, ref in rows(records):
        assert start == len(block) + len(out)
        if ref == start:
            out.append(literals[lit])
            lit += 1
            continue
        r = ref & (RC_MASK - 1)
        src = block[r:r + length]
        assert len(src) == length
        if not ref & RC_MASK:
            out += src
            continue
        for t in range(length):
            c = _COMP.get(src[length - 1 - t], 0)
            if c == 0:
                if faults is None:
                    raise ValueError(f"complement of a non-nucleotide at position {len(out)}")
                faults.append(len(out))
            out.append(c)
    assert lit == len(literals)
    return bytes(out)


def extract(block, records, literals, target_lengths, ranges):
    """-> one bytes object per (target index, lo, hi) range, by slicing the expanded text"""
    text = expand(block, records, literals)
    base = np.concatenate([[0], np.cumsum(np.asarray(target_lengths, dtype=np.int64))]).tolist()
    return [text[base[t] + lo:base[t] + hi] for t, lo, hi in ranges]


def open_refusal(block_len, records, n_literals, target_lengths):
    """-> None, or (rule, record index) as nolzss_rlz_archive_open_records refuses: the first record that breaks a
    structural rule; then the literal count (the first literal too many, or z "behind the last"); then the length sum
    (z)."""
    recs = rows(records)
    z = len(recs)
    bounds = np.concatenate([[block_len], block_len + np.cumsum(np.asarray(target_lengths, dtype=object))]).tolist()
    n = recs[-1][0] + recs[-1][1] if z else block_len
    expect = block_len
    for i, (start, length, ref) in enumerate(recs):
        lit, r = ref == start, ref & (RC_MASK - 1)
        if start != expect or length == 0 or start > n or length > n - start:
            return TILING, i
        if lit and length != 1:
            return LITERAL_LENGTH, i
        if not lit and r + length > block_len:
            return SOURCE_IN_BLOCK, i
        ends = [b for b in bounds if b > start]
        if not ends or start + length > ends[0]:
            return TARGET_BOUNDARY, i
        expect = start + length
    seen = 0
    for i, (start, length, ref) in enumerate(recs):
        if ref == start:
            if seen == n_literals:
                return LITERAL_COUNT, i
            seen += 1
    if seen != n_literals:
        return LITERAL_COUNT, z
    if bounds[-1] != n:
        return TARGET_BOUNDARY, z
    return None


def extract_refusal(target_lengths, ranges, capacity=None):
    """-> None, or (rule, range index) as nolzss_rlz_archive_extract(_device) refuses; a capacity below the total names
    range q, behind the last"""
    total = 0
    for i, (t, lo, hi) in enumerate(ranges):
        if t >= len(target_lengths):
            return BAD_TARGET, i
        if lo > hi:
            return LO_ABOVE_HI, i
        if hi > target_lengths[t]:
            return HI_BEYOND, i
        total += hi - lo
        if total >= 1 << 32:
            return TOO_MANY_BYTES, i
    if capacity is not None and capacity < total:
        return CAPACITY, len(ranges)
    return None


# ---- the boundary input of the GPU tests, built and parsed on the CPU ------------------------------------------------
def parse_to_absolute(reference, targets, with_rc=True):
    """rlz_model.brute_parse of every target -> (block, records, literals, target lengths) through
    genomics.rlz.absolute_records: what RlzArchive.from_factors opens, without a device"""
    import rlz_model
    from nolzss_amd.genomics import rlz
    refs = [reference] if isinstance(reference, (bytes, bytearray)) else list(reference)
    factors = []
    for t in targets:
        f = np.array(rlz_model.brute_parse(refs, t, with_rc), dtype=rlz.RLZ_DTYPE).reshape(-1)
        factors.append(f)
    literals = b"".join(rlz.rlz_literals(targets, factors))
    block, records, lengths = rlz.absolute_records(refs, factors)
    return block, records, literals, lengths


@functools.lru_cache(maxsize=None)
def boundary_input():
    """Two reference records over {A, T}; a first target of one long forward copy, 600 consecutive literals, one
    reverse-complement copy of 900 and a forward copy of 2000 that ends the target; an empty second target; a third
    that repeats the first shifted by 7 bases -> dict(refs, targets, block, records, literals, lengths)"""
    import rlz_model
    rng = np.random.default_rng(8)
    at = np.frombuffer(b"AT", dtype=np.uint8)
    r1 = at[rng.integers(0, 2, size=3000)].tobytes()
    r2 = at[rng.integers(0, 2, size=2000)].tobytes()
    t1 = (r1[100:1500] + b"CG" * 300 + rlz_model.revcomp(r2[200:1100]) + b"C" + r1[2000:2009] + b"G" + r2[0:2000])
    targets = [t1, b"", t1[7:]]
    block, records, literals, lengths = parse_to_absolute([r1, r2], targets)
    return {"refs": [r1, r2], "targets": targets, "block": block, "records": records, "literals": literals,
            "lengths": lengths}


@functools.lru_cache(maxsize=None)
def boundary_cut():
    """300 bases of the first boundary target around its reverse-complement copy's end: all three record kinds"""
    inp = boundary_input()
    targets = [inp["targets"][0][2700:3000]]
    block, records, literals, lengths = parse_to_absolute(inp["refs"], targets)
    return {"refs": inp["refs"], "targets": targets, "block": block, "records": records, "literals": literals,
            "lengths": lengths}


def record_kinds(records):
    """-> array of 'F' (forward copy), 'R' (reverse-complement copy), 'L' (literal) per record"""
    records = np.asarray(records)
    lit = records["ref"] == records["start"]
    rc = (records["ref"] >> np.uint64(63)) != 0
    return np.where(lit, "L", np.where(rc, "R", "F"))


def check_boundary_input(inp):
    """The properties the GPU tests rely on; returns the records of the first target and their kinds."""
    assert [len(t) for t in inp["targets"]] == [4911, 0, 4904] == list(inp["lengths"])
    B = len(inp["block"])
    assert B == 5001
    rec = inp["records"]
    first = rec[rec["start"] < B + 4911]
    kinds = record_kinds(first)
    assert len(first) == 606
    assert (kinds[0], int(first["length"][0])) == ("F", 1400)
    assert (kinds[1:601] == "L").all()  # more than two 256-position sample blocks with a record at every position
    assert (kinds[601], int(first["length"][601])) == ("R", 900)
    assert kinds[602] == "L" and kinds[603] == "F" and int(first["length"][603]) == 9 and kinds[604] == "L"
    assert (kinds[605], int(first["length"][605])) == ("F", 2000)  # spans several sample blocks and ends the target
    assert int(first["start"][605] + first["length"][605]) == B + 4911
    third = rec[rec["start"] >= B + 4911]
    assert len(third) == 606 and int(third["length"][0]) == 1393
    # the same boundaries fall on other residues of the 16-byte chunks and of the 256-position blocks
    d1, d3 = first["start"][601] - np.uint64(B), third["start"][601] - np.uint64(B)
    assert int(d1) % 16 != int(d3) % 16 and int(d1) % 256 != int(d3) % 256
    assert expand(inp["block"], rec, inp["literals"]) == b"".join(inp["targets"])
    return first, kinds

"""The decoder's definition without a device (include/nolzss_hip.h, nolzss_decode): the sequential form, position by
position, with every rule as an exception; the per-factor slicing form the probe times; the literal extractor; and the
hand-built deep chain that no factorizer emits."""
RC_MASK = 1 << 63
COMP = {ord("A"): ord("T"), ord("T"): ord("A"), ord("C"): ord("G"), ord("G"): ord("C")}


class DecodeError(ValueError):
    """rule: tiling, literal length, source range, literal count, complement; record: the first offending index"""

    def __init__(self, rule, record):
        super().__init__(f"record {record} breaks {rule}")
        self.rule, self.record = rule, record


def as_rows(records):
    """(start, length, ref with RC_MASK) rows from a structured array, 3-tuples or 4-tuples (is_rc sets the mask)"""
    if hasattr(records, "dtype") and records.dtype.names:
        return list(zip(records["start"].tolist(), records["length"].tolist(), records["ref"].tolist()))
    rows = []
    for row in records:
        start, length, ref = int(row[0]), int(row[1]), int(row[2])
        if len(row) == 4 and row[3]:
            ref |= RC_MASK
        rows.append((start, length, ref))
    return rows


def check(rows, n_literals, prefix_len):
    """the structural rules in the decoder's order: the first bad record with its rule, then the literal count"""
    expect = prefix_len
    literal_at = []
    for k, (start, length, ref) in enumerate(rows):
        r = ref & ~RC_MASK
        if start != expect or length < 1:
            raise DecodeError("tiling", k)
        if ref == start:
            if length != 1:
                raise DecodeError("literal length", k)
            literal_at.append(k)
        elif r + length > start:
            raise DecodeError("source range", k)
        expect = start + length
    if len(literal_at) > n_literals:
        raise DecodeError("literal count", literal_at[n_literals])
    if len(literal_at) < n_literals:
        raise DecodeError("literal count", len(rows))


def decode(records, literals, prefix=b""):
    """-> (text bytes, chain depth): depth = the largest number of copy hops from a decoded position to the literal or
    prefix byte its symbol comes from (a literal has depth 0, a copy from the prefix depth 1)."""
    rows = as_rows(records)
    literals, prefix = bytes(literals), bytes(prefix)
    check(rows, len(literals), len(prefix))
    text = bytearray(prefix)
    depth = [0] * len(prefix)
    parity_bad = None  # first position whose chain complements a non-nucleotide
    taken = 0
    for k, (start, length, ref) in enumerate(rows):
        if ref == start:
            text.append(literals[taken])
            depth.append(0)
            taken += 1
            continue
        rc, r = bool(ref & RC_MASK), ref & ~RC_MASK
        for t in range(length):
            y = r + length - 1 - t if rc else r + t
            c = text[y]
            if rc:
                if c not in COMP:
                    # the byte at y is what text[y] decodes to; an odd chain over a non-nucleotide is the error
                    if parity_bad is None:
                        parity_bad = (start + t, k)
                else:
                    c = COMP[c]
            text.append(c)
            depth.append(depth[y] + 1)
    if parity_bad is not None:
        raise DecodeError("complement", parity_bad[1])
    return bytes(text), max(depth[len(prefix):], default=0)


def decode_slices(records, literals, prefix=b""):
    """the per-factor form: one bytes slice per copy factor (an overlap-free source makes the slice whole); no checks"""
    table = bytes.maketrans(b"ACGT", b"TGCA")
    text = bytearray(prefix)
    taken = 0
    for start, length, ref in as_rows(records):
        if ref == start:
            text.append(literals[taken])
            taken += 1
        elif ref & RC_MASK:
            r = ref & ~RC_MASK
            text += text[r:r + length].translate(table)[::-1]
        else:
            text += text[ref:ref + length]
    return bytes(text)


def literal_symbols(text, records):
    text = bytes(text)
    return bytes(text[start] for start, length, ref in as_rows(records) if ref == start)


def deep_chain(n, alternate=True, all_rc=False):
    """literals A, C, then records (p, 2, p - 2) for p = 2, 4, .., n - 2: position x copies x - 2, a chain of
    n / 2 - 1 hops.  alternate: RC_MASK on every second record, the first included; all_rc: on every record.
    -> (records as (start, length, ref) rows, literals)"""
    assert n % 2 == 0 and n >= 4
    rows = [(0, 1, 0), (1, 1, 1)]
    for j, p in enumerate(range(2, n, 2)):
        masked = all_rc or (alternate and j % 2 == 0)
        rows.append((p, 2, (p - 2) | (RC_MASK if masked else 0)))
    return rows, b"AC"

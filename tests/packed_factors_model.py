"""A sequential model of the compact container of factor records ("Factor records: the compact
container"; include/nolzss_hip.h, nolzss_factors_pack).  Written from the format, one record after the other, with
Python integers: no scan, no rank, no kernel.  pack / unpack work on FACTOR_DTYPE records and literal bytes and on the
dict of sections the library returns (literal_mode, first_start, z, n_literals, decoded, control, data, literals)."""
import numpy as np

RC_MASK = 1 << 63
FACTOR_DTYPE = np.dtype([("start", "<u8"), ("length", "<u8"), ("ref", "<u8")])
M32 = 0xFFFFFFFF
MAX_TEXT = 0xFFFFFFFF - (1 << 19)  # the 32-bit pipeline
CODE = {65: 0, 67: 1, 71: 2, 84: 3}
BASES = b"ACGT"
LENGTH_BYTES = (0, 1, 2, 4)
CODE_BYTES = (0, 2, 4, 5)

# the rules a pack (1 .. 3, in nolzss_decode's words) and an unpack name, as the library numbers them
RULES = {1: "tiling", 2: "literal length", 3: "source range", 4: "spare nibble", 5: "literal nibble", 6: "length",
         7: "diagonal code", 8: "literal count", 9: "data size", 10: "decoded length"}


class FormatError(ValueError):
    def __init__(self, index, rule):
        super().__init__(f"record {index} breaks {rule}")
        self.index, self.rule = index, rule


def zigzag32(e):
    """e: the difference mod 2^32, read as int32 -> its zigzag code (32 bits)"""
    return ((e << 1) & M32) ^ (M32 if e >> 31 else 0)


def unzigzag32(zz):
    return (zz >> 1) ^ (M32 if zz & 1 else 0)


def pack_2bit(symbols):
    out = bytearray((len(symbols) + 3) // 4)
    for t, c in enumerate(symbols):
        out[t >> 2] |= CODE[c] << (2 * (t & 3))
    return bytes(out)


def unpack_2bit(data, n):
    return bytes(BASES[(data[t >> 2] >> (2 * (t & 3))) & 3] for t in range(n))


def check_records(records):
    """what a pack refuses: FormatError names the first offending record"""
    expect = None
    for k in range(len(records)):
        start, L, ref = (int(records[k][f]) for f in ("start", "length", "ref"))
        x = ref & (RC_MASK - 1)
        if (expect is not None and start != expect) or L == 0 or start + L > MAX_TEXT:
            raise FormatError(k, RULES[1])
        if ref == start and L != 1:
            raise FormatError(k, RULES[2])
        if ref != start and x + L > start:
            raise FormatError(k, RULES[3])
        expect = start + L


def code_records(records):
    """-> (control, data, literal records, the v of every record or None)"""
    z = len(records)
    control, data, codes = bytearray((z + 1) // 2), bytearray(), []
    gc, rc_c, lit = 0, 0, 0
    for i in range(z):
        p, L, ref = (int(records[i][f]) for f in ("start", "length", "ref"))
        if ref == p:
            nib = 0
            lit += 1
            codes.append(None)
        else:
            r = 1 if ref & RC_MASK else 0
            x = ref & (RC_MASK - 1)
            y = (-(x + L)) & M32 if r else x
            g = (y - p) & M32
            v = (zigzag32((g - gc) & M32) << 1) | (r ^ rc_c)
            gc, rc_c = g, r
            a = 1 if L <= 0xFF else 2 if L <= 0xFFFF else 3
            b = 0 if v == 0 else 1 if v < 1 << 16 else 2 if v < 1 << 32 else 3
            data += L.to_bytes(LENGTH_BYTES[a], "little") + v.to_bytes(CODE_BYTES[b], "little")
            nib = a | b << 2
            codes.append(v)
        control[i >> 1] |= nib << (4 * (i & 1))
    return bytes(control), bytes(data), lit, codes


def pack(records, literals=None):
    """-> the sections as a dict (the fields of nolzss_packed_factors); literals None: literal_mode 2"""
    check_records(records)
    z = len(records)
    control, data, lit, _ = code_records(records)
    first = int(records[0]["start"]) if z else 0
    decoded = int(records[-1]["start"] + records[-1]["length"]) - first if z else 0
    if literals is None:
        mode, section = 2, b""
    else:
        literals = bytes(literals)
        if lit != len(literals):
            raise FormatError(min(z, _literal_record(records, len(literals))), RULES[8])
        two_bit = all(c in CODE for c in literals)
        mode, section = (1, pack_2bit(literals)) if two_bit else (0, literals)
    return {"literal_mode": mode, "first_start": first, "z": z, "n_literals": lit, "decoded": decoded,
            "control": control, "data": data, "literals": section}


def _literal_record(records, count):
    """the index of literal record number `count` (0-based), len(records) if there are not that many"""
    seen = 0
    for k in range(len(records)):
        if int(records[k]["ref"]) == int(records[k]["start"]):
            if seen == count:
                return k
            seen += 1
    return len(records)


def unpack(s):
    """sections -> (records, literals or None).  FormatError names the rule and the smallest offending record of the
    first of the three steps of the header that finds a violation; ValueError for what the host checks refuse."""
    mode, first, z, nlit, decoded = (int(s[k]) for k in ("literal_mode", "first_start", "z", "n_literals", "decoded"))
    control, data, section = bytes(s["control"]), bytes(s["data"]), bytes(s["literals"])
    if mode not in (0, 1, 2):
        raise ValueError("literal_mode")
    if first > MAX_TEXT or decoded > MAX_TEXT or first + decoded > MAX_TEXT or z > MAX_TEXT or nlit > MAX_TEXT:
        raise ValueError("text too long")
    if len(control) != (z + 1) // 2 or len(section) != ((nlit + 3) // 4 if mode == 1 else nlit if mode == 0 else 0):
        raise ValueError("section size")
    nib = [(control[i >> 1] >> (4 * (i & 1))) & 15 for i in range(z)]
    # step 1: what the nibbles alone decide; the sizes are settled before a data byte is read
    errors = [(i, RULES[5]) for i in range(z) if not nib[i] & 3 and nib[i] >> 2][:1]
    if z & 1 and control[z >> 1] >> 4:
        errors.append((z, RULES[4]))
    if errors:
        raise FormatError(*min(errors))
    if sum(LENGTH_BYTES[n & 3] + CODE_BYTES[n >> 2] for n in nib) != len(data):
        raise FormatError(z, RULES[9])
    # step 2: lengths and codes
    lengths, codes, off = [], [], 0
    for i in range(z):
        a, b = nib[i] & 3, nib[i] >> 2
        if a == 0:
            lengths.append(1)
            codes.append(None)
            continue
        L = int.from_bytes(data[off:off + LENGTH_BYTES[a]], "little")
        off += LENGTH_BYTES[a]
        v = int.from_bytes(data[off:off + CODE_BYTES[b]], "little")
        off += CODE_BYTES[b]
        lengths.append(L)
        codes.append(v)
    for i in range(z):
        if codes[i] is not None and lengths[i] == 0:
            raise FormatError(i, RULES[6])
        if codes[i] is not None and codes[i] >> 33:
            raise FormatError(i, RULES[7])
    if sum(lengths) != decoded:
        raise FormatError(z, RULES[10])
    # step 3: positions, diagonals, strands
    records = np.zeros(z, dtype=FACTOR_DTYPE)
    gc, rc_c, p, seen = 0, 0, first, 0
    for i in range(z):
        L, v = lengths[i], codes[i]
        if v is None:
            if seen >= nlit:
                raise FormatError(i, RULES[8])
            seen += 1
            ref = p
        else:
            g = (gc + unzigzag32(v >> 1)) & M32
            r = rc_c ^ (v & 1)
            gc, rc_c = g, r
            y = (g + p) & M32
            x = (-y - L) & M32 if r else y
            if x + L > p:
                raise FormatError(i, RULES[3])
            ref = x | (RC_MASK if r else 0)
        records[i] = (p, L, ref)
        p += L
    if seen != nlit:
        raise FormatError(z, RULES[8])
    literals = None if mode == 2 else unpack_2bit(section, nlit) if mode == 1 else section
    return records, literals


# ---- records for the tests -------------------------------------------------------------------------------------------
class Builder:
    """Records laid end to end from first_start, each placed by its source or by the code it must get."""

    def __init__(self, first_start=0):
        self.first, self.p = first_start, first_start
        self.g, self.r = 0, 0  # diagonal and strand of the last copy
        self.rows, self.literals, self.codes = [], bytearray(), []

    def literal(self, symbol=b"A"):
        self.rows.append((self.p, 1, self.p))
        self.literals += symbol
        self.codes.append(None)
        self.p += 1
        return self

    def copy(self, x, L, rc=False):
        assert L >= 1 and 0 <= x and x + L <= self.p, (x, L, self.p)
        r = 1 if rc else 0
        y = (-(x + L)) & M32 if r else x
        g = (y - self.p) & M32
        self.codes.append((zigzag32((g - self.g) & M32) << 1) | (r ^ self.r))
        self.rows.append((self.p, L, x | (RC_MASK if r else 0)))
        self.p, self.g, self.r = self.p + L, g, r
        return self

    def copy_step(self, L, e=0, toggle=False):
        """the copy of length L whose diagonal lies e behind the last copy's, on its strand or (toggle) the other:
        v = (zigzag32(e) << 1) | toggle"""
        r = self.r ^ (1 if toggle else 0)
        y = (self.g + e + self.p) & M32
        x = (-y - L) & M32 if r else y
        return self.copy(x, L, bool(r))

    def records(self):
        return np.array(self.rows, dtype=FACTOR_DTYPE)


def edge_builder():
    """every class edge of v, each reached with copy_step: v = 0, 2^16 - 1 | 2^16, 2^32 - 1 | 2^32, 2^33 - 1"""
    b = Builder(3 << 30)
    b.copy((1 << 30) + (1 << 20), 10)               # forward; a toggle near its diagonal is valid here (y > 2^32 - p)
    b.copy_step(5)                                  # v = 0
    b.copy_step(5, e=-(1 << 14), toggle=True)       # zigzag 2^15 - 1, toggle: v = 2^16 - 1 (2 bytes)
    b.copy_step(5, e=1 << 14)                       # zigzag 2^15: v = 2^16 (4 bytes)
    b.copy_step(5, e=1 << 30, toggle=True)          # zigzag 2^31, toggle: v = 2^32 + 1 (5 bytes)
    b.copy_step(5, e=-(1 << 30), toggle=True)       # zigzag 2^31 - 1, toggle: v = 2^32 - 1 (4 bytes)
    b.copy_step(5, e=1 << 30)                       # v = 2^32 (5 bytes)
    b.copy_step(5, e=-(1 << 31), toggle=True)       # zigzag 2^32 - 1, toggle: v = 2^33 - 1
    b.copy_step(5, e=-(1 << 31))                    # v = 2^33 - 2
    return b


def random_records(rng, z, first_start=0, p_literal=0.2, p_continue=0.5, max_length=300, with_rc=True, alphabet=b"ACGT"):
    """z records from first_start (rng: random.Random): literals, copies that continue the last diagonal, copies placed
    anywhere in front of themselves on either strand -> (records, literals)"""
    b = Builder(first_start)
    for _ in range(z):
        u = rng.random()
        L = min(rng.choice((1, 1, 2, 7, 40, 255, 256, max_length)), max_length)
        if u < p_literal or b.p == 0:
            b.literal(bytes([rng.choice(alphabet)]))
            continue
        L = min(L, b.p)
        placed = False
        if u < p_literal + p_continue and any(c is not None for c in b.codes):
            y = (b.g + b.p) & M32
            x = (-y - L) & M32 if b.r else y
            if x + L <= b.p:
                b.copy(x, L, bool(b.r))
                placed = True
        if not placed:
            b.copy(rng.randrange(0, b.p - L + 1), L, with_rc and rng.random() < 0.4)
    return b.records(), bytes(b.literals)


# ---- planting violations ---------------------------------------------------------------------------------------------
def nibbles(s):
    c = s["control"]
    return [(c[i >> 1] >> (4 * (i & 1))) & 15 for i in range(s["z"])]


def data_offsets(s):
    """the first data byte of every record, from the nibbles"""
    out, at = [], 0
    for n in nibbles(s):
        out.append(at)
        at += LENGTH_BYTES[n & 3] + CODE_BYTES[n >> 2]
    return out


def with_bytes(s, section, at, new):
    """a copy of the sections with section[at : at + len(new)] = new"""
    raw = bytearray(s[section])
    raw[at:at + len(new)] = new
    out = dict(s)
    out[section] = bytes(raw)
    return out

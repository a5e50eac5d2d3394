"""A sequential model of the compact relative-LZ archive format ("Relative-LZ archive: the compact
container"; include/nolzss_hip.h, nolzss_rlz_archive_pack).  Written from the format, one record after the other, with
Python integers: no scan, no rank, no kernel.  pack / unpack work on the host form of an archive (block bytes, FACTOR_DTYPE
records with absolute starts, literal bytes, target lengths); container_bytes / parse_container are the file."""
import struct

import numpy as np

RC_MASK = 1 << 63
FACTOR_DTYPE = np.dtype([("start", "<u8"), ("length", "<u8"), ("ref", "<u8")])
M32 = 0xFFFFFFFF
MAGIC = b"noLZRLZ1"
HEADER = struct.Struct("<8sII12Q")  # magic, version, flags, B, k, z, n_literals, decoded, separators, six section sizes
FLAG_BLOCK_2BIT, FLAG_LITERALS_2BIT, FLAG_HAS_IDS = 1, 2, 4
CODE = {65: 0, 67: 1, 71: 2, 84: 3}
BASES = b"ACGT"

# the rules an unpack names, as the library numbers them
RULES = {1: "spare nibble", 2: "literal nibble", 3: "length", 4: "diagonal code", 5: "source inside the block",
         6: "target boundary", 7: "literal count", 8: "data size", 9: "separator list"}


class FormatError(ValueError):
    def __init__(self, index, rule):
        super().__init__(f"record {index} breaks {rule}")
        self.index, self.rule = index, rule


def zigzag32(d):
    """d: the difference mod 2^32, read as int32 -> its zigzag code (32 bits)"""
    return ((d << 1) & M32) ^ (M32 if d >> 31 else 0)


def unzigzag32(zz):
    return (zz >> 1) ^ (M32 if zz & 1 else 0)


_CODE_TABLE = np.zeros(256, dtype=np.uint8)
for _c, _v in CODE.items():
    _CODE_TABLE[_c] = _v


def pack_2bit(symbols):
    """four symbols to a byte, the first in the low bits; anything but C, G, T packs as 0 (numpy: blocks are long)"""
    codes = _CODE_TABLE[np.frombuffer(bytes(symbols), dtype=np.uint8)]
    codes = np.concatenate([codes, np.zeros(-len(codes) % 4, dtype=np.uint8)]).reshape(-1, 4)
    return (codes[:, 0] | codes[:, 1] << 2 | codes[:, 2] << 4 | codes[:, 3] << 6).astype(np.uint8).tobytes()


def unpack_2bit(data, n):
    q = np.frombuffer(bytes(data), dtype=np.uint8)
    codes = np.stack([(q >> s) & 3 for s in (0, 2, 4, 6)], axis=1).reshape(-1)[:n]
    return np.frombuffer(BASES, dtype=np.uint8)[codes].tobytes()


def pack_block(block):
    arr = np.frombuffer(bytes(block), dtype=np.uint8)
    known = np.zeros(256, dtype=bool)
    known[[1] + list(CODE)] = True
    if known[arr].all():
        seps = np.flatnonzero(arr == 1).astype("<u4")
        return 1, len(seps), pack_2bit(block) + seps.tobytes()
    return 0, 0, bytes(block)


def unpack_block(mode, B, seps, data):
    if mode == 0:
        if seps or len(data) != B:
            raise ValueError("block section size")
        return bytes(data)
    q = (B + 3) // 4
    if len(data) != q + 4 * seps:
        raise ValueError("block section size")
    out = bytearray(unpack_2bit(data[:q], B))
    last = -1
    for t, p in enumerate(struct.unpack(f"<{seps}I", data[q:])):
        if p >= B or p <= last:
            raise FormatError(t, RULES[9])
        out[p] = 1
        last = p
    return bytes(out)


def code_records(B, records):
    """-> (control, data, literal records) of records behind a block of B bytes (only its length matters here)"""
    z = len(records)
    control, data = bytearray((z + 1) // 2), bytearray()
    gc, rc_c, lit = 0, 0, 0
    for i in range(z):
        start, L, ref = (int(records[i][f]) for f in ("start", "length", "ref"))
        p = start - B
        if ref == start:
            assert L == 1
            nib = 0
            lit += 1
        else:
            r = 1 if ref & RC_MASK else 0
            x = ref & (RC_MASK - 1)
            y = (2 * B + 1 - x - L) & M32 if r else x
            g = (y - p) & M32
            v = (zigzag32((g - gc) & M32) << 1) | (r ^ rc_c)
            gc, rc_c = g, r
            a = 1 if L <= 0xFF else 2 if L <= 0xFFFF else 3
            b = 0 if v == 0 else 1 if v < 1 << 8 else 2 if v < 1 << 24 else 3
            data += L.to_bytes((0, 1, 2, 4)[a], "little") + v.to_bytes((0, 1, 3, 5)[b], "little")
            nib = a | b << 2
        control[i >> 1] |= nib << (4 * (i & 1))
    return bytes(control), bytes(data), lit


def pack(block, records, literals, target_lengths):
    """-> the sections of the container as a dict (the fields of nolzss_rlz_archive_packed)"""
    block, literals = bytes(block), bytes(literals)
    B, z = len(block), len(records)
    control, data, lit = code_records(B, records)
    assert lit == len(literals)
    two_bit = all(c in CODE for c in literals)
    mode, seps, blk = pack_block(block)
    decoded = int(records[-1]["start"] + records[-1]["length"]) - B if z else 0
    assert decoded == sum(int(x) for x in target_lengths)
    return {"block_mode": mode, "literal_mode": 1 if two_bit else 0, "block_length": B, "z": z, "n_literals": lit,
            "decoded": decoded, "num_separators": seps, "block": blk, "control": bytes(control), "data": bytes(data),
            "literals": pack_2bit(literals) if two_bit else literals}


def unpack(s, target_lengths):
    """sections -> (block, records, literals); FormatError names the smallest offending record and the rule"""
    block = unpack_block(s["block_mode"], s["block_length"], s["num_separators"], s["block"])
    records, literals = decode_records(s, target_lengths)
    return block, records, literals


def decode_records(s, target_lengths):
    """the control, data and literal sections -> (records, literals); of the block only block_length is read"""
    B, z, nlit = s["block_length"], s["z"], s["n_literals"]
    control, data = s["control"], s["data"]
    if len(control) != (z + 1) // 2 or len(s["literals"]) != ((nlit + 3) // 4 if s["literal_mode"] else nlit):
        raise ValueError("section size")
    symbols = unpack_2bit(s["literals"], nlit) if s["literal_mode"] else bytes(s["literals"])
    ends, at = [], 0
    for n in target_lengths:
        at += int(n)
        ends.append(at)
    nib = [(control[i >> 1] >> (4 * (i & 1))) & 15 for i in range(z)]
    # what the nibbles alone decide comes first: the sizes are settled before a data byte is read
    sized = [i for i in range(z) if not nib[i] & 3 and nib[i] >> 2]
    need = sum((0, 1, 2, 4)[n & 3] + (0, 1, 3, 5)[n >> 2] for n in nib)
    errors = [(i, RULES[2]) for i in sized[:1]]
    if z & 1 and control[z >> 1] >> 4:
        errors.append((z, RULES[1]))
    if not errors and need != len(data):
        errors.append((z, RULES[8]))
    if errors:
        raise FormatError(*min(errors))
    records = np.zeros(z, dtype=FACTOR_DTYPE)
    out_lit = bytearray()
    gc, rc_c, p, off, t = 0, 0, 0, 0, 0
    for i in range(z):
        a, b = nib[i] & 3, nib[i] >> 2
        if a == 0:
            L = 1
        else:
            n = (0, 1, 2, 4)[a]
            L = int.from_bytes(data[off:off + n], "little")
            off += n
            n = (0, 1, 3, 5)[b]
            v = int.from_bytes(data[off:off + n], "little")
            off += n
            if L == 0:
                raise FormatError(i, RULES[3])
            if v >> 33:
                raise FormatError(i, RULES[4])
        if a == 0:
            if len(out_lit) == nlit:
                raise FormatError(i, RULES[7])
            ref = B + p
            out_lit.append(symbols[len(out_lit)])
        else:
            g = (gc + unzigzag32(v >> 1)) & M32
            r = rc_c ^ (v & 1)
            gc, rc_c = g, r
            y = (g + p) & M32
            x = (2 * B + 1 - y - L) & M32 if r else y
            if x + L > B:
                raise FormatError(i, RULES[5])
            ref = x | (RC_MASK if r else 0)
        while t < len(ends) and ends[t] <= p:
            t += 1
        if t == len(ends) or p + L > ends[t]:
            raise FormatError(i, RULES[6])
        records[i] = (B + p, L, ref)
        p += L
    if len(out_lit) != nlit:
        raise FormatError(z, RULES[7])
    if p != s["decoded"] or p != (ends[-1] if ends else 0):
        raise FormatError(z, RULES[6])
    return records, bytes(out_lit)


def _pad(b):
    return bytes(b) + b"\0" * (-len(b) % 8)


def ids_section(ids):
    names = [i.encode("utf-8") if isinstance(i, str) else bytes(i) for i in ids]
    offs, at = [0], 0
    for n in names:
        at += len(n)
        offs.append(at)
    return struct.pack(f"<{len(offs)}Q", *offs) + b"".join(names)


def container_bytes(s, target_lengths, ids=None):
    lengths = [int(x) for x in target_lengths]
    parts = [struct.pack(f"<{len(lengths)}Q", *lengths), b"" if ids is None else ids_section(ids), s["block"], s["control"],
             s["data"], s["literals"]]
    flags = (FLAG_BLOCK_2BIT if s["block_mode"] else 0) | (FLAG_LITERALS_2BIT if s["literal_mode"] else 0) | \
        (0 if ids is None else FLAG_HAS_IDS)
    head = HEADER.pack(MAGIC, 1, flags, s["block_length"], len(lengths), s["z"], s["n_literals"], s["decoded"],
                       s["num_separators"], *[len(x) for x in parts])
    assert len(head) % 8 == 0
    return head + b"".join(_pad(x) for x in parts)


def parse_container(raw):
    """-> (sections, target lengths, ids or None); ValueError for anything the header or the sizes rule out"""
    raw = bytes(raw)
    if len(raw) < HEADER.size or raw[:8] != MAGIC:
        raise ValueError("bad magic")
    f = HEADER.unpack_from(raw)
    version, flags, B, k, z, nlit, decoded, seps = f[1:9]
    sizes = f[9:]
    if version != 1 or flags & ~7:
        raise ValueError("version or flags")
    at, parts = HEADER.size, []
    for n in sizes:
        end = at + n + (-n % 8)
        if end > len(raw):
            raise ValueError("a section ends behind the file")
        if any(raw[at + n:end]):
            raise ValueError("padding")
        parts.append(raw[at:at + n])
        at = end
    if at != len(raw):
        raise ValueError("trailing bytes")
    if sizes[0] != 8 * k:
        raise ValueError("target lengths size")
    lengths = list(struct.unpack(f"<{k}Q", parts[0]))
    ids = None
    if flags & FLAG_HAS_IDS:
        if sizes[1] < 8 * (k + 1):
            raise ValueError("ids size")
        offs = struct.unpack_from(f"<{k + 1}Q", parts[1])
        names = parts[1][8 * (k + 1):]
        if offs[0] != 0 or offs[-1] != len(names) or any(offs[j] > offs[j + 1] for j in range(k)):
            raise ValueError("id offsets")
        ids = [names[offs[j]:offs[j + 1]].decode("utf-8") for j in range(k)]
    elif sizes[1]:
        raise ValueError("ids size")
    s = {"block_mode": flags & 1, "literal_mode": (flags >> 1) & 1, "block_length": B, "z": z, "n_literals": nlit,
         "decoded": decoded, "num_separators": seps, "block": parts[2], "control": parts[3], "data": parts[4],
         "literals": parts[5]}
    want = ((B + 3) // 4 + 4 * seps if flags & 1 else B, (z + 1) // 2, (nlit + 3) // 4 if flags & 2 else nlit)
    if (sizes[2], sizes[3], sizes[5]) != want or (seps and not flags & 1):
        raise ValueError("a section has not the size the counts ask for")
    if sum(lengths) != decoded:
        raise ValueError("the target lengths do not sum to the decoded length")
    return s, lengths, ids


# ---- archives for the tests ----------------------------------------------------------------------------------------
class Builder:
    """Records laid end to end behind a block, each placed by its source or by the code it must get."""

    def __init__(self, block, B=None):
        """B: the length of a block that is not laid out (the record codes read nothing else of it)"""
        self.block, self.B = bytes(block), len(block) if B is None else B
        self.p, self.g, self.r = 0, 0, 0  # decoded length so far; diagonal and strand of the last copy
        self.rows, self.literals, self.codes = [], bytearray(), []

    def literal(self, symbol=b"A"):
        self.rows.append((self.B + self.p, 1, self.B + self.p))
        self.literals += symbol
        self.codes.append(None)
        self.p += 1
        return self

    def copy(self, x, L, rc=False):
        assert L >= 1 and 0 <= x and x + L <= self.B, (x, L, self.B)
        r = 1 if rc else 0
        y = (2 * self.B + 1 - x - L) & M32 if r else x
        g = (y - self.p) & M32
        self.codes.append((zigzag32((g - self.g) & M32) << 1) | (r ^ self.r))
        self.rows.append((self.B + self.p, L, x | (RC_MASK if r else 0)))
        self.p, self.g, self.r = self.p + L, g, r
        return self

    def copy_step(self, L, e=0, toggle=False):
        """the copy of length L whose diagonal lies e behind the last copy's, on its strand or (toggle) the other:
        v = (zigzag32(e) << 1) | toggle"""
        r = self.r ^ (1 if toggle else 0)
        y = (self.g + e + self.p) & M32
        x = (2 * self.B + 1 - y - L) & M32 if r else y
        return self.copy(x, L, bool(r))

    def records(self):
        return np.array(self.rows, dtype=FACTOR_DTYPE)


def random_archive(rng, block, z, p_literal=0.2, p_continue=0.5, max_length=300, with_rc=True, alphabet=b"ACGT",
                   boundary=None):
    """z records over `block` (rng: random.Random): literals, copies that continue the last diagonal, copies placed
    anywhere on either strand -> (records, literals, target lengths); a target ends behind every record whose index
    + 1 is a multiple of `boundary` (None: at random, with empty targets)"""
    b = Builder(block)
    lengths, last_end = [], 0
    for i in range(z):
        u = rng.random()
        L = min(rng.choice((1, 1, 2, 7, 40, 255, 256, max_length)), max_length, b.B)
        if u < p_literal:
            b.literal(bytes([rng.choice(alphabet)]))
        else:
            placed = False
            if u < p_literal + p_continue and any(c is not None for c in b.codes):
                y = (b.g + b.p) & M32
                x = (2 * b.B + 1 - y - L) & M32 if b.r else y
                if x + L <= b.B:
                    b.copy(x, L, bool(b.r))
                    placed = True
            if not placed:
                b.copy(rng.randrange(0, b.B - L + 1), L, with_rc and rng.random() < 0.4)
        cut = (i + 1) % boundary == 0 if boundary else rng.random() < 0.1
        if cut:
            lengths.append(b.p - last_end)
            last_end = b.p
            if not boundary and rng.random() < 0.2:
                lengths.append(0)
    lengths.append(b.p - last_end)
    return b.records(), bytes(b.literals), lengths

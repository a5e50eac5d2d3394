"""Relative Lempel-Ziv against a reference block (extension; DESIGN.md 5, "Relative LZ against a reference block").

Every target is factorized against the reference records and nothing else: no target copies from another target or
from itself, so a target's parse does not depend on the order of the collection.  One suffix sort over
reference + all targets serves them all.  The reference package has no such mode; it sits next to
factorize_dna_w_reference_seq and factorize_dna_rc_w_ref_fasta_files.

Semantics at position p of target T (Rblk = the reference records joined by one separator each):
Lf = the longest prefix of T[p:] that occurs in Rblk, Lr = the longest whose reverse complement does (0 without
with_rc).  Neither: a literal of length 1.  Lf >= Lr: a forward factor, ref = the leftmost occurrence in Rblk.
Otherwise a reverse-complement factor, ref = the leftmost occurrence of the reverse complement in Rblk.

RlzIndex keeps the suffix structures of the reference on the GPU and matches target batches against them by search: the
same records, the reference sorted once, and no limit on the number of targets.
"""
import operator
import struct

import numpy as np

from .. import _noLZSS as _native

RLZ_DTYPE = np.dtype([("start", "<u8"), ("length", "<u8"), ("ref", "<u8"), ("is_rc", "?"), ("is_literal", "?")])
TARGET_HIT_DTYPE = _native.TARGET_HIT_DTYPE  # (target, position, is_rc, primary): RlzArchiveFinder.locate
HIT_DTYPE = _native.HIT_DTYPE  # (position, record, is_rc): an occurrence of a pattern (RlzIndex.locate)
SEED_DTYPE = _native.SEED_DTYPE  # (target, start, length, count): a maximal exact match of a target (RlzIndex.seeds)
REPEAT_DTYPE = _native.REPEAT_DTYPE  # (position, length, count, record, palindrome): a maximal repeat (RlzIndex.repeats)
CHAIN_DTYPE = _native.CHAIN_DTYPE  # a seed chain: one placement of a target in a record and strand (RlzIndex.seed_chains)
CHAIN_ANCHOR_DTYPE = _native.CHAIN_ANCHOR_DTYPE  # (t_start, position, length): one anchor of a seed chain
ALIGN_DTYPE = _native.ALIGN_DTYPE  # the base-level alignment of one seed chain (RlzIndex.align)
ALIGN_LANES = _native.ALIGN_LANES  # diagonals of an alignment job: bandwidth + 2 * band + 1 must not exceed it
VARIANT_DTYPE = _native.VARIANT_DTYPE  # an allele that passed RlzPileup.variants
INSERTION_DTYPE = _native.INSERTION_DTYPE  # an inserted allele that passed RlzPileup.insertions
insertion_bases = _native.insertion_bases  # the bases such a record keeps, as bytes
COHORT_SITE_DTYPE = _native.COHORT_SITE_DTYPE  # a position that varies among the samples of a cohort (RlzCohort.sites)
PILEUP_CHANNELS = _native.PILEUP_CHANNELS  # ("A", "C", "G", "T", "DEL", "INS", "REV", "BREAK"): the columns of RlzPileup.counts
CIGAR_LETTERS = {1: "I", 2: "D", 7: "=", 8: "X"}  # BAM's op codes, as RlzIndex.align reports them
MAX_CHAIN_TARGETS = 1 << 24  # targets per batch of a seed-chain query: the group sort key keeps the target in 24 bits


def cigar_string(ops):
    """The ops of one alignment (uint32: length << 4 | code, as RlzIndex.align returns them in `ops`) as a CIGAR string
    with the extended letters: `=` match, X mismatch, I a target base without a reference base, D the reverse."""
    return "".join(f"{int(op) >> 4}{CIGAR_LETTERS[int(op) & 15]}" for op in np.asarray(ops, dtype=np.uint32))


def split_and_rebase(records, target_offsets, target_lengths):
    """Absolute records (start, length, ref with RC_MASK; a literal has ref == start) in ascending start order, the
    sentinel literals between the targets among them -> one RLZ_DTYPE array per target: start relative to the target,
    ref a reference-block coordinate with the mask stripped (0 for a literal).  Pure numpy, no device."""
    records = np.asarray(records, dtype=_native.FACTOR_DTYPE)
    starts = records["start"]
    out = []
    for off, length in zip(target_offsets, target_lengths):
        lo, hi = np.searchsorted(starts, [off, off + length], side="left")
        out.append(rebase(records[lo:hi], off))
    return out


def rebase(records, offset):
    """The records of ONE target (absolute coordinates) -> RLZ_DTYPE relative to the target that starts at offset."""
    records = np.asarray(records, dtype=_native.FACTOR_DTYPE)
    res = np.zeros(len(records), dtype=RLZ_DTYPE)
    ref = records["ref"]
    literal = ref == records["start"]
    res["start"] = records["start"] - np.uint64(offset)
    res["length"] = records["length"]
    res["is_literal"] = literal
    res["is_rc"] = ~literal & ((ref >> np.uint64(63)) != 0)
    res["ref"] = np.where(literal, np.uint64(0), ref & np.uint64(_native.RC_MASK - 1))
    return res


def rlz_factorize(reference, targets, with_rc: bool = True):
    """reference: one sequence or a list of sequences; targets: a list of sequences -> one RLZ_DTYPE array per target
    (start target-relative, length, ref in reference-block coordinates, is_rc, is_literal)."""
    res = _native.rlz_factorize_arrays(reference, targets, with_rc=with_rc, want_factors=True)
    return [rebase(f, off) for f, off in zip(res["factors"], res["target_offsets"])]


def rlz_count_factors(reference, targets, with_rc: bool = True):
    """Factors per target; only the counts leave the device."""
    return _native.rlz_factorize_arrays(reference, targets, with_rc=with_rc, want_factors=False)["counts"]


def rlz_factorize_fasta(reference_fasta, target_fasta, with_rc: bool = True, sanitize_mode: str = "remove_ambiguous",
                        want_factors: bool = True):
    """The records of reference_fasta as the reference block, every record of target_fasta as a target ->
    dict(reference_ids, target_ids, target_lengths, counts, factors: as rlz_factorize, or None)."""
    res = _native.rlz_factorize_fasta_arrays(str(reference_fasta), str(target_fasta), with_rc=with_rc,
                                             sanitize_mode=sanitize_mode, want_factors=want_factors)
    factors = None
    if want_factors:
        factors = [rebase(f, off) for f, off in zip(res["factors"], res["target_offsets"])]
    return {"reference_ids": res["reference_ids"], "target_ids": res["target_ids"],
            "target_lengths": res["target_lengths"], "counts": res["counts"], "factors": factors}


def rlz_summary(result):
    """result: the list rlz_factorize returns (or the "factors" of rlz_factorize_fasta) -> per target a dict(factors,
    forward_bases, rc_bases, literal_bases); host arrays only."""
    out = []
    for f in result:
        f = np.asarray(f, dtype=RLZ_DTYPE)
        length = f["length"].astype(np.uint64)
        lit, rc = f["is_literal"], f["is_rc"]
        out.append({"factors": int(len(f)),
                    "forward_bases": int(length[~lit & ~rc].sum()),
                    "rc_bases": int(length[~lit & rc].sum()),
                    "literal_bases": int(length[lit].sum())})
    return out


SEPARATOR = b"\x01"  # between the records of the reference block that rlz_decode builds: any byte but A/C/G/T


def _upper_bytes(seq):
    return (seq.encode("ascii") if isinstance(seq, str) else bytes(seq)).upper()


def rlz_literals(targets, factors):
    """targets, and what rlz_factorize returned for them -> per target the symbols of its literal factors in factor
    order (upper case, as the factorization reads the targets).  With `factors`, all rlz_decode needs."""
    out = []
    for t, f in zip(targets, factors):
        f = np.asarray(f, dtype=RLZ_DTYPE)
        sym = np.frombuffer(_upper_bytes(t), dtype=np.uint8)
        out.append(sym[f["start"][f["is_literal"]].astype(np.int64)].tobytes())
    return out


def absolute_records(reference, factors):
    """The reference block, and the per-target RLZ_DTYPE arrays laid end to end behind it as ONE array of absolute
    (start, length, ref with RC_MASK) records -> (block bytes, records, target lengths).  Raises ValueError if a copy
    factor's [ref, ref + length) touches a separator or leaves the block.  Pure numpy, no device."""
    if isinstance(reference, (str, bytes, bytearray)):
        reference = [reference]
    refs = [_upper_bytes(r) for r in reference]
    block = SEPARATOR.join(refs)
    separators = np.cumsum([len(r) + 1 for r in refs[:-1]], dtype=np.int64) - 1  # ascending positions in the block
    parts, lengths = [], []
    at = len(block)
    for j, f in enumerate(factors):
        f = np.asarray(f, dtype=RLZ_DTYPE)
        rec = np.zeros(len(f), dtype=_native.FACTOR_DTYPE)
        start = f["start"] + np.uint64(at)
        copy = ~f["is_literal"]
        ref, length = f["ref"].astype(np.int64), f["length"].astype(np.int64)
        nxt = np.searchsorted(separators, ref, side="left")  # the first separator at or behind ref
        nxt_pos = np.append(separators, len(block))[nxt]
        bad = copy & ((ref + length > len(block)) | (nxt_pos < ref + length))
        if bad.any():
            k = int(np.flatnonzero(bad)[0])
            raise ValueError(f"target {j}, factor {k}: [ref, ref + length) = [{int(ref[k])}, {int(ref[k] + length[k])}) "
                             f"touches a separator or leaves the reference block of {len(block)} bytes")
        rec["start"], rec["length"] = start, f["length"]
        rec["ref"] = np.where(copy, f["ref"] | np.where(f["is_rc"], np.uint64(_native.RC_MASK), np.uint64(0)), start)
        parts.append(rec)
        n = int(f["start"][-1] + f["length"][-1]) if len(f) else 0
        lengths.append(n)
        at += n
    records = np.concatenate(parts) if parts else np.zeros(0, dtype=_native.FACTOR_DTYPE)
    return block, records, lengths


def rlz_decode(reference, factors, literals, return_info: bool = False):
    """The targets back from their relative-LZ factors: `reference` as given to rlz_factorize, `factors` the list it
    returned, `literals` the list rlz_literals returned -> one bytes object per target (b"" for an empty one).  ONE
    decode on the GPU for all targets: the reference block is the known prefix and every copy resolves in one hop.
    return_info: also the info dict of that call."""
    block, records, lengths = absolute_records(reference, factors)
    text, info = _native.decode_array(records, b"".join(bytes(x) for x in literals), prefix=block)
    out, at = [], len(block)
    for n in lengths:
        out.append(text[at:at + n].tobytes())
        at += n
    return (out, info) if return_info else out


ARCHIVE_ARRAYS = ("block", "records", "literals", "target_lengths", "ids", "has_ids")


def archive_arrays(block, records, literals, target_lengths, ids=None):
    """The host form of an archive -> dict of numpy arrays (block and literals uint8, records FACTOR_DTYPE, target
    lengths uint64, ids as a fixed-width bytes array, has_ids), checked for consistent sizes.  ValueError otherwise.
    No device."""
    block = np.frombuffer(bytes(block), dtype=np.uint8)
    literals = np.frombuffer(bytes(literals), dtype=np.uint8)
    records = np.ascontiguousarray(records)
    if records.dtype != _native.FACTOR_DTYPE or records.ndim != 1:
        raise ValueError("records must be a one-dimensional FACTOR_DTYPE array")
    lengths = np.asarray(target_lengths)
    if lengths.size and (lengths.ndim != 1 or lengths.dtype.kind not in "iu" or (lengths.dtype.kind == "i" and
                                                                                  (lengths < 0).any())):
        raise ValueError("target_lengths must be a one-dimensional array of non-negative integers")
    lengths = np.ascontiguousarray(lengths.reshape(-1), dtype=np.uint64)
    covered = int(records["start"][-1] + records["length"][-1]) - len(block) if len(records) else 0
    if int(lengths.sum(dtype=np.uint64)) != covered:
        raise ValueError(f"inconsistent sizes: the target lengths sum to {int(lengths.sum(dtype=np.uint64))} and the "
                         f"records cover {covered} bytes behind the block of {len(block)}")
    n_lit = int((records["ref"] == records["start"]).sum())
    if n_lit != len(literals):
        raise ValueError(f"inconsistent sizes: {n_lit} literal records and {len(literals)} literal symbols")
    if ids is None:
        id_arr = np.zeros(0, dtype="S1")
    else:
        names = [i.encode("utf-8") if isinstance(i, str) else bytes(i) for i in ids]
        if len(names) != len(lengths):
            raise ValueError(f"inconsistent sizes: {len(names)} ids for {len(lengths)} targets")
        if len(set(names)) != len(names):
            raise ValueError("ids must be distinct")
        if any(name.endswith(b"\0") for name in names):
            raise ValueError("an id must not end in a NUL byte")
        id_arr = np.array(names, dtype=f"S{max([len(x) for x in names] + [1])}")
    return {"block": block, "records": records, "literals": literals, "target_lengths": lengths, "ids": id_arr,
            "has_ids": np.array(ids is not None)}


def save_archive_arrays(path, arrays):
    """One .npz (numpy.savez, raw) of what archive_arrays returned.  No device."""
    with open(path, "wb") as fh:
        np.savez(fh, **{k: arrays[k] for k in ARCHIVE_ARRAYS})


def load_archive_arrays(path):
    """-> (block bytes, records, literals bytes, target lengths, ids or None) of a file save_archive_arrays wrote;
    ValueError for missing arrays, wrong types or inconsistent sizes.  allow_pickle is off.  No device."""
    try:
        with np.load(path, allow_pickle=False) as npz:
            a = {k: npz[k] for k in ARCHIVE_ARRAYS if k in npz.files}
    except Exception as e:  # (a truncated or foreign file, pickled object arrays)
        raise ValueError(f"{path}: not a relative-LZ archive ({e})")
    missing = [k for k in ARCHIVE_ARRAYS if k not in a]
    if missing:
        raise ValueError(f"{path}: not a relative-LZ archive, missing arrays {missing}")
    if a["block"].dtype != np.uint8 or a["literals"].dtype != np.uint8 or a["block"].ndim != 1 or a["literals"].ndim != 1:
        raise ValueError(f"{path}: block and literals must be one-dimensional uint8 arrays")
    if a["ids"].dtype.kind != "S" or a["ids"].ndim != 1 or a["has_ids"].shape != () or a["has_ids"].dtype != np.bool_:
        raise ValueError(f"{path}: ids must be a one-dimensional fixed-width bytes array and has_ids a flag")
    if a["target_lengths"].dtype != np.uint64:
        raise ValueError(f"{path}: target_lengths must be a uint64 array")
    ids = [bytes(x).decode("utf-8") for x in a["ids"]] if bool(a["has_ids"]) else None
    chk = archive_arrays(a["block"].tobytes(), a["records"], a["literals"].tobytes(), a["target_lengths"], ids)
    return chk["block"].tobytes(), chk["records"], chk["literals"].tobytes(), chk["target_lengths"], ids


# ---- the compact container ("Relative-LZ archive: the compact container"; the format:
# include/nolzss_hip.h, nolzss_rlz_archive_pack) -------------------------------------------------------------------
PACKED_MAGIC = b"noLZRLZ1"
_PACKED_HEADER = struct.Struct("<8sII12Q")  # magic, version, flags, B, k, z, n_literals, decoded, separators, 6 sizes
_PACKED_SECTIONS = ("block", "control", "data", "literals")


def _packed_ids(ids, k):
    """The id rules of archive_arrays -> the ids section (k + 1 uint64 offsets, then the UTF-8 bytes)"""
    names = [i.encode("utf-8") if isinstance(i, str) else bytes(i) for i in ids]
    if len(names) != k:
        raise ValueError(f"inconsistent sizes: {len(names)} ids for {k} targets")
    if len(set(names)) != len(names):
        raise ValueError("ids must be distinct")
    if any(name.endswith(b"\0") for name in names):
        raise ValueError("an id must not end in a NUL byte")
    offsets = np.zeros(k + 1, dtype="<u8")
    np.cumsum([len(x) for x in names], out=offsets[1:])
    return offsets.tobytes() + b"".join(names)


def _packed_section_sizes(s):
    """The byte sizes the counts of the sections ask for: (block, control, literals); data is free"""
    B, nlit = s["block_length"], s["n_literals"]
    return ((B + 3) // 4 + 4 * s["num_separators"] if s["block_mode"] else B, (s["z"] + 1) // 2,
            (nlit + 3) // 4 if s["literal_mode"] else nlit)


def write_packed_archive(path, sections, target_lengths, ids=None):
    """One compact container file of what RlzArchiveHandle.pack returned (a dict: block_mode, literal_mode,
    block_length, z, n_literals, decoded, num_separators and the bytes of block, control, data, literals), the target
    lengths and the ids (None: the file carries none; the rules of archive_arrays).  ValueError for sizes that do not
    fit the counts.  No device."""
    s = sections
    lengths = np.ascontiguousarray(np.asarray(target_lengths).reshape(-1), dtype="<u8")
    want = _packed_section_sizes(s)
    have = (len(s["block"]), len(s["control"]), len(s["literals"]))
    if have != want or (not s["block_mode"] and s["num_separators"]):
        raise ValueError(f"inconsistent sizes: block, control and literal sections of {have} bytes, the counts ask for {want}")
    if sum(lengths.tolist()) != s["decoded"]:  # (exact: a uint64 sum could wrap)
        raise ValueError(f"inconsistent sizes: the target lengths sum to {sum(lengths.tolist())} and the records cover "
                         f"{s['decoded']} bytes behind the block")
    parts = [lengths.tobytes(), b"" if ids is None else _packed_ids(ids, len(lengths))] + [bytes(s[n]) for n in _PACKED_SECTIONS]
    flags = (1 if s["block_mode"] else 0) | (2 if s["literal_mode"] else 0) | (0 if ids is None else 4)
    head = _PACKED_HEADER.pack(PACKED_MAGIC, 1, flags, s["block_length"], len(lengths), s["z"], s["n_literals"],
                               s["decoded"], s["num_separators"], *[len(x) for x in parts])
    with open(path, "wb") as fh:
        fh.write(head)
        for x in parts:
            fh.write(x)
            fh.write(b"\0" * (-len(x) % 8))


def read_packed_archive(path):
    """-> (sections, target lengths as a uint64 array, ids or None) of a file write_packed_archive wrote.  The container
    is checked here -- magic, version, flags, every section inside the file and of the size the counts ask for, zero
    padding, nothing behind the last section, the id table --, ValueError otherwise; what the sections SAY is checked on
    the device at open.  No device."""
    with open(path, "rb") as fh:
        raw = fh.read()

    def bad(why):
        return ValueError(f"{path}: not a compact relative-LZ archive ({why})")

    if len(raw) < _PACKED_HEADER.size or raw[:8] != PACKED_MAGIC:
        raise bad("bad magic")
    f = _PACKED_HEADER.unpack_from(raw)
    version, flags, B, k, z, nlit, decoded, seps = f[1:9]
    sizes = f[9:]
    if version != 1:
        raise bad(f"version {version}, this reader knows version 1")
    if flags & ~7:
        raise bad(f"unknown flags {flags:#x}")
    at, parts = _PACKED_HEADER.size, []
    for name, n in zip(("target lengths", "ids") + _PACKED_SECTIONS, sizes):
        end = at + n + (-n % 8)
        if end > len(raw):
            raise bad(f"the {name} section ends behind the end of the file")
        if any(raw[at + n:end]):
            raise bad(f"non-zero padding behind the {name} section")
        parts.append(raw[at:at + n])
        at = end
    if at != len(raw):
        raise bad(f"{len(raw) - at} bytes behind the last section")
    if sizes[0] != 8 * k:
        raise bad(f"{sizes[0]} bytes of target lengths for {k} targets")
    lengths = np.frombuffer(parts[0], dtype="<u8").astype(np.uint64)
    ids = None
    if flags & 4:
        if sizes[1] < 8 * (k + 1):
            raise bad("the ids section is shorter than its offsets")
        offs = np.frombuffer(parts[1], dtype="<u8", count=k + 1).tolist()
        names = parts[1][8 * (k + 1):]
        if offs[0] != 0 or offs[-1] != len(names) or any(offs[j] > offs[j + 1] for j in range(k)):
            raise bad("the id offsets do not tile the id bytes")
        try:
            ids = [names[offs[j]:offs[j + 1]].decode("utf-8") for j in range(k)]
        except UnicodeDecodeError as e:
            raise bad(f"an id is not UTF-8: {e}")
        _packed_ids(ids, k)
    elif sizes[1]:
        raise bad("an ids section in a file without ids")
    s = {"block_mode": flags & 1, "literal_mode": (flags >> 1) & 1, "block_length": B, "z": z, "n_literals": nlit,
         "decoded": decoded, "num_separators": seps, "block": parts[2], "control": parts[3], "data": parts[4],
         "literals": parts[5]}
    if (len(s["block"]), len(s["control"]), len(s["literals"])) != _packed_section_sizes(s) or (not s["block_mode"] and seps):
        raise bad("the block, control or literal section has not the size the counts ask for")
    if sum(lengths.tolist()) != decoded:  # (exact: a uint64 sum could wrap)
        raise bad(f"the target lengths do not sum to the {decoded} decoded bytes of the header")
    return s, lengths, ids


class RlzArchive:
    """A relative-LZ collection resident on the GPU: the reference block and the records of every target stay in device
    memory, and any batch of (target, lo, hi) ranges comes back as bytes with one kernel launch -- nothing the caller
    did not ask for is decoded or crosses PCIe ("Relative-LZ archive: ranges from resident records").
    Targets are addressed by index, or by id when ids were given.  A context manager; use after close() raises
    ValueError."""

    def __init__(self, block, records, literals, target_lengths, ids=None, device=None):
        self._bound = None  # (the RlzIndex of an archive made by from_index)
        self._arrays = archive_arrays(block, records, literals, target_lengths, ids)
        self.ids = None if ids is None else [i if isinstance(i, str) else bytes(i).decode("utf-8") for i in ids]
        self._index = target_index_map(self.ids)
        previous = _native.get_device()
        if device is not None:
            _native.set_device(device)
        try:
            self._handle = _native.RlzArchiveHandle.open_records(
                self._arrays["block"], self._arrays["records"], self._arrays["literals"], self._arrays["target_lengths"])
        finally:
            _native.set_device(previous)

    @classmethod
    def build(cls, reference, targets, with_rc: bool = True, ids=None):
        """rlz_factorize + rlz_literals + absolute_records + open: the records make one PCIe round trip here."""
        factors = rlz_factorize(reference, targets, with_rc=with_rc)
        return cls.from_factors(reference, factors, rlz_literals(targets, factors), ids=ids)

    @classmethod
    def from_factors(cls, reference, factors, literals, ids=None):
        """reference as given to rlz_factorize, and what rlz_factorize and rlz_literals returned."""
        block, records, lengths = absolute_records(reference, factors)
        return cls(block, records, b"".join(bytes(x) for x in literals), lengths, ids=ids)

    @classmethod
    def load(cls, path, device=None):
        """The file save() wrote; it is checked on the host (ValueError) before the device is touched.  A file that
        begins with the magic of the compact container (save(path, compact=True)) goes up as it is and is expanded and
        checked on the device; every other file is the .npz."""
        try:
            with open(path, "rb") as fh:
                magic = fh.read(len(PACKED_MAGIC))
        except OSError:  # (the existing way reports a file that cannot be read)
            magic = b""
        if magic != PACKED_MAGIC:
            block, records, literals, lengths, ids = load_archive_arrays(path)
            return cls(block, records, literals, lengths, ids=ids, device=device)
        sections, lengths, ids = read_packed_archive(path)
        self = cls.__new__(cls)
        self._handle, self._arrays, self._bound = None, None, None
        self.ids = ids
        self._index = target_index_map(self.ids)
        previous = _native.get_device()
        if device is not None:
            _native.set_device(device)
        try:
            self._handle = _native.RlzArchiveHandle.open_packed(sections, lengths)
        finally:
            _native.set_device(previous)
        return self

    @classmethod
    def from_index(cls, index, ids=None):
        """An empty archive bound to an RlzIndex, on its device: append() matches batches against the index and keeps
        their records on the GPU ("Relative-LZ archive: batches appended from the index").  ids=[]: the
        archive carries ids and every append must name its targets; None: it does not."""
        if ids is not None and len(ids):
            raise ValueError("from_index opens an empty archive: ids must be None or empty, append() takes the ids")
        self = cls.__new__(cls)
        self._handle, self._arrays, self._bound = None, None, index
        self.ids = None if ids is None else []
        self._index = {}
        self._handle = _native.RlzArchiveHandle.open_index(index._live())
        return self

    def append(self, targets, ids=None, batch_bases=None):
        """Match `targets` against the index of from_index and append them, batch by batch (_plan_append_batches) ->
        the list of the per-batch info dicts (targets_added, records_added, literals_added, bases_added, num_targets, z,
        total_length, capacity_records, device_bytes, reallocated).  ids: one per target exactly when the archive
        carries ids, distinct from each other and from those present.  ValueError before any device work otherwise.  If
        a later batch fails, the batches before it stay appended."""
        h = self._live()
        if self._bound is None:  # (host records, or a loaded file: neither is bound to an index)
            raise ValueError("append needs an archive made by RlzArchive.from_index: this one was built from host records")
        targets = list(targets)
        names = _check_append_ids(self.ids, ids, len(targets))
        ih = self._bound._live()
        plan = _plan_append_batches([len(t) for t in targets], h.info["block_length"], h.info["total_length"], MAX_TEXT,
                                    batch_bases)
        out = []
        for lo, hi in plan:
            out.append(h.append_index(ih, targets[lo:hi]))
            if names is not None:
                for name in names[lo:hi]:
                    self._index[name] = len(self.ids)
                    self.ids.append(name)
        return out

    def finder(self, max_pattern_length: int = 64, prefix_syms: int = 0):
        """-> RlzArchiveFinder: in which targets, and where, do patterns of up to max_pattern_length bases occur?  A
        snapshot of the archive as it is now, built on the GPU from the resident records ("Relative-LZ
        archive: locate through the parse"); after an append, open a new one.  prefix_syms as in RlzIndex.build."""
        h = self._live()
        if self._bound is None:
            raise ValueError("finder needs an archive made by RlzArchive.from_index: this one was built from host records")
        return RlzArchiveFinder(_native.RlzFinderHandle.open(h, self._bound._live(), max_pattern_length, prefix_syms))

    def save(self, path, compact: bool = False):
        """One .npz holding block, records, literals, target lengths and ids, raw.  compact=True: the compact container
        instead, packed on the device from the resident records ("Relative-LZ archive: the compact
        container"); load() reads both."""
        h = self._live()
        if compact:
            write_packed_archive(path, h.pack(), h.target_lengths, self.ids)
            return
        if self._arrays is None:  # index-built or loaded from a container: the host form comes back from the device
            block, records, literals = h.export()
            save_archive_arrays(path, archive_arrays(block, records, literals, h.target_lengths, self.ids))
            return
        save_archive_arrays(path, self._arrays)

    def _live(self):
        if self._handle is None:
            raise ValueError("the archive is closed")
        return self._handle

    def _lengths(self):
        return self._live().target_lengths if self._arrays is None else self._arrays["target_lengths"]

    def __len__(self):
        return len(self._lengths())

    @property
    def target_lengths(self):
        return [int(x) for x in self._lengths()]

    @property
    def info(self):
        return dict(self._live().info)

    def _rows(self, ranges):
        if isinstance(ranges, np.ndarray) and ranges.dtype.kind in "iu":  # (target index, lo, hi) rows as they are
            return ranges
        return [(resolve_target(t, self._index, len(self)), operator.index(lo), operator.index(hi))
                for t, lo, hi in ranges]

    def extract_array(self, ranges):
        """(target, lo, hi) triples, or an integer array of (target index, lo, hi) rows -> (uint8 array of the ranges back
        to back, uint64 offsets of len(ranges) + 1)."""
        return self._live().extract_array(self._rows(ranges))

    def extract(self, ranges):
        """(target, lo, hi) triples -> one bytes object per range; ranges may be empty, overlap, repeat, in any order."""
        data, offsets = self.extract_array(ranges)
        raw, offs = data.tobytes(), offsets.tolist()
        return [raw[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]

    def extract_device(self, ranges, data_ptr: int, capacity: int, stream: int = 0) -> int:
        """The same bytes into device memory on the archive's device (a torch tensor's data_ptr()) -> bytes written."""
        return self._live().extract_device(self._rows(ranges), data_ptr, capacity, stream)

    def fetch(self, target, lo: int, hi: int) -> bytes:
        return self.extract([(target, lo, hi)])[0]

    def target(self, j) -> bytes:
        j = resolve_target(j, self._index, len(self))
        return self.fetch(j, 0, int(self._lengths()[j]))

    def close(self) -> None:
        h, self._handle = getattr(self, "_handle", None), None
        if h is not None:
            h.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RlzArchiveFinder:
    """Pattern queries inside the targets of an RlzArchive (RlzArchive.finder).  A context manager; use after close()
    raises ValueError.  The archive and its index must stay open while it is used."""

    def __init__(self, handle):
        self._handle = handle

    def _live(self):
        if self._handle is None:
            raise ValueError("the finder is closed")
        return self._handle

    @property
    def info(self):
        """dict(num_targets, z, total_length, max_pattern_length, kernel_length, intervals, with_rc, device,
        device_bytes)"""
        return dict(self._live().info)

    @staticmethod
    def _batches(patterns):
        patterns = list(patterns)
        return patterns, plan_index_batches([len(p) for p in patterns], -1, MAX_TEXT)

    def count(self, patterns):
        """Occurrences of every pattern in the targets, both strands together (an index without reverse complement
        counts the forward strand only) -> uint64 array.  An empty pattern counts 0."""
        h = self._live()
        patterns, plan = self._batches(patterns)
        parts = [h.count(patterns[lo:hi]) for lo, hi in plan]
        return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)

    def locate(self, patterns, max_hits: int = 0):
        """Where every pattern occurs in the targets -> dict(counts, offsets, target, position, is_rc, primary).  Pattern
        j owns the hits [offsets[j], offsets[j + 1]), ascending by (target, position, is_rc): target is the 0-based
        target, position the position inside it; is_rc means the stretch equals the pattern's reverse complement;
        primary means the occurrence crosses a record start of the parse or is a literal.  A pattern with more than
        max_hits occurrences (0: no cap) reports its count and no hits."""
        h = self._live()
        patterns, plan = self._batches(patterns)
        counts, offsets, hits, base = [], [np.zeros(1, dtype=np.uint64)], [], 0
        for lo, hi in plan:
            c, o, f = h.locate(patterns[lo:hi], max_hits)
            counts.append(c)
            offsets.append(o[1:] + np.uint64(base))
            hits.append(f)
            base += int(o[-1])
        f = np.concatenate(hits) if hits else np.zeros(0, dtype=TARGET_HIT_DTYPE)
        return {"counts": np.concatenate(counts) if counts else np.zeros(0, dtype=np.uint64),
                "offsets": np.concatenate(offsets), "target": f["target"].copy(), "position": f["position"].copy(),
                "is_rc": f["is_rc"].astype(bool), "primary": f["primary"].astype(bool)}

    def kernel(self):
        """Test hook -> (K bytes, kstart, dstart)"""
        return self._live().kernel()

    def close(self) -> None:
        h, self._handle = getattr(self, "_handle", None), None
        if h is not None:
            h.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


MAX_TEXT = 0xffffffff - (1 << 19)  # positions the 32-bit device pipeline takes (kMaxText of the library)


def plan_index_batches(lengths, block_length, limit=MAX_TEXT, batch_bases=None, max_targets=None):
    """Target lengths -> [(lo, hi)] index ranges of the batches RlzIndex sends, greedy in input order: a batch closes
    when the next target would pass the length rule block_length + 1 + sum(len) + k <= limit, batch_bases bases, or
    max_targets targets (the seed chains: MAX_CHAIN_TARGETS).  A target that breaks a bound alone still gets a batch of
    its own (the library refuses it if it breaks the length rule).  Pure Python, no device."""
    out, lo, bases = [], 0, 0
    for j, n in enumerate(lengths):
        n = operator.index(n)
        k = j - lo
        over = (block_length + 1 + bases + n + k + 1 > limit or (batch_bases is not None and bases + n > batch_bases)
                or (max_targets is not None and k + 1 > max_targets))
        if k and over:
            out.append((lo, j))
            lo, bases = j, 0
        bases += n
    if len(lengths) > lo:
        out.append((lo, len(lengths)))
    return out


def _plan_append_batches(lengths, block_length, decoded, limit=MAX_TEXT, batch_bases=None):
    """Target lengths -> [(lo, hi)] index ranges of the batches an archive that holds `decoded` bytes takes, greedy in
    input order: a batch closes when the next target would pass the length rule block_length + 1 + sum(len) + k <=
    limit, batch_bases bases, or the room left under the limit, decoded + (everything planned so far) + n <= limit.  A
    target that breaks a bound alone still gets a batch of its own (the library refuses it).  Pure Python, no device."""
    out, lo, bases, room = [], 0, 0, limit - decoded
    for j, n in enumerate(lengths):
        n = operator.index(n)
        k = j - lo
        over = (block_length + 1 + bases + n + k + 1 > limit or (batch_bases is not None and bases + n > batch_bases)
                or bases + n > room)
        if k and over:
            out.append((lo, j))
            room -= bases
            lo, bases = j, 0
        bases += n
    if len(lengths) > lo:
        out.append((lo, len(lengths)))
    return out


def _check_append_ids(present, ids, count):
    """The id rules of RlzArchive.append: `present` is the archive's id list (None: it carries none), ids what the call
    got for its `count` targets -> the new ids as str (None without ids).  ValueError otherwise.  Pure Python."""
    if present is None:
        if ids is not None:
            raise ValueError("this archive carries no ids: append takes none")
        return None
    if ids is None:
        raise ValueError("this archive carries ids: append needs one per target")
    raw = [i.encode("utf-8") if isinstance(i, str) else bytes(i) for i in ids]
    if len(raw) != count:
        raise ValueError(f"inconsistent sizes: {len(raw)} ids for {count} targets")
    if any(name.endswith(b"\0") for name in raw):
        raise ValueError("an id must not end in a NUL byte")
    names = [name.decode("utf-8") for name in raw]
    if len(set(names)) != len(names):
        raise ValueError("ids must be distinct")
    taken = set(present) & set(names)
    if taken:
        raise ValueError(f"ids must be distinct: {sorted(taken)[0]!r} is in the archive already")
    return names


class RlzIndex:
    """The suffix structures of a reference block resident on the GPU: target batches are matched against them by
    search, so the reference is sorted once, a match sorts nothing, and the number of targets is bounded by the length
    rule alone -- not by the 250 sentinels of rlz_factorize ("Relative-LZ index: targets matched against a
    resident reference").  Results equal rlz_factorize record for record.  A context manager; use after close() raises
    ValueError."""

    def __init__(self, handle, reference):
        self._handle, self._reference = handle, reference

    @classmethod
    def build(cls, reference, with_rc: bool = True, prefix_syms: int = 0, device=None):
        """reference: one sequence or a list of sequences.  prefix_syms: bases of the prefix table's key (0: chosen
        from the index length)."""
        if isinstance(reference, (str, bytes, bytearray)):
            reference = [reference]
        reference = list(reference)
        return cls(cls._open(device, _native.RlzIndexHandle.open, reference, with_rc=with_rc, prefix_syms=prefix_syms),
                   reference)

    @classmethod
    def from_fasta(cls, path, with_rc: bool = True, sanitize_mode: str = "remove_ambiguous", prefix_syms: int = 0,
                   device=None):
        """Every record of the FASTA file is a reference record."""
        handle = cls._open(device, _native.RlzIndexHandle.open_fasta, str(path), with_rc=with_rc,
                           sanitize_mode=sanitize_mode, prefix_syms=prefix_syms)
        return cls(handle, [seq for _, seq in _native.debug_parse_fasta(str(path), sanitize_mode)])

    @staticmethod
    def _open(device, opener, *args, **kwargs):
        previous = _native.get_device()
        if device is not None:
            _native.set_device(device)
        try:
            return opener(*args, **kwargs)
        finally:
            _native.set_device(previous)

    def _live(self):
        if self._handle is None:
            raise ValueError("the index is closed")
        return self._handle

    def info(self):
        """dict(num_references, block_length, index_length, with_rc, device, prefix_syms, device_bytes)"""
        return dict(self._live().info)

    def _batches(self, targets, batch_bases, want_factors):
        h = self._live()
        targets = list(targets)
        plan = plan_index_batches([len(t) for t in targets], h.info["block_length"], MAX_TEXT, batch_bases)
        return [h.factorize_arrays(targets[lo:hi], want_factors=want_factors) for lo, hi in plan]

    def factorize(self, targets, batch_bases=None):
        """What rlz_factorize returns for the reference and these targets: one RLZ_DTYPE array per target, in input
        order.  A long list goes up in several batches (plan_index_batches)."""
        return [rebase(f, off) for res in self._batches(targets, batch_bases, True)
                for f, off in zip(res["factors"], res["target_offsets"])]

    def count_factors(self, targets, batch_bases=None):
        """Factors per target; only the counts leave the device."""
        return [c for res in self._batches(targets, batch_bases, False) for c in res["counts"]]

    def codes(self, targets):
        """One batch: the code (length, bit 31 = reverse complement, 0 = no match) of every position of
        T1 s T2 s .. Tk s; only target positions are specified."""
        return self._live().codes(list(targets))

    def _pattern_batches(self, patterns):
        # the length rule of a pattern batch is sum(len) + q <= MAX_TEXT: the greedy rule of the targets without a block
        patterns = list(patterns)
        return patterns, plan_index_batches([len(p) for p in patterns], -1, MAX_TEXT)

    def count(self, patterns):
        """Occurrences of every pattern in the reference, both strands together (an index without reverse complement
        counts the forward strand only) -> uint64 array.  Patterns are nucleotide strings, case-insensitive; an empty
        one counts 0.  A long list goes up in several batches."""
        h = self._live()
        patterns, plan = self._pattern_batches(patterns)
        parts = [h.count(patterns[lo:hi]) for lo, hi in plan]
        return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)

    def locate(self, patterns, max_hits: int = 0):
        """Where every pattern occurs in the reference -> dict(counts, offsets, position, record, record_offset, is_rc).
        Pattern j owns the hits [offsets[j], offsets[j + 1]), ascending by (position, is_rc), forward first: position is
        the coordinate in the reference block, record the 0-based reference record, record_offset the position inside
        that record; a reverse-strand hit (is_rc) means the stretch at position equals the pattern's reverse complement.
        A pattern with more than max_hits occurrences (0: no cap) reports its count and no hits.  Sorted on the GPU; a
        long list goes up in several batches, the offsets stitched."""
        h = self._live()
        patterns, plan = self._pattern_batches(patterns)
        counts, offsets, hits, base = [], [np.zeros(1, dtype=np.uint64)], [], 0
        for lo, hi in plan:
            c, o, f = h.locate(patterns[lo:hi], max_hits)
            counts.append(c)
            offsets.append(o[1:] + np.uint64(base))
            hits.append(f)
            base += int(o[-1])
        f = np.concatenate(hits) if hits else np.zeros(0, dtype=HIT_DTYPE)
        starts = np.cumsum([0] + [len(r) + 1 for r in self._reference[:-1]], dtype=np.uint64)  # of every record in Rblk
        return {"counts": np.concatenate(counts) if counts else np.zeros(0, dtype=np.uint64),
                "offsets": np.concatenate(offsets), "position": f["position"].copy(), "record": f["record"].copy(),
                "record_offset": f["position"] - starts[f["record"]], "is_rc": f["is_rc"].astype(bool)}

    def seeds(self, targets, min_length: int = 1, max_hits: int = 0):
        """The maximal exact matches of every target with the reference, and where they occur -> dict(target, start,
        length, counts, offsets, position, record, record_offset, is_rc).  A seed is a stretch [start, start + length) of
        target `target` that occurs in the reference (on either strand with reverse complement) and cannot be extended
        by one base to either side inside its target and still occur; the seeds ascend by (target, start).  Only seeds
        of at least min_length bases are reported (the filter never makes a shorter neighbour maximal).  counts[j] = the
        occurrences of seed j on both strands; seed j owns the hits [offsets[j], offsets[j + 1]), laid out and sorted as
        locate lays out the hits of a pattern; a seed with more than max_hits occurrences (0: no cap) reports its count
        and no hits.  The batch is searched once on the GPU and no per-position array comes down; a long list goes up in
        several batches (plan_index_batches, a target is never split), target indices and offsets stitched."""
        h = self._live()
        min_length, max_hits = operator.index(min_length), operator.index(max_hits)
        if min_length < 0:
            raise ValueError("min_length must not be negative")
        if max_hits < 0:
            raise ValueError("max_hits must not be negative")
        targets = list(targets)
        plan = plan_index_batches([len(t) for t in targets], h.info["block_length"], MAX_TEXT)
        seeds, offsets, hits, base = [], [np.zeros(1, dtype=np.uint64)], [], 0
        for lo, hi in plan:
            s, o, f = h.seeds(targets[lo:hi], min_length, max_hits)
            s["target"] += np.uint64(lo)
            seeds.append(s)
            offsets.append(o[1:] + np.uint64(base))
            hits.append(f)
            base += int(o[-1])
        s = np.concatenate(seeds) if seeds else np.zeros(0, dtype=SEED_DTYPE)
        f = np.concatenate(hits) if hits else np.zeros(0, dtype=HIT_DTYPE)
        starts = np.cumsum([0] + [len(r) + 1 for r in self._reference[:-1]], dtype=np.uint64)  # of every record in Rblk
        return {"target": s["target"].copy(), "start": s["start"].copy(), "length": s["length"].copy(),
                "counts": s["count"].copy(), "offsets": np.concatenate(offsets), "position": f["position"].copy(),
                "record": f["record"].copy(), "record_offset": f["position"] - starts[f["record"]],
                "is_rc": f["is_rc"].astype(bool)}

    def repeat_count(self, min_length: int = 20, min_count: int = 2) -> int:
        """How many records repeats(min_length, min_count) would report: the flags are computed on the GPU and one word
        comes down.  It is how to pick min_length before asking for the records."""
        return self._live().repeat_count(min_length, min_count)

    def repeats(self, min_length: int = 20, min_count: int = 2, max_hits: int = 64):
        """The maximal repeats of the reference itself, on either strand -> dict(position, length, count, record,
        record_offset, palindrome, offsets, hit_position, hit_record, hit_record_offset, hit_is_rc).  A maximal repeat is
        a string with at least two occurrences (both strands together on an index with reverse complement) that do not
        all continue with the same base to the right, nor all to the left; a record's end is a continuation of its own.
        Reported are those of at least min_length bases and min_count occurrences.  With reverse complement w and rc(w)
        are one repeat, reported once at its leftmost forward occurrence; a string that is its own reverse complement
        has palindrome set, lists every locus on both strands, and is reported only with two loci (count >= 4).  position
        is the leftmost forward occurrence in the reference block, record and record_offset say where that lies; the
        repeats ascend by (position, length).  Repeat j owns the hits [offsets[j], offsets[j + 1]), every occurrence laid
        out and sorted as locate lays out the hits of a pattern; a repeat with more than max_hits occurrences (0: no
        cap) reports its count and no hits.  Everything is read off the resident arrays on the GPU; nothing goes up."""
        r, offsets, f = self._live().repeats(min_length, min_count, max_hits)
        starts = np.cumsum([0] + [len(x) + 1 for x in self._reference[:-1]], dtype=np.uint64)  # of every record in Rblk
        return {"position": r["position"].copy(), "length": r["length"].copy(), "count": r["count"].copy(),
                "record": r["record"].copy(), "record_offset": r["position"] - starts[r["record"]],
                "palindrome": r["palindrome"].astype(bool), "offsets": offsets, "hit_position": f["position"].copy(),
                "hit_record": f["record"].copy(), "hit_record_offset": f["position"] - starts[f["record"]],
                "hit_is_rc": f["is_rc"].astype(bool)}

    def seed_chains(self, targets, min_length: int = 15, max_hits: int = 64, max_gap: int = 5000, bandwidth: int = 500,
                    min_score: int = 40, batch_bases=None):
        """Where every target lies in the reference: its seeds (as seeds(targets, min_length, max_hits) finds them; a seed
        with more than max_hits occurrences contributes nothing) chained colinearly on the GPU, one chain per (target,
        strand, record) -> dict(target, record, is_rc, score, t_start, t_end, r_start, r_end, record_offset, num_anchors,
        primary, anchor_offsets, anchor_t_start, anchor_position, anchor_length).  Chain c covers [t_start, t_end) of
        target `target` and [r_start, r_end) of the reference block (record_offset = r_start inside record `record`); on
        the reverse strand (is_rc) the target's reverse complement lies there.  Two anchors are linked when both
        coordinates ascend, neither gap exceeds max_gap and the gaps differ by at most bandwidth; a link scores the new
        bases minus the difference of the gaps, over the 64 anchors in front of an anchor; a chain is reported when its
        score reaches min_score, and primary marks the best chain of its target.  Chain c owns the anchors
        [anchor_offsets[c], anchor_offsets[c + 1]), ascending in the target; anchor_position is the coordinate a hit of
        seeds() reports.  The chains ascend by (target, is_rc, record).  Neither seeds nor hits leave the device; a long
        list goes up in several batches (plan_index_batches, at most 2^24 targets each, a target is never split, so
        batching changes nothing), target indices and offsets stitched.  The read and its reverse complement may score
        a few points apart: the overlap term of a link is not symmetric in direction."""
        h = self._live()
        args = [operator.index(v) for v in (min_length, max_hits, max_gap, bandwidth, min_score)]
        for name, v in zip(("min_length", "max_hits", "max_gap", "bandwidth", "min_score"), args):
            if v < 0:
                raise ValueError(f"{name} must not be negative")
        targets = list(targets)
        plan = plan_index_batches([len(t) for t in targets], h.info["block_length"], MAX_TEXT, batch_bases,
                                  max_targets=MAX_CHAIN_TARGETS)
        chains, offsets, anchors, base = [], [np.zeros(1, dtype=np.uint64)], [], 0
        for lo, hi in plan:
            c, o, a, _, _ = h.seed_chains(targets[lo:hi], *args)
            c["target"] += np.uint64(lo)
            chains.append(c)
            offsets.append(o[1:] + np.uint64(base))
            anchors.append(a)
            base += int(o[-1])
        c = np.concatenate(chains) if chains else np.zeros(0, dtype=CHAIN_DTYPE)
        a = np.concatenate(anchors) if anchors else np.zeros(0, dtype=CHAIN_ANCHOR_DTYPE)
        starts = np.cumsum([0] + [len(r) + 1 for r in self._reference[:-1]], dtype=np.uint64)  # of every record in Rblk
        return {"target": c["target"].copy(), "record": c["record"].copy(), "is_rc": c["is_rc"].astype(bool),
                "score": c["score"].copy(), "t_start": c["t_start"].copy(), "t_end": c["t_end"].copy(),
                "r_start": c["r_start"].copy(), "r_end": c["r_end"].copy(),
                "record_offset": c["r_start"] - starts[c["record"]], "num_anchors": c["num_anchors"].copy(),
                "primary": c["primary"].astype(bool), "anchor_offsets": np.concatenate(offsets),
                "anchor_t_start": a["t_start"].copy(), "anchor_position": a["position"].copy(),
                "anchor_length": a["length"].copy()}

    def align(self, targets, min_length: int = 15, max_hits: int = 64, max_gap: int = 5000, bandwidth: int = 31,
              min_score: int = 40, band: int = 16, max_flank: int = 256, batch_bases=None):
        """The base-level alignment of every chain seed_chains reports at the same first five parameters, in the same
        order, computed on the GPU -> dict(target, record, is_rc, score, primary, t_start, t_end, r_start, r_end,
        record_offset, edit_distance, columns, num_ops, op_offsets, ops).  Alignment c aligns [t_start, t_end) of its
        target with [r_start, r_end) of the reference block (record_offset = r_start inside record `record`) at
        edit_distance mismatches, inserted and deleted bases, and owns ops[op_offsets[c]:op_offsets[c + 1]]: uint32
        (length << 4) | code with BAM's codes I = 1, D = 2, `=` = 7, X = 8 (cigar_string renders them), ascending in the
        target, neighbours never of one code.  On the reverse strand (is_rc) the ops still ascend in the target and
        consume the block from r_end downward, complemented.  Between consecutive anchors of a chain a banded edit
        distance runs over the diagonals within `band` of the two anchors' diagonals; the flanks beside the first and
        the last anchor are aligned end to end in the target and free in the reference, inside the record, unless
        they are longer than max_flank -- then, or when the record ends too early, the flank is clipped and t_start /
        t_end show it.  bandwidth + 2 * band + 1 must not exceed 64 (ValueError).  Batches as seed_chains does."""
        args = [operator.index(v) for v in (min_length, max_hits, max_gap, bandwidth, min_score, band, max_flank)]
        names = ("min_length", "max_hits", "max_gap", "bandwidth", "min_score", "band", "max_flank")
        for name, v in zip(names, args):
            if v < 0:
                raise ValueError(f"{name} must not be negative")
        if args[3] + 2 * args[5] + 1 > ALIGN_LANES:
            raise ValueError(f"an alignment job has at most {ALIGN_LANES} diagonals: bandwidth + 2 * band + 1 is "
                             f"{args[3]} + 2 * {args[5]} + 1; lower bandwidth or band")
        h = self._live()
        targets = list(targets)
        plan = plan_index_batches([len(t) for t in targets], h.info["block_length"], MAX_TEXT, batch_bases,
                                  max_targets=MAX_CHAIN_TARGETS)
        recs, offsets, ops, base = [], [np.zeros(1, dtype=np.uint64)], [], 0
        for lo, hi in plan:
            r, o, p, _, _ = h.align(targets[lo:hi], *args)
            r["target"] += np.uint64(lo)
            recs.append(r)
            offsets.append(o[1:] + np.uint64(base))
            ops.append(p)
            base += int(o[-1])
        r = np.concatenate(recs) if recs else np.zeros(0, dtype=ALIGN_DTYPE)
        starts = np.cumsum([0] + [len(x) + 1 for x in self._reference[:-1]], dtype=np.uint64)  # of every record in Rblk
        return {"target": r["target"].copy(), "record": r["record"].copy(), "is_rc": r["is_rc"].astype(bool),
                "score": r["score"].copy(), "primary": r["primary"].astype(bool), "t_start": r["t_start"].copy(),
                "t_end": r["t_end"].copy(), "r_start": r["r_start"].copy(), "r_end": r["r_end"].copy(),
                "record_offset": r["r_start"] - starts[r["record"]], "edit_distance": r["edit_distance"].copy(),
                "columns": r["columns"].copy(), "num_ops": r["num_ops"].copy(), "op_offsets": np.concatenate(offsets),
                "ops": np.concatenate(ops) if ops else np.zeros(0, dtype=np.uint32)}

    def pileup(self, min_length: int = 15, max_hits: int = 64, max_gap: int = 5000, bandwidth: int = 31,
               min_score: int = 40, band: int = 16, max_flank: int = 256, primary_only: bool = True,
               normalize_indels: bool = False):
        """An RlzPileup over this index: per-position counts of what read batches say, accumulated on the GPU from the
        alignments align would report at the same seven parameters (primary_only: only the best placement of every
        target counts).  normalize_indels: every deletion and insertion behind a run of matches is counted at its
        leftmost position in the block, on both strands alike -- what a consensus needs; off, the counters are the
        aligner's placements.  bandwidth + 2 * band + 1 must not exceed 64 (ValueError).  The index must stay open
        while the pileup is used."""
        params = _native._align_params(min_length, max_hits, max_gap, bandwidth, min_score, band, max_flank)
        args = [int(getattr(params, name)) for name, _ in type(params)._fields_]
        return RlzPileup(_native.RlzPileupHandle.open(self._live(), *args, normalize_indels=bool(normalize_indels)), self,
                         bool(primary_only))

    def cohort(self):
        """An RlzCohort over this index: the base calls of many pileups kept on the GPU at 3 bits per base, their
        pairwise SNP distances and the sites that vary among them.  The index must stay open while the cohort is used."""
        return RlzCohort(_native.RlzCohortHandle.open(self._live()), self)

    def archive(self, targets, ids=None):
        """RlzArchive.from_factors(reference, factors, rlz_literals(targets, factors), ids) for these targets."""
        targets = list(targets)
        factors = self.factorize(targets)
        return RlzArchive.from_factors(self._reference, factors, rlz_literals(targets, factors), ids=ids)

    def archive_on_device(self, targets, ids=None, batch_bases=None):
        """The same archive with the records kept on the GPU: RlzArchive.from_index(self) and one append of these
        targets (several batches for a long list); the archive takes further appends."""
        arc = RlzArchive.from_index(self, ids=None if ids is None else [])
        try:
            arc.append(targets, ids=ids, batch_bases=batch_bases)
        except Exception:
            arc.close()
            raise
        return arc

    def close(self) -> None:
        h, self._handle = getattr(self, "_handle", None), None
        if h is not None:
            h.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RlzPileup:
    """Pileup counts and variant sites of read batches, kept on the GPU next to an RlzIndex (RlzIndex.pileup).  Every
    add aligns a batch as RlzIndex.align would and reduces the alignments on the device: eight uint32 counters per
    position of the reference block, in the order of PILEUP_CHANNELS -- the base observed (A, C, G, T, in the block's
    forward orientation), DEL (deletion columns), INS (insertion ops anchored at the base in front of them), REV
    (columns of reverse-strand alignments over this base) and BREAK (alignment ends with a clipped read remainder).
    Depth is A + C + G + T + DEL.  Neither alignments nor ops come down; counts() and variants() bring down the table.
    insertions() reports the inserted alleles and consensus() the sample's sequence; no genotype is called.  A context manager; use after close(), or after
    the index was closed, raises ValueError."""

    def __init__(self, handle, index, primary_only):
        self._handle, self._index, self._primary_only = handle, index, primary_only

    def _live(self):
        if self._handle is None:
            raise ValueError("the pileup is closed")
        self._index._live()
        return self._handle

    @property
    def info(self):
        """dict(block_length, device_bytes, targets, alignments, ops, columns, adds, device, dirty, primary_only,
        normalize_indels, insertion_events, log_bytes) and the seven align parameters"""
        return dict(self._live().info, primary_only=self._primary_only)

    def add(self, targets, batch_bases=None):
        """Aligns the targets and adds their alignments to the counters -> dict(alignments, ops, columns: of the
        alignments kept, summed over the batches; targets: in the pileup so far).  Batches as RlzIndex.align does (a
        target is never split, so batching changes nothing); a batch the library refuses raises and leaves the
        counters as they were before that batch."""
        h = self._live()
        targets = list(targets)
        plan = plan_index_batches([len(t) for t in targets], h.info["block_length"], MAX_TEXT, batch_bases,
                                  max_targets=MAX_CHAIN_TARGETS)
        total = {"alignments": 0, "ops": 0, "columns": 0, "targets": h.info["targets"]}
        for lo, hi in plan:
            got = h.add(targets[lo:hi], self._primary_only)
            for name in ("alignments", "ops", "columns"):
                total[name] += got[name]
            total["targets"] = got["targets"]
        return total

    def counts(self, start: int = 0, end=None):
        """The (end - start, 8) uint32 counters of the block positions [start, end) (end None: the block's end);
        separator positions are zero."""
        return self._live().counts(start, end)

    def variants(self, min_count: int = 2, min_fraction=(1, 2)):
        """Where the sample differs -> VARIANT_DTYPE array (position, record_offset, record, ref_base, allele, count,
        depth, rev), ascending by (position, allele): one record for every allele among the three bases other than the
        block's and DEL (allele 4) with count >= min_count and count / depth >= num / den, min_fraction = (num, den) in
        integers, and one for INS (allele 5) against the same depth.  A bad fraction or min_count < 1: ValueError."""
        rule = _native._variant_rule(min_count, min_fraction)
        return self._live().variants(rule[0], rule[1:])

    def insertions(self, min_count: int = 2, min_fraction=(1, 2)):
        """What was inserted -> INSERTION_DTYPE array (position, record_offset, record, length, count, depth, ins_total,
        truncated, bases), ascending by (position, length, bases): one record for every inserted allele with count >=
        min_count and count / depth >= num / den.  insertion_bases(record) gives its bases; an allele of more than 64
        bases keeps its first 64 and has truncated = 1.  A bad fraction or min_count < 1: ValueError."""
        rule = _native._variant_rule(min_count, min_fraction)
        return self._live().insertions(rule[0], rule[1:])

    def consensus(self, min_depth: int = 1, min_fraction=(1, 2), low="reference", return_map: bool = False):
        """The sample's own sequence -> dict(records: one bytes per reference record; called, low_positions,
        substitutions, deleted, insertions, inserted_bases, truncated_skipped; with return_map, starts: for every block
        position the offset of its output in the records joined by one separator byte each, and the total length).
        A position with depth below min_depth, or whose best allele stays below min_fraction = (num, den) of the depth,
        is low: it keeps the reference base (low="reference") or becomes N (low="N").  Elsewhere the plurality allele
        is called -- a base, or a deletion --, then the most frequent inserted allele is written behind it if it reaches
        the fraction.  Open the pileup with normalize_indels=True for this: otherwise the two strands place an indel
        inside a repeat at different ends of it and neither place reaches a majority.  No genotypes, no qualities, no
        realignment.  Bad arguments: ValueError."""
        _native._consensus_params(min_depth, min_fraction, low)
        return self._live().consensus(min_depth, min_fraction, low, return_map)

    def close(self) -> None:
        h, self._handle = getattr(self, "_handle", None), None
        if h is not None:
            h.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _cohort_id(id, taken):
    """The id rules of RlzCohort.add / add_calls: None, or a str (bytes are decoded as UTF-8) no sample carries yet ->
    the id as str.  ValueError otherwise.  Pure Python."""
    if id is None:
        return None
    if isinstance(id, (bytes, bytearray)):
        id = bytes(id).decode("utf-8")
    if not isinstance(id, str):
        raise ValueError(f"a sample id is a str or bytes, not {type(id).__name__}")
    if id in taken:
        raise ValueError(f"ids must be distinct: {id!r} is in the cohort already")
    return id


class RlzCohort:
    """A collection of samples over the block of an RlzIndex, kept on the GPU (RlzIndex.cohort): per sample and block
    position a base call or none -- three bit planes, 3 bits per base.  add(pile) takes the calls of an RlzPileup under
    the consensus rule (a deletion, a low position and a separator are no call; insertions play no part), add_calls a
    sequence computed elsewhere.  distances() compares all pairs on the device, sites() finds the positions that vary,
    alignment() gives their columns: the core-SNP alignment.  Samples may carry ids and are then addressed by them.  No
    genotypes, no trees, no removal.  A context manager; use after close(), or after the index was closed, raises
    ValueError."""

    def __init__(self, handle, index):
        self._handle, self._index, self._ids, self._by_id = handle, index, [], {}

    def _live(self):
        if self._handle is None:
            raise ValueError("the cohort is closed")
        self._index._live()
        return self._handle

    @property
    def info(self):
        """dict(samples, capacity, block_length, device_bytes, device)"""
        return self._live().info

    @property
    def ids(self):
        """The id of every sample, in order (None where none was given)."""
        return list(self._ids)

    def __len__(self):
        return len(self._ids)

    def _added(self, got, id):
        self._ids.append(id)
        if id is not None:
            self._by_id[id] = got["sample"]
        return got

    def add(self, pile, id=None, min_depth: int = 1, min_fraction=(1, 2)):
        """The pileup's calls as the next sample -> dict(sample, called, low, deleted, differs).  A position is called
        as RlzPileup.consensus(min_depth, min_fraction) calls it; for the same rule called = consensus called -
        deleted, deleted = deleted, differs = substitutions, low = low_positions.  The pileup must be open over this
        cohort's index; its counters are not changed.  Bad arguments: ValueError, before any native call."""
        _native._consensus_params(min_depth, min_fraction, "reference")
        h = self._live()
        if not isinstance(pile, RlzPileup):
            raise ValueError(f"add takes an RlzPileup, not {type(pile).__name__}")
        id = _cohort_id(id, self._by_id)
        return self._added(h.add_pileup(pile._live(), min_depth, min_fraction), id)

    def add_calls(self, calls, id=None):
        """One byte per block position as the next sample -> the same dict (deleted = 0): A, C, G, T in either case
        are calls, anything else is none.  A length other than the block's: ValueError."""
        h = self._live()
        id = _cohort_id(id, self._by_id)
        return self._added(h.add_calls(calls), id)

    def samples(self):
        """The dict of every sample, in order, with its id."""
        return [dict(got, id=self._ids[got["sample"]]) for got in self._live().samples()]

    def distances(self):
        """All pairs compared on the GPU -> dict(differences, compared: (N, N) uint32 -- the positions both samples call
        where the calls differ, and the positions both call --, called, to_reference: (N,) uint64, the calls of every
        sample and those that differ from the reference)."""
        h = self._live()
        diff, cmp_ = h.distances()
        infos = h.samples()[:len(diff)]
        return {"differences": diff, "compared": cmp_,
                "called": np.array([i["called"] for i in infos], dtype=np.uint64),
                "to_reference": np.array([i["differs"] for i in infos], dtype=np.uint64)}

    def _min_present(self, min_present):
        if min_present is None:
            return len(self._ids)
        min_present = operator.index(min_present)
        if min_present < 0:
            raise ValueError("min_present must not be negative")
        return min_present

    def sites(self, min_present=None, with_reference: bool = True):
        """The positions that vary -> COHORT_SITE_DTYPE array (position, record_offset, record, present, counts,
        reference), ascending by position: at least two distinct bases occur there -- the reference's base counting as
        one with with_reference -- among at least min_present samples with a call (None: all samples, the core genome).
        present and counts (A, C, G, T) never include the reference."""
        min_present = self._min_present(min_present)
        return self._live().sites(min_present, with_reference)

    def alignment(self, positions=None, min_present=None, with_reference: bool = True):
        """(positions, (N, S) uint8 array): the letter of every sample at every position, `N` for no call.  positions
        None: those of sites(min_present, with_reference), the core-SNP alignment; else any block positions, in any
        order (a position beyond the block: ValueError)."""
        min_present = self._min_present(min_present)
        h = self._live()
        if positions is None:
            positions = h.sites(min_present, with_reference)["position"]
        positions = np.asarray(positions)
        letters = h.columns(positions)  # (refuses what is no position)
        return np.ascontiguousarray(positions, dtype=np.uint64), letters

    def calls(self, sample, start: int = 0, end=None):
        """The letters of one sample (an index, or its id) over the block positions [start, end) -> bytes."""
        h = self._live()
        return h.calls(resolve_target(sample, self._by_id, len(self._ids)), start, end)

    def close(self) -> None:
        h, self._handle = getattr(self, "_handle", None), None
        if h is not None:
            h.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def target_index_map(ids):
    """ids (or None) -> {id: index}"""
    return {} if ids is None else {name: j for j, name in enumerate(ids)}


def resolve_target(target, index, count):
    """A target argument -> its index: an id when ids were given (str, or bytes decoded as UTF-8), else an integer in
    [0, count) -- the library refuses an index beyond the archive, with the range's index in the message."""
    if isinstance(target, (bytes, bytearray)):
        target = bytes(target).decode("utf-8")
    if isinstance(target, str):
        if target not in index:
            raise KeyError(f"no target with id {target!r}")
        return index[target]
    j = operator.index(target)
    if j < 0:
        raise ValueError(f"target index {j} is negative")
    return j


__all__ = ["RLZ_DTYPE", "HIT_DTYPE", "SEED_DTYPE", "REPEAT_DTYPE", "CHAIN_DTYPE", "CHAIN_ANCHOR_DTYPE", "ALIGN_DTYPE", "VARIANT_DTYPE", "INSERTION_DTYPE", "insertion_bases", "PILEUP_CHANNELS", "RlzPileup", "COHORT_SITE_DTYPE", "RlzCohort", "cigar_string", "TARGET_HIT_DTYPE", "RlzArchiveFinder", "split_and_rebase", "rebase", "rlz_factorize", "rlz_count_factors", "rlz_factorize_fasta",
           "rlz_summary", "rlz_literals", "rlz_decode", "RlzArchive", "RlzIndex", "plan_index_batches", "write_packed_archive", "read_packed_archive"]

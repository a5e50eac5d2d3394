"""Relative Lempel-Ziv against a reference block (extension; DESIGN.md 5, "Relative LZ against a reference block").

Every target is factorized against the reference records and nothing else: no target copies from another target or
from itself, so a target's parse does not depend on the order of the collection.  One suffix sort over
reference + all targets serves them all.  The reference package has no such mode; it sits next to
factorize_dna_w_reference_seq and factorize_dna_rc_w_ref_fasta_files.

Semantics at position p of target T (Rblk = the reference records joined by one separator each):
Lf = the longest prefix of T[p:] that occurs in Rblk, Lr = the longest whose reverse complement does (0 without
with_rc).  Neither: a literal of length 1.  Lf >= Lr: a forward factor, ref = the leftmost occurrence in Rblk.
Otherwise a reverse-complement factor, ref = the leftmost occurrence of the reverse complement in Rblk.
"""
import numpy as np

from .. import _noLZSS as _native

RLZ_DTYPE = np.dtype([("start", "<u8"), ("length", "<u8"), ("ref", "<u8"), ("is_rc", "?"), ("is_literal", "?")])


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


__all__ = ["RLZ_DTYPE", "split_and_rebase", "rebase", "rlz_factorize", "rlz_count_factors", "rlz_factorize_fasta",
           "rlz_summary", "rlz_literals", "rlz_decode"]

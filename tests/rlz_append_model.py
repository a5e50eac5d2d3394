"""Model of an append to the relative-LZ archive (nolzss_rlz_archive_append_index, include/nolzss_hip.h): the records of
one matched batch, in the coordinates of Tcat = T1 s T2 s .. Tk s and with the separators' own literals among them, become
resident records behind z_old records and decoded_old bytes; the position sample grows over the new positions; export
turns resident records back into the host form.  Plain numpy, no device."""
import numpy as np

import rlz_model as model

RC_MASK = model.RC_MASK
FORWARD, RC, LITERAL = 0, 1, 2
SAMPLE = 256
FACTOR_DTYPE = np.dtype([("start", "<u8"), ("length", "<u8"), ("ref", "<u8")])
ARCHIVE_DTYPE = np.dtype([("start", "<u4"), ("length", "<u4"), ("src", "<u4"), ("meta", "<u4")])


def batch_layout(targets):
    """-> (Tcat upper-cased with 0x01 separators, the k separator positions)"""
    tcat, seps = bytearray(), []
    for t in targets:
        tcat += bytes(t).upper()
        seps.append(len(tcat))
        tcat.append(1)
    return bytes(tcat), seps


def batch_records(refs, targets, with_rc, parse=model.brute_parse):
    """What the match of one batch yields: absolute (start, length, ref) records, start = B + 1 + batch position, the
    literal of every separator included.  parse(refs, target, with_rc) -> rows as rlz_model.brute_parse."""
    B = sum(len(r) for r in refs) + len(refs) - 1
    rows, at = [], B + 1
    for t in targets:
        for start, length, ref, is_rc, is_literal in parse(refs, t, with_rc):
            s = at + start
            rows.append((s, length, s if is_literal else (ref | RC_MASK if is_rc else ref)))
        at += len(t)
        rows.append((at, 1, at))  # the separator
        at += 1
    return np.array(rows, dtype=FACTOR_DTYPE) if rows else np.zeros(0, dtype=FACTOR_DTYPE)


def append(records, seps, tcat, block_length, z_old, decoded_old):
    """-> (index array, ARCHIVE_DTYPE array, first new sample index, new sample entries): record i at batch position p
    with j separators below p goes to index z_old + i - j with start = decoded_old + p - j; a separator's is dropped"""
    seps = np.asarray(seps, dtype=np.int64)
    p = records["start"].astype(np.int64) - (block_length + 1)
    j = np.searchsorted(seps, p, side="left")  # separators below p
    keep = ~np.isin(p, seps)
    i = np.arange(len(records), dtype=np.int64)
    index = (z_old + i - j)[keep]
    f, pk = records[keep], p[keep]
    out = np.zeros(len(f), dtype=ARCHIVE_DTYPE)
    out["start"] = decoded_old + pk - j[keep]
    out["length"] = f["length"]
    lit = f["ref"] == f["start"]
    rc = ~lit & ((f["ref"] >> np.uint64(63)) != 0)
    ref = (f["ref"] & np.uint64(RC_MASK - 1)).astype(np.int64)
    out["src"] = np.where(lit, 0, np.where(rc, ref + f["length"].astype(np.int64) - 1, ref))
    sym = np.frombuffer(tcat, dtype=np.uint8)[pk].astype(np.uint32)
    out["meta"] = np.where(lit, LITERAL | (sym << 8), np.where(rc, RC, FORWARD))
    decoded_new = decoded_old + len(tcat) - len(seps)
    s_lo, s_hi = -(-decoded_old // SAMPLE), -(-decoded_new // SAMPLE)
    pos = np.arange(s_lo, s_hi, dtype=np.int64) * SAMPLE
    sample = z_old + np.searchsorted(out["start"].astype(np.int64), pos, side="right") - 1  # among the new records only
    return index, out, s_lo, sample


def export(block_length, resident):
    """ARCHIVE_DTYPE records -> (FACTOR_DTYPE records in the layout of genomics.rlz.absolute_records, literal bytes)"""
    out = np.zeros(len(resident), dtype=FACTOR_DTYPE)
    out["start"] = resident["start"].astype(np.uint64) + np.uint64(block_length)
    out["length"] = resident["length"]
    kind = resident["meta"] & 3
    src, length = resident["src"].astype(np.uint64), resident["length"].astype(np.uint64)
    out["ref"] = np.where(kind == LITERAL, out["start"],
                          np.where(kind == RC, (src - length + np.uint64(1)) | np.uint64(RC_MASK), src))
    literals = ((resident["meta"][kind == LITERAL] >> 8) & 0xff).astype(np.uint8).tobytes()
    return out, literals


class ArchiveModel:
    """An archive that grows by appends: the resident records, the sample and the per-target lengths"""

    def __init__(self, refs):
        self.refs = [bytes(r).upper() for r in refs]
        self.block_length = sum(len(r) for r in self.refs) + len(self.refs) - 1
        self.records = np.zeros(0, dtype=ARCHIVE_DTYPE)
        self.sample = np.zeros(0, dtype=np.int64)
        self.lengths = []
        self.decoded = 0

    def append(self, targets, with_rc, parse=model.brute_parse):
        tcat, seps = batch_layout(targets)
        recs = batch_records(self.refs, targets, with_rc, parse)
        index, out, s_lo, sample = append(recs, seps, tcat, self.block_length, len(self.records), self.decoded)
        assert len(out) == len(recs) - len(targets), "a batch adds z_batch - k records"
        assert index.tolist() == list(range(len(self.records), len(self.records) + len(out))), "compaction without a scan"
        assert s_lo == len(self.sample)
        self.records = np.concatenate([self.records, out])
        self.sample = np.concatenate([self.sample, sample])
        self.lengths += [len(t) for t in targets]
        self.decoded += len(tcat) - len(seps)

    def export(self):
        return export(self.block_length, self.records)

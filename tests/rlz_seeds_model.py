"""Models of the maximal match seeds of the relative-LZ index (nolzss_rlz_index_seeds, include/nolzss_hip.h).

  brute_seeds     the definition itself: an interval of the target that occurs inside one reference record (bytes.find per
                  record and strand) and no longer does when it is extended by one base to the left or to the right
  ms_seeds        the formulation the kernels run: ms[p] = the longest prefix of target[p:] that occurs, and the seeds are
                  the positions with ms[p] >= 1 and (p == 0 or ms[p - 1] <= ms[p]); ms is computed incrementally from
                  ms[p - 1] - 1, which occurrence being closed under substrings allows
  expected        the dict RlzIndex.seeds returns, the hits from rlz_locate_model.brute_locate
  targets         the seeded generator both the CPU and the GPU tests draw from

A seed is (start, length) inside one target.  Plain Python over bytes.find."""
import numpy as np

import rlz_locate_model as lm
import rlz_model as model


def occurs(refs, piece, with_rc=True):
    """piece (upper case, not empty) lies inside one record, on either strand with reverse complement"""
    if any(piece in r for r in refs):
        return True
    if with_rc:
        rc = model.revcomp(piece)
        return any(rc in r for r in refs)
    return False


def _upper(refs):
    return [bytes(r).upper() for r in refs]


def brute_seeds(refs, target, with_rc=True):
    """-> [(start, length)] ascending, by the definition: every L is tried at every start, nothing is carried over"""
    refs, t = _upper(refs), bytes(target).upper()
    out = []
    for p in range(len(t)):
        for L in range(1, len(t) - p + 1):
            if not occurs(refs, t[p:p + L], with_rc):
                continue
            right = p + L < len(t) and occurs(refs, t[p:p + L + 1], with_rc)
            left = p > 0 and occurs(refs, t[p - 1:p + L], with_rc)
            if not right and not left:
                out.append((p, L))
    return out


def ms_array(refs, target, with_rc=True):
    """ms[p] for every position of the target, each started from ms[p - 1] - 1"""
    refs, t = _upper(refs), bytes(target).upper()
    ms, L = [], 0
    for p in range(len(t)):
        L = max(L - 1, 0)
        while p + L < len(t) and occurs(refs, t[p:p + L + 1], with_rc):
            L += 1
        ms.append(L)
    return ms


def ms_seeds(refs, target, with_rc=True, min_length=1):
    ms = ms_array(refs, target, with_rc)
    return [(p, L) for p, L in enumerate(ms) if L >= max(min_length, 1) and (p == 0 or ms[p - 1] <= L)]


def expected(refs, targets, with_rc=True, min_length=1, max_hits=0):
    """dict as RlzIndex.seeds returns it"""
    starts = lm.record_starts(refs)
    seeds, counts, offsets, hits = [], [], [0], []
    for j, t in enumerate(targets):
        up = bytes(t).upper()
        for p, L in ms_seeds(refs, up, with_rc, min_length):
            h = lm.brute_locate(refs, up[p:p + L], with_rc)
            seeds.append((j, p, L))
            counts.append(len(h))
            if max_hits == 0 or len(h) <= max_hits:
                hits += h
            offsets.append(len(hits))
    return {"target": np.array([s[0] for s in seeds], dtype=np.uint64),
            "start": np.array([s[1] for s in seeds], dtype=np.uint64),
            "length": np.array([s[2] for s in seeds], dtype=np.uint64),
            "counts": np.array(counts, dtype=np.uint64), "offsets": np.array(offsets, dtype=np.uint64),
            "position": np.array([h[0] for h in hits], dtype=np.uint64),
            "record": np.array([h[1] for h in hits], dtype=np.uint32),
            "record_offset": np.array([h[0] - starts[h[1]] for h in hits], dtype=np.uint64),
            "is_rc": np.array([h[2] for h in hits], dtype=bool)}


# ---- the seeded generator ----------------------------------------------------------------------------------------
def target(rng, refs, pieces=8, longest=12, rate=0.08):
    """pieces cut from the records and their reverse complements (rlz_locate_model.patterns: also extended, random,
    across a record boundary, self-reverse-complementary, lower case), joined, with substitutions and a random tail"""
    t = bytearray(b"".join(lm.patterns(rng, refs, rng.randint(1, pieces), longest)))
    for i in range(len(t)):
        if rng.random() < rate:
            t[i] = rng.choice(b"ACGT")
    return bytes(t) + bytes(rng.choice(b"ACGT") for _ in range(rng.randint(0, 4)))


def targets(rng, refs, count, **kw):
    return [target(rng, refs, **kw) for _ in range(count)]

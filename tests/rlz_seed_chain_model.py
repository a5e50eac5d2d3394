"""Model of the colinear seed chains of the relative-LZ index (nolzss_rlz_index_seed_chains, include/nolzss_hip.h).

  anchors         every reported hit of every seed of rlz_seeds_model.expected as (target, group, y, q, L), in group order
  recurrence      f and pred of one group, with a `lookback` argument (None: the unbounded O(n^2) recurrence) and the
                  tie rule as an argument (nearest wins; `farthest` is the rule the kernels must NOT implement)
  chains          ends, backtrack, extents and primary flags over anchors in group order: what the debug hook returns
  expected        the dict RlzIndex.seed_chains returns
  planted         the seeded generator of targets cut from records, mutated, with the truth of every one
  cloud           the seeded generator of arbitrary anchor groups

Plain Python integers throughout: nothing here can wrap."""
import numpy as np

import rlz_locate_model as lm
import rlz_model as model
import rlz_seeds_model as sm

LOOKBACK = 64
NO_PRED = 0xFFFFFFFF
DEFAULTS = dict(min_length=15, max_hits=64, max_gap=5000, bandwidth=500, min_score=40)


def block_length(refs):
    return sum(len(r) for r in refs) + len(refs) - 1


def anchors(refs, targets, with_rc=True, min_length=1, max_hits=0):
    """-> sorted [(target, group, y, q, L)]: group = is_rc * m + record, y = x forward, 2 B - x - L + 1 reverse"""
    e = sm.expected(refs, targets, with_rc, min_length, max_hits)
    B, m = block_length(refs), len(refs)
    out = []
    for j in range(len(e["target"])):
        t, q, L = int(e["target"][j]), int(e["start"][j]), int(e["length"][j])
        for h in range(int(e["offsets"][j]), int(e["offsets"][j + 1])):
            x, r, rc = int(e["position"][h]), int(e["record"][h]), int(e["is_rc"][h])
            out.append((t, rc * m + r, 2 * B - x - L + 1 if rc else x, q, L))
    return sorted(out)


def link(a, b, max_gap, bandwidth):
    """the gain of b = (y, q, L) behind a, or None when a is no candidate of b"""
    dq, dy = b[1] - a[1], b[0] - a[0]
    if dq < 1 or dy < 1 or max(dq, dy) > max_gap or abs(dq - dy) > bandwidth:
        return None
    return min(b[2], dq, dy) - abs(dq - dy)


def recurrence(group, max_gap, bandwidth, lookback=LOOKBACK, farthest=False):
    """group: [(y, q, L)] in (y, q) order -> (f, pred) lists; pred None without a predecessor"""
    f, pred = [], []
    for i, b in enumerate(group):
        best, arg = b[2], None
        lo = 0 if lookback is None else max(0, i - lookback)
        for j in (range(lo, i) if farthest else range(i - 1, lo - 1, -1)):  # the first of equals wins
            gain = link(group[j], b, max_gap, bandwidth)
            if gain is not None and f[j] + gain > best:
                best, arg = f[j] + gain, j
        f.append(best)
        pred.append(arg)
    return f, pred


def walk(f, pred):
    """-> the indices of the chain of a group, ascending: from the smallest index with maximal f back along pred"""
    e = f.index(max(f))
    out = [e]
    while pred[out[-1]] is not None:
        out.append(pred[out[-1]])
    return out[::-1]


def groups_of(anch):
    """sorted anchors -> [((target, group), first, end)]"""
    out, first = [], 0
    for i in range(1, len(anch) + 1):
        if i == len(anch) or anch[i][:2] != anch[first][:2]:
            out.append((anch[first][:2], first, i))
            first = i
    return out


def chains(anch, B, m, max_gap, bandwidth, min_score=0, lookback=LOOKBACK, farthest=False):
    """anchors in group order -> dict(f, pred, chains: list of dicts, anchors: list of (t_start, position, length),
    anchor_offsets)"""
    f_all, pred_all, recs, out_anchors, offsets = [], [], [], [], [0]
    for (t, g), first, end in groups_of(anch):
        group = [(a[2], a[3], a[4]) for a in anch[first:end]]
        f, pred = recurrence(group, max_gap, bandwidth, lookback, farthest)
        f_all += f
        pred_all += [NO_PRED if p is None else p for p in pred]
        idx = walk(f, pred)
        score = f[idx[-1]]
        if score < min_score:
            continue
        rc = 1 if g >= m else 0
        xs = [(2 * B - y - L + 1 if rc else y, q, L) for y, q, L in (group[i] for i in idx)]
        recs.append(dict(target=t, record=g - rc * m, is_rc=rc, score=score, t_start=xs[0][1],
                         t_end=xs[-1][1] + xs[-1][2], r_start=min(x for x, _, _ in xs),
                         r_end=max(x + L for x, _, L in xs), num_anchors=len(xs), primary=0))
        out_anchors += [(q, x, L) for x, q, L in xs]
        offsets.append(len(out_anchors))
    best = {}
    for c, r in enumerate(recs):  # the first of the largest score of its target
        if r["target"] not in best or r["score"] > recs[best[r["target"]]]["score"]:
            best[r["target"]] = c
    for c in best.values():
        recs[c]["primary"] = 1
    return dict(f=f_all, pred=pred_all, chains=recs, anchors=out_anchors, anchor_offsets=offsets)


CHAIN_FIELDS = ("target", "record", "is_rc", "score", "t_start", "t_end", "r_start", "r_end", "num_anchors", "primary")


def as_result(run, refs):
    """chains() -> the dict RlzIndex.seed_chains returns"""
    starts = lm.record_starts(refs)
    recs = run["chains"]
    kinds = dict(record=np.uint32, num_anchors=np.uint32, is_rc=bool, primary=bool)
    out = {k: np.array([r[k] for r in recs], dtype=kinds.get(k, np.uint64)) for k in CHAIN_FIELDS}
    out["record_offset"] = np.array([r["r_start"] - starts[r["record"]] for r in recs], dtype=np.uint64)
    out["anchor_offsets"] = np.array(run["anchor_offsets"], dtype=np.uint64)
    for k, name in enumerate(("anchor_t_start", "anchor_position", "anchor_length")):
        out[name] = np.array([a[k] for a in run["anchors"]], dtype=np.uint64)
    return out


def expected(refs, targets, with_rc=True, lookback=LOOKBACK, **params):
    """dict as RlzIndex.seed_chains returns it"""
    p = dict(DEFAULTS, **params)
    anch = anchors(refs, targets, with_rc, p["min_length"], p["max_hits"])
    run = chains(anch, block_length(refs), len(refs), p["max_gap"], p["bandwidth"], p["min_score"], lookback)
    return as_result(run, refs)


# ---- the seeded generators ---------------------------------------------------------------------------------------
def dna(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def mutate(rng, piece, rate):
    """substitutions at `rate`, each to another base"""
    t = bytearray(piece)
    for i in range(len(t)):
        if rng.random() < rate:
            t[i] = rng.choice([c for c in b"ACGT" if c != t[i]])
    return bytes(t)


MAPPING = dict(min_length=10, max_hits=8, max_gap=1000, bandwidth=50, min_score=20)


def planted(rng, count=24, records=4):
    """-> (refs, targets, truth): targets are pieces of 120 to 300 bases cut from records of 900 to 1500 random bases,
    with 4 % substitutions and one insertion or deletion of 1 to 6 bases, every second one reverse-complemented;
    truth[j] = (record, is_rc, lo, hi), the interval of the record the piece was cut from"""
    refs = [dna(rng, rng.randint(900, 1500)) for _ in range(records)]
    targets, truth = [], []
    for j in range(count):
        r = rng.randrange(records)
        n = rng.randint(120, 300)
        lo = rng.randrange(len(refs[r]) - n + 1)
        t = mutate(rng, refs[r][lo:lo + n], 0.04)
        at, size = rng.randrange(20, len(t) - 20), rng.randint(1, 6)
        t = t[:at] + dna(rng, size) + t[at:] if rng.random() < 0.5 else t[:at] + t[at + size:]
        if j % 2:
            t = model.revcomp(t)
        targets.append(t)
        truth.append((r, j % 2, lo, lo + n))
    return refs, targets, truth


def ring_case(rng):
    """-> (refs, target): a 7 % mutated copy of a record of 1200 random bases, 12 diverged copies of a 37-base unit and
    1200 random bases, beside a second record of 700 bases: the repeat fills one group with anchors"""
    unit = dna(rng, 37)
    record = dna(rng, 1200) + b"".join(mutate(rng, unit, 0.08) for _ in range(12)) + dna(rng, 1200)
    refs = [record, dna(rng, 700)]
    target = mutate(rng, record, 0.07)[:2600]
    return refs, target


RING = dict(min_length=8, max_hits=16, max_gap=2000, bandwidth=100, min_score=20)


def cloud(rng, size, span=None):
    """-> [(y, q, L)] of `size` anchors in (y, q) order, the pairs distinct: 60 % near a few diagonals, the rest uniform,
    lengths 1 to 30"""
    span = span or max(40, 6 * size)
    diagonals = [rng.randint(-span // 4, span // 4) for _ in range(rng.randint(1, 4))]
    seen = set()
    while len(seen) < size:
        q = rng.randrange(span)
        if rng.random() < 0.6:
            y = q + rng.choice(diagonals) + rng.randint(-3, 3) + span
        else:
            y = rng.randrange(2 * span)
        if y >= 0:
            seen.add((y, q))
    return [(y, q, rng.randint(1, 30)) for y, q in sorted(seen)]


def cloud_anchors(rng, sizes):
    """groups of the given sizes -> anchors in group order: four groups per target, both strands of two records (m = 2)"""
    out = []
    for k, size in enumerate(sizes):
        t, g = divmod(k, 4)
        out += [(t, g, y, q, L) for y, q, L in cloud(rng, size)]
    return out

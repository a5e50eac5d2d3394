"""Model of the base-level alignments of the relative-LZ index (nolzss_rlz_index_align, include/nolzss_hip.h).

  banded          D of one job over the allowed diagonals, as a list of {j: D[i][j]} rows
  traceback       the codes of a path back from a cell, by a tie rule given as an argument (diagonal, up, left is the
                  rule of the header; another order is a rule the kernels must NOT implement)
  gap / flank     one job from plain strings -> (cost, end column, codes in job order)
  job             what the debug hook returns for one (kind, q0, nq, y0, ny) over a query and a reference string
  align_chain     trim, jobs, anchors and flanks of one chain -> coordinates, cost and one code per column
  expected        the dict RlzIndex.align returns, driven from a seed_chains result
  wagner_fischer  the unbanded edit distance (independent of everything above)
  replay          rebuilds the aligned stretch of a target from the block and the ops, with an ordinary reverse
                  complement (independent of the mirrored coordinates)

Plain Python integers and strings throughout: nothing here can wrap."""
import numpy as np

I, D, EQ, X = 1, 2, 7, 8
LANES = 64
GAP, RIGHT, LEFT = 0, 1, 2
RULE = ("diag", "up", "left")
DEFAULTS = dict(min_length=15, max_hits=64, max_gap=5000, bandwidth=31, min_score=40, band=16, max_flank=256)
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s):
    return bytes(s).translate(COMP)[::-1]


def banded(Q, R, lo, hi):
    """rows[i] = {j: D[i][j]} for the cells of the rectangle with lo <= j - i <= hi"""
    n, m = len(Q), len(R)
    rows = []
    for i in range(n + 1):
        row = {}
        for j in range(max(0, i + lo), min(m, i + hi) + 1):
            if i == 0 and j == 0:
                row[j] = 0
                continue
            cands = []
            if i and j and j - 1 in rows[i - 1]:
                cands.append(rows[i - 1][j - 1] + (Q[i - 1] != R[j - 1]))
            if i and j in rows[i - 1]:
                cands.append(rows[i - 1][j] + 1)
            if j and j - 1 in row:
                cands.append(row[j - 1] + 1)
            row[j] = min(cands)
        rows.append(row)
    return rows


def traceback(rows, Q, R, i, j, rule=RULE):
    """the codes of the path from (0, 0) to (i, j), in path order: at every cell the first move of `rule` that attains D"""
    out = []
    while i or j:
        moves = {}
        if i and j and j - 1 in rows[i - 1]:
            moves["diag"] = rows[i - 1][j - 1] + (Q[i - 1] != R[j - 1])
        if i and j in rows[i - 1]:
            moves["up"] = rows[i - 1][j] + 1
        if j and j - 1 in rows[i]:
            moves["left"] = rows[i][j - 1] + 1
        move = next(mv for mv in rule if moves.get(mv) == rows[i][j])
        if move == "diag":
            out.append(EQ if Q[i - 1] == R[j - 1] else X)
            i, j = i - 1, j - 1
        elif move == "up":
            out.append(I)
            i -= 1
        else:
            out.append(D)
            j -= 1
    return out[::-1]


def gap(Q, R, band, rule=RULE):
    """-> (cost, codes)"""
    gq, gy = len(Q), len(R)
    if gq == 0 or gy == 0:
        return gq + gy, [D] * gy + [I] * gq
    delta = gy - gq
    rows = banded(Q, R, min(0, delta) - band, max(0, delta) + band)
    return rows[gq][gy], traceback(rows, Q, R, gq, gy, rule)


def flank_end(row, fq, W, band, tie="nearest"):
    """the end column of a flank from its last row, or None when no cell qualifies"""
    cells = [j for j in range(max(0, fq - band), min(W, fq + band) + 1) if j in row]
    if not cells:
        return None
    if tie == "nearest":
        return min(cells, key=lambda j: (row[j], abs(j - fq), j))
    return min(cells, key=lambda j: (row[j], j))  # the rule the kernels must NOT implement


def flank(Q, avail, band, max_flank=None, rule=RULE, tie="nearest"):
    """Q: the query bases in job order; avail: the reference bases of the record span in job order -> None when the flank
    is empty or clipped, else (cost, end column, codes in job order)"""
    fq = len(Q)
    if fq == 0 or (max_flank is not None and fq > max_flank):
        return None
    W = min(len(avail), fq + band)
    if max(0, fq - band) > min(W, fq + band):
        return None
    R = avail[:W]
    rows = banded(Q, R, -band, band)
    j = flank_end(rows[fq], fq, W, band, tie)
    if j is None:
        return None
    return rows[fq][j], j, traceback(rows, Q, R, fq, j, rule)


def job(kind, query, reference, q0, nq, y0, ny, band):
    """the debug hook's answer for one job: (cost, end_col, codes in ascending q)"""
    if kind == GAP:
        cost, codes = gap(query[q0:q0 + nq], reference[y0:y0 + ny], band)
        return cost, ny, codes
    if kind == RIGHT:
        got = flank(query[q0:q0 + nq], reference[y0:y0 + ny], band)
        return (0, 0, []) if got is None else got
    got = flank(query[q0 - nq:q0][::-1], reference[y0 - ny:y0][::-1], band)
    return (0, 0, []) if got is None else (got[0], got[1], got[2][::-1])


def merged(codes):
    """one code per column -> [(length, code)] with no two neighbours of one code"""
    out = []
    for c in codes:
        if out and out[-1][1] == c:
            out[-1][0] += 1
        else:
            out.append([1, c])
    return [(n, c) for n, c in out]


def index_text(refs):
    """X without its last separator: Rblk, a separator, the mirrored block -- position y of the mirrored block holds the
    complement of Rblk[2 B - y]"""
    rblk = b"\x01".join(bytes(r).upper() for r in refs)
    return rblk + b"\x02" + rblk.translate(COMP)[::-1]


def record_span(refs, record, is_rc):
    """[first, end) of a record in y"""
    first = sum(len(r) + 1 for r in refs[:record])
    end = first + len(refs[record])
    B = sum(len(r) for r in refs) + len(refs) - 1
    return (2 * B + 1 - end, 2 * B + 1 - first) if is_rc else (first, end)


def align_chain(target, Xtext, span, anchors, band, max_flank):
    """anchors: [(q, y, L)] ascending -> dict(t_start, t_end, y_begin, y_end, edit, codes)"""
    codes, edit = [], 0
    q0, y0, _ = anchors[0]
    t_start, y_begin = q0, y0
    left = flank(target[:q0][::-1], Xtext[span[0]:y0][::-1], band, max_flank)
    if left is not None:
        edit += left[0]
        codes += left[2][::-1]
        t_start, y_begin = 0, y0 - left[1]
    for (q, y, L), nxt in zip(anchors, anchors[1:] + [None]):
        if nxt is None:
            codes += [EQ] * L
            break
        dq, dy = nxt[0] - q, nxt[1] - y
        assert dq >= 1 and dy >= 1
        keep = L - max(0, L - dq, L - dy)
        codes += [EQ] * keep
        cost, ops = gap(target[q + keep:nxt[0]], Xtext[y + keep:nxt[1]], band)
        edit += cost
        codes += ops
    qe, ye, Le = anchors[-1]
    t_end, y_end = qe + Le, ye + Le
    right = flank(target[t_end:], Xtext[y_end:span[1]], band, max_flank)
    if right is not None:
        edit += right[0]
        codes += right[2]
        t_end, y_end = len(target), y_end + right[1]
    return dict(t_start=t_start, t_end=t_end, y_begin=y_begin, y_end=y_end, edit=edit, codes=codes)


def expected(refs, targets, chains, band=16, max_flank=256):
    """chains: what RlzIndex.seed_chains (or its model) returns -> the dict RlzIndex.align returns"""
    refs = [bytes(r).upper() for r in refs]
    Xtext = index_text(refs)
    B = sum(len(r) for r in refs) + len(refs) - 1
    starts = np.cumsum([0] + [len(r) + 1 for r in refs[:-1]], dtype=np.uint64)
    cols = {k: [] for k in ("t_start", "t_end", "r_start", "r_end", "edit_distance", "columns", "num_ops")}
    ops, offsets = [], [0]
    for c in range(len(chains["target"])):
        target = bytes(targets[int(chains["target"][c])]).upper()
        is_rc, record = bool(chains["is_rc"][c]), int(chains["record"][c])
        anchors = []
        for a in range(int(chains["anchor_offsets"][c]), int(chains["anchor_offsets"][c + 1])):
            q, x, L = (int(chains[k][a]) for k in ("anchor_t_start", "anchor_position", "anchor_length"))
            anchors.append((q, 2 * B - x - L + 1 if is_rc else x, L))
        got = align_chain(target, Xtext, record_span(refs, record, is_rc), anchors, band, max_flank)
        runs = merged(got["codes"])
        cols["t_start"].append(got["t_start"])
        cols["t_end"].append(got["t_end"])
        cols["r_start"].append(2 * B + 1 - got["y_end"] if is_rc else got["y_begin"])
        cols["r_end"].append(2 * B + 1 - got["y_begin"] if is_rc else got["y_end"])
        cols["edit_distance"].append(got["edit"])
        cols["columns"].append(len(got["codes"]))
        cols["num_ops"].append(len(runs))
        ops += [(n << 4) | code for n, code in runs]
        offsets.append(len(ops))
    out = {k: np.asarray(chains[k]).copy() for k in ("target", "record", "is_rc", "score", "primary")}
    for k in ("t_start", "t_end", "r_start", "r_end", "edit_distance", "columns"):
        out[k] = np.array(cols[k], dtype=np.uint64)
    out["num_ops"] = np.array(cols["num_ops"], dtype=np.uint32)
    out["record_offset"] = out["r_start"] - starts[out["record"]] if len(out["record"]) else np.zeros(0, dtype=np.uint64)
    out["op_offsets"] = np.array(offsets, dtype=np.uint64)
    out["ops"] = np.array(ops, dtype=np.uint32)
    return out


# ---- independent helpers -------------------------------------------------------------------------------------------
def wagner_fischer(a, b):
    """the unbanded edit distance"""
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j - 1] + (a[i - 1] != b[j - 1]), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[len(b)]


def replay(ops, target, block, t_start, t_end, r_start, r_end, is_rc):
    """Rebuilds target[t_start:t_end] from block[r_start:r_end] and the ops -> (the rebuilt bytes, the cost).  `=` copies
    a reference base, X and I take the target's base (X must differ from the reference's), D skips a reference base;
    both stretches must be consumed exactly."""
    ref = bytes(block[r_start:r_end])
    if is_rc:
        ref = revcomp(ref)
    want = bytes(target[t_start:t_end])
    out, cost, q, r = bytearray(), 0, 0, 0
    for op in ops:
        n, code = int(op) >> 4, int(op) & 15
        assert n >= 1 and code in (I, D, EQ, X), op
        if code == EQ:
            out += ref[r:r + n]
            q, r = q + n, r + n
        elif code == X:
            assert all(want[q + t] != ref[r + t] for t in range(n)), "an X column over equal bases"
            out += want[q:q + n]
            q, r, cost = q + n, r + n, cost + n
        elif code == I:
            out += want[q:q + n]
            q, cost = q + n, cost + n
        else:
            r, cost = r + n, cost + n
    assert q == len(want) and r == len(ref), "the ops do not consume both stretches"
    return bytes(out), cost


# ---- the seeded generator of the end-to-end test -------------------------------------------------------------------
def random_dna(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def mutate(rng, s, edits, indel=None):
    """`edits` single-base edits at distinct positions, at least 12 apart and 8 from either end, and one indel of `indel`
    bases -> (the mutated bytes, the number of edited bases)"""
    s = bytearray(s)
    spots = []
    while len(spots) < edits + (1 if indel else 0):
        p = rng.randrange(8, len(s) - 8 - (indel or 0))
        if all(abs(p - o) >= 12 + (indel or 0) for o in spots):
            spots.append(p)
    count = 0
    for k, p in enumerate(sorted(spots, reverse=True)):  # from the back: earlier positions stay put
        if indel and k == 0:
            if rng.random() < 0.5:
                del s[p:p + indel]
            else:
                s[p:p] = random_dna(rng, indel)
            count += indel
            continue
        kind = rng.choice("sid")
        if kind == "s":
            s[p] = rng.choice([c for c in b"ACGT" if c != s[p]])
        elif kind == "i":
            s[p:p] = bytes([rng.choice(b"ACGT")])
        else:
            del s[p]
        count += 1
    return bytes(s), count


def planted(rng, reads=200, contigs=3):
    """-> refs (three records of about 3000 bases), targets, truth [(record, is_rc, edits)]: reads of about 150 bases
    with at most 3 edits, some at a record's first or last base, and contigs of 2000 bases with 0.5 % edits and one
    indel of 20"""
    refs = [random_dna(rng, 3000 + 17 * k) for k in range(3)]
    targets, truth = [], []
    for j in range(reads):
        r = rng.randrange(3)
        lo = rng.choice([0, len(refs[r]) - 150]) if j % 10 == 0 else rng.randrange(0, len(refs[r]) - 150)
        piece, edits = mutate(rng, refs[r][lo:lo + 150], rng.randrange(0, 4))
        rc = rng.random() < 0.5
        targets.append(revcomp(piece) if rc else piece)
        truth.append((r, rc, edits))
    for j in range(contigs):
        r = j % 3
        lo = rng.randrange(0, len(refs[r]) - 2000)
        piece, edits = mutate(rng, refs[r][lo:lo + 2000], 10, indel=20)
        rc = j % 2 == 1
        targets.append(revcomp(piece) if rc else piece)
        truth.append((r, rc, edits))
    return refs, targets, truth

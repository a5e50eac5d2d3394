"""Texts on the edges of the decisions of text_pack.hip -- TEST INFRASTRUCTURE ONLY (a plain helper module of
test_gpu_text_intake.py, whose child process runs main()).

pack_text decides the symbol width from the number of byte values present (sigma <= 4: 2 bits, <= 16: 4 bits, else 8), makes
the dense codes from a prefix popcount over the four 64-bit words of the presence mask, and takes a text for SEGMENTED when
it holds at least one upper-case nucleotide and 1 .. 250 other byte values that occur exactly once each.  Every case names
the decision it must get: (name, text, bits, segmented)."""
import sys

import numpy as np

import key_layout_cases as K

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
OTHERS = [b for b in range(256) if b not in K.NUCLEOTIDES]  # the 252 byte values that are no upper-case nucleotide
LENGTHS = (1, 15, 16, 17, 31, 32, 33, 4097)


def over(alphabet, n, seed):
    """random text over `alphabet`, which is written twice in front where there is room (every symbol present, none once)"""
    alpha = np.array(sorted(set(alphabet)), dtype=np.uint8)
    t = alpha[np.random.default_rng(seed).integers(0, len(alpha), size=n)]
    head = np.concatenate([alpha, alpha])[:n]
    t[:len(head)] = head
    return t.tobytes()


def dna_with(n, seed, once, at=None):
    """random upper-case DNA with the bytes of `once` written once each, at the positions `at` (default: spread out)"""
    t = ACGT[np.random.default_rng(seed).integers(0, 4, size=n)].copy()
    t[:4] = ACGT
    at = at if at is not None else [5 + j * ((n - 6) // max(1, len(once))) for j in range(len(once))]
    assert len(set(at)) == len(once)
    for p, b in zip(at, once):
        t[p] = b
    return t.tobytes()


def spread(sigma):
    """sigma byte values from 0x00 to 0xFF"""
    return [0] if sigma == 1 else sorted({int(round(v)) for v in np.linspace(0, 255, sigma)})


def cases():
    out = []
    width = lambda sigma: 2 if sigma <= 4 else (4 if sigma <= 16 else 8)  # noqa: E731
    for sigma in (1, 2, 3, 4, 5, 15, 16, 17, 255, 256):
        alphabet = spread(sigma) if sigma < 255 else list(range(256 - sigma, 256)) if sigma == 255 else list(range(256))
        assert len(alphabet) == sigma and (sigma < 2 or (255 in alphabet and (0 in alphabet or sigma == 255)))
        out.append((f"sigma_{sigma}", over(alphabet, max(700, 3 * sigma), sigma), width(sigma), False))
    # the words of the presence mask: dense codes count the bits of the words in front
    for lo in (63, 127, 191):
        out.append((f"mask_words_{lo}_{lo + 1}", over([lo, lo + 1], 300, lo), 2, False))
    out.append(("mask_words_all_edges", over([0, 63, 64, 127, 128, 191, 192, 255], 500, 1), 4, False))
    out.append(("mask_words_17_around_64", over(list(range(56, 73)), 600, 2), 8, False))
    out.append(("mask_words_17_around_128_192", over(list(range(120, 129)) + list(range(188, 196)), 600, 3), 8, False))
    # nucleotides and other bytes
    out.append(("ACG_and_frequent_N", over(b"ACGN", 500, 4), 2, False))
    out.append(("ACGT_one_N", dna_with(500, 5, b"N"), 2, True))
    out.append(("ACGT_two_N", dna_with(500, 6, b"NN", at=[100, 300]), 4, False))
    out.append(("lower_case_acgt", over(b"acgt", 500, 7), 2, False))
    lower = bytearray(over(b"acgt", 500, 8))
    lower[250] = ord("#")
    out.append(("lower_case_acgt_and_one_byte", bytes(lower), 4, False))
    out.append(("once_only_at_0", dna_with(400, 9, b"#", at=[0]), 2, True))
    out.append(("once_only_at_end", dna_with(400, 10, b"#", at=[399]), 2, True))
    out.append(("once_only_adjacent", dna_with(400, 11, b"#%", at=[200, 201]), 2, True))
    out.append(("once_only_at_both_ends_and_0xff", dna_with(401, 12, bytes([0, 255, 1]), at=[0, 400, 17]), 2, True))
    for count in (249, 250, 251):
        # (251 other values: sigma = 255, 8 bits, not segmented; only 252 values are no nucleotide)
        rng = np.random.default_rng(count)
        once = bytes(rng.permutation(OTHERS)[:count].tolist())
        at = (8 + np.sort(rng.choice(3000, size=count, replace=False))).tolist()
        out.append((f"once_only_{count}_values", dna_with(3100, 13 + count, once, at=at), 2 if count <= 250 else 8, count <= 250))
    out.append(("protein_alphabet_once", b"ACDEFGHIKLMNPQRSTVWY", 2, True))  # 16 terminators between A, C, G and T
    out.append(("once_only_bytes_no_nucleotide", b"0123456789", 4, False))
    many_n = np.frombuffer(dna_with(150_000, 14, b""), dtype=np.uint8).copy()
    many_n[4 + np.random.default_rng(15).choice(149_000, size=70_000, replace=False)] = ord("N")
    out.append(("one_other_value_70000_times", many_n.tobytes(), 4, False))  # (the saturating count must not come out as 1)
    for n in LENGTHS:
        out.append((f"two_bit_{n}", over(b"ACGT", n, 20 + n), 2, False))
        if n >= 15:
            out.append((f"four_bit_{n}", over(b"ACGNT", n, 30 + n), 4, False))
        if n >= 17:
            out.append((f"eight_bit_{n}", over(bytes(range(97, 114)), n, 40 + n), 8, False))
        if n >= 15:
            out.append((f"segmented_{n}", dna_with(n, 50 + n, b"#\x01", at=[n // 2, n - 1]), 2, True))
    assert len({name for name, *_ in out}) == len(out)
    return out


def as_layout_cases():
    """the same as cases of key_layout_cases.check_case, with the plan the trace must name"""
    out = []
    for name, t, bits, segmented in cases():
        plan = "segmented" if segmented else "general"
        out.append(K.Case(name, "text", t, plan, K.Layout(plan, bits, K.plan_k_syms(plan, bits), 256 // bits, 0), []))
    return out


def main():
    K.run_child(as_layout_cases(), sys.argv[1])


if __name__ == "__main__":
    sys.exit(main())

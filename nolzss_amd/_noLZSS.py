"""Python-visible surface of the reference's compiled module `noLZSS._noLZSS`
(reference: src/cpp/bindings.cpp), bound to libnolzss_hip.so through ctypes.

Same names, argument meaning, return shapes and error behaviour as the pybind11 module; ctypes
releases the GIL around every native call just as the reference does with gil_scoped_release
(bindings.cpp:70).  All 42 functions of the reference module are present; every one of them
computes on the GPU through the C ABI (there is no CPU path).
"""
import ctypes as C
import operator
import os

import numpy as np

from . import _lib
from ._lib import lib, check

__version__ = lib.nolzss_version().decode()

RC_MASK = 1 << 63
FACTOR_DTYPE = np.dtype([("start", "<u8"), ("length", "<u8"), ("ref", "<u8")])
# nolzss_rlz_hit (include/nolzss_hip.h): an occurrence of a pattern in the reference block
HIT_DTYPE = np.dtype([("position", "<u8"), ("record", "<u4"), ("is_rc", "<u4")])
# an occurrence of a pattern inside a target of an archive (RlzFinderHandle.locate): nolzss_rlz_target_hit
TARGET_HIT_DTYPE = np.dtype([("target", "<u8"), ("position", "<u8"), ("is_rc", "<u4"), ("primary", "<u4")])
# nolzss_rlz_seed: a maximal exact match of a target with the reference block
SEED_DTYPE = np.dtype([("target", "<u8"), ("start", "<u8"), ("length", "<u8"), ("count", "<u8")])
# nolzss_rlz_repeat: a maximal repeat of the reference block itself
REPEAT_DTYPE = np.dtype([("position", "<u8"), ("length", "<u8"), ("count", "<u8"), ("record", "<u4"), ("palindrome", "<u4")])
# nolzss_rlz_chain and nolzss_rlz_chain_anchor (include/nolzss_hip.h): a seed chain and one of its anchors
CHAIN_DTYPE = np.dtype([("target", "<u8"), ("t_start", "<u8"), ("t_end", "<u8"), ("r_start", "<u8"), ("r_end", "<u8"),
                        ("score", "<u8"), ("record", "<u4"), ("is_rc", "<u4"), ("num_anchors", "<u4"), ("primary", "<u4")])
CHAIN_ANCHOR_DTYPE = np.dtype([("t_start", "<u8"), ("position", "<u8"), ("length", "<u8")])
# nolzss_rlz_alignment: the base-level alignment of one seed chain (RlzIndexHandle.align)
ALIGN_DTYPE = np.dtype([("target", "<u8"), ("t_start", "<u8"), ("t_end", "<u8"), ("r_start", "<u8"), ("r_end", "<u8"),
                        ("score", "<u8"), ("edit_distance", "<u8"), ("columns", "<u8"), ("record", "<u4"), ("is_rc", "<u4"),
                        ("num_ops", "<u4"), ("primary", "<u4")])
# nolzss_rlz_variant: an allele of the pileup that passed a variants query (RlzPileupHandle.variants)
VARIANT_DTYPE = np.dtype([("position", "<u8"), ("record_offset", "<u8"), ("record", "<u4"), ("ref_base", "<u4"),
                          ("allele", "<u4"), ("count", "<u4"), ("depth", "<u4"), ("rev", "<u4")])
# nolzss_rlz_insertion: an inserted allele of the pileup that passed an insertions query (RlzPileupHandle.insertions)
INSERTION_DTYPE = np.dtype([("position", "<u8"), ("record_offset", "<u8"), ("record", "<u4"), ("length", "<u4"),
                            ("count", "<u4"), ("depth", "<u4"), ("ins_total", "<u4"), ("truncated", "<u4"),
                            ("bases", "<u8", (2,))])
PILEUP_NORMALIZE = 1     # NOLZSS_RLZ_PILEUP_NORMALIZE
PILEUP_INS_BASES = 64    # NOLZSS_RLZ_PILEUP_INS_BASES
CONSENSUS_STATS = ("called", "low_positions", "substitutions", "deleted", "insertions", "inserted_bases", "truncated_skipped")


def insertion_bases(record) -> bytes:
    """The bases an INSERTION_DTYPE record keeps: the first min(length, 64) of the allele, as ACGT bytes."""
    words = [int(w) for w in record["bases"]]
    n = min(int(record["length"]), PILEUP_INS_BASES)
    return bytes(b"ACGT"[(words[j >> 5] >> (62 - 2 * (j & 31))) & 3] for j in range(n))


# NOLZSS_RLZ_PILEUP_CHANNELS: the eight counters a pileup keeps per block position, in this order
PILEUP_CHANNELS = ("A", "C", "G", "T", "DEL", "INS", "REV", "BREAK")

_default_device = int(os.environ.get("NOLZSS_DEVICE", os.environ.get("LOCAL_RANK", "0")) or 0)


def set_device(device: int) -> None:
    """Select the HIP device used by the calls below (extension; default LOCAL_RANK or 0)."""
    global _default_device
    _default_device = int(device)


def get_device() -> int:
    return _default_device


class Factor:
    """reference: py::class_<Factor>, bindings.cpp:44-48 (ref is reported with RC_MASK stripped)"""
    __slots__ = ("start", "length", "_raw_ref")

    def __init__(self, start=0, length=0, ref=0):
        self.start, self.length, self._raw_ref = start, length, ref

    @property
    def ref(self):
        return self._raw_ref & (RC_MASK - 1)

    @property
    def is_rc(self):
        return bool(self._raw_ref & RC_MASK)


class FastaFactorizationResult:
    """reference: py::class_<FastaFactorizationResult>, bindings.cpp:51-53"""
    __slots__ = ("factors", "sentinel_factor_indices", "sequence_ids")

    def __init__(self, factors=(), sentinel_factor_indices=(), sequence_ids=()):
        self.factors = list(factors)
        self.sentinel_factor_indices = list(sentinel_factor_indices)
        self.sequence_ids = list(sequence_ids)


class FastaPerSequenceFactorizationResult:
    """reference: py::class_<FastaPerSequenceFactorizationResult>, bindings.cpp:1208-1213"""
    __slots__ = ("per_sequence_factors", "sequence_ids")

    def __init__(self, per_sequence_factors=(), sequence_ids=()):
        self.per_sequence_factors = list(per_sequence_factors)
        self.sequence_ids = list(sequence_ids)


def _as_buffer(data):
    """1-D, itemsize-1 buffer -> (address, nbytes, keepalive)  (bindings.cpp:59-67)."""
    try:
        mv = memoryview(data)
    except TypeError:
        raise TypeError(f"a bytes-like object is required, not '{type(data).__name__}'")
    if mv.itemsize != 1 or mv.ndim != 1:
        raise ValueError("data must be a 1-dimensional bytes-like object")
    if not mv.c_contiguous:
        mv = memoryview(bytes(mv))
    arr = np.frombuffer(mv, dtype=np.uint8)
    return arr.ctypes.data, arr.size, arr


class _Owned:
    """Frees a library-owned block when the last array that views it is gone."""

    def __init__(self, ptr):
        self.ptr = C.c_void_p(ptr.value)

    def __del__(self):
        lib.nolzss_free(self.ptr)


def _take(ptr, z):
    """library-owned factor array -> numpy structured array: a view of the block (a 2^30-base text has
    1.2 GB of factor records; copying them costs as much as downloading them), freed with the array."""
    if not ptr.value:
        return np.zeros(0, dtype=FACTOR_DTYPE)
    owner = _Owned(ptr)
    if z == 0:
        return np.zeros(0, dtype=FACTOR_DTYPE)
    raw = (C.c_uint64 * (3 * z)).from_address(ptr.value)
    raw._owner = owner
    return np.frombuffer(raw, dtype=FACTOR_DTYPE)


def _tuples3(f):
    return list(zip(f["start"].tolist(), f["length"].tolist(), f["ref"].tolist()))


def _tuples4(f):
    ref = f["ref"]
    is_rc = (ref >> np.uint64(63)).astype(bool)
    clean = ref & np.uint64(RC_MASK - 1)
    return list(zip(f["start"].tolist(), f["length"].tolist(), clean.tolist(), is_rc.tolist()))


# ---- plain mode --------------------------------------------------------------------------
def factorize_array(data, start_pos: int = 0) -> np.ndarray:
    """Extension: factors as a numpy structured array (start, length, ref), no tuple building."""
    p, n, keep = _as_buffer(data)
    out, z = C.c_void_p(), C.c_size_t()
    check(lib.nolzss_factorize(p, n, start_pos, _default_device, C.byref(out), C.byref(z)))
    return _take(out, z.value)


def factorize(data):
    """reference: m.def("factorize"), bindings.cpp:56-77 -> list[(start, length, ref)]"""
    return _tuples3(factorize_array(data))


def count_factors(data) -> int:
    """reference: m.def("count_factors"), bindings.cpp:122-141"""
    p, n, keep = _as_buffer(data)
    z = C.c_size_t()
    check(lib.nolzss_count_factors(p, n, 0, _default_device, C.byref(z)))
    return z.value


def factorize_file(path: str, reserve_hint: int = 0):
    """reference: m.def("factorize_file"), bindings.cpp:96-105 (reserve_hint is a host-vector
    hint in the reference and has no effect here)."""
    out, z = C.c_void_p(), C.c_size_t()
    check(lib.nolzss_factorize_file(os.fsencode(path), 0, _default_device, C.byref(out), C.byref(z)))
    return _tuples3(_take(out, z.value))


def count_factors_file(path: str) -> int:
    """reference: m.def("count_factors_file"), bindings.cpp:157-164"""
    z = C.c_size_t()
    check(lib.nolzss_count_factors_file(os.fsencode(path), 0, _default_device, C.byref(z)))
    return z.value


def factorize_device(data_ptr: int, n: int, stream: int = 0, emit: int = 2, start_pos: int = 0):
    """Extension used by bench.py / the shard dispatcher: the text is already in HBM
    (data_ptr = device address, e.g. torch.Tensor.data_ptr()).
    emit 0: count only; 1: build the factor records in HBM, no download; 2: download them.
    Returns (z, factor array or None)."""
    out, z = C.c_void_p(), C.c_size_t()
    check(lib.nolzss_factorize_device(data_ptr, n, start_pos, _default_device, stream or None, emit,
                                      C.byref(out) if emit == 2 else None, C.byref(z)))
    return z.value, (_take(out, z.value) if emit == 2 else None)


def factorize_batch(texts, devices=None, want_factors: bool = True, with_rc: bool = False):
    """Extension: the per-sequence shard unit of read_nucleotide_fasta
    (reference: genomics/fasta.py:110-122).  Returns (counts, [factor arrays] or None).
    with_rc: every record as factorize_dna_w_rc would (ref carries RC_MASK for reverse-complement
    factors; the per-record step of factorize_fasta_dna_w_rc_per_sequence)."""
    devices = list(devices) if devices is not None else [_default_device]
    bufs = [_as_buffer(t) for t in texts]
    m = len(bufs)
    ptrs = (C.c_void_p * max(m, 1))(*[b[0] for b in bufs])
    lens = (C.c_size_t * max(m, 1))(*[b[1] for b in bufs])
    devs = (C.c_int * len(devices))(*devices)
    out = C.POINTER(C.c_void_p)()
    zs = C.POINTER(C.c_size_t)()
    entry = lib.nolzss_factorize_batch_dna_w_rc if with_rc else lib.nolzss_factorize_batch
    check(entry(ptrs, lens, m, devs, len(devices), C.byref(out) if want_factors else None, C.byref(zs)))
    owner = _BatchResult(out if want_factors else None, zs, m)
    counts = np.ctypeslib.as_array(zs, shape=(m,)).tolist() if m else []
    if not want_factors:
        return counts, None
    # the arrays are views of the library's blocks (a merged run delivers the factors of thousands of
    # records in one block); the blocks live as long as any of the views
    arrays = []
    for j in range(m):
        if counts[j] == 0 or not out[j]:
            arrays.append(np.zeros(0, dtype=FACTOR_DTYPE))
        else:
            raw = (C.c_uint64 * (3 * counts[j])).from_address(out[j])
            raw._owner = owner
            arrays.append(np.frombuffer(raw, dtype=FACTOR_DTYPE))
    return counts, arrays


def count_factors_batch_both(texts, devices=None):
    """Extension: (counts_w_rc, counts_no_rc) of every record -- count_factors_dna_w_rc and count_factors of each --
    from one suffix array per pipeline run (C ABI nolzss_count_factors_batch_both; the per-record pair of the
    reference's compute_sequence_complexity_table, genomics/batch_factorize.py:370-429).  Records: upper-case
    A/C/G/T bytes; an invalid nucleotide raises what count_factors_dna_w_rc raises on that record, lower case is
    refused (ValueError)."""
    devices = list(devices) if devices is not None else [_default_device]
    bufs = [_as_buffer(t) for t in texts]
    m = len(bufs)
    ptrs = (C.c_void_p * max(m, 1))(*[b[0] for b in bufs])
    lens = (C.c_size_t * max(m, 1))(*[b[1] for b in bufs])
    devs = (C.c_int * len(devices))(*devices)
    w_rc = (C.c_size_t * max(m, 1))()
    no_rc = (C.c_size_t * max(m, 1))()
    check(lib.nolzss_count_factors_batch_both(ptrs, lens, m, devs, len(devices), w_rc, no_rc))
    return list(w_rc)[:m], list(no_rc)[:m]


# ---- factor lengths for the shuffled-control significance analysis (genomics/significance.py) ------------------
def _seed_arg(seed) -> int:
    """a shuffle key: an integer in [0, 2^64) (the C ABI takes a uint64_t; nothing is wrapped silently)"""
    seed = operator.index(seed)
    if seed < 0 or seed >= 1 << 64:
        raise ValueError(f"seed must be in [0, 2^64), got {seed}")
    return seed


def _take_u32(ptr, count):
    """library-owned uint32 block -> numpy view, freed with the array (no host copy)"""
    owner = _Owned(ptr)
    if count == 0:
        return np.zeros(0, dtype=np.uint32)
    raw = (C.c_uint32 * count).from_address(ptr.value)
    raw._owner = owner
    return np.frombuffer(raw, dtype=np.uint32)


def _unpack_length_hist(res):
    """nolzss_length_hist -> dict: fwd / rc (int64, threshold bins, bin L = factors of length L), tail_lengths (int64),
    tail_rc (bool), z, and lengths (uint32, factor order) when the call filled them."""
    try:
        T = res.threshold
        out = {"threshold": T, "z": res.z,
               "fwd": np.ctypeslib.as_array(res.fwd, shape=(T,)).astype(np.int64) if T else np.zeros(0, np.int64),
               "rc": np.ctypeslib.as_array(res.rc, shape=(T,)).astype(np.int64) if T else np.zeros(0, np.int64)}
        tc = res.tail_count
        out["tail_lengths"] = (np.ctypeslib.as_array(res.tail_lengths, shape=(tc,)).astype(np.int64) if tc
                               else np.zeros(0, np.int64))
        out["tail_rc"] = (np.ctypeslib.as_array(res.tail_rc, shape=(tc,)).astype(bool) if tc
                          else np.zeros(0, bool))
        if res.lengths:  # handed over to the array (nolzss_free_length_hist then skips it)
            ptr = C.c_void_p(C.cast(res.lengths, C.c_void_p).value)
            res.lengths = None
            out["lengths"] = _take_u32(ptr, res.lengths_count)
    finally:
        lib.nolzss_free_length_hist(C.byref(res))
    return out


def factor_length_histogram(data, with_rc: bool = False, shuffle_seed=None):
    """Extension: the factor-length histogram of `data` (plain mode, or the reverse-complement mode of
    count_factors_dna_w_rc) without factor records; shuffle_seed: histogram of the keyed shuffle shuffle_dna(data,
    shuffle_seed) instead.  C ABI nolzss_factor_length_histogram."""
    p, n, keep = _as_buffer(data)
    res = _lib.LengthHist()
    shuffle = shuffle_seed is not None
    check(lib.nolzss_factor_length_histogram(p, n, 1 if with_rc else 0, 1 if shuffle else 0,
                                             _seed_arg(shuffle_seed) if shuffle else 0, _default_device, C.byref(res)))
    return _unpack_length_hist(res)


def factor_length_histogram_with_lengths(data, with_rc: bool = False):
    """Extension: factor_length_histogram plus the lengths in factor order ('lengths'), from one pipeline run."""
    p, n, keep = _as_buffer(data)
    res = _lib.LengthHist()
    check(lib.nolzss_factor_length_histogram_with_lengths(p, n, 1 if with_rc else 0, _default_device, C.byref(res)))
    return _unpack_length_hist(res)


def fasta_factor_length_histogram(fasta_path, with_rc: bool = True, sanitize_mode: str = "remove_ambiguous",
                                  shuffle_seed=None, want_lengths: bool = False):
    """Extension: the factor-length histogram of the concatenated multiple-DNA form of a FASTA file (the factors of
    factorize_fasta_multiple_dna_{w,no}_rc); shuffle_seed: of its records shuffled on the device; want_lengths (no
    shuffle): also the lengths in factor order."""
    res = _lib.LengthHist()
    path = _str_arg(fasta_path, "fasta_path")
    mode = _sanitize_mode(sanitize_mode)
    if want_lengths:
        if shuffle_seed is not None:
            raise ValueError("want_lengths is for the unshuffled text")
        check(lib.nolzss_fasta_factor_length_histogram_with_lengths(path, 1 if with_rc else 0, mode, _default_device,
                                                                    C.byref(res)))
    else:
        shuffle = shuffle_seed is not None
        check(lib.nolzss_fasta_factor_length_histogram(path, 1 if with_rc else 0, mode, 1 if shuffle else 0,
                                                       _seed_arg(shuffle_seed) if shuffle else 0, _default_device,
                                                       C.byref(res)))
    return _unpack_length_hist(res)


def fasta_shuffled_text(fasta_path, seed, with_rc: bool = True, sanitize_mode: str = "remove_ambiguous") -> bytes:
    """Extension: the prepared string S of a FASTA file with its records shuffled on the device (what
    fasta_factor_length_histogram factorizes)."""
    S, S_len = C.c_void_p(), C.c_size_t()
    check(lib.nolzss_fasta_shuffled_text(_str_arg(fasta_path, "fasta_path"), 1 if with_rc else 0,
                                         _sanitize_mode(sanitize_mode), _seed_arg(seed), _default_device, C.byref(S),
                                         C.byref(S_len)))
    try:
        return C.string_at(S, S_len.value) if S.value else b""
    finally:
        lib.nolzss_free(S)


def factor_lengths(data, with_rc: bool = False) -> np.ndarray:
    """Extension: the length of every factor in factor order (uint32), without factor records.  C ABI
    nolzss_factor_lengths."""
    p, n, keep = _as_buffer(data)
    out, z = C.c_void_p(), C.c_size_t()
    check(lib.nolzss_factor_lengths(p, n, 1 if with_rc else 0, _default_device, C.byref(out), C.byref(z)))
    return _take_u32(out, z.value)


def shuffle_dna(data, seed) -> bytes:
    """Extension: the keyed shuffle of `data` on the device (out[i] = data[pi(i)]); any byte values."""
    p, n, keep = _as_buffer(data)
    out = C.c_void_p()
    seed = _seed_arg(seed)
    check(lib.nolzss_shuffle_dna(p, n, seed, _default_device, C.byref(out)))
    try:
        return C.string_at(out, n) if n else b""
    finally:
        lib.nolzss_free(out)


# ---- strand-bias grid and space-scale histogram binned on the device (genomics/plots.py) ------------------------
def _edges_arg(edges, name):
    if edges is None:
        return None
    a = np.ascontiguousarray(edges, dtype=np.float64)
    if a.ndim != 1:
        raise ValueError(f"{name} must be one-dimensional")
    return a


def _map_request(grid, total_length, min_factor_length, length_edges, position_edges, position_min_bins,
                 position_bin_bp):
    """-> (nolzss_factor_map_request, keepalive).  grid: (x_bins, y_bins) or None."""
    rq = _lib.FactorMapRequest()
    if grid is not None:
        rq.x_bins, rq.y_bins = (operator.index(g) for g in grid)
    total_length = 0 if total_length is None else operator.index(total_length)
    min_factor_length = operator.index(min_factor_length)
    if total_length < 0 or min_factor_length < 0:
        raise ValueError("total_length and min_factor_length must not be negative")
    rq.total_length, rq.min_factor_length = total_length, min_factor_length
    le, pe = _edges_arg(length_edges, "length_edges"), _edges_arg(position_edges, "position_edges")
    if le is not None:
        rq.length_edges, rq.n_length_edges = le.ctypes.data_as(C.POINTER(C.c_double)), le.size
    if pe is not None:
        rq.position_edges, rq.n_position_edges = pe.ctypes.data_as(C.POINTER(C.c_double)), pe.size
    rq.position_min_bins, rq.position_bin_bp = operator.index(position_min_bins), operator.index(position_bin_bp)
    return rq, (le, pe)


def _unpack_factor_maps(res):
    """nolzss_factor_maps -> dict of numpy arrays (copies) and integers; absent maps are None"""
    try:
        out = {k: int(getattr(res, k)) for k in ("z", "z_used", "x_max", "y_max", "unit", "x_bins", "y_bins",
                                                  "kept_forward", "kept_rc", "min_length", "max_length", "max_start")}
        shape = (res.y_bins, res.x_bins)
        for k in ("forward_units", "rc_units"):
            p = getattr(res, k)
            out[k] = np.ctypeslib.as_array(p, shape=shape).copy() if p else None
        hshape = (res.n_length_bins, res.n_position_bins)
        for k in ("hist_forward", "hist_rc"):
            p = getattr(res, k)
            out[k] = np.ctypeslib.as_array(p, shape=hshape).copy() if p else None
        out["position_edges"] = (np.ctypeslib.as_array(res.position_edges, shape=(res.n_position_bins + 1,)).copy()
                                 if res.position_edges else None)
    finally:
        lib.nolzss_free_factor_maps(C.byref(res))
    return out


def factor_maps(data, with_rc: bool = False, grid=None, total_length=None, min_factor_length: int = 1,
                length_edges=None, position_edges=None, position_min_bins: int = 50, position_bin_bp: int = 1_000_000):
    """Extension: strand-bias grid units and / or the space-scale histogram of the factors of `data` (factorize, or
    factorize_dna_w_rc with with_rc), binned on the device from one pipeline run.  C ABI nolzss_factor_maps_text."""
    rq, keep_rq = _map_request(grid, total_length, min_factor_length, length_edges, position_edges, position_min_bins,
                               position_bin_bp)
    p, n, keep = _as_buffer(data)
    res = _lib.FactorMaps()
    check(lib.nolzss_factor_maps_text(p, n, 1 if with_rc else 0, _default_device, C.byref(rq), C.byref(res)))
    return _unpack_factor_maps(res)


def fasta_factor_maps(fasta_path, with_rc: bool = True, sanitize_mode: str = "remove_ambiguous", grid=None,
                      total_length=None, min_factor_length: int = 1, length_edges=None, position_edges=None,
                      position_min_bins: int = 50, position_bin_bp: int = 1_000_000):
    """Extension: factor_maps over the factors of factorize_fasta_multiple_dna_{w,no}_rc (sentinel factors are kept
    whatever min_factor_length).  C ABI nolzss_factor_maps_fasta."""
    rq, keep_rq = _map_request(grid, total_length, min_factor_length, length_edges, position_edges, position_min_bins,
                               position_bin_bp)
    res = _lib.FactorMaps()
    check(lib.nolzss_factor_maps_fasta(_str_arg(fasta_path, "fasta_path"), 1 if with_rc else 0,
                                       _sanitize_mode(sanitize_mode), _default_device, C.byref(rq), C.byref(res)))
    return _unpack_factor_maps(res)


def records_factor_maps(factors, sentinel_factor_indices=(), grid=None, total_length=None, min_factor_length: int = 1,
                        length_edges=None, position_edges=None, position_min_bins: int = 50,
                        position_bin_bp: int = 1_000_000):
    """Extension: factor_maps over host records: a FACTOR_DTYPE array (ref carrying RC_MASK) or an (n, 3) uint64
    array.  C ABI nolzss_factor_maps_records."""
    rq, keep_rq = _map_request(grid, total_length, min_factor_length, length_edges, position_edges, position_min_bins,
                               position_bin_bp)
    f, z = _records_array(factors)
    sent = np.ascontiguousarray(sorted(operator.index(i) for i in sentinel_factor_indices), dtype=np.uint64)
    res = _lib.FactorMaps()
    check(lib.nolzss_factor_maps_records(f.ctypes.data if z else None, z, sent.ctypes.data if sent.size else None,
                                         sent.size, _default_device, C.byref(rq), C.byref(res)))
    return _unpack_factor_maps(res)


def _records_array(factors):
    """-> (contiguous array, z): a FACTOR_DTYPE array (ref carrying RC_MASK) or an (n, 3) uint64 array"""
    f = np.asarray(factors)
    if f.dtype != FACTOR_DTYPE:
        f = np.ascontiguousarray(f, dtype=np.uint64)
        if f.size and (f.ndim != 2 or f.shape[1] != 3):
            raise ValueError("factors must be a FACTOR_DTYPE array or an (n, 3) uint64 array")
        return f, (f.shape[0] if f.size else 0)
    f = np.ascontiguousarray(f)
    return f, f.size


# ---- self dot-plot rasters from resident factors (genomics/plots.py) --------------------------------------------
class DotPlot:
    """Extension: the records of one factorisation kept in device memory (C ABI nolzss_dotplot_*), rendered into
    per-strand max-length rasters, count rasters and a hover table, any number of times.  A context manager;
    close() may be called more than once."""

    def __init__(self, handle):
        self._h = handle
        info = _lib.DotPlotSummary()
        try:
            check(lib.nolzss_dotplot_info(self._h, C.byref(info)))
        except Exception:
            self.close()
            raise
        self.info = {k: int(getattr(info, k)) for k in ("z", "x_max", "y_max", "min_length", "max_length",
                                                        "kept_forward", "kept_rc", "device")}
        n = info.n_sentinel_starts
        self.info["sentinel_starts"] = (np.ctypeslib.as_array(info.sentinel_starts, shape=(n,)).copy() if n
                                        else np.zeros(0, dtype=np.uint64))

    @classmethod
    def _open(cls, call):
        h = C.c_void_p()
        check(call(C.byref(h)))
        return cls(h)

    @classmethod
    def from_text(cls, data, with_rc: bool = False):
        """The factors of factorize (or factorize_dna_w_rc with with_rc).  C ABI nolzss_dotplot_open_text."""
        p, n, keep = _as_buffer(data)
        return cls._open(lambda h: lib.nolzss_dotplot_open_text(p, n, 1 if with_rc else 0, _default_device, h))

    @classmethod
    def from_fasta(cls, fasta_path, with_rc: bool = True, sanitize_mode: str = "remove_ambiguous"):
        """The factors of factorize_fasta_multiple_dna_{w,no}_rc.  C ABI nolzss_dotplot_open_fasta."""
        path, mode = _str_arg(fasta_path, "fasta_path"), _sanitize_mode(sanitize_mode)
        return cls._open(lambda h: lib.nolzss_dotplot_open_fasta(path, 1 if with_rc else 0, mode, _default_device, h))

    @classmethod
    def from_records(cls, factors, sentinel_factor_indices=()):
        """Host records, uploaded once.  C ABI nolzss_dotplot_open_records."""
        f, z = _records_array(factors)
        sent = np.ascontiguousarray(sorted(operator.index(i) for i in sentinel_factor_indices), dtype=np.uint64)
        return cls._open(lambda h: lib.nolzss_dotplot_open_records(
            f.ctypes.data if z else None, z, sent.ctypes.data if sent.size else None, sent.size, _default_device, h))

    def render(self, x_range, y_range, width: int = 800, height: int = 800, min_factor_length: int = 1,
               length_range=None, hover_bins: int = 0, counts: bool = False):
        """One view -> dict: max_forward, max_rc (and count_forward, count_rc with counts) as uint32 arrays of shape
        (height, width), row 0 the lowest y; visible_forward, visible_rc; with hover_bins, hover_start, hover_length,
        hover_ref (uint64, shape (hover_bins,), ref carrying RC_MASK).  length_range = (lo, hi), hi = 0 or None: no
        upper bound."""
        if self._h is None:
            raise ValueError("the dot plot is closed")
        v = _lib.DotPlotView()
        bounds = [operator.index(b) for b in (*x_range, *y_range)]
        lo, hi = (0, 0) if length_range is None else length_range
        scalars = [operator.index(width), operator.index(height), operator.index(min_factor_length),
                   operator.index(lo), 0 if hi is None else operator.index(hi), operator.index(hover_bins)]
        if len(bounds) != 4 or min(bounds) < 0 or min(scalars) < 0:
            raise ValueError("x_range and y_range are pairs; no bound, size or length may be negative")
        if max(bounds) >= 1 << 64 or max(scalars[:2] + scalars[5:]) >= 1 << 32 or max(scalars[2:5]) >= 1 << 64:
            raise ValueError("x_range, y_range, width, height, hover_bins or a length is out of range")
        v.x_lo, v.x_hi, v.y_lo, v.y_hi = bounds
        v.width, v.height, v.min_factor_length, v.len_lo, v.len_hi, v.hover_bins = scalars
        v.want_counts = 1 if counts else 0
        res = _lib.DotPlotRaster()
        check(lib.nolzss_dotplot_render(self._h, C.byref(v), C.byref(res)))
        try:
            out = {"visible_forward": int(res.visible_forward), "visible_rc": int(res.visible_rc)}
            for k in ("max_forward", "max_rc", "count_forward", "count_rc"):
                p = getattr(res, k)
                out[k] = np.ctypeslib.as_array(p, shape=(res.height, res.width)).copy() if p else None
            for k in ("hover_start", "hover_length", "hover_ref"):
                p = getattr(res, k)
                out[k] = np.ctypeslib.as_array(p, shape=(res.hover_bins,)).copy() if p else None
        finally:
            lib.nolzss_free_dotplot_raster(C.byref(res))
        return out

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h is not None:
            check(lib.nolzss_dotplot_close(h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def debug_position_edges(genome_end: int, min_bins: int = 50, bin_bp: int = 1_000_000) -> np.ndarray:
    """Host only: the position ladder of the space-scale histogram (C ABI nolzss_debug_position_edges)."""
    e, n = C.c_void_p(), C.c_size_t()
    check(lib.nolzss_debug_position_edges(genome_end, min_bins, bin_bp, C.byref(e), C.byref(n)))
    try:
        return np.ctypeslib.as_array(C.cast(e, C.POINTER(C.c_double)), shape=(n.value,)).copy()
    finally:
        lib.nolzss_free(e)


def factorize_batch_device(data_ptrs, lengths, emit: int = 0):
    """Extension (measurement): per-sequence batch over records resident in device memory
    (C ABI nolzss_factorize_batch_device); returns the factor count of every record."""
    m = len(data_ptrs)
    ptrs = (C.c_void_p * max(m, 1))(*data_ptrs)
    lens = (C.c_size_t * max(m, 1))(*lengths)
    zs = (C.c_size_t * max(m, 1))()
    check(lib.nolzss_factorize_batch_device(ptrs, lens, m, _default_device, emit, zs))
    return [zs[j] for j in range(m)]


class UnsupportedInput(Exception):
    """The native host-side reader does not take this input (NOLZSS_ERR_UNSUPPORTED): parse it in Python."""


class _FastaResult:
    """Frees a nolzss_nucleotide_fasta when the last array that views its blocks is gone."""

    def __init__(self, res):
        self.res = res

    def __del__(self):
        lib.nolzss_free_nucleotide_fasta(C.byref(self.res))


def read_nucleotide_fasta_arrays(path, devices=None, want_factors: bool = True, shard_index: int = 0,
                                 shard_count: int = 1):
    """Extension: the native form of genomics.read_nucleotide_fasta (reference: genomics/fasta.py:79-126;
    C ABI nolzss_read_nucleotide_fasta) -- the file is read, parsed and checked on the host by the
    library, every record of this shard factorized as one per-sequence batch.  Returns
    (ids, lengths, counts, owners, factor arrays or None); arrays of records this shard does not own are
    None.  Raises RuntimeError with the reference's FASTAError text, UnsupportedInput for non-ASCII files."""
    devices = list(devices) if devices is not None else [_default_device]
    devs = (C.c_int * len(devices))(*devices)
    res = _lib.NucleotideFasta()
    rc = lib.nolzss_read_nucleotide_fasta(os.fsencode(str(path)), devs, len(devices), 1 if want_factors else 0,
                                          shard_index, shard_count, C.byref(res))
    if rc == _lib.ERR_UNSUPPORTED:
        raise UnsupportedInput(lib.nolzss_last_error().decode("utf-8", "replace"))
    check(rc)
    owner = _FastaResult(res)
    m = res.num_sequences
    blob = C.string_at(res.sequence_ids, res.sequence_ids_bytes) if res.sequence_ids_bytes else b""
    ids = [x.decode("utf-8") for x in blob.split(b"\x00")[:m]]
    lengths = [res.lengths[j] for j in range(m)]
    counts = [res.counts[j] for j in range(m)]
    owners = [res.owners[j] for j in range(m)]
    arrays = None
    if want_factors:
        arrays = []
        for j in range(m):
            if owners[j] != shard_index:
                arrays.append(None)
            elif counts[j] == 0 or not res.factors[j]:
                arrays.append(np.zeros(0, dtype=FACTOR_DTYPE))
            else:
                raw = (C.c_uint64 * (3 * counts[j])).from_address(res.factors[j])
                raw._owner = owner
                arrays.append(np.frombuffer(raw, dtype=FACTOR_DTYPE))
    return ids, lengths, counts, owners, arrays


class _BatchResult:
    """Frees the result of nolzss_factorize_batch when the last array that views it is gone."""

    def __init__(self, out, zs, m):
        self.out, self.zs, self.m = out, zs, m

    def __del__(self):
        lib.nolzss_free_batch(self.out, self.zs, self.m)


# ---- reverse-complement DNA mode -----------------------------------------------------------
def factorize_dna_w_rc_array(data) -> np.ndarray:
    p, n, keep = _as_buffer(data)
    out, z = C.c_void_p(), C.c_size_t()
    check(lib.nolzss_factorize_dna_w_rc(p, n, _default_device, C.byref(out), C.byref(z)))
    return _take(out, z.value)


def factorize_dna_w_rc(data):
    """reference: bindings.cpp:207-228 -> list[(start, length, ref & ~RC_MASK, is_rc)]"""
    return _tuples4(factorize_dna_w_rc_array(data))


def factorize_dna_w_rc_device(data_ptr: int, n: int, stream: int = 0, emit: int = 2):
    """Extension (bench.py, BASELINE config 5): factorize_dna_w_rc of a text that is already in HBM
    (data_ptr = device address).  emit 0: count only; 1: factor records built in HBM, no download;
    2: download them.  Returns (z, factor array or None)."""
    out, z = C.c_void_p(), C.c_size_t()
    check(lib.nolzss_factorize_dna_w_rc_device(data_ptr, n, _default_device, stream or None, emit,
                                               C.byref(out) if emit == 2 else None, C.byref(z)))
    return z.value, (_take(out, z.value) if emit == 2 else None)


def count_factors_dna_w_rc(data) -> int:
    """reference: bindings.cpp:276-295"""
    p, n, keep = _as_buffer(data)
    z = C.c_size_t()
    check(lib.nolzss_count_factors_dna_w_rc(p, n, _default_device, C.byref(z)))
    return z.value


def factorize_multiple_dna_w_rc_array(data, start_pos: int = 0) -> np.ndarray:
    p, n, keep = _as_buffer(data)
    out, z = C.c_void_p(), C.c_size_t()
    check(lib.nolzss_factorize_multiple_dna_w_rc(p, n, start_pos, _default_device, C.byref(out), C.byref(z)))
    return _take(out, z.value)


def factorize_multiple_dna_w_rc(data):
    """reference: bindings.cpp:361-382"""
    return _tuples4(factorize_multiple_dna_w_rc_array(data))


def count_factors_multiple_dna_w_rc(data) -> int:
    """reference: bindings.cpp:427-446"""
    p, n, keep = _as_buffer(data)
    z = C.c_size_t()
    check(lib.nolzss_count_factors_multiple_dna_w_rc(p, n, 0, _default_device, C.byref(z)))
    return z.value


def prepare_multiple_dna_sequences_w_rc_bytes(sequences):
    """Extension: like prepare_multiple_dna_sequences_w_rc but returns the prepared string as
    bytes, so sentinel values >= 128 (more than ~61 sequences) survive."""
    seqs = [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in sequences]
    k = len(seqs)
    arr = (C.c_char_p * max(k, 1))(*seqs)
    lens = (C.c_size_t * max(k, 1))(*[len(s) for s in seqs])
    S, S_len, orig = C.c_void_p(), C.c_size_t(), C.c_size_t()
    sp, ns = C.c_void_p(), C.c_size_t()
    check(lib.nolzss_prepare_multiple_dna_w_rc(arr, lens, k, C.byref(S), C.byref(S_len), C.byref(orig),
                                               C.byref(sp), C.byref(ns)))
    try:
        data = C.string_at(S, S_len.value) if S.value else b""
        sent = []
        if sp.value and ns.value:
            sent = np.ctypeslib.as_array(C.cast(sp, C.POINTER(C.c_uint64)), shape=(ns.value,)).tolist()
    finally:
        lib.nolzss_free(S)
        lib.nolzss_free(sp)
    return data, orig.value, sent


def prepare_multiple_dna_sequences_w_rc(sequences):
    """reference: bindings.cpp:732-740 -> (prepared_string: str, original_length, sentinel_positions).
    The reference returns a std::string through pybind11, i.e. a UTF-8-decoded str; sentinel
    bytes >= 128 therefore raise UnicodeDecodeError there, and do so here as well."""
    data, orig, sent = prepare_multiple_dna_sequences_w_rc_bytes(sequences)
    return data.decode("utf-8"), orig, sent


# ---- reference + target factorization and v2 binary files -----------
def _str_arg(x, name):
    """pybind11 std::string argument: str (UTF-8 encoded) or bytes."""
    if isinstance(x, str):
        return x.encode("utf-8")
    if isinstance(x, (bytes, bytearray)):
        return bytes(x)
    raise TypeError(f"{name} must be str or bytes, not {type(x).__name__}")


def factorize_w_reference(reference_seq, target_seq):
    """reference: bindings.cpp:868-880 -> list[(start, length, ref)], absolute positions in
    reference + '\\x01' + target."""
    r, t = _str_arg(reference_seq, "reference_seq"), _str_arg(target_seq, "target_seq")
    out, z = C.c_void_p(), C.c_size_t()
    check(lib.nolzss_factorize_w_reference(r, len(r), t, len(t), _default_device, C.byref(out), C.byref(z)))
    return _tuples3(_take(out, z.value))


def factorize_w_reference_file(reference_seq, target_seq, out_path) -> int:
    """reference: bindings.cpp:907-915"""
    r, t = _str_arg(reference_seq, "reference_seq"), _str_arg(target_seq, "target_seq")
    z = C.c_size_t()
    check(lib.nolzss_factorize_w_reference_file(r, len(r), t, len(t), os.fsencode(out_path), _default_device,
                                                C.byref(z)))
    return z.value


def factorize_dna_w_reference_seq(reference_seq, target_seq):
    """reference: bindings.cpp:800-808 -> list[(start, length, ref & ~RC_MASK, is_rc)]"""
    r, t = _str_arg(reference_seq, "reference_seq"), _str_arg(target_seq, "target_seq")
    out, z = C.c_void_p(), C.c_size_t()
    check(lib.nolzss_factorize_dna_w_reference_seq(r, len(r), t, len(t), _default_device, C.byref(out), C.byref(z)))
    return _tuples4(_take(out, z.value))


def factorize_dna_w_reference_seq_file(reference_seq, target_seq, out_path) -> int:
    """reference: bindings.cpp:837-845"""
    r, t = _str_arg(reference_seq, "reference_seq"), _str_arg(target_seq, "target_seq")
    z = C.c_size_t()
    check(lib.nolzss_factorize_dna_w_reference_seq_file(r, len(r), t, len(t), os.fsencode(out_path),
                                                        _default_device, C.byref(z)))
    return z.value


def write_factors_binary_file(in_path, out_path) -> int:
    """reference: bindings.cpp:180-187 (input is a FILE path; v2 footer at the end)"""
    z = C.c_size_t()
    check(lib.nolzss_write_factors_binary_file(_str_arg(in_path, "in_path"), _str_arg(out_path, "out_path"),
                                               _default_device, C.byref(z)))
    return z.value


def write_factors_binary_file_dna_w_rc(in_path, out_path) -> int:
    """reference: bindings.cpp (write_factors_binary_file_dna_w_rc), factorizer.cpp:597-635"""
    z = C.c_size_t()
    check(lib.nolzss_write_factors_binary_file_dna_w_rc(_str_arg(in_path, "in_path"), _str_arg(out_path, "out_path"),
                                                        _default_device, C.byref(z)))
    return z.value


# ---- concatenated multi-sequence FASTA ---------------------------------------
def _sanitize_mode(mode: str) -> int:
    """reference: parse_fasta_sanitization_mode, bindings.cpp:29-37"""
    if mode == "remove_ambiguous":
        return 0
    if mode == "strict":
        return 1
    raise ValueError(f"Invalid sanitize_mode: '{mode}'. Expected 'remove_ambiguous' or 'strict'.")


def prepare_multiple_dna_sequences_no_rc_bytes(sequences):
    seqs = [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in sequences]
    k = len(seqs)
    arr = (C.c_char_p * max(k, 1))(*seqs)
    lens = (C.c_size_t * max(k, 1))(*[len(s) for s in seqs])
    S, S_len, orig = C.c_void_p(), C.c_size_t(), C.c_size_t()
    sp, ns = C.c_void_p(), C.c_size_t()
    check(lib.nolzss_prepare_multiple_dna_no_rc(arr, lens, k, C.byref(S), C.byref(S_len), C.byref(orig),
                                                C.byref(sp), C.byref(ns)))
    try:
        data = C.string_at(S, S_len.value) if S.value else b""
        sent = []
        if sp.value and ns.value:
            sent = np.ctypeslib.as_array(C.cast(sp, C.POINTER(C.c_uint64)), shape=(ns.value,)).tolist()
    finally:
        lib.nolzss_free(S)
        lib.nolzss_free(sp)
    return data, orig.value, sent


def prepare_multiple_dna_sequences_no_rc(sequences):
    """reference: bindings.cpp (prepare_multiple_dna_sequences_no_rc) -> (str, original_length,
    sentinel_positions); sentinel bytes >= 128 raise UnicodeDecodeError as they do through pybind11."""
    data, orig, sent = prepare_multiple_dna_sequences_no_rc_bytes(sequences)
    return data.decode("utf-8"), orig, sent


def _unpack_fasta_result(res):
    try:
        z = res.num_factors
        if z:
            raw = np.ctypeslib.as_array(C.cast(res.factors, C.POINTER(C.c_uint64)), shape=(z * 3,)).copy()
            factors = _tuples4(raw.view(FACTOR_DTYPE))
        else:
            factors = []
        sent = []
        if res.num_sentinels:
            sent = np.ctypeslib.as_array(C.cast(res.sentinel_factor_indices, C.POINTER(C.c_uint64)),
                                         shape=(res.num_sentinels,)).tolist()
        blob = C.string_at(res.sequence_ids, res.sequence_ids_bytes) if res.sequence_ids_bytes else b""
        ids = [x.decode("utf-8") for x in blob.split(b"\x00")[:res.num_sequences]]
    finally:
        lib.nolzss_free_fasta_result(C.byref(res))
    return factors, sent, ids


def _fasta_multiple(fasta_path, sanitize_mode, with_rc):
    res = _lib.FastaResult()
    check(lib.nolzss_factorize_fasta_multiple_dna(_str_arg(fasta_path, "fasta_path"), 1 if with_rc else 0,
                                                  _sanitize_mode(sanitize_mode), _default_device, C.byref(res)))
    return _unpack_fasta_result(res)


def factorize_dna_rc_w_ref_fasta_files(reference_fasta_path, target_fasta_path,
                                       sanitize_mode: str = "remove_ambiguous"):
    """reference: bindings.cpp:563-585 -> (factors, sentinel factor indices, sequence ids); the
    factors cover the target records only and may point into the reference records."""
    res = _lib.FastaResult()
    check(lib.nolzss_factorize_dna_rc_w_ref_fasta_files(
        _str_arg(reference_fasta_path, "reference_fasta_path"), _str_arg(target_fasta_path, "target_fasta_path"),
        _sanitize_mode(sanitize_mode), _default_device, C.byref(res)))
    return _unpack_fasta_result(res)


def write_factors_dna_w_reference_fasta_files_to_binary(reference_fasta_path, target_fasta_path, out_path,
                                                        sanitize_mode: str = "remove_ambiguous") -> int:
    """reference: fasta_processor.cpp:381-390"""
    z = C.c_size_t()
    check(lib.nolzss_write_factors_dna_w_reference_fasta_files_to_binary(
        _str_arg(reference_fasta_path, "reference_fasta_path"), _str_arg(target_fasta_path, "target_fasta_path"),
        _str_arg(out_path, "out_path"), _sanitize_mode(sanitize_mode), _default_device, C.byref(z)))
    return z.value


def parallel_write_factors_dna_w_reference_fasta_files_to_binary(reference_fasta_path, target_fasta_path, out_path,
                                                                 num_threads: int = 0,
                                                                 sanitize_mode: str = "remove_ambiguous") -> int:
    return write_factors_dna_w_reference_fasta_files_to_binary(reference_fasta_path, target_fasta_path, out_path,
                                                               sanitize_mode)


def _read_input_file(path):
    path = os.fsdecode(_str_arg(path, "path"))
    try:
        with open(path, "rb") as fh:
            return fh.read()
    except OSError:
        raise RuntimeError(f"Cannot open input file: {path}")   # factorizer.cpp:498-500


def factorize_file_dna_w_rc(path, reserve_hint: int = 0):
    """reference: noLZSS::factorize_file_dna_w_rc, factorizer.cpp:525-545"""
    return factorize_dna_w_rc(_read_input_file(path))


def count_factors_file_dna_w_rc(path) -> int:
    """reference: factorizer.cpp:575-577"""
    return count_factors_dna_w_rc(_read_input_file(path))


def factorize_file_multiple_dna_w_rc(path, reserve_hint: int = 0):
    """reference: factorizer.cpp:658-686 (the file holds an already prepared string)"""
    return factorize_multiple_dna_w_rc(_read_input_file(path))


def count_factors_file_multiple_dna_w_rc(path) -> int:
    """reference: factorizer.cpp:707-732"""
    return count_factors_multiple_dna_w_rc(_read_input_file(path))


def write_factors_binary_file_multiple_dna_w_rc(in_path, out_path) -> int:
    """reference: factorizer.cpp:751-790: no names, no sentinels, total_length = file size"""
    data = _read_input_file(in_path)
    f = factorize_multiple_dna_w_rc_array(data)
    f = np.ascontiguousarray(f)
    check(lib.nolzss_write_factor_file(_str_arg(out_path, "out_path"), f.ctypes.data if len(f) else None, len(f), 0, 0,
                                       len(data), None, 0))
    return len(f)


def factorize_fasta_multiple_dna_w_rc(fasta_path, sanitize_mode: str = "remove_ambiguous"):
    """reference: bindings.cpp:511-536 -> (factors as (start, length, ref, is_rc), sentinel factor
    indices, sequence ids)."""
    return _fasta_multiple(fasta_path, sanitize_mode, True)


def factorize_fasta_multiple_dna_no_rc(fasta_path, sanitize_mode: str = "remove_ambiguous"):
    """reference: bindings.cpp:611-636"""
    return _fasta_multiple(fasta_path, sanitize_mode, False)


def _write_fasta_multiple(fasta_path, out_path, sanitize_mode, with_rc):
    z = C.c_size_t()
    check(lib.nolzss_write_factors_binary_file_fasta_multiple_dna(
        _str_arg(fasta_path, "fasta_path"), _str_arg(out_path, "out_path"), 1 if with_rc else 0,
        _sanitize_mode(sanitize_mode), _default_device, C.byref(z)))
    return z.value


def write_factors_binary_file_fasta_multiple_dna_w_rc(fasta_path, out_path, sanitize_mode: str = "remove_ambiguous"):
    """reference: fasta_processor.cpp:345-351"""
    return _write_fasta_multiple(fasta_path, out_path, sanitize_mode, True)


def write_factors_binary_file_fasta_multiple_dna_no_rc(fasta_path, out_path, sanitize_mode: str = "remove_ambiguous"):
    """reference: fasta_processor.cpp:353-359"""
    return _write_fasta_multiple(fasta_path, out_path, sanitize_mode, False)


def _fasta_per_sequence(fasta_path, sanitize_mode, with_rc, want_factors, out_dir=None):
    res = _lib.FastaPerSequenceResult()
    check(lib.nolzss_factorize_fasta_per_sequence(
        _str_arg(fasta_path, "fasta_path"), 1 if with_rc else 0, _sanitize_mode(sanitize_mode),
        1 if want_factors else 0, _str_arg(out_dir, "out_dir") if out_dir is not None else None,
        _default_device, C.byref(res)))
    try:
        m = res.num_sequences
        counts = [res.counts[j] for j in range(m)]
        per_seq = None
        if want_factors:
            per_seq = []
            for j in range(m):
                if counts[j] == 0 or not res.factors[j]:
                    per_seq.append([])
                else:
                    raw = np.ctypeslib.as_array(C.cast(res.factors[j], C.POINTER(C.c_uint64)),
                                                shape=(counts[j] * 3,)).copy()
                    per_seq.append(_tuples4(raw.view(FACTOR_DTYPE)))
        blob = C.string_at(res.sequence_ids, res.sequence_ids_bytes) if res.sequence_ids_bytes else b""
        ids = [x.decode("utf-8") for x in blob.split(b"\x00")[:m]]
    finally:
        lib.nolzss_free_fasta_per_sequence_result(C.byref(res))
    return per_seq, counts, ids


def factorize_fasta_dna_w_rc_per_sequence(fasta_path, sanitize_mode: str = "remove_ambiguous"):
    """reference: bindings.cpp:1215-1237 -> (per-sequence factor lists, sequence ids)"""
    per_seq, _, ids = _fasta_per_sequence(fasta_path, sanitize_mode, True, True)
    return per_seq, ids


def factorize_fasta_dna_no_rc_per_sequence(fasta_path, sanitize_mode: str = "remove_ambiguous"):
    """reference: bindings.cpp (no-rc twin); the last base of every record is dropped as in
    fasta_processor.cpp:469-471"""
    per_seq, _, ids = _fasta_per_sequence(fasta_path, sanitize_mode, False, True)
    return per_seq, ids


def count_factors_fasta_dna_w_rc_per_sequence(fasta_path, sanitize_mode: str = "remove_ambiguous"):
    """reference: bindings.cpp:1372-1389 -> (counts, sequence ids, total)"""
    _, counts, ids = _fasta_per_sequence(fasta_path, sanitize_mode, True, False)
    return counts, ids, sum(counts)


def count_factors_fasta_dna_no_rc_per_sequence(fasta_path, sanitize_mode: str = "remove_ambiguous"):
    _, counts, ids = _fasta_per_sequence(fasta_path, sanitize_mode, False, False)
    return counts, ids, sum(counts)


def write_factors_binary_file_fasta_dna_w_rc_per_sequence(fasta_path, out_dir, sanitize_mode: str = "remove_ambiguous"):
    """reference: bindings.cpp:1312-1319 -> total number of factors; one <id>.bin per record"""
    _, counts, _ = _fasta_per_sequence(fasta_path, sanitize_mode, True, False, out_dir)
    return sum(counts)


def write_factors_binary_file_fasta_dna_no_rc_per_sequence(fasta_path, out_dir, sanitize_mode: str = "remove_ambiguous"):
    _, counts, _ = _fasta_per_sequence(fasta_path, sanitize_mode, False, False, out_dir)
    return sum(counts)


def parallel_write_factors_binary_file_fasta_dna_w_rc_per_sequence(fasta_path, out_dir, num_threads: int = 0,
                                                                   sanitize_mode: str = "remove_ambiguous"):
    return write_factors_binary_file_fasta_dna_w_rc_per_sequence(fasta_path, out_dir, sanitize_mode)


def parallel_write_factors_binary_file_fasta_dna_no_rc_per_sequence(fasta_path, out_dir, num_threads: int = 0,
                                                                    sanitize_mode: str = "remove_ambiguous"):
    return write_factors_binary_file_fasta_dna_no_rc_per_sequence(fasta_path, out_dir, sanitize_mode)


# ---- thread-parallel API: same results, num_threads is irrelevant on the GPU ---
def _write_arrays(out_path, f, total_length):
    f = np.ascontiguousarray(f)
    check(lib.nolzss_write_factor_file(os.fsencode(out_path), f.ctypes.data if len(f) else None, len(f), 0, 0,
                                       int(total_length), None, 0))
    return len(f)


def parallel_factorize_to_file(text, output_path, num_threads: int = 0, start_pos: int = 0) -> int:
    """reference: bindings.cpp:978-979 over parallel_factorizer.cpp:55-144 (footer :761-765:
    total_length = sum of factor lengths)."""
    data = _str_arg(text, "text")
    if len(data) == 0:
        return 0                                            # parallel_factorizer.cpp:57
    if start_pos >= len(data):
        raise ValueError("start_pos must be less than text length")   # :59-61
    f = factorize_array(data, start_pos=start_pos)
    return _write_arrays(output_path, f, int(f["length"].sum()))


def parallel_factorize_file_to_file(input_path, output_path, num_threads: int = 0, start_pos: int = 0) -> int:
    with open(os.fsdecode(_str_arg(input_path, "input_path")), "rb") as fh:
        return parallel_factorize_to_file(fh.read(), output_path, num_threads, start_pos)


def parallel_factorize_dna_w_rc_to_file(text, output_path, num_threads: int = 0) -> int:
    """reference: parallel_factorizer.cpp:1001-1017"""
    data = _str_arg(text, "text")
    if len(data) == 0:
        return 0
    f = factorize_dna_w_rc_array(data)
    return _write_arrays(output_path, f, int(f["length"].sum()))


def parallel_factorize_file_dna_w_rc_to_file(input_path, output_path, num_threads: int = 0) -> int:
    """reference: parallel_factorizer.cpp:1031-1041"""
    path = os.fsdecode(_str_arg(input_path, "input_path"))
    try:
        with open(path, "rb") as fh:
            data = fh.read()
    except OSError:
        raise RuntimeError(f"Cannot open input file: {path}")
    return parallel_factorize_dna_w_rc_to_file(data, output_path, num_threads)


def parallel_write_factors_binary_file_fasta_multiple_dna_w_rc(fasta_path, out_path, num_threads: int = 0,
                                                               sanitize_mode: str = "remove_ambiguous"):
    return _write_fasta_multiple(fasta_path, out_path, sanitize_mode, True)


def parallel_write_factors_binary_file_fasta_multiple_dna_no_rc(fasta_path, out_path, num_threads: int = 0,
                                                                sanitize_mode: str = "remove_ambiguous"):
    return _write_fasta_multiple(fasta_path, out_path, sanitize_mode, False)


# ---- relative LZ: many targets against one reference block (extension) -----------
def _seq_args(sequences, name):
    seqs = [_str_arg(s, name) for s in sequences]
    n = len(seqs)
    return (C.c_char_p * max(n, 1))(*seqs), (C.c_size_t * max(n, 1))(*[len(s) for s in seqs]), n


def _rlz_inputs(reference, targets):
    if isinstance(reference, (str, bytes, bytearray)):
        reference = [reference]
    return _seq_args(reference, "reference") + _seq_args(targets, "target")


def rlz_prepare(reference, targets, with_rc: bool = True) -> dict:
    """Host only: the prepared string of a relative-LZ run, S = Rblk s T1 s .. Tk s [pad] rc-block s ->
    dict(S: bytes, target_offsets: list, block_length, rc_block_start, rcN)."""
    args = _rlz_inputs(reference, targets)
    S, off = C.c_void_p(), C.c_void_p()
    S_len, B, E, rcN = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
    check(lib.nolzss_rlz_prepare(*args, 1 if with_rc else 0, C.byref(S), C.byref(S_len), C.byref(off), C.byref(B),
                                 C.byref(E), C.byref(rcN)))
    try:
        k = args[5]
        offsets = np.ctypeslib.as_array(C.cast(off, C.POINTER(C.c_uint64)), shape=(k,)).tolist() if k else []
        data = C.string_at(S, S_len.value)
    finally:
        lib.nolzss_free(S)
        lib.nolzss_free(off)
    return {"S": data, "target_offsets": offsets, "block_length": B.value, "rc_block_start": E.value, "rcN": rcN.value}


def _unpack_rlz_result(res, want_factors):
    try:
        k = res.num_targets
        out = {"block_length": int(res.block_length),
               "target_offsets": [int(res.target_offsets[j]) for j in range(k)],
               "target_lengths": [int(res.target_lengths[j]) for j in range(k)],
               "counts": [int(res.counts[j]) for j in range(k)], "factors": None}
        if want_factors:
            out["factors"] = []
            for j in range(k):
                z = out["counts"][j]
                if z:
                    raw = np.ctypeslib.as_array(C.cast(res.factors[j], C.POINTER(C.c_uint64)), shape=(z * 3,)).copy()
                    out["factors"].append(raw.view(FACTOR_DTYPE))
                else:
                    out["factors"].append(np.zeros(0, dtype=FACTOR_DTYPE))
        if res.reference_ids:
            blob = C.string_at(res.reference_ids, res.reference_ids_bytes)
            out["reference_ids"] = [x.decode("utf-8") for x in blob.split(b"\x00")[:res.num_references]]
            blob = C.string_at(res.target_ids, res.target_ids_bytes)
            out["target_ids"] = [x.decode("utf-8") for x in blob.split(b"\x00")[:k]]
    finally:
        lib.nolzss_free_rlz_result(C.byref(res))
    return out


def rlz_factorize_arrays(reference, targets, with_rc: bool = True, want_factors: bool = True) -> dict:
    """Every target factorized against the reference block only -> dict(block_length, target_offsets, target_lengths,
    counts, factors: one (start, length, ref) array per target in coordinates of the prepared string -- start absolute,
    a match has ref < block_length (plus RC_MASK), a literal ref = start -- or None without want_factors)."""
    args = _rlz_inputs(reference, targets)
    res = _lib.RlzResult()
    check(lib.nolzss_rlz_factorize(*args, 1 if with_rc else 0, 1 if want_factors else 0, _default_device, C.byref(res)))
    return _unpack_rlz_result(res, want_factors)


def rlz_factorize_fasta_arrays(reference_fasta_path, target_fasta_path, with_rc: bool = True,
                               sanitize_mode: str = "remove_ambiguous", want_factors: bool = True) -> dict:
    """rlz_factorize_arrays over the records of two FASTA files, plus reference_ids and target_ids."""
    res = _lib.RlzResult()
    check(lib.nolzss_rlz_factorize_fasta(_str_arg(reference_fasta_path, "reference_fasta_path"),
                                         _str_arg(target_fasta_path, "target_fasta_path"), 1 if with_rc else 0,
                                         _sanitize_mode(sanitize_mode), 1 if want_factors else 0, _default_device,
                                         C.byref(res)))
    return _unpack_rlz_result(res, want_factors)


def debug_rlz_codes(reference, targets, with_rc: bool = True) -> np.ndarray:
    """The relative-LZ code (length, bit 31 = reverse complement, 0 = literal) of every position of the prepared
    string below the sentinel behind the last target; only target positions are specified."""
    args = _rlz_inputs(reference, targets)
    prep = rlz_prepare(reference, targets, with_rc)
    n = prep["target_offsets"][-1] + args[4][args[5] - 1] if args[5] else 0
    code = np.zeros(n, dtype=np.uint32)
    check(lib.nolzss_debug_rlz_codes(*args, 1 if with_rc else 0, _default_device, code.ctypes.data))
    return code


# ---- decoding: factors and literals back to text (extension) ----------------------
def _decode_records(factors):
    """-> contiguous FACTOR_DTYPE array: a FACTOR_DTYPE array (ref carrying RC_MASK), or a sequence of
    (start, length, ref) or (start, length, ref, is_rc) tuples -- with four fields is_rc sets the mask"""
    if isinstance(factors, np.ndarray) and factors.dtype == FACTOR_DTYPE:
        return np.ascontiguousarray(factors)
    rows = list(factors)
    out = np.zeros(len(rows), dtype=FACTOR_DTYPE)
    for k, row in enumerate(rows):
        row = tuple(row)
        if len(row) not in (3, 4):
            raise ValueError("factors must be a FACTOR_DTYPE array or tuples of 3 or 4 fields")
        ref = operator.index(row[2])
        if len(row) == 4 and row[3]:
            ref |= RC_MASK
        out[k] = (operator.index(row[0]), operator.index(row[1]), ref)
    return out


def _info_dict(info):
    return {name: int(getattr(info, name)) for name, _ in _lib.DecodeInfo._fields_}


def literal_symbols(data, factors) -> bytes:
    """Extension: the symbols of the literal records (ref == start) of `factors` in record order, read from `data`:
    with the records, all a decoder needs.  Host only.  C ABI nolzss_literal_symbols."""
    p, n, keep = _as_buffer(data)
    f = _decode_records(factors)
    out, count = C.c_void_p(), C.c_size_t()
    check(lib.nolzss_literal_symbols(p, n, f.ctypes.data if f.size else None, f.size, C.byref(out), C.byref(count)))
    try:
        return C.string_at(out, count.value)
    finally:
        lib.nolzss_free(out)


def decode_array(factors, literals, prefix=b""):
    """Extension: the text of a factorization -> (np.uint8 array of n bytes, info dict).  `literals`: the literal
    symbols in record order (literal_symbols); `prefix`: the known bytes in front of the first record (the reference of
    factorize_w_reference plus its separator, the reference block of relative LZ).  Pointer jumping on the GPU; no
    records: a copy of the prefix, without a device.  C ABI nolzss_decode (its header states the rules)."""
    f = _decode_records(factors)
    lp, ln, keep_l = _as_buffer(literals)
    pp, pn, keep_p = _as_buffer(prefix)
    out, n, info = C.c_void_p(), C.c_size_t(), _lib.DecodeInfo()
    check(lib.nolzss_decode(f.ctypes.data if f.size else None, f.size, lp if ln else None, ln, pp if pn else None, pn,
                            _default_device, C.byref(out), C.byref(n), C.byref(info)))
    owner = _Owned(out)
    if n.value == 0:
        return np.zeros(0, dtype=np.uint8), _info_dict(info)
    raw = (C.c_uint8 * n.value).from_address(out.value)
    raw._owner = owner
    return np.frombuffer(raw, dtype=np.uint8), _info_dict(info)


# ---- factor records: the compact container (extension) ------------------------------------------------
# the fields of nolzss_packed_factors: the counts, and each section with the field that holds its size
PACKED_FACTOR_COUNTS = ("literal_mode", "first_start", "z", "n_literals", "decoded")
PACKED_FACTOR_SECTIONS = (("control", "control_bytes"), ("data", "data_bytes"), ("literals", "literal_bytes"))


def _packed_factors_out(p):
    """a filled nolzss_packed_factors -> the dict of sections; the struct is freed"""
    try:
        out = {name: int(getattr(p, name)) for name in PACKED_FACTOR_COUNTS}
        for name, size in PACKED_FACTOR_SECTIONS:
            out[name] = C.string_at(getattr(p, name), getattr(p, size))
    finally:
        lib.nolzss_free_packed_factors(C.byref(p))
    return out


def _packed_factors_in(sections):
    """the dict of sections -> (nolzss_packed_factors over buffers of this process, keepalive)"""
    p, keep = _lib.PackedFactors(), []
    for name in PACKED_FACTOR_COUNTS:
        setattr(p, name, operator.index(sections[name]))
    for name, size in PACKED_FACTOR_SECTIONS:
        raw = bytes(sections[name])
        buf = C.create_string_buffer(raw, len(raw)) if raw else None
        keep.append(buf)
        setattr(p, name, C.cast(buf, C.c_void_p) if buf is not None else None)
        setattr(p, size, len(raw))
    return p, keep


def factorize_packed(data, with_rc: bool = False, literals: bool = True) -> dict:
    """Extension: factorize (with_rc: as factorize_dna_w_rc) and pack the records on the device -> the sections of the
    compact container: literal_mode, first_start, z, n_literals, decoded and the bytes of control, data and literals
    (`literals` False: literal_mode 2, a factor file without the symbols).  Only the sections cross PCIe.  C ABI
    nolzss_factorize_packed (its header states the format)."""
    ptr, n, keep = _as_buffer(data)
    p = _lib.PackedFactors()
    check(lib.nolzss_factorize_packed(ptr if n else None, n, 1 if with_rc else 0, 1 if literals else 0, _default_device,
                                      C.byref(p)))
    return _packed_factors_out(p)


def factorize_packed_device(data_ptr: int, n: int, with_rc: bool = False, literals: bool = True, stream: int = 0) -> dict:
    """factorize_packed over n bytes resident in device memory (C ABI nolzss_factorize_packed_device)."""
    p = _lib.PackedFactors()
    check(lib.nolzss_factorize_packed_device(C.c_void_p(data_ptr), n, 1 if with_rc else 0, 1 if literals else 0,
                                             _default_device, C.c_void_p(stream), C.byref(p)))
    return _packed_factors_out(p)


def pack_factors(factors, literals=None) -> dict:
    """Extension: host records (a FACTOR_DTYPE array or tuples, as decode takes them) and their literal symbols
    (literal_symbols; None: literal_mode 2) -> the sections of the compact container, packed on the device.  C ABI
    nolzss_factors_pack (its header states what is refused)."""
    f = _decode_records(factors)
    lp, ln, keep = _as_buffer(literals) if literals is not None else (None, 0, None)
    p = _lib.PackedFactors()
    check(lib.nolzss_factors_pack(f.ctypes.data if f.size else None, f.size, lp if ln else None, ln,
                                  0 if literals is None else 1, _default_device, C.byref(p)))
    return _packed_factors_out(p)


def unpack_factors(sections):
    """Extension: the sections of the compact container (UNTRUSTED) -> (FACTOR_DTYPE records, literal bytes or None
    for literal_mode 2), expanded and checked on the device.  C ABI nolzss_factors_unpack (its header states the rules)."""
    p, keep = _packed_factors_in(sections)
    rec, lit, z, ln = C.c_void_p(), C.c_void_p(), C.c_size_t(), C.c_size_t()
    check(lib.nolzss_factors_unpack(C.byref(p), _default_device, C.byref(rec), C.byref(z), C.byref(lit), C.byref(ln)))
    try:
        literals = None if p.literal_mode == 2 else C.string_at(lit, ln.value) if lit.value else b""
    finally:
        lib.nolzss_free(lit)
    return _take(rec, z.value), literals


def decode_packed_array(sections, prefix=b""):
    """Extension: the text of packed factors -> (np.uint8 array of first_start + decoded bytes, info dict); the records
    are expanded and decoded in device memory.  `prefix`: the first_start known bytes in front of the first record.
    C ABI nolzss_decode_packed."""
    p, keep = _packed_factors_in(sections)
    pp, pn, keep_p = _as_buffer(prefix)
    out, n, info = C.c_void_p(), C.c_size_t(), _lib.DecodeInfo()
    check(lib.nolzss_decode_packed(C.byref(p), pp if pn else None, pn, _default_device, C.byref(out), C.byref(n),
                                   C.byref(info)))
    owner = _Owned(out)
    if n.value == 0:
        return np.zeros(0, dtype=np.uint8), _info_dict(info)
    raw = (C.c_uint8 * n.value).from_address(out.value)
    raw._owner = owner
    return np.frombuffer(raw, dtype=np.uint8), _info_dict(info)


# ---- relative-LZ archive: ranges of the targets from resident records (genomics/rlz.py) ------------------------
def _ranges_array(ranges):
    """-> contiguous (q, 3) uint64 array of (target index, lo, hi) rows, the layout of nolzss_rlz_range"""
    r = np.asarray(ranges)
    if r.size == 0:
        return np.zeros((0, 3), dtype=np.uint64)
    if r.ndim != 2 or r.shape[1] != 3 or r.dtype.kind not in "iu":
        raise ValueError("ranges must be (target, lo, hi) rows of integers")
    if r.dtype.kind == "i" and (r < 0).any():
        raise ValueError("ranges: no target, lo or hi may be negative")
    return np.ascontiguousarray(r, dtype=np.uint64)


# the fields of nolzss_rlz_archive_packed: the counts, and each section with the field that holds its size
PACKED_COUNTS = ("block_mode", "literal_mode", "block_length", "z", "n_literals", "decoded", "num_separators")
PACKED_SECTIONS = (("block", "block_bytes"), ("control", "control_bytes"), ("data", "data_bytes"),
                   ("literals", "literal_bytes"))


class RlzArchiveHandle:
    """Extension: the reference block and the records of a relative-LZ collection kept in device memory (C ABI
    nolzss_rlz_archive_*), any number of range extractions from them.  A context manager; close() may be called more
    than once, any other use after it raises ValueError."""

    def __init__(self, handle):
        self._h = handle
        try:
            self._refresh()
        except Exception:
            self.close()
            raise

    def _refresh(self):
        """info and target_lengths from the handle's own table (at open, and after every append)"""
        info = _lib.RlzArchiveSummary()
        check(lib.nolzss_rlz_archive_info(self._h, C.byref(info)))
        self.info = {k: int(getattr(info, k)) for k in ("num_targets", "block_length", "z", "n_literals",
                                                        "total_length", "device", "device_bytes")}
        k = info.num_targets
        self.target_lengths = (np.ctypeslib.as_array(info.target_lengths, shape=(k,)).copy() if k
                               else np.zeros(0, dtype=np.uint64))

    @classmethod
    def open_records(cls, block, records, literals, target_lengths):
        """Host records in the layout of genomics.rlz.absolute_records, uploaded and packed once.  C ABI
        nolzss_rlz_archive_open_records (its header states the rules)."""
        bp, bn, keep_b = _as_buffer(block)
        f = _decode_records(records)
        lp, ln, keep_l = _as_buffer(literals)
        lens = np.ascontiguousarray([operator.index(x) for x in target_lengths], dtype=np.uint64)
        h = C.c_void_p()
        check(lib.nolzss_rlz_archive_open_records(bp if bn else None, bn, f.ctypes.data if f.size else None, f.size,
                                                  lp if ln else None, ln, lens.ctypes.data if lens.size else None,
                                                  lens.size, _default_device, C.byref(h)))
        return cls(h)

    @classmethod
    def open_index(cls, index_handle):
        """An empty archive over the reference block of an RlzIndexHandle, on its device and bound to it; the block is
        unpacked on the device from the index text.  C ABI nolzss_rlz_archive_open_index."""
        h = C.c_void_p()
        check(lib.nolzss_rlz_archive_open_index(index_handle._handle(), C.byref(h)))
        return cls(h)

    def _handle(self):
        if self._h is None:
            raise ValueError("the archive is closed")
        return self._h

    def append_index(self, index_handle, targets) -> dict:
        """One batch matched against the index and appended as len(targets) new targets, the records staying on the
        device -> the call's nolzss_rlz_archive_append_info as a dict.  C ABI nolzss_rlz_archive_append_index."""
        h = self._handle()
        info = _lib.RlzArchiveAppendInfo()
        check(lib.nolzss_rlz_archive_append_index(h, index_handle._handle(), *_seq_args(targets, "target"), C.byref(info)))
        self._refresh()
        return {name: int(getattr(info, name)) for name, _ in _lib.RlzArchiveAppendInfo._fields_}

    def export(self):
        """-> (block bytes, FACTOR_DTYPE records, literals bytes): the host form open_records takes, of an archive of
        either origin.  C ABI nolzss_rlz_archive_export."""
        h = self._handle()
        blk, rec, lit = C.c_void_p(), C.c_void_p(), C.c_void_p()
        bn, z, ln = C.c_size_t(), C.c_size_t(), C.c_size_t()
        check(lib.nolzss_rlz_archive_export(h, C.byref(blk), C.byref(bn), C.byref(rec), C.byref(z), C.byref(lit),
                                            C.byref(ln)))
        try:
            block, literals = C.string_at(blk, bn.value), C.string_at(lit, ln.value)
            if z.value:
                records = np.ctypeslib.as_array(C.cast(rec, C.POINTER(C.c_uint64)), shape=(z.value * 3,)).copy().view(FACTOR_DTYPE)
            else:
                records = np.zeros(0, dtype=FACTOR_DTYPE)
        finally:
            for q in (blk, rec, lit):
                lib.nolzss_free(q)
        return block, records, literals

    def pack(self) -> dict:
        """-> the sections of the compact container, made on the device from the resident records: block_mode,
        literal_mode, block_length, z, n_literals, decoded, num_separators and the bytes of block, control, data and
        literals.  C ABI nolzss_rlz_archive_pack (its header states the format)."""
        h = self._handle()
        p = _lib.RlzArchivePacked()
        check(lib.nolzss_rlz_archive_pack(h, C.byref(p)))
        try:
            out = {name: int(getattr(p, name)) for name in PACKED_COUNTS}
            for name, size in PACKED_SECTIONS:
                out[name] = C.string_at(getattr(p, name), getattr(p, size))
        finally:
            lib.nolzss_free_rlz_archive_packed(C.byref(p))
        return out

    @classmethod
    def open_packed(cls, sections, target_lengths):
        """What pack() returned (or a file held), expanded and checked on the device.  C ABI
        nolzss_rlz_archive_open_packed (its header states the rules)."""
        p = _lib.RlzArchivePacked()
        keep = []
        for name in PACKED_COUNTS:
            setattr(p, name, operator.index(sections[name]))
        for name, size in PACKED_SECTIONS:
            raw = bytes(sections[name])
            buf = C.create_string_buffer(raw, len(raw)) if raw else None
            keep.append(buf)
            setattr(p, name, C.cast(buf, C.c_void_p) if buf is not None else None)
            setattr(p, size, len(raw))
        lens = np.ascontiguousarray([operator.index(x) for x in target_lengths], dtype=np.uint64)
        h = C.c_void_p()
        check(lib.nolzss_rlz_archive_open_packed(C.byref(p), lens.ctypes.data if lens.size else None, lens.size,
                                                 _default_device, C.byref(h)))
        return cls(h)

    def extract_array(self, ranges):
        """(target index, lo, hi) rows -> (uint8 array of the ranges back to back, uint64 offsets of q + 1 entries)."""
        h = self._handle()
        r = _ranges_array(ranges)
        out, offs, total = C.c_void_p(), C.c_void_p(), C.c_uint64()
        check(lib.nolzss_rlz_archive_extract(h, r.ctypes.data if len(r) else None, len(r), C.byref(out), C.byref(offs),
                                             C.byref(total)))
        try:
            offsets = np.ctypeslib.as_array(C.cast(offs, C.POINTER(C.c_uint64)), shape=(len(r) + 1,)).copy()
        finally:
            lib.nolzss_free(offs)
        owner = _Owned(out)
        if total.value == 0:
            return np.zeros(0, dtype=np.uint8), offsets
        raw = (C.c_uint8 * total.value).from_address(out.value)
        raw._owner = owner
        return np.frombuffer(raw, dtype=np.uint8), offsets

    def extract_device(self, ranges, data_ptr: int, capacity: int, stream: int = 0) -> int:
        """The same layout into `capacity` bytes of device memory at data_ptr, on the handle's device (stream as
        factorize_device) -> bytes written.  C ABI nolzss_rlz_archive_extract_device."""
        h = self._handle()
        r = _ranges_array(ranges)
        total = C.c_uint64()
        check(lib.nolzss_rlz_archive_extract_device(h, r.ctypes.data if len(r) else None, len(r),
                                                    C.c_void_p(data_ptr) if data_ptr else None, capacity,
                                                    C.c_void_p(stream) if stream else None, C.byref(total)))
        return total.value

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h is not None:
            check(lib.nolzss_rlz_archive_close(h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- relative-LZ archive: locate patterns inside the targets, through the parse (genomics/rlz.py) ----------------
class RlzFinderHandle:
    """Extension: a snapshot of an index-built archive for pattern queries inside its targets (C ABI
    nolzss_rlz_finder_*).  It keeps the archive and the index handles alive.  A context manager; close() may be called
    more than once, any other use after it raises ValueError."""

    def __init__(self, handle, archive_handle, index_handle):
        self._h, self._archive, self._index = handle, archive_handle, index_handle
        info = _lib.RlzFinderSummary()
        try:
            check(lib.nolzss_rlz_finder_info(self._h, C.byref(info)))
        except Exception:
            self.close()
            raise
        self.info = {name: int(getattr(info, name)) for name, _ in _lib.RlzFinderSummary._fields_}

    @classmethod
    def open(cls, archive_handle, index_handle, max_pattern_length: int = 64, prefix_syms: int = 0):
        """C ABI nolzss_rlz_finder_open (its header states the rules)."""
        M, P = operator.index(max_pattern_length), operator.index(prefix_syms)
        if M < 0 or P < 0:
            raise ValueError("max_pattern_length and prefix_syms must not be negative")
        h = C.c_void_p()
        check(lib.nolzss_rlz_finder_open(archive_handle._handle(), index_handle._handle(), M, P, C.byref(h)))
        return cls(h, archive_handle, index_handle)

    def _handle(self):
        if self._h is None:
            raise ValueError("the finder is closed")
        self._archive._handle()  # (a closed archive or index raises here, not in the library)
        self._index._handle()
        return self._h

    def count(self, patterns) -> np.ndarray:
        """One batch: the occurrences of every pattern in the targets, both strands together (uint64).  C ABI
        nolzss_rlz_finder_count."""
        h = self._handle()
        args = _seq_args(patterns, "pattern")
        counts = np.zeros(args[2], dtype=np.uint64)
        check(lib.nolzss_rlz_finder_count(h, *args, counts.ctypes.data if counts.size else None))
        return counts

    def locate(self, patterns, max_hits: int = 0):
        """One batch -> (counts, offsets, hits): uint64 counts, the q + 1 uint64 offsets of the patterns' hits, and the
        hits as TARGET_HIT_DTYPE, per pattern ascending by (target, position, is_rc); a pattern with more than max_hits
        occurrences (0: no cap) reports its count and no hits.  C ABI nolzss_rlz_finder_locate."""
        h = self._handle()
        max_hits = operator.index(max_hits)
        if max_hits < 0:
            raise ValueError("max_hits must not be negative")
        args = _seq_args(patterns, "pattern")
        counts, offsets = np.zeros(args[2], dtype=np.uint64), np.zeros(args[2] + 1, dtype=np.uint64)
        out, z = C.c_void_p(), C.c_size_t()
        check(lib.nolzss_rlz_finder_locate(h, *args, max_hits, counts.ctypes.data if counts.size else None,
                                           offsets.ctypes.data, C.byref(out), C.byref(z)))
        if not out.value or z.value == 0:
            lib.nolzss_free(out)
            return counts, offsets, np.zeros(0, dtype=TARGET_HIT_DTYPE)
        raw = (C.c_uint64 * (3 * z.value)).from_address(out.value)
        raw._owner = _Owned(out)
        return counts, offsets, np.frombuffer(raw, dtype=TARGET_HIT_DTYPE)

    def kernel(self):
        """Test hook -> (K bytes, kstart, dstart): the kernel text and its interval tables (uint64, intervals + 1
        entries each).  C ABI nolzss_rlz_finder_kernel."""
        h = self._handle()
        K, ks, ds = C.c_void_p(), C.c_void_p(), C.c_void_p()
        n, nI = C.c_size_t(), C.c_size_t()
        check(lib.nolzss_rlz_finder_kernel(h, C.byref(K), C.byref(n), C.byref(ks), C.byref(ds), C.byref(nI)))
        try:
            text = C.string_at(K, n.value)
            kstart = np.ctypeslib.as_array(C.cast(ks, C.POINTER(C.c_uint64)), shape=(nI.value + 1,)).copy()
            dstart = np.ctypeslib.as_array(C.cast(ds, C.POINTER(C.c_uint64)), shape=(nI.value + 1,)).copy()
        finally:
            for p in (K, ks, ds):
                lib.nolzss_free(p)
        return text, kstart, dstart

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h is not None:
            check(lib.nolzss_rlz_finder_close(h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _chain_params(min_length, max_hits, max_gap, bandwidth, min_score):
    """The parameters of a seed-chain query as the C struct; ValueError for a negative one or one beyond 64 bits."""
    values = {"min_length": min_length, "max_hits": max_hits, "max_gap": max_gap, "bandwidth": bandwidth,
              "min_score": min_score}
    params = _lib.RlzChainParams()
    for name, v in values.items():
        v = operator.index(v)
        if v < 0:
            raise ValueError(f"{name} must not be negative")
        if v >= 1 << 64:
            raise ValueError(f"{name} must fit 64 bits")
        setattr(params, name, v)
    return params


def _unpack_seed_chains(res):
    """nolzss_rlz_seed_chains_result -> (chains, anchor_offsets, anchors) as copies; the caller frees the result."""
    n, a = res.num_chains, res.num_anchors
    offsets = np.ctypeslib.as_array(C.cast(res.anchor_offsets, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
    chains, anchors = np.zeros(n, dtype=CHAIN_DTYPE), np.zeros(a, dtype=CHAIN_ANCHOR_DTYPE)
    if n:
        C.memmove(chains.ctypes.data, res.chains, n * CHAIN_DTYPE.itemsize)
    if a:
        C.memmove(anchors.ctypes.data, res.anchors, a * CHAIN_ANCHOR_DTYPE.itemsize)
    return chains, offsets, anchors


ALIGN_LANES = 64  # NOLZSS_RLZ_ALIGN_LANES: the diagonals of an alignment job are the lanes of one wavefront


def _align_params(min_length, max_hits, max_gap, bandwidth, min_score, band, max_flank):
    """The parameters of an align query as the C struct; ValueError for a negative one, one beyond 64 bits, or more than
    ALIGN_LANES diagonals -- before any native call."""
    values = {"min_length": min_length, "max_hits": max_hits, "max_gap": max_gap, "bandwidth": bandwidth,
              "min_score": min_score, "band": band, "max_flank": max_flank}
    params = _lib.RlzAlignParams()
    for name, v in values.items():
        v = operator.index(v)
        if v < 0:
            raise ValueError(f"{name} must not be negative")
        if v >= 1 << 64:
            raise ValueError(f"{name} must fit 64 bits")
        values[name] = v
    if values["bandwidth"] + 2 * values["band"] + 1 > ALIGN_LANES:
        raise ValueError(f"an alignment job has at most {ALIGN_LANES} diagonals: bandwidth + 2 * band + 1 is "
                         f"{values['bandwidth']} + 2 * {values['band']} + 1; lower bandwidth or band")
    for name, v in values.items():
        setattr(params, name, v)
    return params


# ---- relative-LZ index: target batches matched against a resident reference (genomics/rlz.py) -------------------
class RlzIndexHandle:
    """Extension: the suffix structures of a reference block kept in device memory (C ABI nolzss_rlz_index_*), any
    number of target batches matched against them without a suffix sort.  A context manager; close() may be called
    more than once, any other use after it raises ValueError."""

    def __init__(self, handle):
        self._h = handle
        info = _lib.RlzIndexSummary()
        try:
            check(lib.nolzss_rlz_index_info(self._h, C.byref(info)))
        except Exception:
            self.close()
            raise
        self.info = {name: int(getattr(info, name)) for name, _ in _lib.RlzIndexSummary._fields_}

    @classmethod
    def open(cls, reference, with_rc: bool = True, prefix_syms: int = 0):
        """reference: one sequence or a list of sequences.  C ABI nolzss_rlz_index_open (its header states the rules)."""
        if isinstance(reference, (str, bytes, bytearray)):
            reference = [reference]
        h = C.c_void_p()
        check(lib.nolzss_rlz_index_open(*_seq_args(reference, "reference"), 1 if with_rc else 0,
                                        operator.index(prefix_syms), _default_device, C.byref(h)))
        return cls(h)

    @classmethod
    def open_fasta(cls, reference_fasta_path, with_rc: bool = True, sanitize_mode: str = "remove_ambiguous",
                   prefix_syms: int = 0):
        """Every record of the FASTA file is a reference record.  C ABI nolzss_rlz_index_open_fasta."""
        h = C.c_void_p()
        check(lib.nolzss_rlz_index_open_fasta(_str_arg(reference_fasta_path, "reference_fasta_path"), 1 if with_rc else 0,
                                              _sanitize_mode(sanitize_mode), operator.index(prefix_syms), _default_device,
                                              C.byref(h)))
        return cls(h)

    def _handle(self):
        if self._h is None:
            raise ValueError("the index is closed")
        return self._h

    def factorize_arrays(self, targets, want_factors: bool = True) -> dict:
        """One batch -> the dict rlz_factorize_arrays returns for the same references and targets."""
        h = self._handle()
        res = _lib.RlzResult()
        check(lib.nolzss_rlz_index_factorize(h, *_seq_args(targets, "target"), 1 if want_factors else 0, C.byref(res)))
        return _unpack_rlz_result(res, want_factors)

    def codes(self, targets) -> np.ndarray:
        """The code (length, bit 31 = reverse complement, 0 = no match) of every position of T1 s T2 s .. Tk s; only
        target positions are specified.  C ABI nolzss_rlz_index_codes."""
        h = self._handle()
        args = _seq_args(targets, "target")
        code = np.zeros(sum(args[1][j] for j in range(args[2])) + args[2], dtype=np.uint32)
        check(lib.nolzss_rlz_index_codes(h, *args, code.ctypes.data if code.size else None))
        return code

    def count(self, patterns) -> np.ndarray:
        """One batch: the occurrences of every pattern in the reference, both strands together (uint64).  C ABI
        nolzss_rlz_index_count (its header states the rules)."""
        h = self._handle()
        args = _seq_args(patterns, "pattern")
        counts = np.zeros(args[2], dtype=np.uint64)
        check(lib.nolzss_rlz_index_count(h, *args, counts.ctypes.data if counts.size else None))
        return counts

    def locate(self, patterns, max_hits: int = 0):
        """One batch -> (counts, offsets, hits): uint64 counts, the q + 1 uint64 offsets of the patterns' hits, and the
        hits as HIT_DTYPE, per pattern ascending by (position, is_rc); a pattern with more than max_hits occurrences
        (0: no cap) reports its count and no hits.  C ABI nolzss_rlz_index_locate."""
        h = self._handle()
        max_hits = operator.index(max_hits)
        if max_hits < 0:
            raise ValueError("max_hits must not be negative")
        args = _seq_args(patterns, "pattern")
        counts, offsets = np.zeros(args[2], dtype=np.uint64), np.zeros(args[2] + 1, dtype=np.uint64)
        out, z = C.c_void_p(), C.c_size_t()
        check(lib.nolzss_rlz_index_locate(h, *args, max_hits, counts.ctypes.data if counts.size else None,
                                          offsets.ctypes.data, C.byref(out), C.byref(z)))
        if not out.value or z.value == 0:
            lib.nolzss_free(out)
            return counts, offsets, np.zeros(0, dtype=HIT_DTYPE)
        raw = (C.c_uint64 * (2 * z.value)).from_address(out.value)
        raw._owner = _Owned(out)
        return counts, offsets, np.frombuffer(raw, dtype=HIT_DTYPE)

    def seeds(self, targets, min_length: int = 1, max_hits: int = 0):
        """One batch -> (seeds, offsets, hits): the maximal exact matches of the targets as SEED_DTYPE (target index in
        this batch, start inside the target, length, count on both strands), ascending by (target, start); the
        len(seeds) + 1 uint64 offsets of their hits; the hits as HIT_DTYPE, per seed ascending by (position, is_rc).  Only
        seeds of at least min_length bases are reported; a seed with more than max_hits occurrences (0: no cap) reports
        its count and no hits.  C ABI nolzss_rlz_index_seeds (its header states the rules)."""
        h = self._handle()
        min_length, max_hits = operator.index(min_length), operator.index(max_hits)
        if min_length < 0:
            raise ValueError("min_length must not be negative")
        if max_hits < 0:
            raise ValueError("max_hits must not be negative")
        res = _lib.RlzSeedsResult()
        try:
            check(lib.nolzss_rlz_index_seeds(h, *_seq_args(targets, "target"), min_length, max_hits, C.byref(res)))
            S, T = res.num_seeds, res.num_hits
            offsets = np.ctypeslib.as_array(C.cast(res.hit_offsets, C.POINTER(C.c_uint64)), shape=(S + 1,)).copy()
            seeds, hits = np.zeros(S, dtype=SEED_DTYPE), np.zeros(T, dtype=HIT_DTYPE)
            if S:
                C.memmove(seeds.ctypes.data, res.seeds, S * SEED_DTYPE.itemsize)
            if T:
                C.memmove(hits.ctypes.data, res.hits, T * HIT_DTYPE.itemsize)
        finally:
            lib.nolzss_free_rlz_seeds_result(C.byref(res))
        return seeds, offsets, hits

    @staticmethod
    def _repeat_rules(min_length, min_count):
        min_length, min_count = operator.index(min_length), operator.index(min_count)
        if min_length < 0:
            raise ValueError("min_length must not be negative")
        if min_count < 0:
            raise ValueError("min_count must not be negative")
        return min_length, min_count

    def repeat_count(self, min_length: int = 20, min_count: int = 2) -> int:
        """The records repeats(min_length, min_count) would report; only the flags are computed.  C ABI
        nolzss_rlz_index_repeat_count (its header states the rules)."""
        h = self._handle()
        min_length, min_count = self._repeat_rules(min_length, min_count)
        out = C.c_uint64()
        check(lib.nolzss_rlz_index_repeat_count(h, min_length, min_count, C.byref(out)))
        return int(out.value)

    def repeats(self, min_length: int = 20, min_count: int = 2, max_hits: int = 64):
        """-> (repeats, offsets, hits): the maximal repeats of the reference itself, both strands, as REPEAT_DTYPE
        (position, length, count, record, palindrome), ascending by (position, length); the len(repeats) + 1 uint64 offsets
        of their hits; the hits as HIT_DTYPE, per repeat ascending by (position, is_rc).  A repeat with more than max_hits
        occurrences (0: no cap) reports its count and no hits.  C ABI nolzss_rlz_index_repeats (its header states the
        rules)."""
        h = self._handle()
        min_length, min_count = self._repeat_rules(min_length, min_count)
        max_hits = operator.index(max_hits)
        if max_hits < 0:
            raise ValueError("max_hits must not be negative")
        res = _lib.RlzRepeatsResult()
        try:
            check(lib.nolzss_rlz_index_repeats(h, min_length, min_count, max_hits, C.byref(res)))
            S, T = res.num_repeats, res.num_hits
            offsets = np.ctypeslib.as_array(C.cast(res.hit_offsets, C.POINTER(C.c_uint64)), shape=(S + 1,)).copy()
            repeats, hits = np.zeros(S, dtype=REPEAT_DTYPE), np.zeros(T, dtype=HIT_DTYPE)
            if S:
                C.memmove(repeats.ctypes.data, res.repeats, S * REPEAT_DTYPE.itemsize)
            if T:
                C.memmove(hits.ctypes.data, res.hits, T * HIT_DTYPE.itemsize)
        finally:
            lib.nolzss_free_rlz_repeats_result(C.byref(res))
        return repeats, offsets, hits

    def seed_chains(self, targets, min_length: int = 15, max_hits: int = 64, max_gap: int = 5000, bandwidth: int = 500,
                    min_score: int = 40):
        """One batch -> (chains, anchor_offsets, anchors, num_seeds, num_seed_hits): the colinear chain of the seeds of
        every (target, strand, record) as CHAIN_DTYPE, ascending by (target, is_rc, record); the len(chains) + 1 uint64
        offsets of their anchors; the anchors as CHAIN_ANCHOR_DTYPE, per chain ascending by t_start; the seeds reported
        and the hits expanded on the device (diagnostics).  C ABI nolzss_rlz_index_seed_chains (its header states the
        rules)."""
        h = self._handle()
        params = _chain_params(min_length, max_hits, max_gap, bandwidth, min_score)
        res = _lib.RlzSeedChainsResult()
        try:
            check(lib.nolzss_rlz_index_seed_chains(h, *_seq_args(targets, "target"), C.byref(params), C.byref(res)))
            return _unpack_seed_chains(res) + (int(res.num_seeds), int(res.num_seed_hits))
        finally:
            lib.nolzss_free_rlz_seed_chains_result(C.byref(res))

    def align(self, targets, min_length: int = 15, max_hits: int = 64, max_gap: int = 5000, bandwidth: int = 31,
              min_score: int = 40, band: int = 16, max_flank: int = 256):
        """One batch -> (alignments, op_offsets, ops, num_jobs, num_rows): one ALIGN_DTYPE record per chain of
        seed_chains at the same first five parameters, in the same order; the len(alignments) + 1 uint64 offsets of
        their ops; the ops as uint32 (length << 4 | code: I = 1, D = 2, `=` = 7, X = 8), ascending in the target; the
        jobs planned and the DP rows run (diagnostics).  C ABI nolzss_rlz_index_align (its header states the rules)."""
        params = _align_params(min_length, max_hits, max_gap, bandwidth, min_score, band, max_flank)
        h = self._handle()
        res = _lib.RlzAlignResult()
        try:
            check(lib.nolzss_rlz_index_align(h, *_seq_args(targets, "target"), C.byref(params), C.byref(res)))
            n, t = res.num_alignments, res.num_ops
            offsets = np.ctypeslib.as_array(C.cast(res.op_offsets, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
            recs, ops = np.zeros(n, dtype=ALIGN_DTYPE), np.zeros(t, dtype=np.uint32)
            if n:
                C.memmove(recs.ctypes.data, res.alignments, n * ALIGN_DTYPE.itemsize)
            if t:
                C.memmove(ops.ctypes.data, res.ops, t * 4)
            return recs, offsets, ops, int(res.num_jobs), int(res.num_rows)
        finally:
            lib.nolzss_free_rlz_align_result(C.byref(res))

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h is not None:
            check(lib.nolzss_rlz_index_close(h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- relative-LZ index: pileup counts and variant sites of read batches (genomics/rlz.py) -------------------------
def _variant_rule(min_count, min_fraction):
    """(min_count, num, den) of a variants query; ValueError for what the library would refuse -- before any native
    call."""
    min_count = operator.index(min_count)
    try:
        num, den = (operator.index(v) for v in min_fraction)
    except (TypeError, ValueError):
        raise ValueError("min_fraction is a pair of integers (num, den)") from None
    if min_count < 1 or min_count >= 1 << 32:
        raise ValueError("min_count must be at least 1 and fit 32 bits")
    if den < 1 or num < 0 or num > den or den >= 1 << 32:
        raise ValueError(f"min_fraction must be a fraction between 0 and 1 with a denominator below 2^32, not {num} / {den}")
    return min_count, num, den


def _consensus_params(min_depth, min_fraction, low):
    """nolzss_rlz_consensus_params of a consensus query; ValueError for what the library would refuse -- before any
    native call."""
    min_depth = operator.index(min_depth)
    try:
        num, den = (operator.index(v) for v in min_fraction)
    except (TypeError, ValueError):
        raise ValueError("min_fraction is a pair of integers (num, den)") from None
    if min_depth < 1 or min_depth >= 1 << 32:
        raise ValueError("min_depth must be at least 1 and fit 32 bits")
    if den < 1 or num < 0 or num > den or den >= 1 << 32:
        raise ValueError(f"min_fraction must be a fraction between 0 and 1 with a denominator below 2^32, not {num} / {den}")
    if low not in ("reference", "N"):
        raise ValueError(f"low is 'reference' or 'N', not {low!r}")
    return _lib.RlzConsensusParams(min_depth, 1 if low == "N" else 0, num, den)


def _insertions_out(res):
    out = np.zeros(res.num_insertions, dtype=INSERTION_DTYPE)
    if res.num_insertions:
        C.memmove(out.ctypes.data, res.insertions, res.num_insertions * INSERTION_DTYPE.itemsize)
    return out


def _consensus_out(res, return_map, block_length):
    """nolzss_rlz_consensus_result -> dict(records: [bytes, ...], the seven statistics, starts with return_map)"""
    text = C.string_at(res.text, res.length) if res.length else b""
    offsets = np.zeros(res.num_records + 1, dtype=np.uint64)
    if res.record_offsets:
        C.memmove(offsets.ctypes.data, res.record_offsets, offsets.nbytes)
    out = {"records": [text[int(offsets[r]):int(offsets[r + 1]) - 1] for r in range(res.num_records)]}
    out.update({name: int(getattr(res, name)) for name in CONSENSUS_STATS})
    if return_map:
        starts = np.zeros(block_length + 1, dtype=np.uint64)
        if res.starts:
            C.memmove(starts.ctypes.data, res.starts, starts.nbytes)
        out["starts"] = starts
    return out


class RlzPileupHandle:
    """Extension: eight counters per position of the block of an index, kept on the device and fed by batches that go
    through the align path of the index (C ABI nolzss_rlz_pileup_*).  It keeps the index handle alive.  A context
    manager; close() may be called more than once, any other use after it raises ValueError."""

    def __init__(self, handle, index_handle):
        self._h, self._index = handle, index_handle

    @classmethod
    def open(cls, index_handle, min_length: int = 15, max_hits: int = 64, max_gap: int = 5000, bandwidth: int = 31,
             min_score: int = 40, band: int = 16, max_flank: int = 256, normalize_indels: bool = False):
        """C ABI nolzss_rlz_pileup_open / nolzss_rlz_pileup_open_flags (the header states the rules)."""
        params = _align_params(min_length, max_hits, max_gap, bandwidth, min_score, band, max_flank)
        h = C.c_void_p()
        if normalize_indels:
            check(lib.nolzss_rlz_pileup_open_flags(index_handle._handle(), C.byref(params), PILEUP_NORMALIZE, C.byref(h)))
        else:
            check(lib.nolzss_rlz_pileup_open(index_handle._handle(), C.byref(params), C.byref(h)))
        return cls(h, index_handle)

    def _handle(self):
        if self._h is None:
            raise ValueError("the pileup is closed")
        self._index._handle()  # (a closed index raises here, not in the library)
        return self._h

    @property
    def info(self) -> dict:
        """dict(block_length, device_bytes, targets, alignments, ops, columns, adds, device, dirty) and the seven
        align parameters.  C ABI nolzss_rlz_pileup_info."""
        h = self._handle()
        info = _lib.RlzPileupSummary()
        check(lib.nolzss_rlz_pileup_info(h, C.byref(info)))
        out = {name: int(getattr(info, name)) for name, _ in _lib.RlzPileupSummary._fields_ if name != "params"}
        out.update({name: int(getattr(info.params, name)) for name, _ in _lib.RlzAlignParams._fields_})
        flags, events, log_bytes = C.c_uint32(), C.c_uint64(), C.c_uint64()
        check(lib.nolzss_rlz_pileup_log_info(h, C.byref(flags), C.byref(events), C.byref(log_bytes)))
        out.update(normalize_indels=bool(flags.value & PILEUP_NORMALIZE), insertion_events=events.value, log_bytes=log_bytes.value)
        return out

    def add(self, targets, primary_only: bool = True) -> dict:
        """One batch -> dict(alignments, ops, columns: of the alignments kept; targets: in the pileup so far).  C ABI
        nolzss_rlz_pileup_add."""
        h = self._handle()
        info = _lib.RlzPileupAddInfo()
        check(lib.nolzss_rlz_pileup_add(h, *_seq_args(targets, "target"), 1 if primary_only else 0, C.byref(info)))
        return {name: int(getattr(info, name)) for name, _ in _lib.RlzPileupAddInfo._fields_}

    def counts(self, start: int = 0, end=None) -> np.ndarray:
        """The (end - start, 8) uint32 counters of the block positions [start, end), channels in the order of
        PILEUP_CHANNELS.  C ABI nolzss_rlz_pileup_counts."""
        h = self._handle()
        start = operator.index(start)
        end = self.info["block_length"] if end is None else operator.index(end)
        if start < 0 or end < start:
            raise ValueError(f"counts take 0 <= start <= end, not [{start}, {end})")
        out = np.zeros((end - start, len(PILEUP_CHANNELS)), dtype=np.uint32)
        check(lib.nolzss_rlz_pileup_counts(h, start, end, out.ctypes.data if out.size else None))
        return out

    def variants(self, min_count: int = 2, min_fraction=(1, 2)) -> np.ndarray:
        """The alleles that differ from the block and reach min_count observations and min_fraction = (num, den) of
        the depth, as VARIANT_DTYPE ascending by (position, allele).  C ABI nolzss_rlz_pileup_variants."""
        rule = _variant_rule(min_count, min_fraction)
        h = self._handle()
        res = _lib.RlzVariantsResult()
        try:
            check(lib.nolzss_rlz_pileup_variants(h, *rule, C.byref(res)))
            out = np.zeros(res.num_variants, dtype=VARIANT_DTYPE)
            if res.num_variants:
                C.memmove(out.ctypes.data, res.variants, res.num_variants * VARIANT_DTYPE.itemsize)
            return out
        finally:
            lib.nolzss_free_rlz_variants_result(C.byref(res))

    def insertions(self, min_count: int = 2, min_fraction=(1, 2)) -> np.ndarray:
        """The inserted alleles that reach min_count observations and min_fraction = (num, den) of the depth, as
        INSERTION_DTYPE ascending by (position, length, bases).  C ABI nolzss_rlz_pileup_insertions."""
        rule = _variant_rule(min_count, min_fraction)
        h = self._handle()
        res = _lib.RlzInsertionsResult()
        try:
            check(lib.nolzss_rlz_pileup_insertions(h, *rule, C.byref(res)))
            return _insertions_out(res)
        finally:
            lib.nolzss_free_rlz_insertions_result(C.byref(res))

    def consensus(self, min_depth: int = 1, min_fraction=(1, 2), low: str = "reference", return_map: bool = False) -> dict:
        """The sample's sequence as the counters and the insertion alleles call it -> dict(records: one bytes per
        reference record, called, low_positions, substitutions, deleted, insertions, inserted_bases,
        truncated_skipped, and with return_map starts: block_length + 1 offsets into the records joined by one
        separator each).  C ABI nolzss_rlz_pileup_consensus."""
        params = _consensus_params(min_depth, min_fraction, low)
        h = self._handle()
        res = _lib.RlzConsensusResult()
        try:
            check(lib.nolzss_rlz_pileup_consensus(h, C.byref(params), 1 if return_map else 0, C.byref(res)))
            block_length = 0
            if return_map:
                info = _lib.RlzPileupSummary()
                check(lib.nolzss_rlz_pileup_info(h, C.byref(info)))
                block_length = int(info.block_length)
            return _consensus_out(res, return_map, block_length)
        finally:
            lib.nolzss_free_rlz_consensus_result(C.byref(res))

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h is not None:
            check(lib.nolzss_rlz_pileup_close(h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- relative-LZ index: a cohort of samples, SNP distances and variable sites (genomics/rlz.py) -------------------
# a site that varies among the samples of a cohort (RlzCohort.sites): nolzss_rlz_cohort_site, 48 bytes
COHORT_SITE_DTYPE = np.dtype({"names": ["position", "record_offset", "record", "present", "counts", "reference"],
                              "formats": ["<u8", "<u8", "<u4", "<u4", ("<u4", (4,)), "<u4"],
                              "offsets": [0, 8, 16, 20, 24, 40], "itemsize": 48})
COHORT_MAX_SAMPLES = 16384  # NOLZSS_RLZ_COHORT_MAX_SAMPLES


class RlzCohortHandle:
    """Extension: three bit planes per sample over the block of an index, kept on the device (C ABI
    nolzss_rlz_cohort_*).  It keeps the index handle alive.  A context manager; close() may be called more than once,
    any other use after it raises ValueError."""

    def __init__(self, handle, index_handle):
        self._h, self._index = handle, index_handle

    @classmethod
    def open(cls, index_handle):
        """C ABI nolzss_rlz_cohort_open (the header states the rules)."""
        h = C.c_void_p()
        check(lib.nolzss_rlz_cohort_open(index_handle._handle(), C.byref(h)))
        return cls(h, index_handle)

    def _handle(self):
        if self._h is None:
            raise ValueError("the cohort is closed")
        self._index._handle()  # (a closed index raises here, not in the library)
        return self._h

    @property
    def info(self) -> dict:
        """dict(samples, capacity, block_length, device_bytes, device).  C ABI nolzss_rlz_cohort_info."""
        h = self._handle()
        info = _lib.RlzCohortSummary()
        check(lib.nolzss_rlz_cohort_info(h, C.byref(info)))
        return {name: int(getattr(info, name)) for name, _ in _lib.RlzCohortSummary._fields_ if name != "reserved"}

    @staticmethod
    def _sample(info) -> dict:
        return {name: int(getattr(info, name)) for name, _ in _lib.RlzCohortSampleInfo._fields_}

    def add_pileup(self, pileup_handle, min_depth: int = 1, min_fraction=(1, 2)) -> dict:
        """The calls of a pileup under the consensus rule as the next sample -> dict(sample, called, low, deleted,
        differs).  C ABI nolzss_rlz_cohort_add_pileup."""
        params = _consensus_params(min_depth, min_fraction, "reference")
        h = self._handle()
        info = _lib.RlzCohortSampleInfo()
        check(lib.nolzss_rlz_cohort_add_pileup(h, pileup_handle._handle(), C.byref(params), C.byref(info)))
        return self._sample(info)

    def add_calls(self, calls) -> dict:
        """One byte per block position as the next sample -> the same dict.  C ABI nolzss_rlz_cohort_add_calls."""
        h = self._handle()
        if isinstance(calls, str):
            calls = calls.encode("latin-1")
        address, nbytes, keep = _as_buffer(calls)
        info = _lib.RlzCohortSampleInfo()
        check(lib.nolzss_rlz_cohort_add_calls(h, address if nbytes else None, nbytes, C.byref(info)))
        del keep
        return self._sample(info)

    def samples(self) -> list:
        """The dict of every sample, in order.  C ABI nolzss_rlz_cohort_samples."""
        h = self._handle()
        while True:
            n = self.info["samples"]
            out = (_lib.RlzCohortSampleInfo * max(n, 1))()
            count = C.c_size_t()
            check(lib.nolzss_rlz_cohort_samples(h, out, n, C.byref(count)))
            if count.value <= n:  # (another thread may have added meanwhile)
                return [self._sample(out[j]) for j in range(count.value)]

    def distances(self):
        """(differences, compared): two (N, N) uint32 arrays.  C ABI nolzss_rlz_cohort_distances."""
        h = self._handle()
        res = _lib.RlzCohortDistancesResult()
        try:
            check(lib.nolzss_rlz_cohort_distances(h, C.byref(res)))
            n = res.num_samples
            diff, cmp_ = np.zeros((n, n), dtype=np.uint32), np.zeros((n, n), dtype=np.uint32)
            if n:
                C.memmove(diff.ctypes.data, res.differences, diff.nbytes)
                C.memmove(cmp_.ctypes.data, res.compared, cmp_.nbytes)
            return diff, cmp_
        finally:
            lib.nolzss_free_rlz_cohort_distances_result(C.byref(res))

    def sites(self, min_present: int, with_reference: bool = True) -> np.ndarray:
        """The positions where at least two distinct bases occur among at least min_present calling samples, as
        COHORT_SITE_DTYPE ascending by position.  C ABI nolzss_rlz_cohort_sites."""
        min_present = operator.index(min_present)
        if min_present < 0 or min_present >= 1 << 64:
            raise ValueError("min_present must not be negative and fit 64 bits")
        h = self._handle()
        res = _lib.RlzCohortSitesResult()
        try:
            check(lib.nolzss_rlz_cohort_sites(h, min_present, 1 if with_reference else 0, C.byref(res)))
            out = np.zeros(res.num_sites, dtype=COHORT_SITE_DTYPE)
            if res.num_sites:
                C.memmove(out.ctypes.data, res.sites, res.num_sites * COHORT_SITE_DTYPE.itemsize)
            return out
        finally:
            lib.nolzss_free_rlz_cohort_sites_result(C.byref(res))

    def columns(self, positions) -> np.ndarray:
        """The (N, S) uint8 letters of every sample at the S positions (`N`: no call).  C ABI
        nolzss_rlz_cohort_columns."""
        h = self._handle()
        pos = np.asarray(positions)
        if pos.ndim != 1:
            raise ValueError("positions is a one-dimensional sequence of block positions")
        if pos.size and (pos.dtype.kind not in "iu" or (pos.dtype.kind == "i" and int(pos.min()) < 0)):
            raise ValueError("positions are non-negative integers")
        pos = np.ascontiguousarray(pos, dtype=np.uint64)
        out = np.zeros((self.info["samples"], pos.size), dtype=np.uint8)
        check(lib.nolzss_rlz_cohort_columns(h, pos.ctypes.data if pos.size else None, pos.size,
                                            out.ctypes.data if out.size else None))
        return out

    def calls(self, sample: int, start: int = 0, end=None) -> bytes:
        """The letters of one sample over the block positions [start, end) (end None: the block's end).  C ABI
        nolzss_rlz_cohort_calls."""
        h = self._handle()
        sample, start = operator.index(sample), operator.index(start)
        end = self.info["block_length"] if end is None else operator.index(end)
        if sample < 0:
            raise ValueError(f"sample index {sample} is negative")
        if start < 0 or end < start:
            raise ValueError(f"calls take 0 <= start <= end, not [{start}, {end})")
        out = np.zeros(end - start, dtype=np.uint8)
        check(lib.nolzss_rlz_cohort_calls(h, sample, start, end, out.ctypes.data if out.size else None))
        return out.tobytes()

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h is not None:
            check(lib.nolzss_rlz_cohort_close(h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _roundtrip_result(z, mismatches, first, info):
    res = {"z": z.value, "mismatches": mismatches.value,
           "first_mismatch": None if first.value == (1 << 64) - 1 else first.value}
    res.update({k: v for k, v in _info_dict(info).items() if k != "z"})
    return res


def roundtrip_check(data, with_rc: bool = False) -> dict:
    """Extension: factorize (with_rc: as factorize_dna_w_rc), gather the literals, decode and compare with `data`, the
    records never leaving the device -> dict(z, mismatches, first_mismatch (None: no mismatch), n, n_literals,
    resolved_at_expand, rounds, max_active).  C ABI nolzss_roundtrip."""
    p, n, keep = _as_buffer(data)
    z, mism, first, info = C.c_size_t(), C.c_uint64(), C.c_uint64(), _lib.DecodeInfo()
    check(lib.nolzss_roundtrip(p, n, 1 if with_rc else 0, _default_device, C.byref(z), C.byref(mism), C.byref(first),
                               C.byref(info)))
    return _roundtrip_result(z, mism, first, info)


def roundtrip_device(data_ptr: int, n: int, with_rc: bool = False, stream: int = 0) -> dict:
    """roundtrip_check over n bytes resident in device memory (C ABI nolzss_roundtrip_device)."""
    z, mism, first, info = C.c_size_t(), C.c_uint64(), C.c_uint64(), _lib.DecodeInfo()
    check(lib.nolzss_roundtrip_device(C.c_void_p(data_ptr), n, 1 if with_rc else 0, _default_device,
                                      C.c_void_p(stream) if stream else None, C.byref(z), C.byref(mism), C.byref(first),
                                      C.byref(info)))
    return _roundtrip_result(z, mism, first, info)


def debug_count_mismatches(a, b):
    """Debug hook of the round trip's comparison kernel -> (differing positions, the first one or None)."""
    pa, na, keep_a = _as_buffer(a)
    pb, nb, keep_b = _as_buffer(b)
    if na != nb:
        raise ValueError("arrays of different lengths")
    count, first = C.c_uint64(), C.c_uint64()
    check(lib.nolzss_debug_count_mismatches(pa if na else None, pb if nb else None, na, _default_device, C.byref(count),
                                            C.byref(first)))
    return count.value, (None if first.value == (1 << 64) - 1 else first.value)


# ---- measurement hooks ----------------------------------------------------------------------
def profile_enable(on: bool = True) -> None:
    check(lib.nolzss_profile_enable(_default_device, 1 if on else 0))


def profile_reset() -> None:
    check(lib.nolzss_profile_reset(_default_device))


def profile_report() -> dict:
    """{stage name: (launch count, total milliseconds, algorithmic bytes)} measured with HIP
    events on the pipeline stream."""
    buf = C.create_string_buffer(1 << 16)
    check(lib.nolzss_profile_report(_default_device, buf, len(buf)))
    res = {}
    for line in buf.value.decode().splitlines():
        name, count, ms, nbytes = line.split()
        res[name] = (int(count), float(ms), float(nbytes))
    return res


def device_count() -> int:
    c = C.c_int()
    check(lib.nolzss_device_count(C.byref(c)))
    return c.value


# ---- intermediate arrays for the parity tests ------------------------------------------------
def debug_arrays(data):
    """-> dict(sa, isa, lcp (n+1 entries), lstar) as computed on the device."""
    p, n, keep = _as_buffer(data)
    sa = np.zeros(n, dtype=np.uint32)
    isa = np.zeros(n, dtype=np.uint32)
    lcp = np.zeros(n + 1, dtype=np.uint32)
    lstar = np.zeros(n, dtype=np.uint32)
    check(lib.nolzss_debug_arrays(p, n, _default_device, sa.ctypes.data, isa.ctypes.data, lcp.ctypes.data,
                                  lstar.ctypes.data))
    return {"sa": sa, "isa": isa, "lcp": lcp, "lstar": lstar}


def debug_position_factors(data) -> np.ndarray:
    """-> the plain-mode factor record (start, length, ref) of EVERY position of the text, as the device's
    factor kernel gives it for a factor starting there (a literal has ref = start)."""
    p, n, keep = _as_buffer(data)
    out = np.zeros(n, dtype=FACTOR_DTYPE)
    check(lib.nolzss_debug_position_factors(p, n, _default_device, out.ctypes.data))
    return out


RC_COUNTERS = ("far_ranks", "exact_from_tiles", "exact_total", "compact", "pending_relaunch")


def debug_rc_arrays(S, want_plain: bool = False) -> dict:
    """The reverse-complement pipeline over a prepared string S, N = len(S) // 2 - 1 -> dict(sa (len(S) entries),
    lcp (len(S) + 1), isa, code, records (N each), plain (N, only with want_plain: the plain-mode length of every
    position as a by-product, 0 = literal), counters (RC_COUNTERS -> int)).  code: factor length in bits 0..30, bit 31
    = reverse complement, 0 = literal; records: the factor a cursor at each position would emit."""
    p, m, keep = _as_buffer(S)
    N = m // 2 - 1 if m >= 4 else 0
    sa = np.zeros(m if N else 0, dtype=np.uint32)
    lcp = np.zeros(m + 1 if N else 0, dtype=np.uint32)
    isa = np.zeros(N, dtype=np.uint32)
    code = np.zeros(N, dtype=np.uint32)
    plain = np.zeros(N, dtype=np.uint32) if want_plain else None
    records = np.zeros(N, dtype=FACTOR_DTYPE)
    counters = np.zeros(5, dtype=np.uint32)
    check(lib.nolzss_debug_rc_arrays(p, m, _default_device, 1 if want_plain else 0, sa.ctypes.data, isa.ctypes.data,
                                     lcp.ctypes.data, code.ctypes.data, plain.ctypes.data if want_plain else None,
                                     records.ctypes.data, counters.ctypes.data))
    res = {"sa": sa, "isa": isa, "lcp": lcp, "code": code, "records": records,
           "counters": dict(zip(RC_COUNTERS, (int(c) for c in counters)))}
    if want_plain:
        res["plain"] = plain
    return res


def debug_sort_pairs(keys, vals):
    keys = np.ascontiguousarray(keys, dtype=np.uint64).copy()
    vals = np.ascontiguousarray(vals, dtype=np.uint32).copy()
    check(lib.nolzss_debug_sort_pairs(keys.ctypes.data, vals.ctypes.data, keys.size, _default_device))
    return keys, vals


def debug_arena():
    """(capacity, high-water mark) in bytes of the device arena."""
    cap, peak = C.c_size_t(), C.c_size_t()
    check(lib.nolzss_debug_arena(_default_device, C.byref(cap), C.byref(peak)))
    return cap.value, peak.value


def debug_device_buffers():
    """(live buffers, live bytes) of the device allocations the resident handles of this process hold; no device is touched."""
    buffers, nbytes = C.c_size_t(), C.c_size_t()
    check(lib.nolzss_debug_device_buffers(C.byref(buffers), C.byref(nbytes)))
    return buffers.value, nbytes.value


def debug_parse_fasta(path, sanitize_mode: str = "remove_ambiguous"):
    """[(id, sequence bytes)] as the native FASTA reader sees the file (host only)."""
    ids, seqs = C.c_void_p(), C.c_void_p()
    nb_ids, nb_seqs, count = C.c_size_t(), C.c_size_t(), C.c_size_t()
    check(lib.nolzss_debug_parse_fasta(os.fsencode(str(path)), _sanitize_mode(sanitize_mode), C.byref(ids),
                                       C.byref(nb_ids), C.byref(seqs), C.byref(nb_seqs), C.byref(count)))
    try:
        a = C.string_at(ids, nb_ids.value).split(b"\0")[:-1] if nb_ids.value else []
        b = C.string_at(seqs, nb_seqs.value).split(b"\0")[:-1] if nb_seqs.value else []
    finally:
        lib.nolzss_free(ids)
        lib.nolzss_free(seqs)
    assert len(a) == len(b) == count.value
    return list(zip(a, b))


def debug_parse_nucleotide_fasta(path):
    """[(id, sequence bytes)] as the reader behind read_nucleotide_fasta_arrays sees the file (host only);
    raises what that entry point would."""
    ids, seqs = C.c_void_p(), C.c_void_p()
    nb_ids, nb_seqs, count = C.c_size_t(), C.c_size_t(), C.c_size_t()
    rc = lib.nolzss_debug_parse_nucleotide_fasta(os.fsencode(str(path)), C.byref(ids), C.byref(nb_ids), C.byref(seqs),
                                                 C.byref(nb_seqs), C.byref(count))
    if rc == _lib.ERR_UNSUPPORTED:
        raise UnsupportedInput(lib.nolzss_last_error().decode("utf-8", "replace"))
    check(rc)
    try:
        a = C.string_at(ids, nb_ids.value).split(b"\0")[:-1] if nb_ids.value else []
        b = C.string_at(seqs, nb_seqs.value).split(b"\0")[:-1] if nb_seqs.value else []
    finally:
        lib.nolzss_free(ids)
        lib.nolzss_free(seqs)
    assert len(a) == len(b) == count.value
    return list(zip(a, b))


def debug_lpt_plan(lengths, bins: int):
    """owners of the records under the library's shard plan (host only)."""
    m = len(lengths)
    lens = (C.c_size_t * max(m, 1))(*lengths)
    owners = (C.c_size_t * max(m, 1))()
    check(lib.nolzss_debug_lpt_plan(lens, m, bins, owners))
    return [owners[j] for j in range(m)]


def debug_batch_plan(lengths, n_dev: int, with_rc: bool = False):
    """The static plan of factorize_batch for these record lengths on n_dev devices (host only, no device touched):
    (chunk_of, device_of, n_chunks) -- chunk_of[j] = merged run of record j or -1, device_of[j] = slot in the device
    list of the run record j takes on its own or -1."""
    m = len(lengths)
    lens = (C.c_size_t * max(m, 1))(*lengths)
    chunk_of = (C.c_int32 * max(m, 1))()
    device_of = (C.c_int32 * max(m, 1))()
    n_chunks = C.c_size_t()
    check(lib.nolzss_debug_batch_plan(lens, m, n_dev, 1 if with_rc else 0, chunk_of, device_of, C.byref(n_chunks)))
    return [chunk_of[j] for j in range(m)], [device_of[j] for j in range(m)], n_chunks.value


def debug_trim_arenas() -> int:
    """Releases the idle device arenas of the default device; returns the bytes given back."""
    r = C.c_size_t()
    check(lib.nolzss_debug_trim_arenas(_default_device, C.byref(r)))
    return r.value


def debug_batch_counters():
    """(records factorized by merged runs, records factorized one pipeline run each) since load."""
    a, b = C.c_uint64(), C.c_uint64()
    lib.nolzss_debug_batch_counters(C.byref(a), C.byref(b))
    return a.value, b.value


def debug_scan(data, mode: int):
    data = np.ascontiguousarray(data, dtype=np.uint32).copy()
    check(lib.nolzss_debug_scan(data.ctypes.data, data.size, mode, _default_device))
    return data


PYR_NEAREST_LEFT, PYR_NEAREST_RIGHT, PYR_RANGE = range(3)
(NEAR_UP_LESS, NEAR_UP_GREATER, NEAR_DOWN_LESS, NEAR_DOWN_GREATER, NEAR_FAR_UP_LESS, NEAR_FAR_UP_GREATER,
 NEAR_FAR_DOWN_LESS, NEAR_FAR_DOWN_GREATER, NEAR_LCP_INTERVAL, NEAR_LPNF_LEFTMOST, NEAR_LPNF_SEARCH) = range(11)


def debug_pyramid(base, is_max: bool, queries=None, mode: int = 0, level1=None, first_entry: int = 0,
                  flag_min: int = 0, poison: int = 0, want_levels: bool = True):
    """The device pyramid over `base` (u32) and its queries (nolzss_debug_pyramid, test hook).  queries: (nq, 3) rows
    (op, a, b) with op one of PYR_*.  Returns {"nlev", "lens", "levels": one array per level from level 0 (None if not
    wanted), "flag", "results": one u32 per query}."""
    base = np.ascontiguousarray(base, dtype=np.uint32)
    q = np.ascontiguousarray(queries if queries is not None else np.zeros((0, 3)), dtype=np.uint32).reshape(-1, 3)
    l1 = np.ascontiguousarray(level1, dtype=np.uint32) if level1 is not None else None
    if l1 is not None and l1.size < first_entry:
        raise ValueError("level1 holds fewer than first_entry entries")
    lens, length = [], base.size
    while True:  # (room for the levels; the library reports the lengths it used)
        lens.append(length)
        if length <= 1 or len(lens) == 9:
            break
        length = (length + 15) >> 4
    levels = np.zeros(max(sum(lens), 1), dtype=np.uint32)
    got_lens = np.zeros(9, dtype=np.uint32)
    nlev, flag = C.c_int(), C.c_uint32()
    results = np.zeros(max(len(q), 1), dtype=np.uint32)
    check(lib.nolzss_debug_pyramid(base.ctypes.data, base.size, 1 if is_max else 0, mode,
                                   l1.ctypes.data if l1 is not None else None, first_entry, flag_min, poison,
                                   q.ctypes.data, len(q), _default_device, C.byref(nlev), got_lens.ctypes.data,
                                   levels.ctypes.data if want_levels else None, levels.size, C.byref(flag),
                                   results.ctypes.data))
    got_lens = [int(v) for v in got_lens[:nlev.value]]
    ends = np.cumsum(got_lens)
    return {"nlev": nlev.value, "lens": got_lens,
            "levels": [levels[e - n:e] for e, n in zip(ends, got_lens)] if want_levels else None,
            "flag": flag.value, "results": results[:len(q)]}


def debug_nearest(sa, lcp, queries, poison: int = 0):
    """The searches of nearest.hpp on the device over sa (n entries) and lcp (n + 1 entries, first and last 0)
    (nolzss_debug_nearest, test hook).  queries: (nq, 5) rows (op, r, a, b, c) with op one of NEAR_*.  Returns an
    (nq, 2) u32 array: (len, pos), (lo, hi) or (value, 0)."""
    sa = np.ascontiguousarray(sa, dtype=np.uint32)
    lcp = np.ascontiguousarray(lcp, dtype=np.uint32)
    if lcp.size != sa.size + 1:
        raise ValueError("lcp must hold one entry more than sa")
    q = np.ascontiguousarray(queries, dtype=np.uint32).reshape(-1, 5)
    results = np.zeros((max(len(q), 1), 2), dtype=np.uint32)
    check(lib.nolzss_debug_nearest(sa.ctypes.data, lcp.ctypes.data, sa.size, poison, q.ctypes.data, len(q),
                                   _default_device, results.ctypes.data))
    return results[:len(q)]


LOCAL_SORT_FUSED, LOCAL_SORT_LOOKBACK_GAVE_UP, LOCAL_SORT_LANE_ORDER, LOCAL_SORT_LISTED_SHIFT = 1, 2, 4, 8
# the forms of the product: (shift0, npass, key35)
LOCAL_SORT_KEY16, LOCAL_SORT_KEY35, LOCAL_SORT_RECORDS = (8, 2, False), (5, 2, True), (0, 3, False)


def debug_local_sort(words, values, starts, shift0: int, npass: int, key35: bool = False, want_regroup: bool = False):
    """The LDS sub-bucket sort on the device over caller pairs (nolzss_debug_local_sort, test hook): `words` / `values`
    lie in the buckets given by `starts` (nb + 1 offsets from 0 to n); one segmented pass by the byte at bit 24, then
    every sub-bucket by npass digits from shift0 up (local_sort_sub_buckets).  Returns {"words" (None where the form
    with the regroup on the way completed: it does not write them), "values", "fused", "lookback_gave_up",
    "lane_order", "listed"} and, where fused, "lcp", "new_slot", "new_grp", "survivors"."""
    words = np.ascontiguousarray(words, dtype=np.uint32)
    values = np.ascontiguousarray(values, dtype=np.uint32)
    starts = np.ascontiguousarray(starts, dtype=np.uint32)
    if values.size != words.size:
        raise ValueError("words and values differ in length")
    n = words.size
    words_out, values_out = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
    lcp, slot, grp = (np.zeros(max(n, 1), dtype=np.uint32) for _ in range(3)) if want_regroup else (None, None, None)
    surv, status = C.c_uint32(), C.c_uint32()
    ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    check(lib.nolzss_debug_local_sort(words.ctypes.data, values.ctypes.data, n, starts.ctypes.data, max(starts.size, 1) - 1,
                                      shift0, npass, 1 if key35 else 0, 1 if want_regroup else 0, _default_device,
                                      words_out.ctypes.data, values_out.ctypes.data, ptr(lcp), ptr(slot), ptr(grp),
                                      C.byref(surv) if want_regroup else None, C.byref(status)))
    st = status.value
    out = {"words": None if st & LOCAL_SORT_FUSED else words_out[:n], "values": values_out[:n],
           "fused": bool(st & LOCAL_SORT_FUSED), "lookback_gave_up": bool(st & LOCAL_SORT_LOOKBACK_GAVE_UP),
           "lane_order": bool(st & LOCAL_SORT_LANE_ORDER), "listed": st >> LOCAL_SORT_LISTED_SHIFT}
    if out["fused"]:
        out.update(lcp=lcp[:n], new_slot=slot[:surv.value], new_grp=grp[:surv.value], survivors=surv.value)
    return out


(TEXT_ORDER_KEEP_INPUT, TEXT_ORDER_KEEP_VAL, TEXT_ORDER_SHORT_CODES, TEXT_ORDER_OUT2, TEXT_ORDER_NARROW,
 TEXT_ORDER_PERMUTE_PACKED) = 1, 2, 4, 8, 16, 32
TEXT_ORDER_FORMS = ("none", "plain", "partial_then_plain", "window_perm", "two_value_hist", "packed", "record_plan",
                    "record_plan2", "permute_plain", "permute_windows")


def debug_text_order(idx, val=None, n_out=None, *, packed=None, keep_input: bool = True, keep_val: bool = True,
                     short_codes: bool = True, want_out2: bool = False, narrow=None, rec_ends=None, fill: int = 0):
    """The permutation into text order on the device over caller pairs (nolzss_debug_text_order, test hook):
    bucketed_scatter(idx, val) into targets of n_out words pre-filled with `fill`, or with `packed` (u64)
    permute_packed(idx, packed).  narrow = (list capacity, saturation value): the codes leave as uint16.  rec_ends: the
    ends of the records of a block-diagonal permutation, for a RecordScatterPlan.  Returns {"out", "out2" (None unless
    wanted), "narrow", "list" (the stored (position | code << 32) items), "listed", "idx_after", "val_after", "result",
    "plan_made", "form" (one of TEXT_ORDER_FORMS), "packed_tried", "escaped", "list_overflow", "lookback_gave_up",
    "nbits", "wb", "partition_passes"}."""
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    count = idx.size
    permute = packed is not None
    if permute:
        packed = np.ascontiguousarray(packed, dtype=np.uint64)
        if val is not None or packed.size != count:
            raise ValueError("permute_packed takes idx and as many packed words")
        n_out = count if n_out is None else n_out
    else:
        val = np.ascontiguousarray(val, dtype=np.uint32)
        if val.size != count or n_out is None:
            raise ValueError("idx and val differ in length, or n_out is not given")
    if not 0 < n_out < 1 << 32:
        raise ValueError("n_out 1 .. 2^32 - 1")
    flags = ((TEXT_ORDER_KEEP_INPUT if keep_input else 0) | (TEXT_ORDER_KEEP_VAL if keep_val else 0) |
             (TEXT_ORDER_SHORT_CODES if short_codes else 0) | (TEXT_ORDER_OUT2 if want_out2 else 0) |
             (TEXT_ORDER_NARROW if narrow is not None else 0) | (TEXT_ORDER_PERMUTE_PACKED if permute else 0))
    list_cap, code_max = (int(narrow[0]), int(narrow[1])) if narrow is not None else (0, 0)
    if list_cap < 0 or list_cap >= 1 << 32:
        raise ValueError("list capacity below 2^32")
    ends = np.ascontiguousarray(rec_ends, dtype=np.uint32) if rec_ends is not None else None
    out = np.zeros(n_out, dtype=np.uint32)
    out2 = np.zeros(n_out, dtype=np.uint32) if (want_out2 or permute) else None
    narrow_out = np.zeros(n_out, dtype=np.uint16) if narrow is not None else None
    items = np.zeros(max(list_cap, 1), dtype=np.uint64) if narrow is not None else None
    idx_after = np.zeros(max(count, 1), dtype=np.uint32) if not permute else None
    val_after = np.zeros(max(count, 1), dtype=np.uint32) if not permute else None
    report = np.zeros(12, dtype=np.uint32)
    ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    check(lib.nolzss_debug_text_order(idx.ctypes.data, ptr(val), ptr(packed), count, n_out, flags, fill & 0xffffffff, list_cap,
                                      code_max, ptr(ends), ends.size if ends is not None else 0, _default_device,
                                      out.ctypes.data, ptr(out2), ptr(narrow_out), ptr(items), ptr(idx_after), ptr(val_after),
                                      report.ctypes.data))
    r = [int(x) for x in report]
    return {"out": out, "out2": out2, "narrow": narrow_out, "list": items[:min(r[10], list_cap)] if items is not None else None,
            "listed": r[10], "idx_after": idx_after[:count] if not permute else None,
            "val_after": val_after[:count] if not permute else None, "result": bool(r[8]), "plan_made": bool(r[9]),
            "form": TEXT_ORDER_FORMS[r[0]], "packed_tried": bool(r[1]), "escaped": r[2], "list_overflow": bool(r[3]),
            "lookback_gave_up": bool(r[4]), "nbits": r[5], "wb": r[6], "partition_passes": r[7]}


GROUP_SORT_ROUNDS = 24


def debug_group_sort(text, sa, slot, grp, h0: int, pivot: bool = False, max_rounds: int = GROUP_SORT_ROUNDS,
                     depth_cap: int = 0xffffffff, lcp_mark=None):
    """The rounds of one group-sort pass of the suffix-array construction on the device over caller groups
    (nolzss_debug_group_sort, test hook): group_dir_kernel and the four forms of group_sort_kernel, as window rounds or
    (pivot) as pivot rounds at most depth_cap symbols deep, with no regroup behind them.  `text` (bytes) is packed as
    every text is; `sa` holds n entries, of which only the slots of the listed groups are read and written; `slot` /
    `grp` are the active list (ascending slots, grp = head slot of the group, groups of at least two members on
    consecutive list positions and slots); `lcp_mark` (n entries) is the equalising round's filter.
    PRECONDITION, not checked: the members of every group agree on their first h0 symbols and none of them ends in front
    of h0.  Returns {"sa", "out_lo", "lcp_list", "min_depth", "bits", "terms", "segmented"}."""
    text = np.frombuffer(bytes(text), dtype=np.uint8)
    sa = np.array(sa, dtype=np.uint32)  # (a copy: the call writes it)
    slot = np.ascontiguousarray(slot, dtype=np.uint32)
    grp = np.ascontiguousarray(grp, dtype=np.uint32)
    if sa.size != text.size or slot.size != grp.size:
        raise ValueError("sa holds one entry per symbol, slot and grp one per list entry")
    mark = np.ascontiguousarray(lcp_mark, dtype=np.uint32) if lcp_mark is not None else None
    if mark is not None and mark.size != text.size:
        raise ValueError("lcp_mark holds one entry per symbol")
    if not (0 <= h0 < 1 << 32 and 0 <= max_rounds < 1 << 32 and 0 <= depth_cap < 1 << 32):
        raise ValueError("h0, max_rounds and depth_cap are 32-bit values")
    m = slot.size
    out_lo, lcp_list = np.zeros(max(m, 1), dtype=np.uint32), np.zeros(max(m, 1), dtype=np.uint32)
    depth, info = C.c_uint32(), np.zeros(3, dtype=np.uint32)
    check(lib.nolzss_debug_group_sort(text.ctypes.data, text.size, sa.ctypes.data, slot.ctypes.data, grp.ctypes.data, m, h0,
                                      1 if pivot else 0, max_rounds, depth_cap, mark.ctypes.data if mark is not None else None,
                                      _default_device, out_lo.ctypes.data, lcp_list.ctypes.data, C.byref(depth),
                                      info.ctypes.data))
    return {"sa": sa, "out_lo": out_lo[:m], "lcp_list": lcp_list[:m], "min_depth": depth.value, "bits": int(info[0]),
            "terms": int(info[1]), "segmented": bool(info[2])}


DIRECT_ROUND_NO_STRAGGLERS, DIRECT_ROUND_TIMED, DIRECT_ROUND_WITH_RANKS = 1, 2, 4


def debug_direct_round(text, sa, slot, grp, h0: int, cap: int, flags: int = DIRECT_ROUND_WITH_RANKS, lcp_in=None,
                       fill: int = 0):
    """The first direct round of the suffix-array construction on the device over caller groups
    (nolzss_debug_direct_round, test hook): group_refine_kernel and the compaction of what it leaves tied.  `text`, `sa`,
    `slot` / `grp` as for debug_group_sort, with groups of any size >= 2; `cap`: the depth at which the round gives up;
    `lcp_in` (n entries, default all 0xffffffff) and `fill`: what lcp and rank_by_slot hold before the call.
    PRECONDITION, not checked: the members of every group agree on their first h0 symbols and none of them ends in front
    of h0.  Returns {"sa", "lcp", "rank_by_slot", "new_slot", "new_grp", "new_m", "min_depth" (3 values), "bits",
    "terms", "segmented"}."""
    text = np.frombuffer(bytes(text), dtype=np.uint8)
    sa = np.array(sa, dtype=np.uint32)  # (a copy: the call writes it)
    slot = np.ascontiguousarray(slot, dtype=np.uint32)
    grp = np.ascontiguousarray(grp, dtype=np.uint32)
    if sa.size != text.size or slot.size != grp.size:
        raise ValueError("sa holds one entry per symbol, slot and grp one per list entry")
    lcp_in = np.full(text.size, 0xffffffff, dtype=np.uint32) if lcp_in is None else np.ascontiguousarray(lcp_in, dtype=np.uint32)
    if lcp_in.size != text.size:
        raise ValueError("lcp_in holds one entry per symbol")
    if not (0 <= h0 < 1 << 32 and 0 <= cap < 1 << 32 and 0 <= fill < 1 << 32 and 0 <= flags < 1 << 32):
        raise ValueError("h0, cap, flags and fill are 32-bit values")
    n, m = text.size, slot.size
    lcp, rank = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
    new_slot, new_grp = np.zeros(max(m, 1), dtype=np.uint32), np.zeros(max(m, 1), dtype=np.uint32)
    new_m, depth, info = C.c_uint32(), np.zeros(3, dtype=np.uint32), np.zeros(3, dtype=np.uint32)
    check(lib.nolzss_debug_direct_round(text.ctypes.data, n, sa.ctypes.data, slot.ctypes.data, grp.ctypes.data, m, h0, cap, flags,
                                        lcp_in.ctypes.data, fill, _default_device, lcp.ctypes.data, rank.ctypes.data,
                                        new_slot.ctypes.data, new_grp.ctypes.data, C.byref(new_m), depth.ctypes.data,
                                        info.ctypes.data))
    k = new_m.value
    return {"sa": sa, "lcp": lcp[:n], "rank_by_slot": rank[:n], "new_slot": new_slot[:k], "new_grp": new_grp[:k], "new_m": k,
            "min_depth": [int(x) for x in depth], "bits": int(info[0]), "terms": int(info[1]), "segmented": bool(info[2])}


REPEAT_PASS_COUNTS, REPEAT_PASS_PERIODIC, REPEAT_PASS_PAIR_RUNS = 0, 1, 2


def debug_repeat_pass(text, sa, lcp, rank, slot, grp, h: int, which: int, arg: int = 0):
    """The periodic pass or the pair-run passes of the suffix-array construction on the device over a caller's partial
    state (nolzss_debug_repeat_pass, test hook): periodic_pass / pair_run_pass of sa_repeats.hip behind the driver's own
    set-up.  `sa` (n), `lcp` (n + 1: a decided value at the first slot of every group, a pending code inside; lcp[n] goes
    in as it is) and `rank` (n, by position: head slot + 1) as they stand behind write_all_ranks; `slot` / `grp`: exactly
    the slots of the groups of two and more, as for debug_group_sort; `h`: the symbols every group agrees on.  `which`:
    REPEAT_PASS_COUNTS, REPEAT_PASS_PERIODIC (`arg` = per_attempts on entry, 0 .. 3) or REPEAT_PASS_PAIR_RUNS (`arg`
    passes, 1 .. 10).  PRECONDITION, not checked: the state is a true partial order of the text.  Returns {"sa", "lcp",
    "rank", "new_slot", "new_grp", "new_m", "counts" (4 values), "ret", "per_hint", "per_attempts", "bits", "terms",
    "segmented"}."""
    text = np.frombuffer(bytes(text), dtype=np.uint8)
    sa = np.array(sa, dtype=np.uint32)  # (copies: the call writes the three)
    lcp = np.array(lcp, dtype=np.uint32)
    rank = np.array(rank, dtype=np.uint32)
    slot = np.ascontiguousarray(slot, dtype=np.uint32)
    grp = np.ascontiguousarray(grp, dtype=np.uint32)
    n, m = text.size, slot.size
    if sa.size != n or rank.size != n or lcp.size != n + 1 or grp.size != m:
        raise ValueError("sa and rank hold one entry per symbol, lcp one more, slot and grp one per list entry")
    if not (0 <= h < 1 << 32 and -(1 << 31) <= which < 1 << 31 and -(1 << 31) <= arg < 1 << 31):
        raise ValueError("h is a 32-bit value, which and arg are ints")
    new_slot, new_grp = np.zeros(max(m, 1), dtype=np.uint32), np.zeros(max(m, 1), dtype=np.uint32)
    new_m, counts = C.c_uint32(), np.zeros(4, dtype=np.uint32)
    info, per = np.zeros(3, dtype=np.uint32), np.zeros(3, dtype=np.uint32)
    check(lib.nolzss_debug_repeat_pass(text.ctypes.data, n, sa.ctypes.data, lcp.ctypes.data, rank.ctypes.data, slot.ctypes.data,
                                       grp.ctypes.data, m, h, which, arg, _default_device, new_slot.ctypes.data,
                                       new_grp.ctypes.data, C.byref(new_m), counts.ctypes.data, info.ctypes.data,
                                       per.ctypes.data))
    k = new_m.value
    return {"sa": sa, "lcp": lcp, "rank": rank, "new_slot": new_slot[:k], "new_grp": new_grp[:k], "new_m": k,
            "counts": [int(x) for x in counts], "ret": bool(per[0]), "per_hint": int(per[1]), "per_attempts": int(per[2]),
            "bits": int(info[0]), "terms": int(info[1]), "segmented": bool(info[2])}


LDS_PLAIN, LDS_RC = 0, 1
LDS_OVERFLOW = 0xffffffff


def debug_lds_search(sa, lcp, form: int = LDS_PLAIN, strand: int = 0, poison: int = 0):
    """The LDS tile searches of nearest_lds.hpp on the device over sa (n distinct entries) and lcp (n + 1 entries, first
    and last 0), as the plain (LDS_PLAIN, two searches) or the reverse-complement candidate kernel (LDS_RC, four
    searches of the ranks with sa[r] < strand) runs them (nolzss_debug_lds_search, test hook).  Returns (len, pos):
    (searches, n) and (2, n) u32 arrays; len has bit 31 set where the search left the reach (bound in the low bits)."""
    sa = np.ascontiguousarray(sa, dtype=np.uint32)
    lcp = np.ascontiguousarray(lcp, dtype=np.uint32)
    if lcp.size != sa.size + 1:
        raise ValueError("lcp must hold one entry more than sa")
    searches = 4 if form == LDS_RC else 2
    length = np.zeros((searches, max(sa.size, 1)), dtype=np.uint32)
    pos = np.zeros((2, max(sa.size, 1)), dtype=np.uint32)
    check(lib.nolzss_debug_lds_search(sa.ctypes.data, lcp.ctypes.data, sa.size, form, strand, poison, _default_device,
                                      length.ctypes.data, pos.ctypes.data))
    return length, pos


LENGTH_HIST_BINS = 2048


def debug_chain(codes, start_pos: int = 0, width: int = 32, poison: int = 0, wide_list=None, listed=None,
                list_max: int = 0, with_strand: bool = False, bounds=None, want_lengths: bool = True,
                want_hist: bool = True):
    """The greedy cursor on the device over caller codes (nolzss_debug_chain, test hook): mark_chain, chain_starts and
    chain_lengths of the pipeline itself.  `codes`: one u32 per position (length in bits 0..30, 0 = literal, bit 31 the
    strand).  width 16: the codes are narrowed into a uint16 array padded as the pipeline's own, the padding filled
    with the half-word `poison`.  list_max (width 16): `wide_list` holds (position | code << 32) entries of which the
    first `listed` (default: all) are applied by widened_lstar; the cursor then runs on the widened 32-bit array.
    `bounds`: 2k ascending u32 for counts of the starts per [lo, hi).  Returns {"z", "starts", "lengths", "hist", "tail"
    (sorted: the kernel writes it in no particular order), "widened", "counts", "cursor"}; what was not asked for is
    None.  "cursor" = (path, failed tiles) of the call (debug_cursor)."""
    codes = np.ascontiguousarray(codes, dtype=np.uint32)
    n = codes.size
    if not (0 <= start_pos < 1 << 64 and 0 <= poison < 1 << 32 and 0 <= list_max < 1 << 32):
        raise ValueError("start_pos, poison and list_max are unsigned values")
    items = np.ascontiguousarray(wide_list, dtype=np.uint64) if wide_list is not None else None
    list_len = items.size if items is not None else 0
    listed = list_len if listed is None else int(listed)
    bnd = np.ascontiguousarray(bounds, dtype=np.uint32) if bounds is not None else None
    if bnd is not None and bnd.size % 2:
        raise ValueError("the bounds come in pairs")
    k = bnd.size // 2 if bnd is not None else 0
    bins = LENGTH_HIST_BINS * (2 if with_strand else 1)
    z, tail_count = C.c_uint32(), C.c_uint32()
    starts = np.zeros(max(n, 1), dtype=np.uint32)
    lengths = np.zeros(max(n, 1), dtype=np.uint32) if want_lengths else None
    hist = np.zeros(bins, dtype=np.uint32) if want_hist else None
    tail = np.zeros(n // LENGTH_HIST_BINS + 1, dtype=np.uint64) if want_hist else None
    widened = np.zeros(max(n, 1), dtype=np.uint32) if list_max else None
    counts = np.zeros(max(k, 1), dtype=np.uint32) if bnd is not None else None
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
    check(lib.nolzss_debug_chain(ptr(codes), n, start_pos, width, poison, ptr(items), list_len, listed, list_max,
                                 1 if with_strand else 0, ptr(bnd), k, _default_device, C.byref(z), starts.ctypes.data,
                                 ptr(lengths), ptr(hist), ptr(tail), C.byref(tail_count) if want_hist else None,
                                 ptr(widened), ptr(counts)))
    return {"z": z.value, "starts": starts[:z.value], "lengths": lengths[:z.value] if want_lengths else None,
            "hist": hist, "tail": np.sort(tail[:tail_count.value]) if want_hist else None,
            "widened": widened[:n] if list_max else None, "counts": counts[:k] if bnd is not None else None,
            "cursor": debug_cursor() if hasattr(lib, "nolzss_debug_cursor") else None}  # (NOLZSS_LIB: an older build)


CURSOR_PATHS = ("none", "speculative", "failed_over", "exact")


def debug_cursor():
    """(path, failed tiles) of the last run of the cursor on the device (nolzss_debug_cursor): path "none" (nothing to
    walk), "speculative", "failed_over" (the speculative walk raised its flag, the exact stages ran) or "exact"
    (NOLZSS_NO_SPEC_CURSOR); the tiles whose walk from the entry did not meet the speculative walk."""
    info = np.zeros(2, dtype=np.uint32)
    check(lib.nolzss_debug_cursor(_default_device, info.ctypes.data))
    return CURSOR_PATHS[int(info[0])], int(info[1])


def debug_rlz_seed_chain(target, group, y, q, length, block_length: int, records: int, max_gap: int, bandwidth: int,
                         min_score: int = 0):
    """The seed-chain stages from the group heads to the chain records on caller anchors (nolzss_debug_rlz_seed_chain,
    test hook): five arrays of n entries ordered by (target, group, y, q), group = is_rc * records + record.  Returns
    {"f", "pred" (uint32 per anchor, group-local; 0xffffffff: none), "chains", "anchor_offsets", "anchors"}."""
    arrays = [np.ascontiguousarray(a, dtype=np.uint32) for a in (target, group, y, q, length)]
    n = arrays[0].size
    if any(a.size != n for a in arrays):
        raise ValueError("the anchor arrays hold one entry per anchor")
    params = _chain_params(0, 0, max_gap, bandwidth, min_score)
    f, pred = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
    res = _lib.RlzSeedChainsResult()
    try:
        check(lib.nolzss_debug_rlz_seed_chain(*[a.ctypes.data if n else None for a in arrays], n, C.byref(params),
                                              operator.index(block_length), operator.index(records), _default_device,
                                              f.ctypes.data, pred.ctypes.data, C.byref(res)))
        chains, offsets, anchors = _unpack_seed_chains(res)
    finally:
        lib.nolzss_free_rlz_seed_chains_result(C.byref(res))
    return {"f": f[:n], "pred": pred[:n], "chains": chains, "anchor_offsets": offsets, "anchors": anchors}


def debug_rlz_align_jobs(query, reference, kind, q0, nq, y0, ny, band: int):
    """The alignment stages from the job offsets to the traceback on caller jobs (nolzss_debug_rlz_align_jobs, test
    hook): query and reference are ACGT strings; job j is (kind: 0 gap, 1 right flank, 2 left flank; q0, nq; y0, ny -- of
    a flank the query bases to align and the reference bases available, of a left flank below q0 / y0).  Returns {"cost",
    "end_col" (uint32 per job), "col_offsets" (uint64, n + 1), "cols" (uint8: one code per alignment column of every
    job, ascending in the query)}."""
    query = query.encode("ascii") if isinstance(query, str) else bytes(query)
    reference = reference.encode("ascii") if isinstance(reference, str) else bytes(reference)
    arrays = [np.ascontiguousarray(a, dtype=np.uint32) for a in (kind, q0, nq, y0, ny)]
    n = arrays[0].size
    if any(a.size != n for a in arrays):
        raise ValueError("the job arrays hold one entry per job")
    band = operator.index(band)
    if band < 0 or band >= 1 << 32:
        raise ValueError("band must fit 32 bits")
    cost, end_col = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    cols = C.c_void_p()
    try:
        check(lib.nolzss_debug_rlz_align_jobs(query, len(query), reference, len(reference),
                                              *[a.ctypes.data if n else None for a in arrays], n, band, _default_device,
                                              cost.ctypes.data, end_col.ctypes.data, offsets.ctypes.data, C.byref(cols)))
        total = int(offsets[-1])
        out = np.zeros(total, dtype=np.uint8)
        if total:
            C.memmove(out.ctypes.data, cols, total)
    finally:
        if cols:
            lib.nolzss_free(cols)
    return {"cost": cost[:n], "end_col": end_col[:n], "col_offsets": offsets, "cols": out}


def debug_rlz_pileup(block, targets, alignments, op_offsets, ops, primary_only: bool = False):
    """The pileup stages on caller alignments (nolzss_debug_rlz_pileup, test hook): block is the reference block as
    bytes, ACGT and any other byte for a separator; targets plain ACGT strings; alignments an ALIGN_DTYPE array with its
    len + 1 uint64 op_offsets and the uint32 ops (length << 4 | code).  Returns the (len(block), 8) uint32 counters."""
    block = block.encode("ascii") if isinstance(block, str) else bytes(block)
    recs = np.ascontiguousarray(alignments, dtype=ALIGN_DTYPE)
    offsets = np.ascontiguousarray(op_offsets, dtype=np.uint64)
    ops = np.ascontiguousarray(ops, dtype=np.uint32)
    if offsets.size != recs.size + 1:
        raise ValueError("op_offsets holds one entry per alignment and one more")
    out = np.zeros((len(block), len(PILEUP_CHANNELS)), dtype=np.uint32)
    check(lib.nolzss_debug_rlz_pileup(block, len(block), *_seq_args(targets, "target"),
                                      recs.ctypes.data if recs.size else None, offsets.ctypes.data, recs.size,
                                      ops.ctypes.data if ops.size else None, ops.size, 1 if primary_only else 0,
                                      _default_device, out.ctypes.data if out.size else None))
    return out


def debug_rlz_pileup_consensus(block, targets, alignments, op_offsets, ops, primary_only: bool = False,
                               normalize_indels: bool = False, min_depth: int = 1, min_fraction=(1, 2), low: str = "reference"):
    """The pileup, allele-table and consensus stages on caller alignments (nolzss_debug_rlz_pileup_consensus, test hook);
    the inputs of debug_rlz_pileup, the flag of an open and the parameters of a consensus.  Returns dict(counts: the
    (len(block), 8) counters, insertions: the full allele table as INSERTION_DTYPE, consensus: as
    RlzPileupHandle.consensus returns it, with its map)."""
    params = _consensus_params(min_depth, min_fraction, low)
    block = block.encode("ascii") if isinstance(block, str) else bytes(block)
    recs = np.ascontiguousarray(alignments, dtype=ALIGN_DTYPE)
    offsets = np.ascontiguousarray(op_offsets, dtype=np.uint64)
    ops = np.ascontiguousarray(ops, dtype=np.uint32)
    if offsets.size != recs.size + 1:
        raise ValueError("op_offsets holds one entry per alignment and one more")
    out = np.zeros((len(block), len(PILEUP_CHANNELS)), dtype=np.uint32)
    ins, cons = _lib.RlzInsertionsResult(), _lib.RlzConsensusResult()
    try:
        check(lib.nolzss_debug_rlz_pileup_consensus(block, len(block), *_seq_args(targets, "target"),
                                                    recs.ctypes.data if recs.size else None, offsets.ctypes.data, recs.size,
                                                    ops.ctypes.data if ops.size else None, ops.size, 1 if primary_only else 0,
                                                    PILEUP_NORMALIZE if normalize_indels else 0, C.byref(params), _default_device,
                                                    out.ctypes.data if out.size else None, C.byref(ins), C.byref(cons)))
        return {"counts": out, "insertions": _insertions_out(ins), "consensus": _consensus_out(cons, bool(len(block)), len(block))}
    finally:
        lib.nolzss_free_rlz_insertions_result(C.byref(ins))
        lib.nolzss_free_rlz_consensus_result(C.byref(cons))

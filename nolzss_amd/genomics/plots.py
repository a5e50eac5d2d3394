"""Data layer of the reference's noLZSS.genomics.plots for the two plots that read every factor (reference:
src/noLZSS/genomics/plots.py): the strand-bias grid of plot_strand_bias_heatmap (_compute_strand_bias_grid,
plots.py:1961-2075) and the space-scale histogram of plot_space_scale_heatmap (:2559-2614).

Both are binned on the device from the factor records the pipeline leaves there (C ABI nolzss_factor_maps_*): no
record crosses PCIe and no tuple is built.  The strand grid comes back as exact integers -- nucleotides in units of
1 / (x_bins * y_bins) -- and the reference's float grids, edges and log2 bias follow from them on the host.

The self dot plot of plot_multiple_seq_self_lz_factor_plot_from_file (:352-900) is served the same way: self_dotplot
keeps the records of one factorisation on the device and renders any number of views into exact integer rasters (C
ABI nolzss_dotplot_*).

Drawing is not part of this package (no matplotlib), nor are the CCDF weighting and `sequence_index` of
plot_space_scale_heatmap or the other plots of the reference's module.
"""
import os
from collections.abc import Sequence
from pathlib import Path
from typing import Any, Dict, Optional, Tuple, Union

import numpy as np

from .. import _noLZSS as _native
from ..utils import NoLZSSError, _read_footer, read_binary_file_metadata

__all__ = ["PlotError", "bias_from_grids", "strand_bias_grid", "fasta_strand_bias_grid", "factors_strand_bias_grid",
           "space_scale_histogram", "DotPlot", "self_dotplot"]

RC_MASK = 1 << 63
_INVALID = "Invalid factor coordinates for strand bias grid"
_MAX_LENGTH_EDGES = 4097  # include/nolzss_hip.h


class PlotError(NoLZSSError):
    """reference: class PlotError(NoLZSSError), plots.py"""


def _grid_arg(grid_size) -> Tuple[int, int]:
    """plots.py:1983-1991"""
    if isinstance(grid_size, int):
        x_bins = y_bins = grid_size
    elif isinstance(grid_size, Sequence) and len(grid_size) == 2:
        x_bins, y_bins = grid_size
    else:
        raise ValueError("grid_size must be an int or a tuple of two ints")
    if x_bins <= 0 or y_bins <= 0:
        raise ValueError("grid_size must be positive")
    return int(x_bins), int(y_bins)


def bias_from_grids(forward_grid, rc_grid):
    """log2 of the ratio of the per-strand normalised coverage, masked where neither strand covers the cell
    (plots.py:2064-2073)."""
    forward_grid = np.asarray(forward_grid, dtype=float)
    rc_grid = np.asarray(rc_grid, dtype=float)
    total_forward = forward_grid.sum()
    total_rc = rc_grid.sum()
    eps = 1e-9
    norm_forward = forward_grid / (total_forward if total_forward > 0 else 1.0)
    norm_rc = rc_grid / (total_rc if total_rc > 0 else 1.0)
    bias_grid = np.log2((norm_forward + eps) / (norm_rc + eps))
    mask = (forward_grid + rc_grid) == 0
    return np.ma.array(bias_grid, mask=mask)


def units_to_grid(units, unit: int) -> np.ndarray:
    """exact integer cell sums (1 / unit nucleotides) -> the reference's float64 nucleotides"""
    units = np.asarray(units, dtype=np.uint64)
    u = np.uint64(unit)
    return (units // u).astype(np.float64) + (units % u).astype(np.float64) / float(unit)


def _check_total_length(total_length):
    if total_length is not None and total_length <= 0:  # x_max = float(total_length) <= 0, plots.py:1999
        raise PlotError(_INVALID)


def _run(call):
    try:
        return call()
    except ValueError as e:
        if str(e) == _INVALID:
            raise PlotError(_INVALID)
        raise


def _grid_result(m: Dict[str, Any]) -> Dict[str, Any]:
    if m["z_used"] == 0:
        raise PlotError("No factors available to compute strand bias grid")  # plots.py:1994
    forward_grid = units_to_grid(m["forward_units"], m["unit"])
    rc_grid = units_to_grid(m["rc_units"], m["unit"])
    return {"x_edges": np.linspace(0, float(m["x_max"]), m["x_bins"] + 1),
            "y_edges": np.linspace(0, float(m["y_max"]), m["y_bins"] + 1),
            "forward_grid": forward_grid, "rc_grid": rc_grid, "bias_grid": bias_from_grids(forward_grid, rc_grid),
            "forward_units": m["forward_units"], "rc_units": m["rc_units"], "unit": m["unit"], "z": m["z"],
            "z_used": m["z_used"]}


def strand_bias_grid(data, with_rc: bool = True, grid_size=50, total_length: Optional[int] = None,
                     min_factor_length: int = 1) -> Dict[str, Any]:
    """_compute_strand_bias_grid over the factors of factorize_dna_w_rc(data) (with_rc) or factorize(data), binned on
    the device.  Returns x_edges, y_edges, forward_grid, rc_grid, bias_grid as the reference computes them (grids of
    shape (y_bins, x_bins), bias_grid masked), plus the exact forward_units / rc_units (uint64, nucleotides * unit),
    unit, z and z_used."""
    grid = _grid_arg(grid_size)
    _check_total_length(total_length)
    return _grid_result(_run(lambda: _native.factor_maps(data, with_rc=with_rc, grid=grid, total_length=total_length,
                                                         min_factor_length=min_factor_length)))


def fasta_strand_bias_grid(fasta_filepath, with_rc: bool = True, sanitize_mode: str = "remove_ambiguous",
                           grid_size=50, min_factor_length: int = 1) -> Dict[str, Any]:
    """The fasta_filepath branch of plot_strand_bias_heatmap (plots.py:2139-2164, total_length = None): the factors of
    factorize_fasta_multiple_dna_w_rc (or _no_rc), sentinel factors kept whatever min_factor_length."""
    grid = _grid_arg(grid_size)
    if not Path(fasta_filepath).exists():
        raise FileNotFoundError(f"Input file not found: {fasta_filepath}")
    return _grid_result(_run(lambda: _native.fasta_factor_maps(os.fspath(fasta_filepath), with_rc=with_rc,
                                                               sanitize_mode=sanitize_mode, grid=grid,
                                                               min_factor_length=min_factor_length)))


def _file_records(path: Path) -> np.ndarray:
    """the records of a v2 factor file as an array (the checks and messages of utils.read_factors_binary_file)"""
    if not path.exists():
        raise NoLZSSError(f"File not found: {path}")
    try:
        with open(path, "rb") as f:
            nf = _read_footer(f)[0]
            f.seek(0)
            data = f.read(24 * nf)
    except OSError as e:
        raise NoLZSSError(f"Error reading file {path}: {e}")
    if len(data) != 24 * nf:
        raise NoLZSSError(f"Insufficient data for factor {len(data) // 24}")
    return np.frombuffer(data, dtype=_native.FACTOR_DTYPE)


def _records_arg(factors, total_length, sentinel_factor_indices):
    """-> (records array, total_length, sentinel factor indices).  A path: the v2 file's records, and its footer's
    total_length and sentinel indices (plots.py:2143-2147).  A list: 3- and 4-tuples (start, length, ref[, is_rc]);
    tuples of another size are skipped as in plots.py:2012-2018."""
    if isinstance(factors, (str, os.PathLike)):
        path = Path(factors)
        meta = read_binary_file_metadata(path)
        return _file_records(path), meta["total_length"], meta["sentinel_factor_indices"]
    if isinstance(factors, np.ndarray):
        return factors, total_length, sentinel_factor_indices
    sent = set(sentinel_factor_indices)
    rows, kept_sent = [], []
    for idx, f in enumerate(factors):
        if len(f) == 4:
            row = (f[0], f[1], f[2] | RC_MASK if f[3] else f[2])
        elif len(f) == 3:
            row = tuple(f)
        else:
            continue
        if idx in sent:
            kept_sent.append(len(rows))
        rows.append(row)
    return np.array(rows, dtype=np.uint64).reshape(len(rows), 3), total_length, kept_sent


def factors_strand_bias_grid(factors, grid_size=50, total_length: Optional[int] = None, min_factor_length: int = 1,
                             sentinel_factor_indices=()) -> Dict[str, Any]:
    """The factors_filepath branch of plot_strand_bias_heatmap: `factors` is the path of a v2 factor file (total_length
    and the sentinel factor indices then come from its footer), a list of factor tuples, or a record array."""
    grid = _grid_arg(grid_size)
    recs, total_length, sent = _records_arg(factors, total_length, sentinel_factor_indices)
    if len(recs) == 0:
        raise PlotError("No factors available to compute strand bias grid")
    _check_total_length(total_length)
    return _grid_result(_run(lambda: _native.records_factor_maps(recs, sent, grid=grid, total_length=total_length,
                                                                 min_factor_length=min_factor_length)))


def length_ladder(length_log_base: float) -> np.ndarray:
    """base ** (j / 4), j = 0 .. 4 * K, K the first power with base ** K >= 2^32: every length ladder of
    plot_space_scale_heatmap (plots.py:2584-2590) is the slice j = 4 * min_log .. 4 * max_log of it, bit for bit."""
    base = float(length_log_base)
    if not base > 1.0:
        raise ValueError("length_log_base must be greater than 1")
    top = int(np.ceil(np.log(2.0 ** 32) / np.log(base))) + 1
    if 4 * top + 1 > _MAX_LENGTH_EDGES:
        raise ValueError(f"length_log_base {length_log_base} needs more than {_MAX_LENGTH_EDGES} length edges")
    return base ** np.linspace(0, top, 4 * top + 1)


def space_scale_histogram(data=None, *, fasta_filepath=None, factors=None, with_rc: bool = True,
                          sanitize_mode: str = "remove_ambiguous", genome_bin_size: float = 1.0,
                          length_log_base: float = 2.0, min_factor_length: int = 1,
                          sentinel_factor_indices=()) -> Dict[str, Any]:
    """The 2-D histograms of plot_space_scale_heatmap (plots.py:2566-2614) from one device run: exactly one of `data`
    (a sequence), `fasta_filepath` or `factors` (a v2 file path, tuples or a record array).  Returns genome_bins,
    length_bin_edges, forward_hist, reverse_hist (float arrays of counts, [length_bin][position_bin]) and the kept
    counts, min_length, max_length, max_start."""
    if sum(x is not None for x in (data, fasta_filepath, factors)) != 1:
        raise ValueError("Exactly one of data, fasta_filepath or factors must be provided")
    genome_bin_bp = int(genome_bin_size * 1_000_000)
    if genome_bin_bp <= 0:
        raise ValueError("genome_bin_size must be at least 1e-6 Mb")
    ladder = length_ladder(length_log_base)

    def run(length_edges):
        kw = dict(min_factor_length=min_factor_length, length_edges=length_edges, position_min_bins=50,
                  position_bin_bp=genome_bin_bp)
        if data is not None:
            return _native.factor_maps(data, with_rc=with_rc, **kw)
        if fasta_filepath is not None:
            if not Path(fasta_filepath).exists():
                raise FileNotFoundError(f"Input file not found: {fasta_filepath}")
            return _native.fasta_factor_maps(os.fspath(fasta_filepath), with_rc=with_rc, sanitize_mode=sanitize_mode,
                                             **kw)
        recs, _, sent = _records_arg(factors, None, sentinel_factor_indices)
        if len(recs) == 0:
            raise PlotError("No factors found in input file")
        return _native.records_factor_maps(recs, sent, **kw)

    m = run(ladder)
    if m["z_used"] == 0:
        raise PlotError("No valid factors to plot")
    if m["hist_forward"] is None:  # genome_end = 0: the reference's linspace(0, 0, ..) has no bins to speak of
        raise PlotError("No valid factor positions")
    min_length = max(1, m["min_length"])
    max_length = m["max_length"]
    min_log = int(np.floor(np.log(min_length) / np.log(length_log_base)))
    max_log = int(np.ceil(np.log(max_length) / np.log(length_log_base)))
    lo, hi = 4 * min_log, 4 * max_log
    if hi - lo < 1:
        raise PlotError("Fewer than one length bin: all factors have the same length class")
    edges = ladder[lo:hi + 1]
    if max_length <= edges[-1]:
        # rows lo .. hi - 1 of the one run; a length equal to the last edge sits in row hi and belongs to the last bin
        fwd, rev = (h[lo:hi].astype(np.float64) for h in (m["hist_forward"], m["hist_rc"]))
        if hi < m["hist_forward"].shape[0]:
            fwd[-1] += m["hist_forward"][hi]
            rev[-1] += m["hist_rc"][hi]
    else:  # ceil(log) came out one short in floating point: the reference drops the lengths above its last edge
        m = run(edges)
        fwd, rev = m["hist_forward"].astype(np.float64), m["hist_rc"].astype(np.float64)
    return {"genome_bins": m["position_edges"], "length_bin_edges": edges, "forward_hist": fwd, "reverse_hist": rev,
            "kept_forward": m["kept_forward"], "kept_rc": m["kept_rc"], "min_length": m["min_length"],
            "max_length": max_length, "max_start": m["max_start"], "z": m["z"], "z_used": m["z_used"]}


def sequence_boundaries_from(sentinel_starts, sequence_names, max_pos: Optional[int]):
    """[(start_pos, end_pos, sequence_name)] as plots.py:522-553 computes them: one sequence between two sentinel
    factors (the sentinel itself is skipped), names from `sequence_names` or seq_<i>; the last one ends at max_pos, the
    largest x or y of any factor.  max_pos = None: no factors (the reference's 1000 / the last sentinel + 1)."""
    names = list(sequence_names) if sequence_names else []
    positions = [int(p) for p in sentinel_starts]
    if not positions:
        return [(0, 1000 if max_pos is None else max_pos, names[0] if names else "sequence")]
    out, prev_pos = [], 0
    for i, pos in enumerate(positions):
        out.append((prev_pos, pos, names[i] if i < len(names) else f"seq_{i}"))
        prev_pos = pos + 1
    last_name = names[len(positions)] if len(names) > len(positions) else f"seq_{len(positions)}"
    out.append((prev_pos, prev_pos if max_pos is None else max_pos, last_name))
    return out


def default_view(x_max: int, y_max: int, width: int, height: int, x_range=None, y_range=None):
    """-> ((x_lo, x_hi), (y_lo, y_hi)).  A range that is not given is [0, max(x_max, y_max)), the reference's diagonal
    extent, raised so that it spans at least one base per pixel; a given range is passed on as it is."""
    extent = max(int(x_max), int(y_max))
    if x_range is None:
        x_range = (0, max(extent, int(width)))
    if y_range is None:
        y_range = (0, max(extent, int(height)))
    (x_lo, x_hi), (y_lo, y_hi) = x_range, y_range
    return (int(x_lo), int(x_hi)), (int(y_lo), int(y_hi))


class DotPlot(_native.DotPlot):
    """What self_dotplot returns: .info (z, x_max, y_max, min_length, max_length, kept_forward, kept_rc, device,
    sentinel_starts), .sequence_boundaries and .render(); a context manager that frees the device records."""

    _names = None
    _fasta = None

    @property
    def sequence_boundaries(self):
        names = self._names
        if names is None and self._fasta is not None:
            path, mode = self._fasta
            names = self._names = [i.decode("utf-8", "replace") for i, _ in _native.debug_parse_fasta(path, mode)]
        max_pos = max(self.info["x_max"], self.info["y_max"]) if self.info["z"] else None
        return sequence_boundaries_from(self.info["sentinel_starts"], names, max_pos)

    def render(self, x_range=None, y_range=None, width: int = 800, height: int = 800, min_factor_length: int = 1,
               length_range=None, hover_bins: int = 0, counts: bool = False) -> Dict[str, Any]:
        """The view x_range x y_range (half-open nucleotide windows; default: the square [0, max(x_max, y_max)))
        as width x height pixels: max_forward, max_rc, count_forward, count_rc (uint32, shape (height, width), row 0
        the lowest y), visible_forward, visible_rc, hover_start, hover_length, hover_ref, and the x_range / y_range
        used.  length_range: the reference's slider, inclusive."""
        x_range, y_range = default_view(self.info["x_max"], self.info["y_max"], width, height, x_range, y_range)
        out = super().render(x_range, y_range, width=width, height=height, min_factor_length=min_factor_length,
                             length_range=length_range, hover_bins=hover_bins, counts=counts)
        out["x_range"], out["y_range"] = x_range, y_range
        return out


def self_dotplot(data=None, *, fasta_filepath=None, factors=None, with_rc: bool = True,
                 sanitize_mode: str = "remove_ambiguous", sentinel_factor_indices=(), sequence_names=None) -> DotPlot:
    """The data of the reference's self LZ factor plots (plots.py:352-900) without the download of the records:
    factorise once -- exactly one of `data` (a sequence), `fasta_filepath` or `factors` (a v2 factor file path, tuples
    or a record array) --, then render views.  The hover table keeps a factor with a base pair in view, where the
    reference tests its bounding box against the view padded by 10 %."""
    if sum(x is not None for x in (data, fasta_filepath, factors)) != 1:
        raise ValueError("Exactly one of data, fasta_filepath or factors must be provided")
    if data is not None:
        dp = DotPlot.from_text(data, with_rc=with_rc)
    elif fasta_filepath is not None:
        if not Path(fasta_filepath).exists():
            raise FileNotFoundError(f"Input file not found: {fasta_filepath}")
        dp = DotPlot.from_fasta(os.fspath(fasta_filepath), with_rc=with_rc, sanitize_mode=sanitize_mode)
        dp._fasta = (os.fspath(fasta_filepath), sanitize_mode)
    else:
        if isinstance(factors, (str, os.PathLike)) and sequence_names is None:
            sequence_names = read_binary_file_metadata(Path(factors)).get("sequence_names")
        recs, _, sent = _records_arg(factors, None, sentinel_factor_indices)
        dp = DotPlot.from_records(recs, sent)
    if sequence_names is not None:
        dp._names = list(sequence_names)
    return dp

"""Factor-length significance against a shuffled control (mirror of the reference's noLZSS.genomics.significance,
reference: src/noLZSS/genomics/significance.py).

From which factor length on is a repeat signal and not noise?  The factor lengths of a genome are compared with those
of a shuffled copy: S0(L) = P(shuffled length >= L), its one-sided Clopper-Pearson upper bound S0^U(L), and the
threshold L* = the smallest observed L with N_real * S0^U(L) <= tau_expected_fp.

The four names of the reference keep their signatures, dictionary keys, values, warnings and error messages.  The work
inside runs on counts: the tail counts come from one cumulative sum over np.unique(..., return_counts=True) instead of
one pass over all lengths per unique length, so O(N + U log U) instead of O(U N); the integer counts are the same,
and so is every float derived from them.  Drawing is not part of this package (data layer of the plots: plots.py).

Extensions (GPU): shuffled_control_significance / fasta_shuffled_control_significance take the factor lengths of the
text and of its keyed shuffle straight from the device (histograms and lengths, no factor records).
"""
import os
import warnings
from pathlib import Path
from typing import Any, Dict, List, Optional, Tuple, Union

import numpy as np

from ..utils import NoLZSSError, _read_footer

__all__ = ["clopper_pearson_upper", "extract_factor_lengths", "infer_length_significance",
           "calculate_factor_length_threshold", "shuffled_control_significance",
           "fasta_shuffled_control_significance", "factor_length_histogram", "shuffle_dna"]


def clopper_pearson_upper(k: int, n: int, alpha: float = 0.05) -> float:
    """One-sided (1 - alpha) Clopper-Pearson upper confidence bound for Binomial(n, p) after k successes: the
    (1 - alpha) quantile of Beta(k + 1, n - k); 1 for k = n, 1 - alpha^(1/n) for k = 0.  Without scipy: the Wilson
    score bound for alpha in {0.01, 0.025, 0.05}, with a UserWarning."""
    if n <= 0:
        raise ValueError(f"n must be positive, got {n}")
    if k < 0 or k > n:
        raise ValueError(f"k must be between 0 and n, got k={k}, n={n}")
    if alpha <= 0 or alpha >= 1:
        raise ValueError(f"alpha must be in (0, 1), got {alpha}")
    if k == n:
        return 1.0
    if k == 0:
        return 1.0 - (alpha ** (1.0 / n))
    try:
        from scipy.stats import beta
    except ImportError:
        warnings.warn(
            "scipy not available, using Wilson score approximation for Clopper-Pearson bound. "
            "Install scipy for exact bounds: pip install scipy",
            UserWarning
        )
        if alpha == 0.05:
            z = 1.645
        elif alpha == 0.025:
            z = 1.96
        elif alpha == 0.01:
            z = 2.326
        else:
            raise ValueError(
                f"Wilson score fallback only supports alpha in [0.01, 0.025, 0.05], got {alpha}. "
                "Install scipy for arbitrary alpha values: pip install scipy"
            )
        p_hat = k / n
        denominator = 1 + z**2 / n
        center = (p_hat + z**2 / (2*n)) / denominator
        margin = z * np.sqrt((p_hat * (1 - p_hat) / n + z**2 / (4*n**2))) / denominator
        return float(min(center + margin, 1.0))
    return float(beta.ppf(1.0 - alpha, k + 1, n - k))


def _file_lengths(path: Path) -> np.ndarray:
    """The length column of a v2 factor file, read with numpy (the checks and messages of
    utils.read_factors_binary_file, without a tuple per factor)."""
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
    if nf == 0:
        return np.array([], dtype=np.int64)
    return np.frombuffer(data, dtype="<u8").reshape(nf, 3)[:, 1].astype(np.int64)


def extract_factor_lengths(factors: Union[List[Tuple[int, ...]], str, Path]) -> np.ndarray:
    """Factor lengths (int64) from a list of (pos, length, ...) tuples or from a v2 binary factor file."""
    if isinstance(factors, (str, Path)):
        return _file_lengths(Path(factors))
    elif isinstance(factors, list):
        if not factors:
            return np.array([], dtype=np.int64)
        for i, factor in enumerate(factors):
            if not isinstance(factor, tuple) or len(factor) < 2:
                raise ValueError(
                    f"Factor at index {i} must be a tuple with at least 2 elements "
                    f"(pos, length, ...), got {type(factor)}"
                )
        return np.array([f[1] for f in factors], dtype=np.int64)
    else:
        raise ValueError(
            f"factors must be a list of tuples or a file path, got {type(factors)}"
        )


def _check_sizes(N_real: int, N_shuf: int) -> None:
    if N_real == 0:
        warnings.warn("Real genome has no factors - analysis is meaningless", UserWarning)
    if N_shuf == 0:
        raise ValueError("Shuffled genome must have at least one factor")


def _rarity(real_lengths: np.ndarray, uniq_L: np.ndarray, S0: np.ndarray) -> np.ndarray:
    """np.interp(real_lengths, uniq_L, S0, left=1.0, right=0.0).  Many integer lengths below a small maximum: the
    same np.interp over 0..max once, then a gather -- every element gets the value np.interp gives it (the same
    float64 input), 10x less time for 5*10^7 factors."""
    n = len(real_lengths)
    if n and np.issubdtype(real_lengths.dtype, np.integer):
        lo, top = int(real_lengths.min()), int(real_lengths.max())
        if lo >= 0 and top < n and top < 1 << 24:
            return np.interp(np.arange(top + 1), uniq_L, S0, left=1.0, right=0.0)[real_lengths]
    return np.interp(real_lengths, uniq_L, S0, left=1.0, right=0.0)


def _significance(real_lengths: np.ndarray, uniq_L: np.ndarray, counts: np.ndarray, tau_expected_fp: float,
                  alpha_cp: float) -> Dict[str, Any]:
    """The statistics of infer_length_significance from the shuffled lengths as (ascending unique values, counts);
    the sizes have been checked (_check_sizes)."""
    N_real = len(real_lengths)
    N_shuf = int(counts.sum())
    counts = np.asarray(counts, dtype=np.int64)
    # ge[j] = number of shuffled lengths >= uniq_L[j]
    ge = N_shuf - np.concatenate(([0], np.cumsum(counts)[:-1]))
    S0 = ge / N_shuf
    S0_upper = np.array([clopper_pearson_upper(int(k), N_shuf, alpha_cp) for k in ge])
    expected_fp_upper = N_real * S0_upper
    L_star = None
    valid_indices = np.where(expected_fp_upper <= tau_expected_fp)[0]
    if len(valid_indices) > 0:
        L_star = int(uniq_L[valid_indices[0]])
    rarity_scores_real = _rarity(real_lengths, uniq_L, S0)

    def p_any_ge(L: float) -> float:
        """Poisson approximation of P(at least one real factor has length >= L) = 1 - exp(-N_real * S0(L))."""
        s0_L = np.interp(L, uniq_L, S0, left=1.0, right=0.0)
        lambda_val = N_real * s0_L
        return 1.0 - np.exp(-lambda_val)

    return {
        'N_real': N_real,
        'N_shuf': N_shuf,
        'L_star': L_star,
        'tau_expected_fp': tau_expected_fp,
        'alpha_cp': alpha_cp,
        'rarity_scores_real': rarity_scores_real,
        'p_any_ge': p_any_ge,
        'uniq_L': uniq_L,
        'S0': S0,
        'S0_upper': S0_upper,
        'expected_fp_upper': expected_fp_upper,
    }


def infer_length_significance(
    real_lengths: Union[np.ndarray, List[int]],
    shuf_lengths: Union[np.ndarray, List[int]],
    tau_expected_fp: float = 1.0,
    alpha_cp: float = 0.05
) -> Dict[str, Any]:
    """Length-only inference against ONE shuffled genome: S0(L) = P0(len >= L) over the unique shuffled lengths,
    S0_upper = its Clopper-Pearson bound, L_star = the smallest L with N_real * S0_upper(L) <= tau_expected_fp (None
    if there is none), rarity_scores_real = S0 interpolated at every real length (1 below, 0 above the shuffled
    range) and p_any_ge(L) = 1 - exp(-N_real * S0(L)).  Keys: N_real, N_shuf, L_star, tau_expected_fp, alpha_cp,
    rarity_scores_real, p_any_ge, uniq_L, S0, S0_upper, expected_fp_upper."""
    real_lengths = np.asarray(real_lengths, dtype=np.int64)
    shuf_lengths = np.asarray(shuf_lengths, dtype=np.int64)
    _check_sizes(len(real_lengths), len(shuf_lengths))
    uniq_L, counts = np.unique(shuf_lengths, return_counts=True)
    return _significance(real_lengths, uniq_L, counts, tau_expected_fp, alpha_cp)


def calculate_factor_length_threshold(
    real_factors_file: Union[str, Path],
    shuffled_factors_file: Union[str, Path],
    tau_expected_fp: float = 1.0,
    alpha_cp: float = 0.05,
    plot_output: Optional[Union[str, Path]] = None
) -> Dict[str, Any]:
    """infer_length_significance over the factor lengths of two v2 binary factor files (the genome and its shuffled
    copy).  plot_output must be None: plots are not part of this package."""
    if plot_output is not None:
        raise ValueError("plot_output is not supported: plots are not part of this package")
    real_path = Path(real_factors_file)
    shuf_path = Path(shuffled_factors_file)
    if not real_path.exists():
        raise FileNotFoundError(f"Real factors file not found: {real_path}")
    if not shuf_path.exists():
        raise FileNotFoundError(f"Shuffled factors file not found: {shuf_path}")
    real_lengths = extract_factor_lengths(real_path)
    shuf_lengths = extract_factor_lengths(shuf_path)
    return infer_length_significance(real_lengths, shuf_lengths, tau_expected_fp=tau_expected_fp, alpha_cp=alpha_cp)


# ---- GPU: the lengths of a text and of its keyed shuffle, straight from the device ------------------------------
def hist_values_counts(hist: Dict[str, Any]) -> Tuple[np.ndarray, np.ndarray]:
    """A device length histogram (both strands) as ascending unique lengths and their counts."""
    dense = np.asarray(hist["fwd"], dtype=np.int64) + np.asarray(hist["rc"], dtype=np.int64)
    vals = np.nonzero(dense)[0].astype(np.int64)
    counts = dense[vals]
    if len(hist["tail_lengths"]):  # (all >= the dense range)
        tv, tc = np.unique(hist["tail_lengths"], return_counts=True)
        vals = np.concatenate((vals, tv.astype(np.int64)))
        counts = np.concatenate((counts, tc.astype(np.int64)))
    return vals, counts


def factor_length_histogram(data, with_rc: bool = False, shuffle_seed: Optional[int] = None) -> Dict[str, Any]:
    """The factor-length histogram of `data` on the GPU (see nolzss_amd._noLZSS.factor_length_histogram)."""
    from .. import _noLZSS
    return _noLZSS.factor_length_histogram(data, with_rc=with_rc, shuffle_seed=shuffle_seed)


def shuffle_dna(data, seed: int) -> bytes:
    """The keyed shuffle of `data` on the GPU: a control text with the same composition."""
    from .. import _noLZSS
    return _noLZSS.shuffle_dna(data, seed)


def _draw_seed(seed: Optional[int]) -> int:
    if seed is None:
        return int.from_bytes(os.urandom(8), "little")
    from .._noLZSS import _seed_arg
    return _seed_arg(seed)


def _from_hists(real: Dict[str, Any], shuf: Dict[str, Any], seed: int, with_rc: bool, tau_expected_fp: float,
                alpha_cp: float) -> Dict[str, Any]:
    uniq_L, counts = hist_values_counts(shuf)
    real_lengths = real["lengths"]  # (uint32: np.interp converts to float64 exactly, as it does the int64 lengths)
    _check_sizes(len(real_lengths), int(counts.sum()))
    result = _significance(real_lengths, uniq_L, counts, tau_expected_fp, alpha_cp)
    real = {k: v for k, v in real.items() if k != "lengths"}
    result.update({"seed": seed, "with_rc": with_rc, "real_hist": real, "shuf_hist": shuf})
    return result


def shuffled_control_significance(data, with_rc: bool = False, seed: Optional[int] = None,
                                  tau_expected_fp: float = 1.0, alpha_cp: float = 0.05) -> Dict[str, Any]:
    """infer_length_significance(lengths of data, lengths of shuffle_dna(data, seed)) with both factorizations on
    the GPU and no factor record leaving it.  with_rc: the reverse-complement mode of count_factors_dna_w_rc.  seed
    None: drawn from os.urandom and reported back.  Extra keys: seed, with_rc, real_hist, shuf_hist."""
    from .. import _noLZSS
    seed = _draw_seed(seed)
    real = _noLZSS.factor_length_histogram_with_lengths(data, with_rc=with_rc)
    shuf = _noLZSS.factor_length_histogram(data, with_rc=with_rc, shuffle_seed=seed)
    return _from_hists(real, shuf, seed, with_rc, tau_expected_fp, alpha_cp)


def fasta_shuffled_control_significance(path, with_rc: bool = True, sanitize_mode: str = "remove_ambiguous",
                                        seed: Optional[int] = None, tau_expected_fp: float = 1.0,
                                        alpha_cp: float = 0.05) -> Dict[str, Any]:
    """The same over the concatenated multiple-DNA form of a FASTA file (the factors that
    write_factors_binary_file_fasta_multiple_dna_{w,no}_rc write), the control being every record shuffled on its own
    with the sentinels in place."""
    from .. import _noLZSS
    seed = _draw_seed(seed)
    path = str(path)
    real = _noLZSS.fasta_factor_length_histogram(path, with_rc=with_rc, sanitize_mode=sanitize_mode,
                                                 want_lengths=True)
    shuf = _noLZSS.fasta_factor_length_histogram(path, with_rc=with_rc, sanitize_mode=sanitize_mode,
                                                 shuffle_seed=seed)
    return _from_hists(real, shuf, seed, with_rc, tau_expected_fp, alpha_cp)

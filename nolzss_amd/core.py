"""The user-facing factorize API of the hot path, written once for both import names.

`bind(native)` builds the seven functions of the reference's `noLZSS.core` (reference:
src/noLZSS/core.py:25-257 -- names, argument meaning, error behaviour), the two of the decoder (extension:
`decode`, `literal_symbols`) and the four of the compact container of factor records (extension: `factorize_packed`,
`pack_factors`, `unpack_factors`, `decode_packed`) over a native module:
`nolzss_amd.core` binds them to the ctypes mirror `nolzss_amd._noLZSS`, `noLZSS.core` to the compiled
pybind11 module `noLZSS._noLZSS`.  Both native modules call the same C ABI (include/nolzss_hip.h).
"""
from pathlib import Path
from typing import List, Tuple, Union

from .utils import validate_input

__all__ = ["factorize", "factorize_file", "count_factors", "count_factors_file", "write_factors_binary_file",
           "factorize_w_reference", "factorize_w_reference_file", "decode", "literal_symbols", "factorize_packed",
           "pack_factors", "unpack_factors", "decode_packed"]

Factors = List[Tuple[int, int, int]]
Text = Union[str, bytes]
PathLike = Union[str, Path]


def _existing(filepath: PathLike) -> str:
    p = Path(filepath)
    if not p.exists():  # before the extension is touched (reference: core.py:61-63, 102-104)
        raise FileNotFoundError(f"File not found: {p}")
    return str(p)


def _writable(filepath: PathLike) -> str:
    p = Path(filepath)
    p.parent.mkdir(parents=True, exist_ok=True)  # reference: core.py:130-131, 254-255
    return str(p)


def bind(native) -> dict:
    """the functions of `__all__` over `native` (a module with the reference's `_noLZSS` surface)"""

    def checked(data: Text, validate: bool):
        return validate_input(data) if validate else data

    def factorize(data: Text, validate: bool = True) -> Factors:
        """(start, length, ref) of every factor of `data` (reference: core.py:25-43)"""
        return native.factorize(checked(data, validate))

    def count_factors(data: Text, validate: bool = True) -> int:
        """number of factors of `data` (reference: core.py:68-86)"""
        return native.count_factors(checked(data, validate))

    def factorize_file(filepath: PathLike, reserve_hint: int = 0) -> Factors:
        """factors of the bytes of a file (reference: core.py:46-65)"""
        return native.factorize_file(_existing(filepath), reserve_hint)

    def count_factors_file(filepath: PathLike, validate: bool = True) -> int:
        """number of factors of the bytes of a file (reference: core.py:89-107; `validate` is unused there too)"""
        return native.count_factors_file(_existing(filepath))

    def write_factors_binary_file(data: Text, output_filepath: PathLike) -> None:
        """Kept from the reference (core.py:110-132 against bindings.cpp:180-187): the validated `data` goes to a
        parameter of the native function that is an input FILE PATH, so `data` must name a file (README.md:65).
        (No `validate` parameter: the reference's signature has none and always validates.)"""
        native.write_factors_binary_file(validate_input(data), _writable(output_filepath))

    def as_ascii_str(seq: Text) -> str:
        # the reference hands the two sequences to its binding as str: bytes are decoded as ASCII first, and bytes
        # above 0x7f raise UnicodeDecodeError there (core.py:201-205, 247-251)
        return seq.decode("ascii") if isinstance(seq, bytes) else seq

    def factorize_w_reference(reference_seq: Text, target_seq: Text, validate: bool = True) -> Factors:
        """the target factorized against reference + '\\x01' + target, positions absolute in that string
        (reference: core.py:164-207)"""
        return native.factorize_w_reference(as_ascii_str(checked(reference_seq, validate)),
                                            as_ascii_str(checked(target_seq, validate)))

    def factorize_w_reference_file(reference_seq: Text, target_seq: Text, output_path: PathLike,
                                   validate: bool = True) -> int:
        """the same into a v2 binary factor file; returns the number of factors (reference: core.py:210-257)"""
        return native.factorize_w_reference_file(as_ascii_str(checked(reference_seq, validate)),
                                                 as_ascii_str(checked(target_seq, validate)), _writable(output_path))

    def as_bytes(data: Text) -> bytes:
        return data.encode("ascii") if isinstance(data, str) else data

    def literal_symbols(data: Text, factors) -> bytes:
        """Extension: the symbols of the literal factors (ref == start) of `factors` in factor order, read from
        `data` -- a factor record does not carry them, and `decode` needs them."""
        return native.literal_symbols(as_bytes(data), factors)

    def decode(factors, literals: Text, prefix: Text = b"") -> bytes:
        """Extension: the text of a factorization.  `factors`: what `factorize` (3-tuples) or the reverse-complement
        forms (4-tuples with is_rc) return, or a structured array; `literals`: `literal_symbols` of the text;
        `prefix`: the known bytes in front of the first factor (for `factorize_w_reference`: reference + '\x01')."""
        return native.decode_array(factors, as_bytes(literals), as_bytes(prefix))[0].tobytes()

    def factorize_packed(data: Text, with_rc: bool = False, literals: bool = True) -> dict:
        """Extension: factorize `data` (with_rc: as `factorize_dna_w_rc`) and pack the factors on the GPU -> the sections
        of the compact container (a dict: literal_mode, first_start, z, n_literals, decoded, control, data, literals);
        only they leave the device.  `literals` False leaves the literal symbols out (a factor file like v2).
        `utils.write_packed_factors` writes the sections to a file."""
        return native.factorize_packed(as_bytes(data), with_rc, literals)

    def pack_factors(factors, literals=None) -> dict:
        """Extension: the sections of the compact container from factors any mode returned (3-tuples, 4-tuples with
        is_rc, or a structured array) and, optionally, `literal_symbols` of the text."""
        return native.pack_factors(factors, None if literals is None else as_bytes(literals))

    def unpack_factors(sections):
        """Extension: sections -> (structured array of (start, length, ref), ref carrying the reverse-complement mask;
        the literal symbols, or None when the sections hold none).  The sections are checked on the GPU."""
        return native.unpack_factors(sections)

    def decode_packed(sections, prefix: Text = b"") -> bytes:
        """Extension: the text of the sections, expanded and decoded on the GPU; `prefix`: the first_start known bytes in
        front of the first factor (for `factorize_w_reference`: reference + '\x01')."""
        return native.decode_packed_array(sections, as_bytes(prefix))[0].tobytes()

    fns = locals()
    return {name: fns[name] for name in __all__}


from . import _noLZSS as _mirror  # noqa: E402

globals().update(bind(_mirror))

"""Input validation for the factorize path (mirror of the reference's noLZSS.utils,
reference: src/noLZSS/utils.py:16-58; only what the hot path needs), the readers of v2 factor files and the file of
the compact container of factor records (extension: write_packed_factors / read_packed_factors)."""
import struct
from pathlib import Path
from typing import Any, Dict, List, Tuple, Union


class NoLZSSError(Exception):
    """Base exception of the package (reference: utils.py:16-18)."""


class InvalidInputError(NoLZSSError):
    """Input data is invalid for factorization (reference: utils.py:21-23)."""


def validate_input(data: Union[str, bytes]) -> bytes:
    """str -> ASCII bytes; reject non-ASCII, empty input and NUL bytes anywhere but the last
    position; TypeError for anything that is neither str nor bytes (reference: utils.py:26-58)."""
    if isinstance(data, str):
        try:
            data = data.encode("ascii")
        except UnicodeEncodeError as e:
            raise InvalidInputError(f"Input string must contain only ASCII characters (1 byte each): {e}")
    elif not isinstance(data, bytes):
        raise TypeError(f"Input must be str or bytes, got {type(data)}")
    if len(data) == 0:
        raise InvalidInputError("Input data cannot be empty")
    if b"\x00" in data[:-1]:
        raise InvalidInputError("Input data contains null bytes")
    return data


# ---- v2 binary factor files (reference: utils.py:106-357; format factorizer.hpp:64-77) --------
_FOOTER = struct.Struct("<8sQQQQQ")  # magic, num_factors, num_sequences, num_sentinels, footer_size, total_length


def _read_footer(f) -> Tuple[int, int, int, int, int]:
    # (a file shorter than the footer fails in the seek, as in the reference: the caller reports
    # "Error reading file ...: [Errno 22] Invalid argument" -- pinned by tests/golden/python_ref_utils.json)
    f.seek(-_FOOTER.size, 2)
    raw = f.read(_FOOTER.size)
    if len(raw) != _FOOTER.size:
        raise NoLZSSError("File too small to contain valid footer")
    magic, nf, nseq, nsent, fsize, total = _FOOTER.unpack(raw)
    if magic != b"noLZSSv2":
        raise NoLZSSError("Invalid file format: missing noLZSS magic footer (expected v2 format)")
    return nf, nseq, nsent, fsize, total


def read_factors_binary_file(filepath: Union[str, Path]) -> List[Tuple[int, int, int]]:
    """[(start, length, ref)] from a v2 factor file (reference: utils.py:106-155)."""
    filepath = Path(filepath)
    if not filepath.exists():
        raise NoLZSSError(f"File not found: {filepath}")
    try:
        with open(filepath, "rb") as f:
            nf = _read_footer(f)[0]
            f.seek(0)
            data = f.read(24 * nf)
    except OSError as e:
        raise NoLZSSError(f"Error reading file {filepath}: {e}")
    if len(data) != 24 * nf:
        raise NoLZSSError(f"Insufficient data for factor {len(data) // 24}")
    return [struct.unpack_from("<QQQ", data, 24 * i) for i in range(nf)]


def read_binary_file_metadata(filepath: Union[str, Path]) -> Dict[str, Any]:
    """Footer metadata only: names, sentinel factor indices, counts (reference: utils.py:158-251)."""
    filepath = Path(filepath)
    if not filepath.exists():
        raise NoLZSSError(f"File not found: {filepath}")
    try:
        with open(filepath, "rb") as f:
            nf, nseq, nsent, fsize, total = _read_footer(f)
            f.seek(-fsize, 2)
            full = f.read(fsize)
    except OSError as e:
        raise NoLZSSError(f"Error reading file {filepath}: {e}")
    if len(full) != fsize:
        raise NoLZSSError(f"Could not read full footer: expected {fsize}, got {len(full)}")
    meta = full[:fsize - _FOOTER.size]
    names, off = [], 0
    for _ in range(nseq):
        end = meta.find(b"\x00", off)
        if end < 0:
            raise NoLZSSError("Invalid sequence name format")
        names.append(meta[off:end].decode("utf-8"))
        off = end + 1
    if off + 8 * nsent > len(meta):
        raise NoLZSSError("Insufficient data for sentinel indices")
    sentinels = list(struct.unpack_from(f"<{nsent}Q", meta, off)) if nsent else []
    return {"sentinel_factor_indices": sentinels, "sequence_names": names, "num_sequences": nseq,
            "num_sentinels": nsent, "num_factors": nf, "total_length": total}


def read_factors_binary_file_with_metadata(filepath: Union[str, Path]) -> Dict[str, Any]:
    """Factors as (start, length, ref & ~RC_MASK, is_rc) plus the metadata (reference: utils.py:254-357)."""
    meta = read_binary_file_metadata(filepath)
    rc_mask = 1 << 63
    factors = [(s, l, r & (rc_mask - 1), bool(r & rc_mask)) for s, l, r in read_factors_binary_file(filepath)]
    # (the reference's dictionary has no 'num_factors' here, unlike read_binary_file_metadata: utils.py:350-357;
    # pinned by tests/golden/python_ref_utils.json)
    return {"factors": factors, "sentinel_factor_indices": meta["sentinel_factor_indices"],
            "sequence_names": meta["sequence_names"], "num_sequences": meta["num_sequences"],
            "num_sentinels": meta["num_sentinels"], "total_length": meta["total_length"]}


# ---- the file of the compact container of factor records (extension; format: include/nolzss_hip.h) ----------------
_PACKED_MAGIC = b"noLZFAC1"
_PACKED_HEADER = struct.Struct("<8sII7Q")  # magic, version, flags, first_start, z, n_literals, decoded, three sizes
_PACKED_SECTIONS = ("control", "data", "literals")


def _packed_literal_bytes(mode: int, n_literals: int) -> int:
    return (n_literals + 3) // 4 if mode == 1 else n_literals if mode == 0 else 0


def write_packed_factors(path: Union[str, Path], sections: Dict[str, Any]) -> int:
    """The sections of `factorize_packed` / `pack_factors` -> a compact factor file; returns its size in bytes.
    Host only.  Sections whose sizes disagree with their counts are refused (ValueError) before anything is written."""
    mode, z, nlit = (int(sections[k]) for k in ("literal_mode", "z", "n_literals"))
    parts = [bytes(sections[name]) for name in _PACKED_SECTIONS]
    if mode not in (0, 1, 2):
        raise ValueError(f"packed factors: literal_mode {mode} is none of 0, 1, 2")
    if len(parts[0]) != (z + 1) // 2 or len(parts[2]) != _packed_literal_bytes(mode, nlit):
        raise ValueError("packed factors: a section has not the size the counts ask for")
    head = _PACKED_HEADER.pack(_PACKED_MAGIC, 1, mode, int(sections["first_start"]), z, nlit, int(sections["decoded"]),
                               *[len(x) for x in parts])
    raw = head + b"".join(x + b"\0" * (-len(x) % 8) for x in parts)
    Path(path).write_bytes(raw)
    return len(raw)


def read_packed_factors(path: Union[str, Path]) -> Dict[str, Any]:
    """A compact factor file -> the sections `unpack_factors` / `decode_packed` take.  Host only: the header and the
    sizes are checked here (NoLZSSError naming what is wrong), the records themselves on the GPU when they are expanded."""
    path = Path(path)
    if not path.exists():
        raise NoLZSSError(f"File not found: {path}")
    raw = path.read_bytes()

    def bad(what: str) -> NoLZSSError:
        return NoLZSSError(f"{path}: not a compact factor file: {what}")

    if len(raw) < _PACKED_HEADER.size:
        raise bad(f"truncated: {len(raw)} bytes are fewer than the {_PACKED_HEADER.size} of the header")
    magic, version, flags, first_start, z, nlit, decoded, *sizes = _PACKED_HEADER.unpack_from(raw)
    if magic != _PACKED_MAGIC:
        raise bad(f"wrong magic {magic!r} (expected {_PACKED_MAGIC!r})")
    if version != 1:
        raise bad(f"unknown version {version} (this reader knows 1)")
    if flags & ~3 or (flags & 3) == 3:
        raise bad(f"unknown flag bits {flags:#x}")
    mode = flags & 3
    want = ((z + 1) // 2, sizes[1], _packed_literal_bytes(mode, nlit))
    for name, have, need in zip(_PACKED_SECTIONS, sizes, want):
        if have != need:
            raise bad(f"section sizes disagree with the counts: the {name} section holds {have} bytes, "
                      f"the counts ask for {need}")
    at, parts = _PACKED_HEADER.size, []
    for name, n in zip(_PACKED_SECTIONS, sizes):
        end = at + n + (-n % 8)
        if end > len(raw):
            raise bad(f"truncated: the {name} section ends at byte {end}, the file holds {len(raw)}")
        if any(raw[at + n:end]):
            raise bad(f"the padding behind the {name} section is not zero")
        parts.append(raw[at:at + n])
        at = end
    if at != len(raw):
        raise bad(f"{len(raw) - at} trailing bytes behind the last section")
    return {"literal_mode": mode, "first_start": first_start, "z": z, "n_literals": nlit, "decoded": decoded,
            "control": parts[0], "data": parts[1], "literals": parts[2]}

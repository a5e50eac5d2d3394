"""Host restatement of the keyed shuffle ("Factor-length histograms and the keyed shuffle"): the
permutation pi of one record and the shuffled bytes, byte for byte what the device computes.  Test infrastructure."""
import numpy as np

_M1, _M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
_GOLDEN = 0x9E3779B97F4A7C15
_MASK64 = (1 << 64) - 1


def mix64(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint64, copy=True)
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(30)
        x *= _M1
        x ^= x >> np.uint64(27)
        x *= _M2
        x ^= x >> np.uint64(31)
    return x


def permutation(length: int, seed: int, record: int = 0) -> np.ndarray:
    """pi as an array: out[i] = in[pi[i]]"""
    if length == 0:
        return np.zeros(0, np.int64)
    key = int(mix64(np.array([(seed + _GOLDEN * (record + 1)) & _MASK64], np.uint64))[0])
    k = 1
    while (1 << (2 * k)) < length:
        k += 1
    mask = np.uint64((1 << k) - 1)
    keyv = np.uint64(key)

    def E(x):
        hi, lo = x >> np.uint64(k), x & mask
        for r in range(4):
            t = hi ^ (mix64(keyv ^ ((np.uint64(r + 1) << np.uint64(32)) | lo)) & mask)
            hi, lo = lo, t
        return (hi << np.uint64(k)) | lo

    x = E(np.arange(length, dtype=np.uint64))
    todo = np.nonzero(x >= np.uint64(length))[0]
    while len(todo):
        x[todo] = E(x[todo])
        todo = todo[x[todo] >= np.uint64(length)]
    return x.astype(np.int64)


def shuffle_bytes(data: bytes, seed: int, record: int = 0) -> bytes:
    a = np.frombuffer(bytes(data), np.uint8)
    return a[permutation(len(a), seed, record)].tobytes()


def shuffle_records(records, seed: int):
    """every record shuffled on its own, keyed by its index among the records (empty records are skipped, as the
    prepare functions skip them)"""
    out, r = [], 0
    for rec in records:
        if rec:
            out.append(shuffle_bytes(rec, seed, r))
            r += 1
    return out

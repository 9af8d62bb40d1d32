"""The weight and key corpus the model-text tests share (tests/test_modeltext.py on the
CPU, tests/test_modeltext_gpu.py on the device)."""
import numpy as np

SEED = 20241019
KEYS = [0, 9, 10, 1 << 32, (1 << 63) - 1, 1 << 63, (1 << 64) - 1]
OK, BAD, DEFER, SKIP = 0, 1, 2, 3
LO, HI = 1e-22, 1e9  # the formatter's exact domain: LO <= |w| < HI, normal f32


def weights(n_random: int = 1_000_000) -> np.ndarray:
    """float32: ``n_random`` random bit patterns, every binade with its smallest and largest
    mantissa, the two round-half-even ties, +- powers of ten from 1e-22 to 1e9, the values
    on each side of the 1e-4 and 1e9 notation switches, f32(999999999), out-of-domain
    values."""
    rng = np.random.default_rng(SEED)
    parts = [rng.integers(0, 1 << 32, n_random, dtype=np.uint64).astype(np.uint32)]
    be = np.arange(0, 256, dtype=np.uint32) << 23
    for frac in (0, 1, 0x7fffff):
        for sign in (0, 0x80000000):
            parts.append(be | np.uint32(frac) | np.uint32(sign))
    hand = [1000000.125, 1000000.375, 999999999.0, 0.5, 1.0, 0.1, 123456789.0, 3e9, 1e-30,
            float("inf"), 1e-40, 1.4e-45]
    hand += [10.0 ** e for e in range(-22, 10)]
    h32 = np.array(hand, dtype=np.float32)
    for pivot in (1e-4, 1e9, 1e-22, 1e-5, 1e8):
        p = np.float32(pivot)
        h32 = np.concatenate([h32, [np.nextafter(p, np.float32(0)), p,
                                    np.nextafter(p, np.float32(np.inf))]]).astype(np.float32)
    parts.append(np.concatenate([h32, -h32]).view(np.uint32))
    return np.concatenate(parts).view(np.float32)


def in_domain(w: np.ndarray) -> np.ndarray:
    with np.errstate(invalid="ignore"):  # (signalling NaN patterns among the random bits)
        a = np.abs(w.astype(np.float64))
    normal = (w.view(np.uint32) & np.uint32(0x7f800000)) != 0
    return np.isfinite(w) & normal & (a >= LO) & (a < HI)


def keys_for(n: int) -> np.ndarray:
    """uint64: the boundary keys in rotation among random keys of every length."""
    rng = np.random.default_rng(SEED + 1)
    k = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + \
        rng.integers(0, 2, n, dtype=np.uint64)
    k >>= rng.integers(0, 64, n, dtype=np.uint64)
    k[::3] = np.array(KEYS, dtype=np.uint64)[np.arange(len(k[::3])) % len(KEYS)]
    return k


def python_lines(k: np.ndarray, w: np.ndarray) -> list[bytes]:
    """The line ``utils/checkpoint.write_text_model`` writes per entry."""
    return [f"{int(kk)}\t{float(np.float32(vv)):.9g}\n".encode() for kk, vv in zip(k, w)]

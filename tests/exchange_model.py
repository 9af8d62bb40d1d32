"""Host model of the fixed-capacity exchange rows, shared by test_exchange_model.py,
test_exchange_rows_gpu.py and test_kvapi_rows_gpu.py. Written from the row description at
the top of csrc/hip/exchange.hip and csrc/hip/kvapi.hip, in numpy on the CPU; it calls
nothing of the package.

A buffer is G rows of H 32-bit words (numpy uint32 [G, H]):
  [0] nkeys  [1] ngrads  [2..3] FixingFloat min / max (order-preserving ints), else padding
  [4, 4 + C*kw)      keys: u32 (kw = 1) or u64 (kw = 2, little endian word pairs)
  [4 + C*kw, ..)     C f32 gradients | C nb-byte FixingFloat codes | C*k f32 values (kvapi)
The unique keys of a step are owner-ordered, off[G + 1] are the owner run offsets and entry i
of run p is unique-key position off[p] + i; entries at i >= C are dropped. Every packer
takes the buffer to write into (``send``), so a buffer prefilled with ``SENTINEL`` shows
what a kernel must leave alone."""
import numpy as np

SENTINEL = 0x5A5A5A5A
FF_INIT_LO, FF_INIT_HI = np.float32(3.4e38), np.float32(-3.4e38)  # identities of min / max


def row_words(C, kw, nb=0, k=None, merged=False):
    """H, the words of one row. k = None: a trainer row (C gradients, or C codes of nb
    bytes; merged: + C weights). k >= 1: a k-value push row of the KVWorker API (kw = 0:
    key-less); k = 0: its pull rows (keys only, one word of slack)."""
    if k is None:
        w0 = 4 + C * kw + ((C * nb + 3) // 4 if nb else C)
        return (w0 + (C if merged else 0) + 3) // 4 * 4
    if k == 0:
        return (4 + C * kw + 1 + 3) // 4 * 4
    return (4 + C * kw + C * k + 3) // 4 * 4


def new_rows(G, H):
    return np.full((G, H), SENTINEL, dtype=np.uint32)


def offsets(runs):
    """off[G + 1] of owner runs of the given lengths."""
    return np.concatenate([[0], np.cumsum(np.asarray(runs, dtype=np.int64))]).astype(np.int64)


def owner_of(off, j):
    """Largest p with off[p] <= j, at most G - 1 (empty runs own nothing)."""
    off = np.asarray(off, dtype=np.int64)
    p = np.searchsorted(off, np.asarray(j, dtype=np.int64), side="right") - 1
    return np.clip(p, 0, off.size - 2)


def live_counts(off, C):
    cnt = np.diff(np.asarray(off, dtype=np.int64))
    return np.minimum(cnt, C), int(np.maximum(cnt - C, 0).sum())


def _entries(off, C):
    """(j, p, i) of every kept entry: unique-key position, owner row, index in the row."""
    off = np.asarray(off, dtype=np.int64)
    j = np.arange(int(off[-1]), dtype=np.int64)
    p = owner_of(off, j)
    i = j - off[p]
    keep = i < C
    return j[keep], p[keep], i[keep]


def pack_keys(ukeys, off, C, kw, H, send=None):
    """(send, overflow count): word 0 and the key region of every row."""
    G = len(off) - 1
    send = new_rows(G, H) if send is None else send.copy()
    cnt, ovf = live_counts(off, C)
    send[:, 0] = cnt.astype(np.uint32)
    k = np.asarray(ukeys).astype(np.uint64)
    j, p, i = _entries(off, C)
    if kw == 1:
        send[p, 4 + i] = (k[j] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    else:
        send[p, 4 + 2 * i] = (k[j] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        send[p, 5 + 2 * i] = (k[j] >> np.uint64(32)).astype(np.uint32)
    return send, ovf


def pack_grads(grad, perm, off, C, kw, H, send=None):
    """send: word 1 and the f32 gradient region (grad[perm[j]] of position j)."""
    G = len(off) - 1
    send = new_rows(G, H) if send is None else send.copy()
    send[:, 1] = live_counts(off, C)[0].astype(np.uint32)
    g = np.asarray(grad, dtype=np.float32).view(np.uint32)
    j, p, i = _entries(off, C)
    u = j if perm is None else np.asarray(perm, dtype=np.int64)[j]
    send[p, 4 + C * kw + i] = g[u]
    return send


def unpack_w(recv_w, perm, off, C, wstride, n, w_local=None):
    """w_local (f32 bit patterns, uint32 [n]): position j's reply recv_w[p * wstride + i],
    0.0 for a dropped key, written at perm[j]."""
    off = np.asarray(off, dtype=np.int64)
    out = np.full(n, SENTINEL, dtype=np.uint32) if w_local is None else w_local.copy()
    rw = np.asarray(recv_w, dtype=np.float32).view(np.uint32)
    j = np.arange(int(off[-1]), dtype=np.int64)
    p = owner_of(off, j)
    i = j - off[p]
    v = np.where(i < C, rw[np.minimum(p * wstride + i, rw.size - 1)], np.uint32(0))
    u = j if perm is None else np.asarray(perm, dtype=np.int64)[j]
    out[u] = v
    return out


# ------------------------------------------------------------------------- FixingFloat
def ff_ord(f):
    """Order-preserving int32 of a float32: b >= 0 ? b : b ^ 0x7fffffff."""
    b = np.asarray(f, dtype=np.float32).view(np.int32)
    return np.where(b >= 0, b, b ^ np.int32(0x7FFFFFFF)).astype(np.int32)


def ff_unord(b):
    b = np.asarray(b, dtype=np.int32)
    return np.where(b >= 0, b, b ^ np.int32(0x7FFFFFFF)).astype(np.int32).view(np.float32)


def ff_ratio(nb):
    return float((1 << (8 * nb)) - 2)


def ff_minmax(g_row):
    """(min, max) float32 over the non-NaN entries in ff_ord order (so -0.0 < +0.0); the
    init identities for a row without any."""
    g = np.asarray(g_row, dtype=np.float32)
    g = g[~np.isnan(g)]
    if g.size == 0:
        return FF_INIT_LO, FF_INIT_HI
    o = ff_ord(g)
    return ff_unord(o.min())[()], ff_unord(o.max())[()]


def ff_range(mn, mx):
    """(lo, hi) the codes span: hi = float32(max) + float32(1e-6), added in float32."""
    return np.float32(mn), np.float32(np.float32(mx) + np.float32(1e-6))


def ff_targets(g_row, nb, lo=None, hi=None):
    """(lo, hi, t): t float64, the real-valued code of every entry (NaN for a NaN entry);
    0 where hi - lo <= 0. A code is floor(t) or floor(t) + 1."""
    g = np.asarray(g_row, dtype=np.float32)
    if lo is None:
        lo, hi = ff_range(*ff_minmax(g))
    lo, hi = np.float32(lo), np.float32(hi)
    b = float(hi) - float(lo)
    if not b > 0:
        return lo, hi, np.where(np.isnan(g), np.nan, 0.0)
    v = np.clip(g.astype(np.float64), float(lo), float(hi))
    return lo, hi, (v - float(lo)) / b * ff_ratio(nb)


def ff_decode(r, lo, hi, nb):
    """float32(double(r) / ratio * bin + lo), bin = double(hi) - double(lo)."""
    b = float(np.float32(hi)) - float(np.float32(lo))
    return (np.asarray(r, dtype=np.float64) / ff_ratio(nb) * b + float(np.float32(lo))).astype(
        np.float32)


def ff_codes(code_bytes, n, nb):
    """The first n little-endian nb-byte codes of a byte array, as int64."""
    c = np.asarray(code_bytes, dtype=np.uint8)[: n * nb].reshape(n, nb).astype(np.int64)
    return sum(c[:, b] << (8 * b) for b in range(nb)) if n else np.zeros(0, dtype=np.int64)


def ulp32(x):
    """Spacing of float32 at |x| (the 1-ulp tolerance of a float32 result)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def ff_round_stats(r, t):
    """Of stochastic rounding draws r of targets t: (sum of round-ups, its expectation
    sum(p), its standard deviation sqrt(sum p (1 - p))), p = frac(t)."""
    t = np.asarray(t, dtype=np.float64)
    f = np.floor(t)
    p = t - f
    return float((np.asarray(r, dtype=np.float64) - f).sum()), float(p.sum()), \
        float(np.sqrt((p * (1 - p)).sum()))


def ff_expected_differing(t):
    """Expected fraction of entries whose codes differ between two independent draws:
    mean(2 p (1 - p))."""
    t = np.asarray(t, dtype=np.float64)
    p = t - np.floor(t)
    return float((2 * p * (1 - p)).mean())


# ------------------------------------------------------------------ k-value rows (kvapi)
def kvv_pack_vals(vals, k, pos_s, seg_start, off, C, kw, H, send=None):
    """(send, sum32 [U, k], sum64 [U, k]): per unique key u the sum of vals[pos, :] over its
    positions pos_s[seg_start[u] : seg_start[u + 1]] in that (ascending) order, accumulated
    sequentially in float32 from 0.0, and the same sum in float64. Row p entry i carries
    sum32 of u = off[p] + i at word 4 + C*kw + i*k; word 1 (kw = 0: word 0 too) the count."""
    G = len(off) - 1
    send = new_rows(G, H) if send is None else send.copy()
    vals = np.asarray(vals, dtype=np.float32).reshape(-1, k)
    U = int(off[-1])
    s32 = np.zeros((U, k), dtype=np.float32)
    s64 = np.zeros((U, k), dtype=np.float64)
    for u in range(U):
        for r in range(int(seg_start[u]), int(seg_start[u + 1])):
            row = vals[int(pos_s[r])]
            s32[u] = s32[u] + row  # float32 + float32, one rounding per addend
            s64[u] += row.astype(np.float64)
    cnt = live_counts(off, C)[0].astype(np.uint32)
    send[:, 1] = cnt
    if kw == 0:
        send[:, 0] = cnt
    j, p, i = _entries(off, C)
    bits = s32.view(np.uint32)
    for c in range(k):
        send[p, 4 + C * kw + i * k + c] = bits[j, c]
    return send, s32, s64

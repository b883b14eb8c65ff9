"""numpy restatement of geot_sample_draw's contract (include/geot_hip.h), written from the contract alone: nothing of
geot_amd is imported.  Vectorised over elements and draws; every value is held in uint64 and kept below 2^32 where the
contract says "32-bit word", so a 32 x 32 -> 64 bit product never overflows.

    philox4x32(counter words, key words)         Philox4x32-10, four output words
    feistel(x, d, b, seed)                       the keyed bijection pi_d on [0, 2^b)
    draw_rows(n, m, seed, draws)                 (len(draws), m) int64: one row per draw id, all on a scan of n vertices
    sample_draw_ref(sizes, m, seed, draw_base)   (sel (S, m) int64, bad (S,) int32): slot i has size sizes[i] (0: unusable)
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
LOW = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
CHUNK = 1 << 15          # elements per pass: the temporaries of one pass stay in cache


def _u64(v):
    return np.asarray(v, dtype=np.uint64)


def philox4x32(c0, c1, c2, c3, k0, k1):
    """Ten rounds; the key is bumped by the Weyl constants between rounds (nine times).  Arguments broadcast."""
    c0, c1, c2, c3 = np.broadcast_arrays(_u64(c0), _u64(c1), _u64(c2), _u64(c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for rnd in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ np.uint64(k0), p1 & LOW, (p0 >> S32) ^ c3 ^ np.uint64(k1), p0 & LOW
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def _words(v):
    v = _u64(v)
    return v & LOW, v >> S32


def width(n):
    return max(10, int(n - 1).bit_length())


def feistel(x, d, b, seed):
    """pi_d(x) on [0, 2^b): eight alternating unbalanced Feistel rounds, lb = b // 2 high bits L, rb = b - lb low bits R."""
    lb = b // 2
    rb = b - lb
    mask_l, mask_r = np.uint64((1 << lb) - 1), np.uint64((1 << rb) - 1)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    d_lo, d_hi = _words(d)
    x = _u64(x)
    left, right = x >> np.uint64(rb), x & mask_r
    for r in range(8):
        if r % 2 == 0:
            left = left ^ (philox4x32(right, r, d_lo, d_hi, k0, k1)[0] & mask_l)
        else:
            right = right ^ (philox4x32(left, r, d_lo, d_hi, k0, k1)[0] & mask_r)
    return (left << np.uint64(rb)) | right


def _tabled_feistel(draws, b, seed):
    """feistel() for the rows of `draws`, with the round function looked up: F(v, r) of every half value v (2^rb of them),
    round and draw is computed once.  The same values as feistel(); it pays where a draw calls F more often than that --
    the small scans, which walk 2^b / n times per element."""
    lb = b // 2
    rb = b - lb
    mask_l, mask_r = np.uint64((1 << lb) - 1), np.uint64((1 << rb) - 1)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    d_lo, d_hi = _words(_u64(draws)[:, None])
    v = np.arange(1 << rb, dtype=np.uint64)[None, :]
    tables = [philox4x32(v, r, d_lo, d_hi, k0, k1)[0] for r in range(8)]

    def permute(x, row):
        left, right = x >> np.uint64(rb), x & mask_r
        for r in range(8):
            if r % 2 == 0:
                left = left ^ (tables[r][row, right.astype(np.intp)] & mask_l)
            else:
                right = right ^ (tables[r][row, left.astype(np.intp)] & mask_r)
        return (left << np.uint64(rb)) | right
    return permute


def _without_replacement(n, m, seed, draws, tabled=None):
    b = width(n)
    rb = b - b // 2
    if tabled is None:
        tabled = m * (1 << b) > n * (1 << rb)          # calls of F per round and draw, expected, against half values
    out = np.empty((len(draws), m), dtype=np.uint64)
    rows_per_pass = max(1, CHUNK // max(m, (1 << rb) if tabled else 1))
    for lo in range(0, len(draws), rows_per_pass):
        ds = draws[lo:lo + rows_per_pass]
        if tabled:
            permute = _tabled_feistel(ds, b, seed)
        else:
            def permute(x, row, ds=ds):
                return feistel(x, ds[row], b, seed)
        row, col = np.repeat(np.arange(len(ds)), m), np.tile(np.arange(m), len(ds))
        x = col.astype(np.uint64)
        while row.size:                 # cycle walking: apply pi_d until the value is back in [0, n)
            x = permute(x, row)
            done = x < np.uint64(n)
            out[lo + row[done], col[done]] = x[done]
            row, col, x = row[~done], col[~done], x[~done]
    return out.astype(np.int64)


def _with_replacement(n, m, seed, draws):
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    d_lo, d_hi = _words(_u64(draws)[:, None])
    j = np.arange(m, dtype=np.uint64)[None, :]
    w0, w1, _, _ = philox4x32(j, 0xFFFFFFFF, d_lo, d_hi, k0, k1)
    # mulhi64(w0 | w1 << 32, n) with n < 2^31: (w1 n + (w0 n >> 32)) >> 32, every term below 2^64
    nn = np.uint64(n)
    return ((w1 * nn + ((w0 * nn) >> S32)) >> S32).astype(np.int64)


def draw_rows(n, m, seed, draws):
    n, m = int(n), int(m)
    assert 1 <= n < 2 ** 31 and m >= 1
    draws = _u64(draws).reshape(-1)
    return _without_replacement(n, m, seed, draws) if n >= m else _with_replacement(n, m, seed, draws)


def sample_draw_ref(sizes, m, seed, draw_base):
    """Slot i draws with id (draw_base + i) mod 2^64 on a scan of sizes[i] vertices; sizes[i] == 0 marks an unusable slot
    (a row of zeros, bad = 2)."""
    sizes = [int(n) for n in sizes]
    sel = np.zeros((len(sizes), int(m)), dtype=np.int64)
    bad = np.zeros(len(sizes), dtype=np.int32)
    ids = [(int(draw_base) + i) & 0xFFFFFFFFFFFFFFFF for i in range(len(sizes))]
    for n in sorted(set(sizes)):
        slots = [i for i, v in enumerate(sizes) if v == n]
        if n == 0:
            bad[slots] = 2
            continue
        sel[slots] = draw_rows(n, m, seed, [ids[i] for i in slots])
    return sel, bad

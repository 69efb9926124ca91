"""CPU restatement of the stratified resampler (include/cusmc_hip.h), bit for bit.

Rules:
  1. w_max = largest non-NaN entry; degenerate (none, w_max <= 0, w_max = +inf) -> a[i] = i.
  2. L = ceil(log2 N), k = 63 - L; r_j = w_j / w_max for w_j > 0 else 0; q_j = floor(r_j 2^k) (uint64);
     C = inclusive integer prefix sum of q, S = C[N-1].
  3. U_i = ((word1 << 32 | word0) >> 11) 2^-53 of Philox4x32-10, key = seed, counter = (i, 0, step, 9);
     x_i = (i + U_i) / N;  T_i = (uint64)(x_i (double)S).
  4. a[i] = smallest j with C_j > T_i; none (x_i rounded to 1) -> the largest j with q_j > 0.
  5. log-weights: lw_max as above (degenerate: none, -inf, +inf), r_j = exp_nonpos(lw_j - lw_max) (the oracle's
     function, which the kernels evaluate with the same operations), NaN and -inf entries q = 0.
"""
import ctypes as C

import numpy as np

PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
DOMAIN = 9


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised Philox4x32-10 (Salmon et al., SC'11): uint32 arrays (broadcast) -> four uint32 words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint32) for c in (c0, c1, c2, c3))
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0 = np.asarray(k0, dtype=np.uint32).copy()
    k1 = np.asarray(k1, dtype=np.uint32).copy()
    with np.errstate(over="ignore"):
        for _ in range(10):
            p0 = PHILOX_M0 * c0.astype(np.uint64)
            p1 = PHILOX_M1 * c2.astype(np.uint64)
            n0 = (p1 >> np.uint64(32)).astype(np.uint32) ^ c1 ^ k0
            n2 = (p0 >> np.uint64(32)).astype(np.uint32) ^ c3 ^ k1
            c1 = p1.astype(np.uint32)
            c3 = p0.astype(np.uint32)
            c0, c2 = n0, n2
            k0 = k0 + PHILOX_W0
            k1 = k1 + PHILOX_W1
    return c0, c1, c2, c3


def uniforms(i, seed, step):
    """U_i of rule 3 for the global output indices i (uint64 array)."""
    i = np.asarray(i, dtype=np.uint64)
    seed = int(seed)
    w0, w1, _, _ = philox4x32_10(i.astype(np.uint32), 0, np.uint32(step), DOMAIN,
                                 np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32))
    v = (w1.astype(np.uint64) << np.uint64(32)) | w0.astype(np.uint64)
    return (v >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


_exp_nonpos = None


def exp_nonpos(t):
    """The oracle's exp_nonpos, element by element (fdlibm-style, fixed operation sequence)."""
    global _exp_nonpos
    if _exp_nonpos is None:
        from oracle import oracle as O
        f = O.lib().oracle_exp_nonpos
        f.restype = C.c_double
        f.argtypes = [C.c_double]
        _exp_nonpos = f
    t = np.asarray(t, dtype=np.float64)
    return np.fromiter((_exp_nonpos(float(x)) for x in t.ravel()), dtype=np.float64, count=t.size).reshape(t.shape)


def quantised(w, log=False):
    """(q, degenerate) of rules 1, 2 and 5."""
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    N = w.shape[0]
    ok = ~np.isnan(w)
    if not ok.any():
        return np.zeros(N, dtype=np.uint64), True
    m = w[ok].max()
    degenerate = not np.isfinite(m) if log else not (m > 0 and m < np.inf)
    if degenerate:
        return np.zeros(N, dtype=np.uint64), True
    k = 63 - (N - 1).bit_length()
    with np.errstate(invalid="ignore", divide="ignore"):
        if log:
            r = np.zeros(N)
            r[ok] = exp_nonpos(w[ok] - m)
        else:
            r = np.where(w > 0, w / m, 0.0)
    return np.floor(np.ldexp(r, k)).astype(np.uint64), False


def stratified(w, seed, step=1, log=False, first=0, count=None):
    """Ancestors (uint32) of outputs [first, first + count) (default: all N)."""
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    N = w.shape[0]
    count = N - first if count is None else count
    i = np.arange(first, first + count, dtype=np.uint64)
    q, degenerate = quantised(w, log)
    if degenerate:
        return i.astype(np.uint32)
    Cs = np.cumsum(q, dtype=np.uint64)
    S = Cs[-1]
    x = (i.astype(np.float64) + uniforms(i, seed, step)) / np.float64(N)
    T = (x * np.float64(S)).astype(np.uint64)
    T = np.minimum(T, S - np.uint64(1))  # rule 4's fallback: the first j with C_j = S
    return np.searchsorted(Cs, T, side="right").astype(np.uint32)

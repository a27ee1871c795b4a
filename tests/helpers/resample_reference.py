"""The mixed-rate resampler's arithmetic in numpy (include/same_resample.h): the design of the taps in float64,
the f32 form the device reproduces bit for bit, and a float64 form (unrounded taps, float64 sums) that makes test sources and
measures the f32 form's error.  It reads no library of the project: it is the independent restatement the tests compare with.

    g = gcd(r_in, r_out), L = r_out / g, M = r_in / g;  L == M == 1: one tap 1.0, the stream passes through
    T = 2 ceil(8 max(1, M / L)) taps per phase; prototype of n = T L points
        w = 2 * 0.45 * min(r_in, r_out) / (L r_in),  ctr = (n - 1) / 2
        h[i] = L w sinc(w (i - ctr)) I0(8.6 sqrt(1 - ((i - ctr) / (n / 2))^2)) / I0(8.6)
    taps[p][j] = h[p + j L];  output n:  k = floor(n M / L), p = (n M) mod L,
        acc = 0;  for j = 0 .. T-1:  acc = acc + taps[p][j] * x[k - j]        (x[i] = 0 for i < 0)
    after N source samples ceil(N L / M) outputs exist.
"""
import math

import numpy as np

MAX_L, MAX_T = 1024, 96


def plan(r_in: int, r_out: int):
    """(L, M, T); ValueError where the resampler refuses the ratio (SAME_ERATE)."""
    g = math.gcd(r_in, r_out)
    L, M = r_out // g, r_in // g
    if L == 1 and M == 1:
        return 1, 1, 1
    T = 2 * (-(-8 * M // L) if M > L else 8)
    if L > MAX_L or T > MAX_T:
        raise ValueError(f"{r_in} -> {r_out}: L = {L}, T = {T}")
    return L, M, T


def bessel_i0(x: np.ndarray) -> np.ndarray:
    """sum_k ((x/2)^k / k!)^2 in float64"""
    x = np.asarray(x, dtype=np.float64)
    q = x * x / 4.0
    term = np.ones_like(q)
    total = np.ones_like(q)
    for k in range(1, 500):
        term = term * (q / (float(k) * float(k)))
        total = total + term
        if np.all(term < total * 1e-17):
            break
    return total


def taps64(r_in: int, r_out: int) -> np.ndarray:
    """The taps in float64, [L, T]."""
    L, M, T = plan(r_in, r_out)
    if T == 1:
        return np.ones((1, 1))
    n = T * L
    w = 2.0 * 0.45 * min(r_in, r_out) / (L * r_in)
    t = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
    h = L * w * np.sinc(w * t) * bessel_i0(8.6 * np.sqrt(1.0 - (t / (n / 2.0)) ** 2)) / bessel_i0(8.6)
    return np.ascontiguousarray(h.reshape(T, L).T)             # [p][j] = h[p + j L]


def taps32(r_in: int, r_out: int) -> np.ndarray:
    return taps64(r_in, r_out).astype(np.float32)


def outputs_after(n_in: int, L: int, M: int) -> int:
    return -(-n_in * L // M)


def delay(r_in: int, r_out: int) -> float:
    """Output samples by which the output stream lags the source."""
    L, M, T = plan(r_in, r_out)
    return (T * L - 1) / (2.0 * M)


def _run(x, r_in, r_out, start_in, h, dtype):
    L, M, T = plan(r_in, r_out)
    x = np.asarray(x)
    n0, n1 = outputs_after(start_in, L, M), outputs_after(start_in + len(x), L, M)
    if T == 1:
        return x.astype(dtype)
    n = np.arange(n0, n1, dtype=np.int64)
    k = n * M // L - start_in                                   # the newest sample each output reads, as an index of x
    p = n * M % L
    xp = np.concatenate([np.zeros(T - 1, dtype), x.astype(dtype)])      # xp[i + T - 1] = x[i]; zeros before the stream
    acc = np.zeros(len(n), dtype)
    for j in range(T):
        acc = acc + h[p, j] * xp[k - j + (T - 1)]
    return acc


def resample_f32(x, r_in: int, r_out: int, start_in: int = 0) -> np.ndarray:
    """The f32 form: x (int16 or float32) is the stream from source position start_in on, with silence before it; the result
    is every output that exists after it, ceil((start_in + len) L / M) - ceil(start_in L / M) of them, as float32.  One f32
    multiply and one f32 add per tap, in tap order."""
    x = np.asarray(x)
    assert x.dtype in (np.int16, np.float32), x.dtype
    out = _run(x, r_in, r_out, start_in, taps32(r_in, r_out), np.float32)
    assert out.dtype == np.float32
    return out


def resample_f64(x, r_in: int, r_out: int) -> np.ndarray:
    """The same sums with unrounded taps in float64."""
    return _run(np.asarray(x, dtype=np.float64), r_in, r_out, 0, taps64(r_in, r_out), np.float64)

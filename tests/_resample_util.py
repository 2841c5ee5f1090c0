"""float64 numpy restatement of the sample-rate converter of include/fsnp_resample.h, shared by tests/test_host_resample.py and
tests/test_gpu_resample.py.  Written from the header's formula, not from the C++:

    g = gcd(from, to), up = to / g, down = from / g, M = max(up, down), Z = 32, rho = 0.91, beta = 8.6, half = Z M
    h[i] = (rho / M) sinc(rho i / M) I0(beta sqrt(1 - (i / half)^2)) / I0(beta),   |i| <= half
    n_out = ceil(n up / down)
    y[m] = sum over 0 <= k < n with |m down - k up| <= half of t[m down - k up] x[k],   t = up h

The oracle also returns, per output sample, S = sum |t x| and the number of terms K: a K-term fmaf chain in fp32 that starts from 0
differs from the exact sum by at most (K + 1) 2^-24 S to first order (Higham, Accuracy and Stability, 3.1 - each partial sum is rounded
once, gamma_K <= (K + 1) u for K u << 1), which is the bound the GPU tests assert."""
import math

import numpy as np

Z, RHO, BETA = 32, 0.91, 8.6
PAIRS = [(48000, 16000), (16000, 48000), (44100, 16000), (16000, 44100), (16000, 8000), (22050, 16000)]     # the six pairs of the feature's specification
TERMS = {(48000, 16000): 193, (16000, 48000): 65, (44100, 16000): 177, (16000, 44100): 65, (16000, 8000): 129, (22050, 16000): 89}


def plan(from_rate, to_rate):
    g = math.gcd(from_rate, to_rate)
    up, down = to_rate // g, from_rate // g
    return up, down, Z * max(up, down)


def out_length(n, from_rate, to_rate):
    up, down, _ = plan(from_rate, to_rate)
    return -(-n * up // down)


def taps64(from_rate, to_rate):
    """h[i + half] for |i| <= half, float64 (NOT multiplied by up)."""
    up, down, half = plan(from_rate, to_rate)
    M = max(up, down)
    i = np.arange(-half, half + 1, dtype=np.float64)
    return (RHO / M) * np.sinc(RHO * i / M) * np.i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - (i / half) ** 2))) / np.i0(BETA)


def resample64(x, from_rate, to_rate, taps=None):
    """x [n] -> (y [n_out], S [n_out], K [n_out]) in float64.  taps: t[i + half] = up h[i] to use instead of up * taps64 (the
    library's own fp32 taps, widened)."""
    up, down, half = plan(from_rate, to_rate)
    t = up * taps64(from_rate, to_rate) if taps is None else np.asarray(taps, dtype=np.float64)
    assert t.shape == (2 * half + 1,)
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    n_out = -(-n * up // down)
    y, S, K = np.zeros(n_out), np.zeros(n_out), np.zeros(n_out, dtype=np.int64)
    for m in range(n_out):
        c = m * down
        k0 = max(0, -((half - c) // up))          # ceil((c - half) / up)
        k1 = min(n - 1, (c + half) // up)
        if k1 < k0:
            continue
        k = np.arange(k0, k1 + 1)
        prod = t[c - k * up + half] * x[k]
        y[m], S[m], K[m] = prod.sum(), np.abs(prod).sum(), k.size
    return y, S, K


def fma_chain_bound(S, K):
    """the forward error bound of a K-term fp32 fmaf chain from 0.0f: (K + 1) 2^-24 S, plus 1e-37 for the subnormal range"""
    return (K + 1) * 2.0 ** -24 * S + 1e-37

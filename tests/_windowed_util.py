"""Float restatement of include/ext/fsnp_windowed.h, independent of the library: the window plan, the fade and the merge, and the
oracle of a windowed call (oracle.fsnp_torch.enhance_wave per window, merged in float64).  Shared by tests/test_host_windowed.py and
tests/test_gpu_windowed.py."""
import numpy as np
import torch


def window_plan(L, W, V):
    """-> [(start, length)] of the windows of a clip of L samples: stride S = W - V, one window if L <= W, else ceil((L - V) / S);
    window k covers [k S, min(k S + W, L))."""
    S = W - V
    K = 1 if L <= W else -(-(L - V) // S)
    return [(k * S, min(k * S + W, L) - k * S) for k in range(K)]


def fade(V):
    """g[j] = 0.5 - 0.5 cos(pi j / V), j = 0 ... V - 1, in float64"""
    return 0.5 - 0.5 * np.cos(np.pi * np.arange(V, dtype=np.float64) / V)


def merge(rows, L, W, V, dtype=np.float64):
    """rows[k] = the enhanced samples of window k of window_plan(L, W, V) -> the clip's L samples in `dtype`: sample i belongs to window
    k = min(i // S, K - 1) at j = i - k S; for k > 0 and j < V it is prev + g[j] (cur - prev) with prev = rows[k - 1][S + j], taken as
    ONE fused multiply-add in `dtype` (float32: computed in float64 and rounded once, which is what fmaf gives)."""
    S, K = W - V, len(rows)
    g = fade(V).astype(dtype)
    out = np.empty(L, dtype=dtype)
    for k, row in enumerate(rows):
        row = np.asarray(row, dtype=dtype)
        lo = k * S
        hi = L if k == K - 1 else lo + S
        out[lo:hi] = row[:hi - lo]
        if k > 0:
            prev, cur = np.asarray(rows[k - 1], dtype=dtype)[S:S + V].astype(np.float64), row[:V].astype(np.float64)
            sub = (cur.astype(dtype) - prev.astype(dtype)).astype(np.float64)      # the subtraction rounds in `dtype`
            out[lo:lo + V] = (g.astype(np.float64) * sub + prev).astype(dtype)
    return out


@torch.no_grad()
def oracle_windowed(sd, wav, W, V, fullsubnet=False, **kw):
    """wav [L] (float32 tensor) -> float64 [L]: oracle.fsnp_torch.enhance_wave of every window as a clip of its own, merged in float64."""
    from oracle import fsnp_torch
    L = wav.shape[-1]
    rows = [fsnp_torch.enhance_wave(sd, wav[None, a:a + n], fullsubnet=fullsubnet, **kw)[0].double().numpy() for a, n in window_plan(L, W, V)]
    return merge(rows, L, W, V, np.float64)

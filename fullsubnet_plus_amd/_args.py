"""Host-side conversion of call arguments for the C ABI."""
import ctypes
import operator

import torch


RESAMPLE_Z = 32             # kResampleZ (csrc/resample.h): half = RESAMPLE_Z * max(up, down)
RESAMPLE_MAX_RATIO = 640    # kResampleMaxRatio


def _rate(rate, what):
    """A sample rate in Hz as a positive int; ValueError otherwise (16000.0 is refused too: rates are integers)."""
    try:
        if isinstance(rate, bool):
            raise TypeError
        value = operator.index(rate)
    except TypeError:
        raise ValueError(f"{what}: a sample rate must be an integer number of Hz, got {rate!r}") from None
    if not 0 < value < 2 ** 31:
        raise ValueError(f"{what}: a sample rate must be positive (and an int32), got {value}")
    return value


def resample_plan(from_rate, to_rate, what="resample_plan"):
    """-> (up, down, half) of from_rate -> to_rate as include/fsnp_resample.h defines them, in Python integers; ValueError for a rate
    that is no positive integer and for max(up, down) > 640.  Touches neither the library nor a GPU."""
    import math
    f, t = _rate(from_rate, what), _rate(to_rate, what)
    g = math.gcd(f, t)
    up, down = t // g, f // g
    if max(up, down) > RESAMPLE_MAX_RATIO:
        raise ValueError(f"{what}: {f} Hz -> {t} Hz is the ratio {up} : {down}; max(up, down) is limited to {RESAMPLE_MAX_RATIO}")
    return up, down, RESAMPLE_Z * max(up, down)


def resample_length(n, from_rate, to_rate):
    """Samples that n samples at from_rate become at to_rate: ceil(n * up / down) (include/fsnp_resample.h)."""
    up, down, _ = resample_plan(from_rate, to_rate, "resample_length")
    n = operator.index(n)
    if n < 0:
        raise ValueError(f"resample_length: n = {n}")
    return -(-n * up // down)


def _host_lengths(lengths, batch, what):
    """Per-utterance lengths (a Python sequence or a CPU integer tensor) -> ctypes int32[batch].  They are read on the host and
    reach the device as kernel arguments: a CUDA tensor is refused, because reading it would synchronise."""
    if isinstance(lengths, torch.Tensor):
        if lengths.device.type != "cpu":
            raise ValueError(f"{what}: lengths must be a CPU tensor or a Python sequence, not a {lengths.device} tensor "
                             "(reading it would synchronise the device)")
        if lengths.is_floating_point() or lengths.is_complex() or lengths.dtype == torch.bool:
            raise TypeError(f"{what}: lengths must hold integers, got {lengths.dtype}")
        vals = [int(v) for v in lengths.reshape(-1).tolist()]
    else:
        vals = [operator.index(v) for v in lengths]
    if len(vals) != batch:
        raise ValueError(f"{what}: {len(vals)} lengths for a batch of {batch}")
    for b, v in enumerate(vals):
        if not -2 ** 31 <= v < 2 ** 31:
            raise ValueError(f"{what}: utterance {b}: length {v} is not an int32")
    return (ctypes.c_int32 * batch)(*vals)

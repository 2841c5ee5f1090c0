"""Host-side conversion of call arguments for the C ABI."""
import ctypes
import operator

import torch

from . import _lib


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


def window_plan_args(window, overlap, max_batch, num_freqs, what):
    """The host-checkable arguments of a windowed call (include/ext/fsnp_windowed.h) -> (window, overlap, max_batch) as ints; ValueError
    for a window or overlap that is no integer, an overlap outside [n_fft / 2, window / 2] (n_fft = 2 (num_freqs - 1)) and
    max_batch < 1.  Touches neither the library nor a GPU."""
    vals = []
    for name, v in (("window", window), ("overlap", overlap), ("max_batch", max_batch)):
        try:
            if isinstance(v, bool):
                raise TypeError
            vals.append(operator.index(v))
        except TypeError:
            raise ValueError(f"{what}: {name} must be an integer, got {v!r}") from None
    w, v, mb = vals
    half = num_freqs - 1
    if not (half <= v and 2 * v <= w and w < 2 ** 30):
        raise ValueError(f"{what}: overlap {v} outside [n_fft / 2, window / 2] = [{half}, {w // 2}] (window {w}, n_fft = {2 * half})")
    if not 1 <= mb < 2 ** 31:
        raise ValueError(f"{what}: max_batch {mb} < 1")
    return w, v, mb


def window_count(samples, window, overlap):
    """Windows that a clip of `samples` samples is cut into at `window` and `overlap` (include/ext/fsnp_windowed.h): 1 if
    samples <= window, else ceil((samples - overlap) / (window - overlap)).  Python integers, no library, no GPU; ValueError unless
    window >= 2, 1 <= overlap <= window / 2 and samples >= 1."""
    n, w, v = operator.index(samples), operator.index(window), operator.index(overlap)
    if w < 2 or v < 1 or 2 * v > w or n < 1:
        raise ValueError(f"window_count: samples = {n}, window = {w}, overlap = {v}: need window >= 2, 1 <= overlap <= window / 2, samples >= 1")
    return 1 if n <= w else -(-(n - v) // (w - v))


def window_stream_plan(pushed, count, window, overlap):
    """-> (first, num): a push of `count` samples on a window-session slot that held `pushed` completes windows first ... first + num - 1
    (window k is complete at k (window - overlap) + window samples; include/session/fsnp_window_stream.h).  The library's own host
    arithmetic (fsnp_window_stream_plan), no GPU; ValueError for what it answers with -1: window < 2, overlap outside
    [1, window / 2], pushed < 0, count < 0."""
    p, c, w, v = (operator.index(x) for x in (pushed, count, window, overlap))
    first, num = ctypes.c_int64(), ctypes.c_int64()
    fits = max(abs(p), abs(c)) < 2 ** 62 and max(abs(w), abs(v)) < 2 ** 31
    if not fits or _lib.load().fsnp_window_stream_plan(p, c, w, v, ctypes.byref(first), ctypes.byref(num)) != 0:
        raise ValueError(f"window_stream_plan: pushed = {p}, count = {c}, window = {w}, overlap = {v}: need window >= 2, "
                         "1 <= overlap <= window / 2, pushed >= 0, count >= 0")
    return int(first.value), int(num.value)


def window_stream_args(slots, window, overlap, max_samples, max_batch, num_freqs, what):
    """The host-checkable arguments of open_window_stream -> ints: window_plan_args' checks, and slots, max_samples >= 1."""
    window, overlap, max_batch = window_plan_args(window, overlap, max_batch, num_freqs, what)
    vals = []
    for name, v in (("slots", slots), ("max_samples", max_samples)):
        try:
            if isinstance(v, bool):
                raise TypeError
            vals.append(operator.index(v))
        except TypeError:
            raise ValueError(f"{what}: {name} must be an integer, got {v!r}") from None
        if vals[-1] < 1:
            raise ValueError(f"{what}: {name} {vals[-1]} < 1")
        if vals[-1] >= 2 ** 31:
            raise ValueError(f"{what}: {name} {vals[-1]} is not an int32")
    return vals[0], window, overlap, vals[1], max_batch


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


def require_cuda(tensor):
    """The one refusal of a tensor that is not on a GPU: nothing here computes on the CPU."""
    if not tensor.is_cuda:
        raise RuntimeError("fullsubnet_plus_amd runs on MI355X (HIP) only; move the model and inputs to 'cuda'. "
                           "There is deliberately no CPU fallback.")


def other_rate(sample_rate, model_rate, what):
    """A call's sample_rate argument -> None (None, or the model's own rate) or the int rate, after resample_plan has accepted both
    directions (ValueError otherwise)."""
    if sample_rate is None:
        return None
    resample_plan(sample_rate, model_rate, what)
    resample_plan(model_rate, sample_rate, what)
    return None if _rate(sample_rate, what) == model_rate else int(sample_rate)


def reads_in_place(wav):
    """Whether [B, samples] goes to the PCM entry points, which read int16 and strided fp32 where they lie (include/fsnp_pcm.h); every
    other tensor goes to the fp32 entry points as it always has, as contiguous rows after .float()."""
    return wav.dtype == torch.int16 or (wav.dtype == torch.float32 and wav.shape[1] > 1 and wav.stride(1) != 1)


def f32_rows(wav):
    """[B, samples] -> fp32 with contiguous rows, what the fp32 entry points read"""
    wav = wav.float()
    return wav if wav.stride(1) == 1 else wav.contiguous()


def pcm_input(wav):
    """[B, samples] -> (tensor, FSNP_SAMPLE_* code, row stride, step) as the PCM entry points take them: int16 or fp32, copied only where
    the step between samples is below 1 (an expanded tensor)."""
    if wav.dtype not in (torch.int16, torch.float32):
        wav = wav.float()
    if wav.shape[1] > 1 and wav.stride(1) < 1:
        wav = wav.contiguous()
    return wav, _lib.SAMPLE_S16 if wav.dtype == torch.int16 else _lib.SAMPLE_F32, wav.stride(0), max(wav.stride(1), 1)


def output_format(out_format, like, what, peak=True):
    """An out_format argument -> (FSNP_SAMPLE_* code, torch dtype of the result).  None follows the dtype `like`: int16 -> "s16", anything
    else -> "f32".  peak=False: a stream session, which has no "s16_peak".  ValueError under the caller's name `what` otherwise."""
    allowed = ("f32", "s16", "s16_peak") if peak else ("f32", "s16")
    if out_format is None:
        out_format = "s16" if like == torch.int16 else "f32"
    elif out_format not in allowed:
        raise ValueError(f"{what}: out_format {out_format!r} is none of None, " + ", ".join(repr(f) for f in allowed)
                         + (" (a stream has no peak: 's16_peak' is a format of enhance_wave only)" if out_format == "s16_peak" else ""))
    code = _lib.SAMPLE_FORMATS[out_format]
    return code, torch.float32 if code == _lib.SAMPLE_F32 else torch.int16


def clipped_pointer(clipped, batch, device, what):
    """A call's `clipped` argument -> None or the device pointer of its int32 [batch]; ValueError under the caller's name `what`."""
    if clipped is None:
        return None
    if not (clipped.is_cuda and clipped.device == device and clipped.dtype == torch.int32 and clipped.shape == (batch,)
            and clipped.is_contiguous()):
        raise ValueError(f"{what}: clipped must be a contiguous torch.int32 tensor [{batch}] on {device}")
    return clipped.data_ptr()

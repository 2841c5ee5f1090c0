"""Host-side conversion of call arguments for the C ABI."""
import ctypes
import operator

import torch


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

"""The one path from a torch caller into libfsnp_hip.so: device context, the current stream as the entry point's last argument, the
return code checked under the entry point's own name.  `hip_stream` is the last parameter of every entry point that takes one
(include/*.h), so the three functions below are the whole plumbing; model.py, stream.py and _debug.py state only the arguments."""
import ctypes

import torch

from . import _lib


def resolve_device(device):
    """"cuda" -> the current device with its index (a handle is bound to one device)."""
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def enqueue(fn, device, *args, stream=True):
    """fn(*args, hip_stream) on `device`, hip_stream being its current stream -> fn's return code, unchecked: the body of the enqueue()
    closures that _policy.enqueue_retrying_stale may call twice.  stream=False: an entry point without that parameter."""
    with torch.cuda.device(device):
        if stream:
            return fn(*args, ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream))
        return fn(*args)


def call(fn, device, *args, stream=True, what=None):
    """enqueue(), and _lib.FsnpError under the entry point's name (or `what`) unless it returned 0."""
    _lib.check(enqueue(fn, device, *args, stream=stream), what or fn.__name__)


def check(fn, *args):
    """fn(*args) checked the same way, for entry points that take no stream and touch no device (setters, queries of the handle)."""
    _lib.check(fn(*args), fn.__name__)

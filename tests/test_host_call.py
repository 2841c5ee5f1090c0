"""fullsubnet_plus_amd._call with torch.cuda's device context and current stream replaced by recorders: the stream goes last, the
call happens inside the device context, and a code other than 0 raises under the entry point's own name.  No GPU, no library."""
import contextlib
import ctypes

import pytest
import torch

from fullsubnet_plus_amd import _call, _lib


@pytest.fixture
def cuda(monkeypatch):
    events = []

    @contextlib.contextmanager
    def device(dev):
        events.append(("enter", dev))
        yield
        events.append(("exit", dev))

    class Stream:
        cuda_stream = 0xABC0

    def current_stream(dev=None):
        events.append(("stream", dev))
        return Stream()
    monkeypatch.setattr(torch.cuda, "device", device)
    monkeypatch.setattr(torch.cuda, "current_stream", current_stream)
    monkeypatch.setattr(_lib, "last_error", lambda: "stub")
    return events


def entry(events, rc):
    def fsnp_entry(*args):
        events.append(("call", args))
        return rc
    return fsnp_entry


def test_enqueue_appends_the_current_stream_inside_the_device_context(cuda):
    assert _call.enqueue(entry(cuda, 6), "dev1", 1, None, "x") == 6            # the code comes back unchecked
    kinds = [e[0] for e in cuda]
    assert kinds == ["enter", "stream", "call", "exit"] and cuda[0][1] == cuda[1][1] == "dev1"
    args = cuda[2][1]
    assert args[:3] == (1, None, "x") and isinstance(args[3], ctypes.c_void_p) and args[3].value == 0xABC0 and len(args) == 4


def test_enqueue_without_a_stream(cuda):
    assert _call.enqueue(entry(cuda, 0), "dev1", 1, 2, stream=False) == 0
    assert cuda == [("enter", "dev1"), ("call", (1, 2)), ("exit", "dev1")]


def test_call_checks_under_the_entry_points_name(cuda):
    assert _call.call(entry(cuda, 0), "dev0", 5) is None
    with pytest.raises(_lib.FsnpError, match=r"fsnp_entry failed \(code 3\): stub") as e:
        _call.call(entry(cuda, 3), "dev0", 5)
    assert e.value.code == 3
    with pytest.raises(_lib.FsnpError, match=r"fsnp_set_weight\(a\.b\) failed \(code 2\)"):
        _call.call(entry(cuda, 2), "dev0", 5, what="fsnp_set_weight(a.b)")
    assert cuda[-1] == ("exit", "dev0")                                         # the context is left before the error is raised


def test_check_touches_neither_device_nor_stream(cuda):
    assert _call.check(entry(cuda, 0), 7, 8) is None
    assert cuda == [("call", (7, 8))]
    with pytest.raises(_lib.FsnpError, match=r"fsnp_entry failed \(code 1\)"):
        _call.check(entry(cuda, 1), 7)


def test_bound_entry_points_carry_their_names():
    """what _call reads the name from: ctypes names a library's function pointers after their symbols"""
    lib = _lib.load()
    assert lib.fsnp_forward.__name__ == "fsnp_forward" and lib.fsnp_wave_rate_stream_push_pcm.__name__ == "fsnp_wave_rate_stream_push_pcm"

"""Host-side checks of the live-session surface (include/fsnp_stream_live.h, the `live` keyword of open_stream / open_wave_stream) on the
cross-compiled library.  No GPU is touched."""
import ctypes
import os
import re

import pytest

from fullsubnet_plus_amd import FullSubNet, FullSubNet_Plus, _lib
from oracle.ref_loader import DEFAULT_MODEL_ARGS, FULLSUBNET_MODEL_ARGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_live_header_declares_exactly_the_live_stream_symbols():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "fsnp_stream_live.h")).read()
    declared = set(re.findall(r"^(?:int|void|int64_t) (fsnp_[a-z0-9_]+)\s*\(", header, flags=re.M))
    assert declared == set(_lib.LIVE_STREAM_SYMBOLS) and len(declared) == 3, declared ^ set(_lib.LIVE_STREAM_SYMBOLS)
    assert declared == {"fsnp_stream_create_live", "fsnp_wave_stream_create_live", "fsnp_stream_is_live"}
    for name in declared:
        fn = getattr(lib, name)                     # present in the library, and typed by load()
        assert fn.argtypes == _lib.LIVE_STREAM_SYMBOLS[name][1], name
    for other in (_lib.SYMBOLS, _lib.LENGTHS_SYMBOLS, _lib.STREAM_SYMBOLS, _lib.WAVE_STREAM_SYMBOLS):
        assert not set(_lib.LIVE_STREAM_SYMBOLS) & set(other)
    assert lib.fsnp_abi_version() == 13 == _lib.ABI_VERSION


def test_core_header_includes_the_live_header():
    core = open(os.path.join(ROOT, "include", "fsnp.h")).read()
    assert '#include "fsnp_stream_live.h"' in core


def test_null_arguments_give_code_1():
    lib = _lib.load()
    sp = ctypes.c_void_p()
    assert lib.fsnp_stream_create_live(None, 1, 1, ctypes.byref(sp)) == 1 and "null" in _lib.last_error()
    assert "fsnp_stream_create_live" in _lib.last_error()
    assert lib.fsnp_wave_stream_create_live(None, 1, 256, ctypes.byref(sp)) == 1 and "null" in _lib.last_error()
    assert "fsnp_wave_stream_create_live" in _lib.last_error()
    assert lib.fsnp_stream_is_live(None) == 0


def test_models_that_cannot_stream_say_why_before_any_gpu_is_touched():
    with pytest.raises(NotImplementedError, match="not causal"):
        FullSubNet_Plus(**DEFAULT_MODEL_ARGS).open_stream(1, live=True)
    with pytest.raises(NotImplementedError, match="not causal"):
        FullSubNet_Plus(**DEFAULT_MODEL_ARGS).open_wave_stream(1, live=True)
    with pytest.raises(NotImplementedError, match="GRU"):
        FullSubNet(**dict(FULLSUBNET_MODEL_ARGS, norm_type="cumulative_laplace_norm", sequence_model="GRU")).open_stream(1, live=True)
    with pytest.raises(NotImplementedError, match="whole clip's total"):
        FullSubNet(**dict(FULLSUBNET_MODEL_ARGS, norm_type="offline_laplace_norm")).open_stream(1, live=True)
    with pytest.raises(NotImplementedError, match="whole clip's total"):
        FullSubNet(**dict(FULLSUBNET_MODEL_ARGS, norm_type="offline_gaussian_norm")).open_wave_stream(1, max_samples=256, live=True)

"""Host-side checks of the batches-of-clips-of-different-lengths surface (include/fsnp_lengths.h), on the cross-compiled library."""
import ctypes
import os
import re

import pytest
import torch

from fullsubnet_plus_amd import _lib
from fullsubnet_plus_amd.model import _host_lengths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_version_and_lengths_symbols():
    lib = _lib.load()
    assert lib.fsnp_abi_version() == 12 == _lib.ABI_VERSION
    header = open(os.path.join(ROOT, "include", "fsnp_lengths.h")).read()
    declared = set(re.findall(r"^int (fsnp_[a-z0-9_]+)\s*\(", header, flags=re.M))
    assert declared == set(_lib.LENGTHS_SYMBOLS) == {"fsnp_forward_lengths", "fsnp_forward_complex_lengths", "fsnp_enhance_wave_lengths"}
    for name in declared:
        assert hasattr(lib, name), name
    assert '#include "fsnp_lengths.h"' in open(os.path.join(ROOT, "include", "fsnp.h")).read()


def test_null_handle_and_lengths_are_refused():
    lib = _lib.load()
    st = (ctypes.c_int64 * 3 * 3)()
    assert lib.fsnp_forward_lengths(None, None, None, None, ctypes.byref(st), None, None, 1, 1, None) == 1
    assert "null" in _lib.last_error()
    st1 = (ctypes.c_int64 * 3)()
    assert lib.fsnp_forward_complex_lengths(None, None, ctypes.byref(st1), None, None, 1, 1, None) == 1
    assert lib.fsnp_enhance_wave_lengths(None, None, 0, None, 0, None, 1, 1000, None) == 1


def test_host_lengths_conversion():
    arr = _host_lengths([3, 1, 2], 3, "f")
    assert list(arr) == [3, 1, 2] and ctypes.sizeof(arr) == 12
    assert list(_host_lengths(torch.tensor([5, 6], dtype=torch.int64), 2, "f")) == [5, 6]
    with pytest.raises(ValueError, match="2 lengths for a batch of 3"):
        _host_lengths([1, 2], 3, "f")
    with pytest.raises(TypeError):
        _host_lengths(torch.tensor([1.0, 2.0]), 2, "f")
    with pytest.raises(TypeError):
        _host_lengths([1.5, 2], 2, "f")
    with pytest.raises(ValueError, match="int32"):
        _host_lengths([2 ** 32 + 5], 1, "f")

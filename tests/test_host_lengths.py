"""Host-side checks of the batches-of-clips-of-different-lengths surface (include/fsnp_lengths.h), on the cross-compiled library."""
import ctypes
import os
import re

import pytest
import torch

from fullsubnet_plus_amd import _lib
from fullsubnet_plus_amd.model import _host_lengths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_13_version_and_lengths_symbols():
    """ABI 13 added fsnp_apply_cirm_lengths (the cIRM epilogue of enhance(X, lengths=)): the version and all four lengths symbols."""
    lib = _lib.load()
    assert lib.fsnp_abi_version() == 13 == _lib.ABI_VERSION
    header = open(os.path.join(ROOT, "include", "fsnp_lengths.h")).read()
    declared = set(re.findall(r"^int (fsnp_[a-z0-9_]+)\s*\(", header, flags=re.M))
    assert declared == set(_lib.LENGTHS_SYMBOLS) == {"fsnp_forward_lengths", "fsnp_forward_complex_lengths", "fsnp_enhance_wave_lengths",
                                                     "fsnp_apply_cirm_lengths"}
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
    st3 = (ctypes.c_int64 * 3)()
    assert lib.fsnp_apply_cirm_lengths(None, None, ctypes.byref(st3), None, ctypes.byref(st3), None, 1, 3, 4, None) == 1
    assert "null" in _lib.last_error()


@pytest.mark.parametrize("lengths,bad", [([4, 0], 1), ([5, 4], 0), ([4, 4, -1], 2)])
def test_apply_cirm_lengths_are_validated_before_any_launch(lengths, bad):
    """A length outside [1, frames] is refused on the host, naming the utterance; nothing is launched (the device pointers below
    are never dereferenced)."""
    lib = _lib.load()
    st = (ctypes.c_int64 * 3)(12, 1, 3)
    lens = (ctypes.c_int32 * len(lengths))(*lengths)
    fake = ctypes.c_void_p(0x1000)
    assert lib.fsnp_apply_cirm_lengths(fake, fake, ctypes.byref(st), fake, ctypes.byref(st), lens, len(lengths), 3, 4, None) == 2
    assert f"utterance {bad}" in _lib.last_error()


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


def test_edge_lengths_chooser():
    from tests._util import edge_lengths
    assert edge_lengths(300, 2, 8) == [8, 29, 30, 31, 61, 62, 63, 125, 126, 127, 253, 254, 255, 300]
    assert edge_lengths(24, 2, 8, edges=(8, 16, 24)) == [8, 13, 14, 15, 21, 22, 23, 24]
    assert edge_lengths(626, 2, 1, edges=(8, 256), extra=(255, 256, 257, 999)) == [1, 5, 6, 7, 253, 254, 255, 256, 257, 626]
    assert edge_lengths(9, 0, 1) == [1, 7, 8, 9]

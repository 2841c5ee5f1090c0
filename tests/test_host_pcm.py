"""CPU tests of 16-bit PCM at the boundary of the waveform path (include/fsnp_pcm.h): the numpy restatement of the sample formats
against hand-written cases, the binding of the new entry points, and every refusal that happens before a GPU is touched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from fullsubnet_plus_amd import FullSubNet, FullSubNet_Plus, _lib
from fullsubnet_plus_amd.stream import WaveStream
from oracle.ref_loader import DEFAULT_MODEL_ARGS, FULLSUBNET_MODEL_ARGS
from tests._pcm_util import crafted, peak_rows, peak_s16, quantise_rows, quantise_s16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSB = 1.0 / 32768.0


# ------------------------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("v,q,clipped", [
    (0.5 * LSB, 0, 0), (-0.5 * LSB, 0, 0), (1.5 * LSB, 2, 0), (-1.5 * LSB, -2, 0), (2.5 * LSB, 2, 0),
    (32766.5 * LSB, 32766, 0), (32767.5 * LSB, 32767, 1),
    (1.0, 32767, 1), (-1.0, -32768, 0), (-1.0 - 2.0 ** -15, -32768, 1),
    (float("inf"), 32767, 1), (float("-inf"), -32768, 1), (float("nan"), 0, 1), (2.0 ** -140, 0, 0),
    (0.3, 9830, 0), (-0.3, -9830, 0)])
def test_quantise_s16_hand_written_cases(v, q, clipped):
    got, n = quantise_s16(np.array([v], dtype=np.float32))
    assert got.dtype == np.int16 and got.shape == (1,)
    assert (int(got[0]), n) == (q, clipped)


def test_crafted_vector_is_its_own_expectation():
    v, q, clip = crafted()
    got, n = quantise_s16(v)
    assert np.array_equal(got, q) and n == int(clip.sum())
    rows, counts = quantise_rows(np.stack([v, v]), [v.size, 7])
    assert np.array_equal(rows[0], q) and np.array_equal(rows[1, :7], q[:7]) and not rows[1, 7:].any()
    assert counts.tolist() == [int(clip.sum()), int(clip[:7].sum())]


def test_peak_s16_hand_written_cases():
    # the peak is a negative sample: it maps to -trunc(26213.6) and everything else scales with it
    v = np.array([0.1, -0.5, 0.25, 0.0, 0.499], dtype=np.float32)
    got = peak_s16(v)
    assert got.dtype == np.int16
    k = np.float32(0.8 * 32767)
    want = [int(np.float32(k * x) / np.float32(0.5)) for x in v]       # int(): truncation toward zero
    assert got.tolist() == want and got[1] == -26213 and got[3] == 0
    # fp32 arithmetic, not fp64: a value whose fp64 quotient truncates differently would show here
    x = np.array([1.0, 1.0 / 3.0], dtype=np.float32)
    assert peak_s16(x).tolist() == [26213, int(np.float32(k * x[1]) / np.float32(1.0))]
    # an all-zero clip is all zeros (numpy alone would give NaN)
    assert not peak_s16(np.zeros(5, dtype=np.float32)).any()
    rows = peak_rows(np.stack([v, v]), [5, 3])
    assert np.array_equal(rows[0], got) and np.array_equal(rows[1, :3], peak_s16(v[:3])) and not rows[1, 3:].any()


# ------------------------------------------------------------------------------------------------ the binding
PCM_NAMES = {"fsnp_enhance_wave_pcm", "fsnp_stft_pcm", "fsnp_wave_stream_push_pcm", "fsnp_wave_stream_finish_pcm"}


def test_new_symbols_are_declared_bound_and_the_abi_version_stays():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "fsnp_pcm.h")).read()
    declared = set(re.findall(r"^int (fsnp_[a-z0-9_]+)\(", header, flags=re.M))
    assert declared == PCM_NAMES == set(_lib.PCM_SYMBOLS)
    for name in PCM_NAMES | {"fsnp_debug_pcm_convert"}:
        assert getattr(lib, name).argtypes is not None, name
    assert "fsnp_debug_pcm_convert" in _lib.SYMBOLS
    assert '#include "fsnp_pcm.h"' in open(os.path.join(ROOT, "include", "fsnp.h")).read()
    assert lib.fsnp_abi_version() == 13 == _lib.ABI_VERSION
    for name, value in (("F32", 0), ("S16", 1), ("S16_PEAK", 2)):
        assert re.search(rf"#define FSNP_SAMPLE_{name} {value}\b", header), name
    assert (_lib.SAMPLE_F32, _lib.SAMPLE_S16, _lib.SAMPLE_S16_PEAK) == (0, 1, 2)
    assert _lib.SAMPLE_FORMATS == {"f32": 0, "s16": 1, "s16_peak": 2}


def test_c_refusals_that_need_no_device():
    """A NULL handle, session or buffer is code 1 with a message that names the entry point (the format and step refusals come behind
    the NULL checks and need a handle: tests/test_gpu_pcm.py)."""
    lib = _lib.load()
    buf = (ctypes.c_int16 * 8)()
    p = ctypes.addressof(buf)
    assert lib.fsnp_enhance_wave_pcm(None, p, 1, 8, 1, p, 1, 8, 1, None, 1, 8, None, None) == 1
    assert b"fsnp_enhance_wave_pcm" in lib.fsnp_last_error()
    assert lib.fsnp_stft_pcm(None, p, 1, 8, 1, p, 1, 8, None) == 1
    assert b"fsnp_stft_pcm" in lib.fsnp_last_error()
    assert lib.fsnp_wave_stream_push_pcm(None, p, 1, 8, 1, None, p, 1, 8, 1, 8, None) == 1
    assert b"fsnp_wave_stream_push_pcm" in lib.fsnp_last_error()
    assert lib.fsnp_wave_stream_finish_pcm(None, None, 0, p, 1, 8, 1, None) == 1
    assert b"fsnp_wave_stream_finish_pcm" in lib.fsnp_last_error()
    assert lib.fsnp_debug_pcm_convert(None, p, p, 1, 8, None, 1, None, None) == 1
    assert b"fsnp_debug_pcm_convert" in lib.fsnp_last_error()


# ------------------------------------------------------------------------------------------------ Python refusals, no GPU touched
@pytest.mark.parametrize("cls,args", [(FullSubNet_Plus, DEFAULT_MODEL_ARGS), (FullSubNet, FULLSUBNET_MODEL_ARGS)])
def test_enhance_wave_refuses_before_a_gpu_is_touched(cls, args):
    m = cls(**args)
    x = torch.zeros(2, 1000, dtype=torch.int16)
    for bad in ("u8", "S16", "int16", 1):
        with pytest.raises(ValueError, match="out_format"):
            m.enhance_wave(x, out_format=bad)
    for fmt in (None, "f32", "s16", "s16_peak"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.enhance_wave(x, out_format=fmt)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.enhance_wave(x.float(), out_format="s16", clipped=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.stft(x)
    assert m._hip.handle is None


def test_wave_stream_refuses_a_peak_and_unknown_formats_before_a_gpu_is_touched():
    """The format is checked before the session is looked at: a WaveStream that was never opened is enough to see it."""
    ws = object.__new__(WaveStream)
    x = torch.zeros(1, 256, dtype=torch.int16)
    for bad in ("s16_peak", "u8"):
        with pytest.raises(ValueError, match="out_format"):
            ws.push(x, out_format=bad)
        with pytest.raises(ValueError, match="out_format"):
            ws.finish(out_format=bad)
    with pytest.raises(ValueError, match="no peak"):
        ws.push(x, out_format="s16_peak")
    with pytest.raises(ValueError, match="no peak"):
        ws.finish(out_format="s16_peak")

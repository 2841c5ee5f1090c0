"""Host tests of the sample-rate converter (include/fsnp_resample.h): the float64 oracle of tests/_resample_util.py against scipy and
against hand cases, the filter's conditions, the library's taps and pair arithmetic against the oracle and Python integers, the binding,
and the Python refusals that must not touch a GPU.

Bounds.  The filter conditions and the round-trip bound are conditions on the formula with margin over what it gives (passband ripple
0.0003 dB, stop band -86.3 dB, per-phase DC gain within 1.2e-5 of 1, round trip 2.3e-5 / 2.7e-5); the tap bound is one fp32 rounding
of up * h (2^-24 relative) plus as much again for two double evaluations of I0 that differ in their last bits, i.e. 2^-23 |up h| + 1e-12."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import fullsubnet_plus_amd
from fullsubnet_plus_amd import FullSubNet, FullSubNet_Plus, _lib
from oracle.ref_loader import DEFAULT_MODEL_ARGS, FULLSUBNET_MODEL_ARGS
from tests._resample_util import PAIRS, TERMS, out_length, plan, resample64, taps64

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
SCIPY_PAIRS = [(48000, 16000), (16000, 48000), (44100, 16000), (16000, 44100), (8000, 16000), (16000, 8000), (22050, 16000)]
RATES = [8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 192000]


def _noise(n, seed):
    return np.random.RandomState(seed).uniform(-1.0, 1.0, size=n)


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("pair", SCIPY_PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_oracle_is_scipy_resample_poly(pair):
    signal = pytest.importorskip("scipy.signal")
    up, down, _ = plan(*pair)
    worst = 0.0
    for n in (1, 7, 500, 1237):
        x = _noise(n, 100 + n)
        y, _, _ = resample64(x, *pair)
        want = signal.resample_poly(x, up, down, window=taps64(*pair))      # (scipy multiplies the window by up itself)
        assert y.shape == want.shape == (out_length(n, *pair),)
        worst = max(worst, float(np.abs(y - want).max()))
    print(f"{pair}: max |oracle - scipy| = {worst:.2e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_hand_cases(pair):
    up, down, half = plan(*pair)
    t = up * taps64(*pair)
    n = 400
    # an impulse at k: y[m] = t[m down - k up] wherever that index is inside the filter, 0 elsewhere
    for k in (0, 1, 199, n - 1):
        x = np.zeros(n)
        x[k] = 1.0
        y, S, K = resample64(x, *pair)
        want = np.zeros(out_length(n, *pair))
        for m in range(want.size):
            i = m * down - k * up
            if abs(i) <= half:
                want[m] = t[i + half]
        assert np.array_equal(y, want) and np.array_equal(S, np.abs(want))
    # terms per output in the middle of a long clip (the centre tap included), as the feature's specification counts them
    _, _, K = resample64(np.ones(3000), *pair)
    assert K.max() == TERMS[pair], (pair, K.max())
    # n = 1: ceil(up / down) outputs, each one tap times the sample
    y, _, K = resample64(np.array([0.5]), *pair)
    assert y.size == -(-up // down) and np.array_equal(y, 0.5 * t[half + np.arange(y.size) * down]) and (K == 1).all()


def test_length_rule():
    assert out_length(0, 48000, 16000) == 0 and out_length(1, 48000, 16000) == 1 and out_length(3, 48000, 16000) == 1
    assert out_length(4, 48000, 16000) == 2 and out_length(5, 16000, 48000) == 15
    assert out_length(441, 44100, 16000) == 160 and out_length(442, 44100, 16000) == 161 and out_length(160, 16000, 44100) == 441
    for pair in PAIRS:
        for n in (1, 2, 999, 1000, 96000):
            assert out_length(n, *pair) == math.ceil(n * pair[1] / pair[0] - 1e-9)
            assert fullsubnet_plus_amd.resample_length(n, *pair) == out_length(n, *pair)
            # what comes back covers the clip: n <= ceil(n16 down' / up') (the way out of enhance_wave cuts to n)
            assert out_length(out_length(n, *pair), pair[1], pair[0]) >= n


@pytest.mark.parametrize("pair", SCIPY_PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_filter_conditions(pair):
    up, down, half = plan(*pair)
    M = max(up, down)
    h = taps64(*pair)
    # the response on the grid of rate from * up: frequency f in cycles per sample there; the lower rate's Nyquist is 1 / (2 M)
    # (a zero-padded FFT: 32 points per tap, i.e. 64 Z = 2048 points between 0 and the lower Nyquist; |H(0)| is about 1)
    N = 1 << int(np.ceil(np.log2(32 * h.size)))
    H = np.abs(np.fft.rfft(h, N))
    f = np.arange(H.size) / N
    nyq = 0.5 / M
    pb = 20 * np.log10(H[f <= 0.8 * nyq])
    sb = 20 * np.log10(np.maximum(H[f >= nyq], 1e-300))
    gains = np.array([up * h[(p + half) % up::up].sum() for p in range(up)])
    print(f"{pair}: ripple {np.abs(pb).max():.5f} dB, stop band {sb.max():.1f} dB, phase DC gain within {np.abs(gains - 1).max():.1e}")
    assert np.abs(pb).max() <= 0.002
    assert sb.max() <= -80.0
    if up > 1:
        assert np.abs(gains - 1).max() <= 5e-5


@pytest.mark.parametrize("rate", [48000, 44100])
def test_oracle_round_trip(rate):
    n = int(0.05 * rate)
    tt = np.arange(n) / rate
    x = sum(a * np.sin(2 * np.pi * fr * tt + ph) for a, fr, ph in ((0.3, 300, 0.1), (0.25, 1000, 0.7), (0.25, 3000, 1.3), (0.2, 6400, 2.1)))
    down16, _, _ = resample64(x, rate, 16000)
    back, _, _ = resample64(down16, 16000, rate)
    assert back.size >= n
    err = float(np.abs(back[400:n - 400] - x[400:n - 400]).max())
    print(f"{rate} -> 16000 -> {rate}: max error {err:.2e}")
    assert err <= 1e-4


# ------------------------------------------------------------------------------------------------ the library's host arithmetic
def _lib_taps(lib, pair):
    _, _, half = plan(*pair)
    buf = np.zeros(2 * half + 1, dtype=np.float32)
    assert lib.fsnp_resample_taps(pair[0], pair[1], buf.ctypes.data, buf.size) == 0, _lib.last_error()
    return buf


@pytest.mark.parametrize("pair", SCIPY_PAIRS + [(44100, 192000), (192000, 44100)], ids=lambda p: f"{p[0]}-{p[1]}")
def test_library_taps_against_oracle(pair):
    lib = _lib.load()
    up, _, half = plan(*pair)
    t = _lib_taps(lib, pair)
    want = up * taps64(*pair)
    err = np.abs(t.astype(np.float64) - want)
    assert (err <= 2.0 ** -23 * np.abs(want) + 1e-12).all(), float((err / (np.abs(want) + 1e-30)).max())
    assert np.array_equal(t, t[::-1])
    small = np.zeros(2 * half, dtype=np.float32)
    assert lib.fsnp_resample_taps(pair[0], pair[1], small.ctypes.data, small.size) == 2 and "capacity" in _lib.last_error()
    assert lib.fsnp_resample_taps(pair[0], pair[1], None, 1 << 20) == 1


def test_plan_and_length_against_python_integers():
    lib = _lib.load()
    up, down, half, n_out = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
    refused = set()
    for a in RATES:
        for b in RATES:
            rc = lib.fsnp_resample_plan(a, b, ctypes.byref(up), ctypes.byref(down), ctypes.byref(half))
            if max(plan(a, b)[:2]) > 640:      # the limit decides, not a list of rates
                assert rc == 2 and "640" in _lib.last_error(), (a, b)
                refused.add(frozenset((a, b)))
                continue
            assert rc == 0, (a, b, _lib.last_error())
            assert (up.value, down.value, half.value) == plan(a, b) and max(up.value, down.value) <= 640
            for n in (0, 1, 257, 2 ** 31 - 1, 2 ** 31 - 2, 2 ** 31 + 5, 2 ** 40):
                assert lib.fsnp_resample_length(a, b, n, ctypes.byref(n_out)) == 0
                assert n_out.value == -(-n * up.value // down.value), (a, b, n)
    # among the common rates four pairs are past the limit: 11.025 kHz against 32 / 96 / 192 kHz (1280 : 441, 1280 : 147, 2560 : 147)
    # and 22.05 kHz against 192 kHz (1280 : 147); every rate of the list converts to and from the model's 16 kHz
    assert refused == {frozenset((11025, r)) for r in (32000, 96000, 192000)} | {frozenset((22050, 192000))}
    assert lib.fsnp_resample_plan(48000, 16000, None, None, None) == 0
    # the 640 limit from both sides, in both directions
    for a, b, ok in ((640, 1, True), (1, 640, True), (641, 1, False), (1, 641, False), (16000, 44101, False), (44101, 16000, False),
                     (640 * 7, 639 * 7, True), (641 * 3, 640 * 3, False)):
        rc = lib.fsnp_resample_plan(a, b, ctypes.byref(up), ctypes.byref(down), ctypes.byref(half))
        assert rc == (0 if ok else 2), (a, b)
        if not ok:
            assert "640" in _lib.last_error() and "fsnp_resample_plan" in _lib.last_error()
            assert lib.fsnp_resample_length(a, b, 10, ctypes.byref(n_out)) == 2
    for a, b in ((0, 16000), (16000, 0), (-8000, 16000), (16000, -1)):
        assert lib.fsnp_resample_plan(a, b, None, None, None) == 2 and "positive" in _lib.last_error()
        assert lib.fsnp_resample_length(a, b, 10, ctypes.byref(n_out)) == 2
    assert lib.fsnp_resample_length(48000, 16000, -1, ctypes.byref(n_out)) == 2
    assert lib.fsnp_resample_length(48000, 16000, 5, None) == 1


# ------------------------------------------------------------------------------------------------ the binding
def test_header_symbols_and_abi():
    with open(os.path.join(INCLUDE, "fsnp_resample.h")) as f:
        declared = set(re.findall(r"^int (fsnp_\w+)\(", f.read(), flags=re.M))
    assert declared == set(_lib.RESAMPLE_SYMBOLS) and len(declared) == 6, declared ^ set(_lib.RESAMPLE_SYMBOLS)
    with open(os.path.join(INCLUDE, "fsnp.h")) as f:
        assert '#include "fsnp_resample.h"' in f.read()
    for other in (_lib.SYMBOLS, _lib.LENGTHS_SYMBOLS, _lib.STREAM_SYMBOLS, _lib.WAVE_STREAM_SYMBOLS, _lib.LIVE_STREAM_SYMBOLS,
                  _lib.SPEC_STREAM_SYMBOLS, _lib.DEVICE_WEIGHTS_SYMBOLS, _lib.STFT_GEOMETRY_SYMBOLS, _lib.PCM_SYMBOLS):
        assert not set(_lib.RESAMPLE_SYMBOLS) & set(other)
    lib = _lib.load()
    assert lib.fsnp_abi_version() == 13 == _lib.ABI_VERSION
    for name, (res, args) in _lib.RESAMPLE_SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype == res and fn.argtypes == args, name


def test_null_handle_is_code_1_and_names_the_entry_point():
    lib = _lib.load()
    buf = (ctypes.c_float * 8)()
    p = ctypes.addressof(buf)
    assert lib.fsnp_resample_pcm(None, p, 0, 8, 1, p, 0, 8, 1, None, 1, 8, 48000, 16000, None, None) == 1
    assert "fsnp_resample_pcm" in _lib.last_error()
    assert lib.fsnp_enhance_wave_rate(None, p, 0, 8, 1, p, 0, 8, 1, None, 1, 8, None, 48000, 16000, None) == 1
    assert "fsnp_enhance_wave_rate" in _lib.last_error()
    assert lib.fsnp_reserve_rate(None, 1, 8, 48000, 16000, None) == 1
    assert "fsnp_reserve_rate" in _lib.last_error()


# ------------------------------------------------------------------------------------------------ Python refusals: no GPU is touched
@pytest.mark.parametrize("cls,args", [(FullSubNet_Plus, DEFAULT_MODEL_ARGS), (FullSubNet, FULLSUBNET_MODEL_ARGS)], ids=["plus", "fullsubnet"])
def test_python_refusals_touch_no_gpu(cls, args):
    m = cls(**dict(args, weight_init=False))
    assert m.sample_rate == 16000
    x = torch.zeros(1, 4800)
    for bad in (0, -16000, 16000.0, "48000", None, True):
        with pytest.raises(ValueError, match="sample rate"):
            m.sample_rate = bad
    assert m.sample_rate == 16000
    m.sample_rate = 8000
    assert m.sample_rate == 8000
    m.sample_rate = 16000
    for bad in (0, -1, 44100.0, "48k"):
        with pytest.raises(ValueError, match="sample rate"):
            m.enhance_wave(x, sample_rate=bad)
        with pytest.raises(ValueError, match="sample rate"):
            m.resample(x, bad, 16000)
        with pytest.raises(ValueError, match="sample rate"):
            m.resample(x, 16000, bad)
        with pytest.raises(ValueError, match="sample rate"):
            m.reserve(1, 10, max_samples=4800, sample_rate=bad)
    with pytest.raises(ValueError, match="640"):
        m.enhance_wave(x, sample_rate=44101)
    with pytest.raises(ValueError, match="640"):
        m.resample(x, 16000, 44101)
    with pytest.raises(ValueError, match="640"):
        m.reserve(1, 10, max_samples=4800, sample_rate=44101)
    with pytest.raises(ValueError, match="640"):
        fullsubnet_plus_amd.resample_length(10, 44101, 16000)
    with pytest.raises(ValueError, match="out_format"):
        m.resample(x, 48000, 16000, out_format="u8")
    for call in (lambda: m.enhance_wave(x, sample_rate=48000), lambda: m.enhance_wave(x, sample_rate=16000),
                 lambda: m.resample(x, 48000, 16000), lambda: m.resample(x.short(), 16000, 16000)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    assert m._hip.handle is None

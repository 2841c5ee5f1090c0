"""Host-side checks of rate sessions (include/fsnp_wave_rate_stream.h, FullSubNet.open_wave_stream(..., sample_rate=R)) on the cross-compiled
library: the contract restated in float64 against the whole-clip oracle, the host arithmetic against Python integers, and the binding."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from fullsubnet_plus_amd import FullSubNet, FullSubNet_Plus, _lib
from oracle.ref_loader import DEFAULT_MODEL_ARGS, FULLSUBNET_MODEL_ARGS
from oracle.weights import make_state_dict_fullsubnet
from tests._resample_util import PAIRS, plan
from tests._stream_util import stream_kwargs
from tests._wave_rate_stream_util import TorchWaveRateStream, oracle_rate, rate_delay, ready, shortest_clip, total
from tests._wave_stream_util import random_schedule, wave_clip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 16000
RATES = [48000, 44100, 8000]


# ------------------------------------------------------------------------------------------------ 1. the contract in fp64
def _small_model(num_freqs, look_ahead=2):
    """a FullSubNet small enough for fp64 on the CPU (as tests/test_host_stft_geometry.py): the contract under test lies around the model"""
    args = dict(FULLSUBNET_MODEL_ARGS, num_freqs=num_freqs, norm_type="cumulative_layer_norm", look_ahead=look_ahead, sb_num_neighbors=4,
                fb_model_hidden_size=24, sb_model_hidden_size=16)
    sd = make_state_dict_fullsubnet(6, "default", num_freqs=num_freqs, fb_hidden=24, sb_hidden=16, sb_num_neighbors=4)
    return {k: v.double() for k, v in sd.items()}, stream_kwargs(args)


def _schedules(L, rate, seed):
    ones, block = min(L, 300), rate // 100
    rest = [min(block, L - ones - i) for i in range(0, L - ones, block)]
    return {"one push": [0, L, 0], "1 sample x 300, then 10 ms": [1] * ones + [0] + rest,
            "random": random_schedule(L, seed, 3 * block)}


@pytest.mark.parametrize("num_freqs,hop", [(257, 256), (161, 80)])
@pytest.mark.parametrize("rate", RATES)
def test_chunked_rate_restatement_equals_the_whole_clip_oracle(rate, num_freqs, hop):
    """A clip at rate R pushed in blocks of any size (idle pushes mixed in), then finish(), is L + D_R samples; the first D_R are exactly
    0 and the rest is resample64 -> the oracle's enhance_wave at the model's rate -> resample64, cut to L.  Bar: 1e-9 of max |want|, the
    bar of tests/test_host_stft_geometry.py for the same kind of comparison.  fp64: this pins ready(P), the delay, both histories'
    sizes and both clamps at finish (the restatement asserts them), not fp32 summation order."""
    sd, kw = _small_model(num_freqs)
    up, down, half = plan(rate, M)
    rs = TorchWaveRateStream(sd, hop, rate, M, **kw)
    D, DM = rs.delay, 2 * (num_freqs - 1) + 2 * hop
    assert rs.DM == DM and D == rate_delay(DM, up, down, half)
    if (num_freqs, hop) == (257, 256):
        assert D == {48000: 3264, 44100: 2998, 8000: 576}[rate]
    assert (rs.HI, rs.HE) == {48000: (192, 64), 44100: (176, 64), 8000: (64, 128)}[rate]
    n_half = num_freqs - 1
    shortest = shortest_clip(up, down, n_half)
    assert total(shortest, up, down) > n_half >= total(shortest - 1, up, down)
    lengths = [(9 * hop + 77) * down // up, D - 100, shortest]              # longer than D_R, shorter, the shortest clip allowed
    assert lengths[0] > D > lengths[1] >= shortest
    worst = 0.0
    for n, L in enumerate(lengths):
        clip = wave_clip(L, 1200 + n).double()
        want = oracle_rate(sd, clip, rate, M, num_freqs, hop, **kw)
        assert want.shape == (L,) and want.dtype == torch.float64
        scale = float(want.abs().max())
        for name, chunks in _schedules(L, rate, 60 + n).items():
            assert sum(chunks) == L and 0 in chunks, (name, chunks)
            outs, pos = [], 0
            for c in chunks:
                o = rs.push(clip[pos:pos + c].numpy())
                assert o.shape == (c,)
                outs.append(o)
                pos += c
            assert rs.P == L
            fin = rs.finish()
            assert fin.shape == (D,) and rs.P == 0
            got = torch.cat(outs + [fin])
            assert got.shape == (L + D,)
            assert torch.count_nonzero(got[:D]) == 0, (L, name)
            err = float((got[D:] - want).abs().max()) / scale
            worst = max(worst, err)
            assert err < 1e-9, (rate, L, name, err)
    assert rs.most_at_finish == -(-half // down) == (64 if rate == 8000 else 32)
    print(f"{rate} Hz F={num_freqs} hop={hop}: worst rel err of the chunked rate restatement {worst:.3e}")


def test_restatement_refuses_a_clip_one_sample_too_short_and_finishes_an_empty_slot_with_zeros():
    sd, kw = _small_model(161)
    rs = TorchWaveRateStream(sd, 80, 48000, M, **kw)
    assert torch.count_nonzero(rs.finish()) == 0
    rs.push(wave_clip(shortest_clip(1, 3, 160) - 1, 3).double().numpy())
    with pytest.raises(ValueError, match="reflect padding"):
        rs.finish()


# ------------------------------------------------------------------------------------------------ 2. host arithmetic
TO_MODEL = [p for p in PAIRS if p[1] == M] + [(32000, M), (24000, M), (8000, M)]


@pytest.mark.parametrize("pair", TO_MODEL)
def test_resample_ready_against_python_integers(pair):
    lib = _lib.load()
    up, down, half = plan(*pair)
    v = ctypes.c_int64()
    for P in list(range(0, 700)) + [half // up, half // up + 1, 10 ** 6 + 7, 2 ** 40 + 12345]:
        assert lib.fsnp_resample_ready(pair[0], pair[1], P, ctypes.byref(v)) == 0, _lib.last_error()
        assert v.value == ready(P, up, down, half), (pair, P)
        assert v.value <= total(P, up, down)
        if v.value:                                                         # the definition: the last ready sample's window has arrived, the next one's not
            assert ((v.value - 1) * down + half) // up <= P - 1 < (v.value * down + half) // up


@pytest.mark.parametrize("pair", TO_MODEL)
@pytest.mark.parametrize("DM", [1024, 640, 480])
def test_the_delay_is_sufficient_and_one_less_is_not(pair, DM):
    """Every push can return as many samples as it took exactly when output P - 1 - D of a slot that holds P samples reads no enhanced
    sample past ready(P) - DM - 1; by enumeration of P, D_R passes and D_R - 1 does not.  The same enumeration gives the histories."""
    up, down, half = plan(*pair)
    D = rate_delay(DM, up, down, half)

    def enough(delay, P):
        m = P - 1 - delay
        return m < 0 or (m * up + half) // down <= ready(P, up, down, half) - DM - 1
    most_in = most_e = 0
    for P in range(1, 6000):
        assert enough(D, P), (pair, P)
        r = ready(P, up, down, half)
        if r:                                                               # sample ready(P) is the next to be made: how far below P it reads
            most_in = max(most_in, P - max(0, -((half - r * down) // up)))
        m = P - D                                                           # the next output: how far below ready(P) - DM it reads
        if m >= 0:
            most_e = max(most_e, (r - DM) - max(0, -((half - m * up) // down)))
    assert not all(enough(D - 1, P) for P in range(1, 6000)), pair
    assert most_in <= 2 * half // up and most_e <= -(-2 * half // down), (pair, most_in, most_e)
    assert most_in >= 2 * half // up - 1 and most_e >= -(-2 * half // down) - 1                      # ... and they are no larger than needed


def test_session_numbers_at_the_default_geometry():
    for rate, D, ms in ((48000, 3264, 68.0), (44100, 2998, 67.98), (8000, 576, 72.0)):
        up, down, half = plan(rate, M)
        assert rate_delay(1024, up, down, half) == D and abs(1000.0 * D / rate - ms) < 0.005


# ------------------------------------------------------------------------------------------------ 3. the binding
def test_header_symbols_and_abi():
    with open(os.path.join(ROOT, "include", "fsnp_wave_rate_stream.h")) as f:
        declared = set(re.findall(r"^(?:int|void|int64_t) (fsnp_[a-z0-9_]+)\s*\(", f.read(), flags=re.M))
    assert declared == set(_lib.WAVE_RATE_STREAM_SYMBOLS) and len(declared) == 14, declared ^ set(_lib.WAVE_RATE_STREAM_SYMBOLS)
    with open(os.path.join(ROOT, "include", "fsnp.h")) as f:
        assert '#include "fsnp_wave_rate_stream.h"' in f.read()
    for other in (_lib.SYMBOLS, _lib.LENGTHS_SYMBOLS, _lib.STREAM_SYMBOLS, _lib.WAVE_STREAM_SYMBOLS, _lib.LIVE_STREAM_SYMBOLS,
                  _lib.SPEC_STREAM_SYMBOLS, _lib.DEVICE_WEIGHTS_SYMBOLS, _lib.STFT_GEOMETRY_SYMBOLS, _lib.PCM_SYMBOLS, _lib.RESAMPLE_SYMBOLS):
        assert not set(_lib.WAVE_RATE_STREAM_SYMBOLS) & set(other)
    lib = _lib.load()
    assert lib.fsnp_abi_version() == 13 == _lib.ABI_VERSION
    for name, (res, args) in _lib.WAVE_RATE_STREAM_SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype == res and fn.argtypes == args, name


def test_null_arguments_give_code_1_and_name_the_entry_point():
    lib = _lib.load()
    sp, v = ctypes.c_void_p(), ctypes.c_int64()
    buf = (ctypes.c_float * 8)()
    p = ctypes.addressof(buf)
    for name, call in (("fsnp_wave_rate_stream_create", lambda: lib.fsnp_wave_rate_stream_create(None, 1, 480, 48000, M, ctypes.byref(sp))),
                     ("fsnp_wave_rate_stream_create_live", lambda: lib.fsnp_wave_rate_stream_create_live(None, 1, 480, 48000, M, ctypes.byref(sp))),
                     ("fsnp_wave_rate_stream_push_pcm", lambda: lib.fsnp_wave_rate_stream_push_pcm(None, p, 0, 8, 1, None, p, 0, 8, 1, 8, None)),
                     ("fsnp_wave_rate_stream_finish_pcm", lambda: lib.fsnp_wave_rate_stream_finish_pcm(None, None, 0, p, 0, 8, 1, None)),
                     ("fsnp_wave_rate_stream_reset", lambda: lib.fsnp_wave_rate_stream_reset(None, None, 0, None)),
                     ("fsnp_wave_rate_stream_get_state", lambda: lib.fsnp_wave_rate_stream_get_state(None, 0, p, None)),
                     ("fsnp_wave_rate_stream_set_state", lambda: lib.fsnp_wave_rate_stream_set_state(None, 0, p, None)),
                     ("fsnp_wave_rate_stream_samples", lambda: lib.fsnp_wave_rate_stream_samples(None, 0, ctypes.byref(v))),
                     ("fsnp_resample_ready", lambda: lib.fsnp_resample_ready(48000, M, 5, None))):
        rc = call()
        assert rc == 1 and name in _lib.last_error() and "null" in _lib.last_error(), name
    assert lib.fsnp_wave_rate_stream_state_bytes(None) == 0 and lib.fsnp_wave_rate_stream_delay(None) == 0
    assert lib.fsnp_wave_rate_stream_model_delay(None) == 0 and lib.fsnp_wave_rate_stream_model_max_samples(None) == 0
    lib.fsnp_wave_rate_stream_destroy(None)
    assert lib.fsnp_resample_ready(16000, 44101, 5, ctypes.byref(v)) == 2 and "640" in _lib.last_error()
    assert lib.fsnp_resample_ready(48000, M, -1, ctypes.byref(v)) == 2


def test_refusals_of_the_rate_touch_no_gpu():
    m = FullSubNet(**dict(FULLSUBNET_MODEL_ARGS, norm_type="cumulative_laplace_norm"))
    for bad, why in ((0, "positive"), (-48000, "positive"), (48000.0, "integer"), ("48000", "integer"), (True, "integer"), (44101, "640")):
        with pytest.raises(ValueError, match=why) as e:
            m.open_wave_stream(1, max_samples=480, live=True, sample_rate=bad)
        assert "open_wave_stream" in str(e.value)
    assert m._hip.handle is None                                            # no handle was made: no GPU was touched
    with pytest.raises(NotImplementedError, match="not causal"):
        FullSubNet_Plus(**DEFAULT_MODEL_ARGS).open_wave_stream(4, sample_rate=48000)
    with pytest.raises(NotImplementedError, match="whole clip's total"):
        FullSubNet(**dict(FULLSUBNET_MODEL_ARGS, norm_type="offline_laplace_norm")).open_wave_stream(4, sample_rate=48000)

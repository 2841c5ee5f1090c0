"""Host-side checks of the STFT geometry surface (include/fsnp_stft_geometry.h, model.hop_length) on the cross-compiled library, and the
wave-session contract at any hop length restated in torch-CPU fp64 against the whole-clip oracle composed at the same geometry."""
import ctypes
import os
import re

import pytest
import torch

from fullsubnet_plus_amd import FullSubNet, FullSubNet_Plus, _lib
from fullsubnet_plus_amd.stream import wave_refusal
from oracle.ref_loader import DEFAULT_MODEL_ARGS, FULLSUBNET_MODEL_ARGS
from oracle.weights import make_state_dict_fullsubnet
from tests._stream_util import stream_kwargs
from tests._wave_geometry_util import TorchWaveStreamAt, clip_lengths, frames_held, oracle_enhance_wave
from tests._wave_stream_util import TorchWaveStream, random_schedule, schedule, wave_clip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ 1. header and symbols
def test_geometry_header_declares_exactly_the_geometry_symbols():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "fsnp_stft_geometry.h")).read()
    declared = set(re.findall(r"^(?:int|void|int32_t|int64_t) (fsnp_[a-z0-9_]+)\s*\(", header, flags=re.M))
    assert declared == set(_lib.STFT_GEOMETRY_SYMBOLS) == {"fsnp_set_hop_length", "fsnp_hop_length"}
    for name in declared:
        assert hasattr(lib, name), name
    for other in (_lib.SYMBOLS, _lib.LENGTHS_SYMBOLS, _lib.STREAM_SYMBOLS, _lib.WAVE_STREAM_SYMBOLS, _lib.LIVE_STREAM_SYMBOLS,
                  _lib.SPEC_STREAM_SYMBOLS, _lib.DEVICE_WEIGHTS_SYMBOLS):
        assert not set(_lib.STFT_GEOMETRY_SYMBOLS) & set(other)
    assert '#include "fsnp_stft_geometry.h"' in open(os.path.join(ROOT, "include", "fsnp.h")).read()
    assert lib.fsnp_abi_version() == 13 == _lib.ABI_VERSION


def test_null_handle_gives_code_1():
    lib = _lib.load()
    assert lib.fsnp_set_hop_length(None, 128) == 1 and "null" in _lib.last_error()
    assert lib.fsnp_hop_length(None) == 0


# ------------------------------------------------------------------------------------------------ 2. the setter
def _models(num_freqs):
    return [FullSubNet_Plus(**dict(DEFAULT_MODEL_ARGS, num_freqs=num_freqs)),
            FullSubNet(**dict(FULLSUBNET_MODEL_ARGS, num_freqs=num_freqs, norm_type="cumulative_laplace_norm"))]


@pytest.mark.parametrize("num_freqs", [257, 161])
def test_hop_length_is_validated_on_assignment_without_a_gpu(num_freqs):
    n_fft = 2 * (num_freqs - 1)
    for m in _models(num_freqs):
        assert m.hop_length == num_freqs - 1 and "hop_length" not in m.__dict__        # a property, not an attribute someone set
        for bad, rule in ((n_fft // 2 + 4, r"outside \[n_fft / 8, n_fft / 2\]"), (n_fft // 8 - 4, r"outside \[n_fft / 8, n_fft / 2\]"),
                          (0, "outside"), (-64, "outside"), (n_fft // 4 + 2, "multiple of 4"), (n_fft // 4 + 1, "multiple of 4"),
                          (n_fft / 4, "integer"), (float(n_fft // 4), "integer"), ("128", "integer"), (True, "integer"), (None, "integer")):
            with pytest.raises(ValueError, match=rule):
                m.hop_length = bad
            assert m.hop_length == num_freqs - 1                                       # a refused value changes nothing
        for good in (n_fft // 2, n_fft // 4, n_fft // 8, n_fft // 4 + 4):
            m.hop_length = good
            assert m.hop_length == good and isinstance(m.hop_length, int)
        assert m._hip.handle is None                                                   # no handle was made: no GPU was touched


def test_hop_length_is_no_constructor_keyword():
    with pytest.raises(TypeError):
        FullSubNet(**dict(FULLSUBNET_MODEL_ARGS, hop_length=128))
    with pytest.raises(TypeError):
        FullSubNet_Plus(**dict(DEFAULT_MODEL_ARGS, hop_length=128))


def test_a_161_bin_model_is_no_longer_refused_for_its_bin_count():
    m = FullSubNet(**dict(FULLSUBNET_MODEL_ARGS, num_freqs=161, norm_type="cumulative_laplace_norm"))
    assert wave_refusal(m) is None
    m.hop_length = 80
    assert wave_refusal(m) is None
    # what is left is the alignment rule for a default hop nobody chose: num_freqs - 1 = 162 is no multiple of 4
    odd = FullSubNet(**dict(FULLSUBNET_MODEL_ARGS, num_freqs=163, norm_type="cumulative_laplace_norm"))
    assert "multiple of 4" in wave_refusal(odd)
    with pytest.raises(NotImplementedError, match="multiple of 4"):
        odd.open_wave_stream(1)
    odd.hop_length = 160
    assert wave_refusal(odd) is None


# ------------------------------------------------------------------------------------------------ 3. the session contract in fp64
GEOMETRIES = [(161, 160), (161, 80), (161, 40), (33, 12)]


def _small_model(num_freqs, look_ahead, norm_type="cumulative_layer_norm"):
    """a FullSubNet small enough for fp64 on the CPU; the contract under test lies around the model, not in it"""
    args = dict(FULLSUBNET_MODEL_ARGS, num_freqs=num_freqs, norm_type=norm_type, look_ahead=look_ahead, sb_num_neighbors=4,
                fb_model_hidden_size=24, sb_model_hidden_size=16)
    sd = make_state_dict_fullsubnet(6, "default", num_freqs=num_freqs, fb_hidden=24, sb_hidden=16, sb_num_neighbors=4)
    return {k: v.double() for k, v in sd.items()}, stream_kwargs(args)


def _schedules(L, hop, seed):
    return {"one push": [0, L, 0], "hop": schedule(L, hop), "hop-1": schedule(L, hop - 1), "hop+1": schedule(L, hop + 1),
            "97": schedule(L, 97), "random": random_schedule(L, seed, 3 * hop)}


@pytest.mark.parametrize("look_ahead", [0, 2])
@pytest.mark.parametrize("num_freqs,hop", GEOMETRIES)
def test_chunked_wave_restatement_at_any_hop_equals_the_whole_clip_oracle(num_freqs, hop, look_ahead):
    """The contract, independent of the GPU: a clip pushed in blocks of any size (idle pushes mixed in), then finish(), is L + D samples;
    the first D = n_fft + look_ahead * hop are exactly 0 and the rest is the oracle's stft -> model -> cIRM -> istft of the clip at that
    geometry.  fp64: this pins frame completion, the frames a finish adds, the delay, and the record's sizes (carry n_fft + 1, partial
    sums n_fft - hop, fifo <= hop: the restatement asserts them), not fp32 summation order."""
    sd, kw = _small_model(num_freqs, look_ahead)
    n_fft = 2 * (num_freqs - 1)
    ws = TorchWaveStreamAt(sd, hop, **kw)
    D = ws.delay
    assert D == n_fft + look_ahead * hop
    worst, most_finish_frames = 0.0, 0
    for n, L in enumerate(clip_lengths(n_fft, hop)):
        clip = wave_clip(L, 1000 + n).double()
        want = oracle_enhance_wave(sd, clip.unsqueeze(0), num_freqs, hop, fullsubnet=True, **kw)[0]
        assert want.shape == (L,) and want.dtype == torch.float64
        scale = float(want.abs().max())
        for name, chunks in _schedules(L, hop, 50 + n).items():
            assert sum(chunks) == L and 0 in chunks, (name, chunks)
            outs, pos = [], 0
            for c in chunks:
                o = ws.push(clip[pos:pos + c])
                assert o.shape == (c,)
                outs.append(o)
                pos += c
            assert ws.P == L and ws.frames == frames_held(L, hop, n_fft // 2)
            fin = ws.finish()
            most_finish_frames = max(most_finish_frames, ws.finish_frames)
            assert fin.shape == (D,) and ws.P == 0
            got = torch.cat(outs + [fin])
            assert got.shape == (L + D,)
            assert torch.count_nonzero(got[:D]) == 0, (L, name)
            err = float((got[D:] - want).abs().max()) / scale
            worst = max(worst, err)
            assert err < 1e-9, (L, name, err)
    assert most_finish_frames == -(-n_fft // (2 * hop))          # some clip does need ceil(n_fft / (2 hop)) frames at its end
    print(f"F={num_freqs} hop={hop} look_ahead={look_ahead}: worst rel err of the chunked wave restatement {worst:.3e}")


def test_the_restatement_at_the_default_hop_is_the_existing_one():
    """hop = n_fft / 2: TorchWaveStreamAt returns what tests/_wave_stream_util.py TorchWaveStream returns, bit for bit, delay included."""
    sd, kw = _small_model(33, 1)
    a, b = TorchWaveStreamAt(sd, 32, **kw), TorchWaveStream(sd, **kw)
    assert a.delay == b.delay == 3 * 32
    clip = wave_clip(9 * 32 + 7, 77).double()
    pos = 0
    for c in random_schedule(clip.numel(), 5, 80):
        assert torch.equal(a.push(clip[pos:pos + c]), b.push(clip[pos:pos + c]))
        pos += c
    assert torch.equal(a.finish(), b.finish())

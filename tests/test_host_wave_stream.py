"""Host-side checks of the wave-session surface (include/fsnp_wave_stream.h, fullsubnet_plus_amd.stream.WaveStream) on the cross-compiled
library, and the contract itself restated in torch-CPU fp64 against the oracle's whole-clip enhance_wave."""
import ctypes
import os
import re

import pytest
import torch

from fullsubnet_plus_amd import FullSubNet, FullSubNet_Plus, _lib
from oracle import fsnp_torch
from oracle.ref_loader import DEFAULT_MODEL_ARGS, FULLSUBNET_MODEL_ARGS
from oracle.weights import make_state_dict_fullsubnet
from tests._stream_util import stream_kwargs
from tests._wave_stream_util import TorchWaveStream, random_schedule, schedule, wave_clip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP = 256


def test_wave_stream_header_declares_exactly_the_wave_stream_symbols():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "fsnp_wave_stream.h")).read()
    declared = set(re.findall(r"^(?:int|void|int64_t) (fsnp_[a-z0-9_]+)\s*\(", header, flags=re.M))
    assert declared == set(_lib.WAVE_STREAM_SYMBOLS) and len(declared) == 10, declared ^ set(_lib.WAVE_STREAM_SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name
    for other in (_lib.SYMBOLS, _lib.LENGTHS_SYMBOLS, _lib.STREAM_SYMBOLS):
        assert not set(_lib.WAVE_STREAM_SYMBOLS) & set(other)
    core = open(os.path.join(ROOT, "include", "fsnp.h")).read()
    assert '#include "fsnp_wave_stream.h"' in core
    assert lib.fsnp_abi_version() == 13 == _lib.ABI_VERSION


def test_null_arguments_give_code_1():
    lib = _lib.load()
    sp = ctypes.c_void_p()
    assert lib.fsnp_wave_stream_create(None, 1, 256, ctypes.byref(sp)) == 1 and "null" in _lib.last_error()
    assert lib.fsnp_wave_stream_push(None, None, 0, None, None, 0, 1, None) == 1 and "null" in _lib.last_error()
    assert lib.fsnp_wave_stream_finish(None, None, 0, None, 0, None) == 1 and "null" in _lib.last_error()
    assert lib.fsnp_wave_stream_reset(None, None, 0, None) == 1
    assert lib.fsnp_wave_stream_get_state(None, 0, None, None) == 1
    assert lib.fsnp_wave_stream_set_state(None, 0, None, None) == 1
    v = ctypes.c_int64()
    assert lib.fsnp_wave_stream_samples(None, 0, ctypes.byref(v)) == 1
    assert lib.fsnp_wave_stream_state_bytes(None) == 0 and lib.fsnp_wave_stream_delay(None) == 0
    lib.fsnp_wave_stream_destroy(None)


LENGTHS = [HOP + 1, 2 * HOP, 5 * HOP - 1, 5 * HOP, 5 * HOP + 1, 9 * HOP + 77]


def _schedules(L, seed):
    return {"one push": [0, L, 0], "hop": schedule(L, HOP), "hop-1": schedule(L, HOP - 1), "hop+1": schedule(L, HOP + 1),
            "160": schedule(L, 160), "97": schedule(L, 97), "random": random_schedule(L, seed, 3 * HOP)}


@pytest.mark.parametrize("norm_type", ["cumulative_laplace_norm", "cumulative_layer_norm"])
@pytest.mark.parametrize("look_ahead", [0, 2])
def test_chunked_wave_restatement_equals_the_whole_clip_oracle(norm_type, look_ahead):
    """The contract, independent of the GPU: a clip pushed in blocks of any size (idle pushes mixed in), then finish(), is L + D samples; the
    first D = (2 + look_ahead) hop are exactly 0 and the rest is the oracle's enhance_wave of the clip.  fp64: this pins the delay and both
    ends of the clip (lengths just above hop, at and around a multiple of hop), not fp32 summation order."""
    args = dict(FULLSUBNET_MODEL_ARGS, norm_type=norm_type, look_ahead=look_ahead)
    sd = {k: v.double() for k, v in make_state_dict_fullsubnet(6, "default").items()}
    kw = stream_kwargs(args)
    ws = TorchWaveStream(sd, **kw)
    D = ws.delay
    assert D == (2 + look_ahead) * HOP
    worst = 0.0
    for n, L in enumerate(LENGTHS):
        clip = wave_clip(L, 1000 + n).double()
        want = fsnp_torch.enhance_wave(sd, clip.unsqueeze(0), fullsubnet=True, **kw)[0]
        assert want.shape == (L,) and want.dtype == torch.float64
        scale = float(want.abs().max())
        for name, chunks in _schedules(L, 50 + n).items():
            assert sum(chunks) == L and 0 in chunks, (name, chunks)
            outs, pos = [], 0
            for c in chunks:
                o = ws.push(clip[pos:pos + c])
                assert o.shape == (c,)
                outs.append(o)
                pos += c
            assert ws.P == L
            fin = ws.finish()
            assert fin.shape == (D,) and ws.P == 0
            got = torch.cat(outs + [fin])
            assert got.shape == (L + D,)
            assert torch.count_nonzero(got[:D]) == 0, (L, name)
            err = float((got[D:] - want).abs().max()) / scale
            worst = max(worst, err)
            assert err < 1e-9, (L, name, err)
    print(f"{norm_type} look_ahead={look_ahead}: worst rel err of the chunked wave restatement {worst:.3e}")


def test_restatement_refuses_a_clip_of_hop_samples_and_finishes_an_empty_slot_with_zeros():
    args = dict(FULLSUBNET_MODEL_ARGS, norm_type="cumulative_layer_norm")
    ws = TorchWaveStream({k: v.double() for k, v in make_state_dict_fullsubnet(6, "default").items()}, **stream_kwargs(args))
    assert torch.count_nonzero(ws.finish()) == 0
    ws.push(wave_clip(HOP, 3).double())
    with pytest.raises(ValueError, match="reflect padding"):
        ws.finish()


def test_models_that_cannot_stream_waveforms_say_why_without_a_gpu():
    with pytest.raises(NotImplementedError, match="not causal"):
        FullSubNet_Plus(**DEFAULT_MODEL_ARGS).open_wave_stream(4)
    with pytest.raises(NotImplementedError, match="whole clip's total"):
        FullSubNet(**dict(FULLSUBNET_MODEL_ARGS, norm_type="offline_laplace_norm")).open_wave_stream(4)
    with pytest.raises(NotImplementedError, match="GRU"):
        FullSubNet(**dict(FULLSUBNET_MODEL_ARGS, norm_type="cumulative_laplace_norm", sequence_model="GRU")).open_wave_stream(4)
    with pytest.raises(NotImplementedError, match="row-tile kernel"):
        FullSubNet(**dict(FULLSUBNET_MODEL_ARGS, norm_type="cumulative_laplace_norm", sb_model_hidden_size=320)).open_wave_stream(4)
    m = FullSubNet(**dict(FULLSUBNET_MODEL_ARGS, norm_type="cumulative_laplace_norm"))
    m.output_size = 3
    with pytest.raises(NotImplementedError, match="output_size = 2"):
        m.open_wave_stream(4)

"""Host-side checks of the spectrum-session surface (include/fsnp_spec_stream.h, fullsubnet_plus_amd.stream.SpecStream) on the
cross-compiled library, and the contract itself restated in torch-CPU fp64 against the oracle's whole-clip mask and cIRM epilogue."""
import ctypes
import os
import re

import pytest
import torch

from fullsubnet_plus_amd import FullSubNet, FullSubNet_Plus, _lib
from oracle.ref_loader import DEFAULT_MODEL_ARGS, FULLSUBNET_MODEL_ARGS
from oracle.weights import make_state_dict_fullsubnet
from tests._spec_stream_util import TorchSpecStream, crel_err, oracle_enhance, random_schedule, spec_clip
from tests._stream_util import stream_kwargs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_spec_stream_header_declares_exactly_the_spec_stream_symbols():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "fsnp_spec_stream.h")).read()
    declared = set(re.findall(r"^(?:int|void|int64_t) (fsnp_[a-z0-9_]+)\s*\(", header, flags=re.M))
    assert declared == set(_lib.SPEC_STREAM_SYMBOLS) and len(declared) == 9, declared ^ set(_lib.SPEC_STREAM_SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name
    for other in (_lib.SYMBOLS, _lib.LENGTHS_SYMBOLS, _lib.STREAM_SYMBOLS, _lib.WAVE_STREAM_SYMBOLS, _lib.LIVE_STREAM_SYMBOLS):
        assert not set(_lib.SPEC_STREAM_SYMBOLS) & set(other)
    # the live creator is declared here, not in fsnp_stream_live.h
    live = open(os.path.join(ROOT, "include", "fsnp_stream_live.h")).read()
    assert "fsnp_spec_stream_create_live" in declared and "fsnp_spec_stream" not in live
    core = open(os.path.join(ROOT, "include", "fsnp.h")).read()
    assert '#include "fsnp_spec_stream.h"' in core
    assert lib.fsnp_abi_version() == 13 == _lib.ABI_VERSION


def test_null_arguments_give_code_1():
    lib = _lib.load()
    sp = ctypes.c_void_p()
    assert lib.fsnp_spec_stream_create(None, 1, 1, ctypes.byref(sp)) == 1 and "null" in _lib.last_error()
    assert lib.fsnp_spec_stream_create_live(None, 1, 1, ctypes.byref(sp)) == 1 and "fsnp_spec_stream_create_live" in _lib.last_error()
    st = (ctypes.c_int64 * 3)()
    assert lib.fsnp_spec_stream_push(None, None, ctypes.byref(st), None, None, ctypes.byref(st), 1, None) == 1 and "null" in _lib.last_error()
    assert lib.fsnp_spec_stream_reset(None, None, 0, None) == 1
    assert lib.fsnp_spec_stream_get_state(None, 0, None, None) == 1
    assert lib.fsnp_spec_stream_set_state(None, 0, None, None) == 1
    v = ctypes.c_int64()
    assert lib.fsnp_spec_stream_frames(None, 0, ctypes.byref(v)) == 1
    assert lib.fsnp_spec_stream_state_bytes(None) == 0
    lib.fsnp_spec_stream_destroy(None)


def test_models_that_cannot_stream_spectra_say_why_without_a_gpu():
    with pytest.raises(NotImplementedError, match="not causal"):
        FullSubNet_Plus(**DEFAULT_MODEL_ARGS).open_spec_stream(4)
    with pytest.raises(NotImplementedError, match="whole clip's total"):
        FullSubNet(**dict(FULLSUBNET_MODEL_ARGS, norm_type="offline_laplace_norm")).open_spec_stream(4)
    with pytest.raises(NotImplementedError, match="whole clip's total"):
        FullSubNet(**dict(FULLSUBNET_MODEL_ARGS, norm_type="offline_gaussian_norm")).open_spec_stream(1, live=True)
    with pytest.raises(NotImplementedError, match="GRU"):
        FullSubNet(**dict(FULLSUBNET_MODEL_ARGS, norm_type="cumulative_laplace_norm", sequence_model="GRU")).open_spec_stream(4)
    with pytest.raises(NotImplementedError, match="row-tile kernel"):
        FullSubNet(**dict(FULLSUBNET_MODEL_ARGS, norm_type="cumulative_laplace_norm", sb_model_hidden_size=320)).open_spec_stream(4)
    m = FullSubNet(**dict(FULLSUBNET_MODEL_ARGS, norm_type="cumulative_laplace_norm"))
    m.output_size = 3
    with pytest.raises(NotImplementedError, match="output_size = 2"):
        m.open_spec_stream(4)


T = 23


def _schedules(la):
    """seven ways to cut T frames; every one is padded with an idle push so that c = 0 is always among them"""
    def by(c):
        return [c] * (T // c) + ([T % c] if T % c else [])
    return {"all at once": [T], "one frame per push": by(1), "c < look_ahead": by(max(la - 1, 1)), "c = look_ahead": by(max(la, 1)),
            "c = look_ahead + 1": by(la + 1), "mixed with idle pushes": [1, 0, 5, 1, 1, 0, 12, 3], "random": random_schedule(T, 11 + la, 9)}


@pytest.mark.parametrize("norm_type", ["cumulative_laplace_norm", "cumulative_layer_norm"])
@pytest.mark.parametrize("look_ahead", [0, 1, 2, 4])
def test_chunked_spec_restatement_equals_the_whole_clip_oracle(norm_type, look_ahead):
    """The contract, independent of the GPU: a clip of noisy spectra pushed in any chunking (shorter than, as long as and longer than the
    ring of waiting frames; idle pushes), then look_ahead zero frames, is [look_ahead columns of exactly 0 | apply_cirm(whole-clip mask,
    clip)].  fp64: this pins which noisy frame meets which mask, not fp32 summation order."""
    args = dict(FULLSUBNET_MODEL_ARGS, norm_type=norm_type, look_ahead=look_ahead)
    sd = {k: v.double() for k, v in make_state_dict_fullsubnet(5, "default").items()}
    kw = stream_kwargs(args)
    X = spec_clip(1, T, 17).to(torch.complex128)
    want = oracle_enhance(sd, X, **kw)
    assert want.shape == X.shape and want.dtype == torch.complex128
    ts = TorchSpecStream(sd, **kw)
    scheds = _schedules(look_ahead)
    assert len(scheds) == 7
    worst = 0.0
    for name, chunks in scheds.items():
        assert sum(chunks) == T, (name, chunks)
        ts.reset()
        cols, pos = [], 0
        for c in chunks + [0]:
            o = ts.push(X[..., pos:pos + c])
            assert o.shape == (1, X.shape[1], c)
            cols.append(o)
            pos += c
            assert len(ts.waiting) == min(pos, look_ahead)
        cols.append(ts.tail())
        got = torch.cat(cols, dim=-1)
        assert got.shape[-1] == T + look_ahead and ts.P == T + look_ahead
        assert torch.count_nonzero(got[..., :look_ahead]) == 0, name
        err = crel_err(got[..., look_ahead:], want)
        worst = max(worst, err)
        assert err < 1e-10, (name, err)
    print(f"{norm_type} look_ahead={look_ahead}: worst rel err of the chunked spectrum restatement {worst:.3e}")

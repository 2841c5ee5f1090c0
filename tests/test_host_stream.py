"""Host-side checks of the streaming surface (include/fsnp_stream.h, fullsubnet_plus_amd/stream.py), on the cross-compiled library,
and the contract itself restated in torch-CPU fp64 against the oracle's whole-clip forward."""
import ctypes
import os
import re

import pytest
import torch

from fullsubnet_plus_amd import FullSubNet, FullSubNet_Plus, _lib
from oracle import fsnp_torch
from oracle.make_golden import make_spec
from oracle.ref_loader import DEFAULT_MODEL_ARGS, FULLSUBNET_MODEL_ARGS
from oracle.weights import make_state_dict_fullsubnet
from tests._stream_util import TorchStream, chunked, stream_kwargs
from tests._util import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_header_declares_exactly_the_stream_symbols():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "fsnp_stream.h")).read()
    declared = set(re.findall(r"^(?:int|void|int64_t) (fsnp_[a-z0-9_]+)\s*\(", header, flags=re.M))
    assert declared == set(_lib.STREAM_SYMBOLS) and len(declared) == 8, declared ^ set(_lib.STREAM_SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name
    assert not set(_lib.STREAM_SYMBOLS) & set(_lib.SYMBOLS)
    core = open(os.path.join(ROOT, "include", "fsnp.h")).read()
    assert '#include "fsnp_stream.h"' in core
    assert lib.fsnp_abi_version() == 13 == _lib.ABI_VERSION
    assert lib.fsnp_config_size() == ctypes.sizeof(_lib.FsnpConfig) == 76


def test_null_arguments_give_code_1():
    lib = _lib.load()
    sp = ctypes.c_void_p()
    assert lib.fsnp_stream_create(None, 1, 1, ctypes.byref(sp)) == 1 and "null" in _lib.last_error()
    st = (ctypes.c_int64 * 3)()
    assert lib.fsnp_stream_push(None, None, ctypes.byref(st), None, None, 1, None) == 1 and "null" in _lib.last_error()
    assert lib.fsnp_stream_reset(None, None, 0, None) == 1
    assert lib.fsnp_stream_get_state(None, 0, None, None) == 1
    assert lib.fsnp_stream_set_state(None, 0, None, None) == 1
    v = ctypes.c_int64()
    assert lib.fsnp_stream_frames(None, 0, ctypes.byref(v)) == 1
    assert lib.fsnp_stream_state_bytes(None) == 0
    lib.fsnp_stream_destroy(None)


@pytest.mark.parametrize("norm_type", ["cumulative_laplace_norm", "cumulative_layer_norm"])
@pytest.mark.parametrize("look_ahead", [0, 2, 4])
def test_chunked_restatement_equals_the_whole_clip_oracle(norm_type, look_ahead):
    """The contract, independent of the GPU: a clip pushed in chunks (chunks of 1, idle pushes, one long chunk), then look_ahead zero frames,
    is - after dropping the first look_ahead columns, which must be exactly 0 - the oracle's whole-clip mask.  fp64: this pins the delay, the
    warm-up zeros and the carried state, not fp32 summation order."""
    args = dict(FULLSUBNET_MODEL_ARGS, norm_type=norm_type, look_ahead=look_ahead)
    sd = {k: v.double() for k, v in make_state_dict_fullsubnet(5, "default").items()}
    T = 23
    mag = make_spec(1, T, 17)[0].double()
    kw = stream_kwargs(args)
    want = fsnp_torch.forward_fullsubnet_full(sd, mag, **kw)
    ts = TorchStream(sd, **kw)
    cols = []
    for s, c in chunked(T, [1, 0, 5, 1, 1, 0, 12, 3]):
        o = ts.push(mag[..., s:s + c])
        assert o.shape == (1, 2, mag.shape[2], c)
        cols.append(o)
    cols.append(ts.push(torch.zeros(1, 1, mag.shape[2], look_ahead, dtype=torch.float64)))
    got = torch.cat(cols, dim=-1)
    assert got.shape[-1] == T + look_ahead and ts.P == T + look_ahead
    assert torch.all(got[..., :look_ahead] == 0)
    err = rel_err(got[..., look_ahead:].numpy(), want.numpy())
    print(f"{norm_type} look_ahead={look_ahead}: rel err of the chunked restatement {err:.3e}")
    assert err < 1e-9, err


def test_models_that_cannot_be_streamed_say_why_without_a_gpu():
    with pytest.raises(NotImplementedError, match="not causal"):
        FullSubNet_Plus(**DEFAULT_MODEL_ARGS).open_stream(4)
    with pytest.raises(NotImplementedError, match="whole clip's total"):
        FullSubNet(**dict(FULLSUBNET_MODEL_ARGS, norm_type="offline_laplace_norm")).open_stream(4)
    with pytest.raises(NotImplementedError, match="GRU"):
        FullSubNet(**dict(FULLSUBNET_MODEL_ARGS, norm_type="cumulative_laplace_norm", sequence_model="GRU")).open_stream(4)
    with pytest.raises(NotImplementedError, match="row-tile kernel"):
        FullSubNet(**dict(FULLSUBNET_MODEL_ARGS, norm_type="cumulative_laplace_norm", sb_model_hidden_size=320)).open_stream(4)

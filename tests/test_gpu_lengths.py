"""GPU tests of batches of clips of different lengths (fsnp_forward_lengths, include/fsnp_lengths.h).

Row b of a batch with lengths[b] must be, at frames [0, lengths[b]), what the reference's B = 1 forward returns for that clip alone
(x[b:b+1, ..., :lengths[b]]), and exactly 0 past it; what the input holds past lengths[b] (here: garbage and NaN) must never matter.
The expected values come from the real reference's golden vectors and from the oracle (oracle/fsnp_torch.py) run per trimmed clip.
"""
import os
import re
import time

import numpy as np
import pytest
import torch

from fullsubnet_plus_amd import FullSubNet, FullSubNet_Plus, _lib
from oracle import fsnp_torch
from oracle.make_golden import make_spec
from oracle.ref_loader import DEFAULT_MODEL_ARGS
from oracle.weights import make_inputs, make_state_dict
from fullsubnet_plus_amd.synthetic import FULLSUBNET_MODEL_ARGS, make_state_dict_fullsubnet, make_wave
from tests._util import Golden, check_rows, garbage_tails, oracle_kwargs, oracle_rows, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-3                   # the suite's golden / oracle tolerance (tests/test_gpu_parity.py)
BF16_FORWARD_TOL = 4e-3      # whole forward under bf16_ih vs fp32 (tests/test_gpu_parity.py)

torch.set_num_threads(min(16, os.cpu_count() or 1))


def _model(args, sd, cls=FullSubNet_Plus):
    m = cls(**args)
    m.load_state_dict(sd, strict=True)
    m = m.to("cuda").eval()
    m.batch_mode = "full"
    return m


def _cuda(t):
    g = torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device="cuda")
    g.copy_(t)
    return g


# ------------------------------------------------------------------------------------------------ 1. the real reference
def test_ragged_pair_matches_reference_golden():
    """A 2 s and a 10 s clip of the golden fixtures in ONE batch: each row equals the reference's own B = 1 output."""
    g2, g10 = Golden("b1_2s_default"), Golden("b1_10s_default")
    assert g2.args == g10.args and g2.meta["wseed"] == g10.meta["wseed"] == 0
    short, long_ = g2.inputs(), g10.inputs()
    T2, T = short[0].shape[-1], long_[0].shape[-1]
    assert (T2, T) == (126, 626)
    ins = []
    for a, b in zip(short, long_):
        x = torch.full((2, 1, a.shape[2], T), float("nan"), dtype=torch.float32)
        x[0, :, :, :T2] = a[0]
        x[1] = b[0]
        ins.append(x.cuda())
    m = _model(g2.args, g2.state_dict())
    out = m(*ins, lengths=[T2, T]).cpu()
    assert not torch.isnan(out).any()
    assert torch.count_nonzero(out[0, :, :, T2:]) == 0
    e0 = rel_err(out[0:1, :, ::g2.sub, :T2].numpy(), g2.arrays["out"])
    e1 = rel_err(out[1:2, :, ::g10.sub, :].numpy(), g10.arrays["out"])
    assert e0 < TOL and e1 < TOL, (e0, e1)


# ------------------------------------------------------------------------------------------------ 2. the oracle, config by config
CONFIGS = [
    ("default", {}, {}),
    ("SE", {"channel_attention_model": "SE"}, {"attention": "SE"}),
    ("ECA", {"channel_attention_model": "ECA"}, {"attention": "ECA"}),
    ("CBAM", {"channel_attention_model": "CBAM"}, {"attention": "CBAM"}),
    ("gaussian", {"norm_type": "offline_gaussian_norm"}, {}),
    ("cum_laplace", {"norm_type": "cumulative_laplace_norm"}, {}),
    ("cum_layer", {"norm_type": "cumulative_layer_norm"}, {}),
    ("GRU", {"sequence_model": "GRU"}, {"sequence_model": "GRU"}),
    ("la0", {"look_ahead": 0}, {}),
    ("la4", {"look_ahead": 4}, {}),
    ("k247", {"kersize": [2, 4, 7]}, {"kersize": (2, 4, 7)}),
    ("h256", {"sb_model_hidden_size": 256}, {"sb_hidden": 256}),
    ("h320_runtime_sized", {"sb_model_hidden_size": 320}, {"sb_hidden": 320}),
    ("bf16_ih", {}, {}),
]


def _lengths_for(args, T):
    la = args["look_ahead"]
    kmax = max(args["kersize"]) if args.get("channel_attention_model", "TSSE") == "TSSE" else 1
    shortest = max(1, kmax - la)                      # TSSE: exactly the smallest clip the valid convs accept
    return [T, 1 + max(kmax - la, 0), T // 2, max(3, shortest), T - 1] if kmax > 1 else [T, 1, T // 2, 3, T - 1]


@pytest.mark.parametrize("name,over,sd_kw", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_ragged_rows_match_oracle(name, over, sd_kw):
    args = dict(DEFAULT_MODEL_ARGS, **over)
    sd = make_state_dict(3, "default", **sd_kw)
    T = 37
    lengths = _lengths_for(args, T)
    if name == "k247":
        assert min(lengths) + args["look_ahead"] == 7
    mag, real, imag = make_spec(5, T, 40 + len(name))
    ins = garbage_tails((mag, real, imag), lengths, 7)
    m = _model(args, sd)
    tol = TOL
    if name == "bf16_ih":
        m.set_precision("bf16_ih")
        tol = BF16_FORWARD_TOL
    got = m(*[t.cuda() for t in ins], lengths=lengths).cpu()
    kw = oracle_kwargs(args)
    want = [fsnp_torch.forward_full(sd, mag[b:b + 1, :, :, :n], real[b:b + 1, :, :, :n], imag[b:b + 1, :, :, :n], **kw)
            for b, n in enumerate(lengths)]
    check_rows(got, want, lengths, tol)
    if name == "default":
        # the complex-input path (fsnp_forward_complex_lengths), NaN past the lengths of the interleaved buffer too
        X = torch.complex(ins[1][:, 0], ins[2][:, 0])
        gotc = m.forward_complex(X.cuda(), lengths=torch.tensor(lengths, dtype=torch.int64)).cpu()
        check_rows(gotc, want, lengths, tol)


def test_ragged_fullsubnet_matches_oracle():
    """The original FullSubNet: its full-band LSTM is causal, only its two norms need the lengths."""
    sd = make_state_dict_fullsubnet(4, "default")
    args = dict(FULLSUBNET_MODEL_ARGS)
    T = 33
    lengths = [T, 9, T // 2, 1, T - 1]
    mag, _, _ = make_spec(5, T, 77)
    (ins,) = garbage_tails((mag,), lengths, 8)
    m = _model(args, sd, FullSubNet)
    got = m(ins.cuda(), lengths=lengths).cpu()
    kw = {k: args[k] for k in ("look_ahead", "sb_num_neighbors", "fb_num_neighbors", "norm_type", "num_groups_in_drop_band",
                               "fb_output_activate_function", "sb_output_activate_function")}
    want = [fsnp_torch.forward_fullsubnet_full(sd, mag[b:b + 1, :, :, :n], **kw) for b, n in enumerate(lengths)]
    check_rows(got, want, lengths, TOL)


# ------------------------------------------------------------------------------------------------ 3. bit identity
@pytest.mark.parametrize("B", [1, 8, 32, 64])
def test_full_lengths_are_bit_identical_to_the_plain_forward(B):
    sd = make_state_dict(0, "default")
    m = _model(DEFAULT_MODEL_ARGS, sd)
    ins = [_cuda(t) for t in make_inputs(B, 2.0, 60 + B)]
    T = ins[0].shape[-1]
    plain = m(*ins)
    ragged = m(*ins, lengths=[T] * B)
    assert torch.equal(plain, ragged)


def test_other_rows_do_not_change_a_row():
    sd = make_state_dict(0, "default")
    m = _model(DEFAULT_MODEL_ARGS, sd)
    T, lengths = 90, [50, 90, 17, 64]
    a = garbage_tails(make_spec(4, T, 5), lengths, 1)
    b = garbage_tails(make_spec(4, T, 6), lengths, 2)
    for t_a, t_b in zip(a, b):
        t_b[0] = t_a[0]
        t_b[0, :, :, lengths[0]:] = -3.0                  # row 0's own padding differs too
    out_a = m(*[t.cuda() for t in a], lengths=lengths).cpu()
    out_b = m(*[t.cuda() for t in b], lengths=lengths).cpu()
    assert torch.equal(out_a[0], out_b[0])
    assert not torch.equal(out_a[1], out_b[1])


# ------------------------------------------------------------------------------------------------ 4. a mixed-length serving batch
def _serving_batch(B=32, seed=11):
    rng = np.random.default_rng(seed)
    mag, real, imag = make_inputs(B, 10.0, seed)
    T = mag.shape[-1]
    lengths = sorted(int(v) for v in rng.integers(1 + 16000 // 256, T + 1, size=B))   # 1 ... 10 s
    lengths[-1] = T
    return (mag, real, imag), lengths


def _ws_bytes(m):
    return int(re.search(r"workspace=(\d+) bytes", m.dump_config()).group(1))


def test_mixed_length_batch_of_32():
    (mag, real, imag), lengths = _serving_batch()
    ins = garbage_tails((mag, real, imag), lengths, 3)
    sd = make_state_dict(0, "default")
    m = _model(DEFAULT_MODEL_ARGS, sd)
    gins = [t.cuda() for t in ins]
    got = m(*gins, lengths=lengths).cpu()
    # every row against the oracle (a row-indexing slip in one kernel shows in some rows only)
    want = oracle_rows(lambda *x: fsnp_torch.forward_full(sd, *x), (mag, real, imag), lengths)
    check_rows(got, want, lengths, TOL)
    # the pipelined loop: deferred chunks and their tail zeroing on the side stream, bit-identical to the plain call
    p = _model(DEFAULT_MODEL_ARGS, sd)
    p.set_pipeline(True)
    outs = [p(*gins, lengths=lengths) for _ in range(3)]
    p.flush()
    for o in outs:
        assert torch.equal(o.cpu(), got)
    # the verification pass re-runs the column-split launches and compares BEFORE the tails are zeroed: no code 7
    v = _model(DEFAULT_MODEL_ARGS, sd)
    v.set_verify(1)
    for _ in range(2):
        assert torch.equal(v(*gins, lengths=lengths).cpu(), got)
    v.check_errors()
    assert v.verify_count() > 0


def _sleep_cycles_for(seconds):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    torch.cuda._sleep(20_000_000)
    torch.cuda.synchronize()
    return int(seconds / ((time.perf_counter() - t0) / 20_000_000))


def test_ragged_calls_after_reserve_never_synchronise():
    (mag, real, imag), lengths = _serving_batch(seed=12)
    sd = make_state_dict(0, "default")
    m = _model(DEFAULT_MODEL_ARGS, sd)
    m.error_check = "deferred"
    short = [_cuda(t) for t in make_inputs(2, 2.0, 5)]
    m(*short, lengths=[126, 100])                          # creates the handle
    m.reserve(32, 626)
    torch.cuda.synchronize()
    ws = _ws_bytes(m)
    gins = [_cuda(t) for t in (mag, real, imag)]
    ticks = _sleep_cycles_for(1.5)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        torch.cuda._sleep(ticks)
    t0 = time.perf_counter()
    lens = list(lengths)
    a = m(*gins, lengths=lens)
    lens[0] = 5                                            # the caller may reuse its buffer as soon as the call returns
    b = m(*gins, lengths=lengths)
    host_s = time.perf_counter() - t0
    still_running = not side.query()
    torch.cuda.synchronize()
    m.check_errors()
    assert still_running and host_s < 0.5, (still_running, host_s)
    assert _ws_bytes(m) == ws
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 5. the waveform path
def test_enhance_wave_lengths_matches_oracle_per_clip():
    sd = make_state_dict(41, "harsh")
    m = _model(DEFAULT_MODEL_ARGS, sd)
    samples = [16000 + 77, 9000 + 13, 12345]
    L = max(samples)
    wav = torch.from_numpy(make_wave(3, L / 16000, 501))
    assert wav.shape[1] == L
    padded = wav.clone()
    for b, n in enumerate(samples):
        padded[b, n:] = 1e3                                # garbage past each clip: never reflected into it
    got = m.enhance_wave(padded.cuda(), lengths=samples).cpu()
    for b, n in enumerate(samples):
        want = fsnp_torch.enhance_wave(sd, wav[b:b + 1, :n])
        assert rel_err(got[b:b + 1, :n].numpy(), want.numpy()) < TOL, b
        assert torch.count_nonzero(got[b, n:]) == 0


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals():
    sd = make_state_dict(0, "default")
    m = _model(DEFAULT_MODEL_ARGS, sd)
    mag, real, imag = [t.cuda() for t in make_spec(3, 20, 9)]
    ok = m(mag, real, imag, lengths=[20, 12, 8])
    for bad, what in (([20, 0, 8], "utterance 1"), ([20, 21, 8], "utterance 1"), ([20, 12, 7], "utterance 2")):
        with pytest.raises(_lib.FsnpError, match=what) as e:
            m(mag, real, imag, lengths=bad)
        assert e.value.code == 2
    with pytest.raises(ValueError, match="CPU"):
        m(mag, real, imag, lengths=torch.tensor([20, 12, 8], device="cuda"))
    with pytest.raises(ValueError, match="batch_offset"):
        m(mag, real, imag, batch_offset=0, global_batch=3, lengths=[20, 12, 8])
    m.batch_mode = "parity"
    with pytest.raises(ValueError, match='batch_mode = "full"'):
        m(mag, real, imag, lengths=[20, 12, 8])
    m.batch_mode = "full"
    assert torch.equal(m(mag, real, imag, lengths=[20, 12, 8]), ok)      # nothing of the refused calls was left behind
    m.check_errors()
    eca2 = _model(dict(DEFAULT_MODEL_ARGS, channel_attention_model="ECA", subband_num=2), make_state_dict(0, "default", attention="ECA"))
    with pytest.raises(_lib.FsnpError, match="subband_num"):
        eca2(mag, real, imag, lengths=[20, 12, 8])
    tcn = _model(dict(DEFAULT_MODEL_ARGS, sequence_model="TCN"), make_state_dict(0, "default", sequence_model="TCN"))
    with pytest.raises(_lib.FsnpError, match="TCN"):
        tcn(mag, real, imag, lengths=[20, 12, 8])

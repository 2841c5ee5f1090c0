"""GPU tests of batches of clips of different lengths at the places such code goes wrong: a per-utterance frame count
(lengths[b] + look_ahead) compared against a row index inside a tile, a sub-tile or a workgroup's slice of frames.

Every length comes from tests/_util.py edge_lengths: L + look_ahead one below, at and one above each multiple of 8 / 32 / 64 / 128 /
256 (/ 512) that fits, the shortest legal clip and the whole buffer.  Each test runs a pool of clips (one per length), cut into
batches of the size under test, and compares every row with the oracle (oracle/fsnp_torch.py) of that clip alone, computed once
per pool: the clip's frames within tolerance, exactly 0 past it, no NaN anywhere although the input past each length holds huge
values and NaN.  Every test also asserts which kernel or mode it ran, so it cannot pass on a path it did not take.
"""
import os

import numpy as np
import pytest
import torch

from fullsubnet_plus_amd import FullSubNet, FullSubNet_Plus
from fullsubnet_plus_amd.synthetic import FULLSUBNET_MODEL_ARGS, make_state_dict_fullsubnet, make_wave
from oracle import fsnp_torch
from oracle.make_golden import make_spec
from oracle.ref_loader import DEFAULT_MODEL_ARGS
from oracle.weights import make_inputs, make_state_dict
from tests._util import (check_rows, edge_lengths, fullsubnet_oracle_kwargs, garbage_tails, oracle_kwargs, oracle_rows,
                         rel_err)

pytestmark = pytest.mark.gpu
TOL = 1e-3                   # the suite's golden / oracle tolerance (tests/test_gpu_parity.py)
HOP = 256                    # n_fft / 2 of the default 257-bin STFT

torch.set_num_threads(min(16, os.cpu_count() or 1))


def _model(args, sd, cls=FullSubNet_Plus):
    m = cls(**args)
    m.load_state_dict(sd, strict=True)
    m = m.to("cuda").eval()
    m.batch_mode = "full"
    return m


def _batches(n_pool, B):
    """Pool indices cut into batches of B; the last batch is filled up from the start of the pool."""
    return [[(k + i) % n_pool for i in range(B)] for k in range(0, n_pool, B)]


def _run_pool(m, pool, lengths, B, seed):
    """Run the pool (tensors [N, 1, F, T]) batch by batch with garbage past each length -> [N, ...] outputs (CPU)."""
    out = [None] * len(lengths)
    for k, idx in enumerate(_batches(len(lengths), B)):
        lens = [lengths[i] for i in idx]
        ins = garbage_tails([t[idx] for t in pool], lens, seed + k)
        got = m(*[t.cuda() for t in ins], lengths=lens).cpu()
        for j, i in enumerate(idx):
            if out[i] is None:
                out[i] = got[j:j + 1]
    return torch.cat(out)


def _plus_oracle(sd, args, pool, lengths):
    kw = oracle_kwargs(args)
    return oracle_rows(lambda *x: fsnp_torch.forward_full(sd, *x, **kw), pool, lengths)


def _fsn_oracle(sd, pool, lengths):
    kw = fullsubnet_oracle_kwargs(FULLSUBNET_MODEL_ARGS)
    return oracle_rows(lambda x: fsnp_torch.forward_fullsubnet_full(sd, x, **kw), pool, lengths)


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ 1. TCN GEMM kernels x edges
# (B, T, what mode 1 runs).  Split-K (tcn_gemm_sk_kernel) is chosen per GEMM while its 32-row tiles x column tiles x 3 branches fit
# 6 workgroups per CU: conv1x1 has 8 column tiles (CH = 512), the sconv and the final Linear 5 (F = 257).  3 x 300 frames: every GEMM
# split-K; 4 x 10 s: conv1x1 on the 128-row tcn_gemm_dma_kernel at a small batch, the others split-K; 32 x 3 s: no split-K at all,
# conv1x1 / Linear on the 128-row kernel, launch_gemm_dma64 takes the sconv GEMMs.  Mode 2 = mode 1 without split-K, mode 3 = the
# 128-row kernel for the sconv GEMMs too.
GEMM_SHAPES = [(3, 300, "splitk"), (4, 626, "rows128"), (32, 188, "rows64")]


@pytest.mark.parametrize("B,T,path", GEMM_SHAPES, ids=[f"B{b}_T{t}_{p}" for b, t, p in GEMM_SHAPES])
def test_tcn_gemm_modes_on_ragged_batches(B, T, path):
    """csrc/tcn.hip launch_gemm_dma: debug modes 0 (the general tcn_gemm_kernel: PRO_GN prologue, t_stats in EPI_PRELU_STATS),
    1 (default), 2 (no split-K) and 3 (the 128-row kernel for every GEMM) on ragged batches; the same cost formulas as
    tests/test_gpu_parity.py test_dma_gemm_equals_general_gemm say which modes must differ."""
    args = dict(DEFAULT_MODEL_ARGS)
    la = args["look_ahead"]
    sd = make_state_dict(21, "default")
    lengths = edge_lengths(T, la, max(args["kersize"]) - la)
    if len(lengths) < B:
        lengths = [lengths[i % len(lengths)] for i in range(B)]
    if T >= 300:      # the shortest clip leaves two or more whole 128-row tiles of its plane unused
        assert _cdiv(T + la, 128) - _cdiv(min(lengths) + la, 128) >= 2
    pool = make_spec(len(lengths), T, 500 + B)
    want = _plus_oracle(sd, args, pool, lengths)
    m = _model(args, sd)
    outs, errs = {}, {}
    for mode in (1, 0, 2, 3):
        m.debug_set_gemm_dma(mode)
        outs[mode] = _run_pool(m, pool, lengths, B, 9)
        errs[mode] = max(check_rows(outs[mode], want, lengths, TOL))
    m.debug_set_gemm_dma(1)
    m.check_errors()
    Tp = T + la
    splitk_ch, splitk_f = (nt * _cdiv(Tp, 32) * B * 3 <= 6 * 256 for nt in (8, 5))
    cost64, cost128 = _cdiv(4 * _cdiv(Tp, 64) * B * 3, 256), 2 * _cdiv(5 * _cdiv(Tp, 128) * B * 3, 256)
    assert (splitk_ch, splitk_f) == {"splitk": (True, True), "rows128": (False, True), "rows64": (False, False)}[path]
    assert cost64 <= cost128, (cost64, cost128)
    o = {k: v.numpy() for k, v in outs.items()}
    assert not np.array_equal(o[0], o[1])                          # the general kernel really ran in mode 0
    assert np.array_equal(o[1], o[2]) != splitk_f                  # mode 2 differs exactly where mode 1 ran split-K
    assert not np.array_equal(o[2], o[3])                          # mode 2 ran the 64-row sconv kernel, mode 3 the 128-row one
    for a in (0, 2, 3):
        assert rel_err(o[a], o[1]) < 1e-4, (a, rel_err(o[a], o[1]))
    print(f"gemm B{B} T{T}: worst rel_err per mode {errs}")


# ------------------------------------------------------------------------------------------------ 2. grids that depend on B
@pytest.mark.parametrize("norm", ["offline_laplace_norm", "offline_gaussian_norm", "cumulative_layer_norm"])
def test_norms_on_every_batch_grid(norm):
    """fe_fsum_kernel (4 / 8 / 16 / 32 rows per workgroup at B = 1 / 2-3 / 4-7 / >= 8) and sb_offline_stats_kernel (2 / 4 / 8 / 16):
    one pool of clips on a 300-frame buffer, run at B = 1, 2, 3, 4, 7, 8, 9 - B = 1 with every length, most of them shorter than
    the buffer.  The outputs of one clip must agree across batch sizes too (per-utterance semantics)."""
    args = dict(DEFAULT_MODEL_ARGS, norm_type=norm)
    la = args["look_ahead"]
    sd = make_state_dict(5, "default")
    T = 300
    lengths = edge_lengths(T, la, max(args["kersize"]) - la)
    assert min(lengths) < T and len(lengths) >= 9
    pool = make_spec(len(lengths), T, 600)
    want = _plus_oracle(sd, args, pool, lengths)
    m = _model(args, sd)
    first, worst = None, 0.0
    for B in (1, 2, 3, 4, 7, 8, 9):
        got = _run_pool(m, pool, lengths, B, 20 + B)
        worst = max(worst, max(check_rows(got, want, lengths, TOL)))
        if first is None:
            first = got
        else:
            assert rel_err(got.numpy(), first.numpy()) < 1e-4, B
    m.check_errors()
    print(f"norm {norm}: worst rel_err {worst:.2e}")


# ------------------------------------------------------------------------------------------------ 3. attention pooling at long T
@pytest.mark.parametrize("att", ["SE", "ECA", "CBAM"])
def test_attention_pooling_at_10s(att):
    """SE / ECA / CBAM pool over each clip's own frames (CBAM's max over time must skip the garbage tails) at T = 626, B = 4: lengths
    across 255 / 256 / 257 frames, and length 1."""
    args = dict(DEFAULT_MODEL_ARGS, channel_attention_model=att)
    assert args["channel_attention_model"] != "TSSE"
    sd = make_state_dict(7, "default", attention=att)
    T = 626
    lengths = edge_lengths(T, args["look_ahead"], 1, edges=(8, 64, 256), extra=(255, 256, 257))
    assert {1, 255, 256, 257, T} <= set(lengths)
    pool = make_spec(len(lengths), T, 700 + len(att))
    want = _plus_oracle(sd, args, pool, lengths)
    m = _model(args, sd)
    got = _run_pool(m, pool, lengths, 4, 31)
    m.check_errors()
    print(f"attention {att}: worst rel_err {max(check_rows(got, want, lengths, TOL)):.2e}")


# ------------------------------------------------------------------------------------------------ 4. the original FullSubNet
FSN_T = 700


@pytest.fixture(scope="module")
def fsn_pool():
    """~700-frame clips whose lengths cross the 256-frame chunks of fe_scan_kernel's non-cumulative branch, and their oracle."""
    sd = make_state_dict_fullsubnet(4, "default")
    lengths = edge_lengths(FSN_T, FULLSUBNET_MODEL_ARGS["look_ahead"], 1, edges=(8, 32, 128, 256, 512))
    (mag,) = make_spec(len(lengths), FSN_T, 88)[:1]
    return sd, lengths, mag, _fsn_oracle(sd, (mag,), lengths)


@pytest.mark.parametrize("B", [1, 3, 4, 5, 40])
def test_fullsubnet_ragged_batches(B, fsn_pool):
    """B <= 4 runs the full-band LSTM on the VALU (csrc/lstm_fbv.hip): its output must be close to, but not bit-equal to, the K-split
    MFMA kernel's (debug_set_lstm_coop(2)) on each clip's frames - the other kernel really ran.  B = 5 and 40 run the MFMA plans."""
    sd, lengths, mag, want = fsn_pool
    m = _model(dict(FULLSUBNET_MODEL_ARGS), sd, FullSubNet)
    got = _run_pool(m, (mag,), lengths, B, 40 + B)
    m.check_errors()
    errs = check_rows(got, want, lengths, TOL)
    if B <= 4:
        idx = _batches(len(lengths), B)[-1]
        lens = [lengths[i] for i in idx]
        (x,) = garbage_tails([mag[idx]], lens, 3)
        x = x.cuda()
        out = m(x, lengths=lens)
        fb_valu = m.read_stage("fb_mag", B, FSN_T).numpy()
        m.debug_set_lstm_coop(2)
        ref = m(x, lengths=lens)
        fb_mfma = m.read_stage("fb_mag", B, FSN_T).numpy()
        m.debug_set_lstm_coop(1)
        m.check_errors()
        la = FULLSUBNET_MODEL_ARGS["look_ahead"]
        for j, n in enumerate(lens):
            a, b = fb_valu[j, :n + la], fb_mfma[j, :n + la]
            assert rel_err(a, b) < 1e-5, (j, n, rel_err(a, b))
        assert not np.array_equal(np.concatenate([fb_valu[j, :n + la] for j, n in enumerate(lens)]),
                                  np.concatenate([fb_mfma[j, :n + la] for j, n in enumerate(lens)]))
        assert rel_err(out.cpu().numpy(), ref.cpu().numpy()) < 1e-5
    print(f"fullsubnet B{B}: worst rel_err {max(errs):.2e}")


def test_fullsubnet_pipelined_ragged_loop_is_bit_identical(fsn_pool):
    """set_pipeline(True) ... flush() at B = 32 with lengths: the deferred remainder chunk and its tail zeroing on the side stream."""
    sd, lengths, mag, want = fsn_pool
    idx = _batches(len(lengths), 32)[0]
    lens = [lengths[i] for i in idx]
    (x,) = garbage_tails([mag[idx]], lens, 5)
    x = x.cuda()
    m = _model(dict(FULLSUBNET_MODEL_ARGS), sd, FullSubNet)
    plain = m(x, lengths=lens).cpu()
    check_rows(plain, [want[i] for i in idx], lens, TOL)
    p = _model(dict(FULLSUBNET_MODEL_ARGS), sd, FullSubNet)
    p.set_pipeline(True)
    outs = [p(x, lengths=lens) for _ in range(3)]
    p.flush()
    p.check_errors()
    for o in outs:
        assert torch.equal(o.cpu(), plain)


# ------------------------------------------------------------------------------------------------ 5. more than 256 utterances
def _lengths_300(T, la, min_len, edges):
    """300 lengths cycling through the edge set, with rows 255 / 256 / 257 (the last row of the first 256-row launch and the first two
    of the second) set to three different lengths that no neighbour has."""
    base = edge_lengths(T, la, min_len, edges=edges)
    assert len(base) >= 5
    lengths = [base[i % len(base)] for i in range(300)]
    lengths[255], lengths[256], lengths[257] = base[1], base[-1], base[2]
    lengths[254], lengths[258] = base[0], base[0]
    return lengths


def test_plus_300_utterances():
    """launch_set_lengths passes 256 rows per launch (kLengthsPerLaunch): rows 256 ... 299 come from the second launch."""
    args = dict(DEFAULT_MODEL_ARGS)
    la = args["look_ahead"]
    sd = make_state_dict(3, "default")
    T = 24
    lengths = _lengths_300(T, la, max(args["kersize"]) - la, (8, 16, 24))
    pool = make_spec(300, T, 901)
    want = _plus_oracle(sd, args, pool, lengths)
    m = _model(args, sd)
    ins = garbage_tails(pool, lengths, 77)
    got = m(*[t.cuda() for t in ins], lengths=lengths).cpu()
    m.check_errors()
    print(f"plus B300: worst rel_err {max(check_rows(got, want, lengths, TOL)):.2e}")


def test_fullsubnet_300_utterances():
    sd = make_state_dict_fullsubnet(9, "default")
    T = 24
    lengths = _lengths_300(T, FULLSUBNET_MODEL_ARGS["look_ahead"], 1, (8, 16, 24))
    (mag,) = make_spec(300, T, 902)[:1]
    want = _fsn_oracle(sd, (mag,), lengths)
    m = _model(dict(FULLSUBNET_MODEL_ARGS), sd, FullSubNet)
    (x,) = garbage_tails([mag], lengths, 78)
    got = m(x.cuda(), lengths=lengths).cpu()
    m.check_errors()
    print(f"fullsubnet B300: worst rel_err {max(check_rows(got, want, lengths, TOL)):.2e}")


# the waveform tests run FullSubNet+ with SE attention: TSSE needs clips of 8 frames or more (1 + samples / 256: 1,792 samples), SE
# takes any clip the STFT takes, down to 257 samples; the STFT path is the same for every attention type
WAVE_ARGS = dict(DEFAULT_MODEL_ARGS, channel_attention_model="SE")


def _wave_oracle(sd, wav, samples, fullsubnet=False):
    if fullsubnet:
        kw = dict(fullsubnet=True, **fullsubnet_oracle_kwargs(FULLSUBNET_MODEL_ARGS))
    else:
        kw = oracle_kwargs(WAVE_ARGS)
    return oracle_rows(lambda w: fsnp_torch.enhance_wave(sd, w, **kw), (wav,), samples)


def _nan_past(wav, samples):
    padded = wav.clone()
    for b, n in enumerate(samples):
        padded[b, n:] = float("nan")
    return padded


def test_enhance_wave_300_utterances():
    """launch_stft_pad / launch_istft_ola / the cIRM epilogue with lengths: 256 rows per launch, rows 256 ... 299 in the second."""
    sd = make_state_dict(41, "harsh", attention="SE")
    L = 4 * HOP + 1
    base = [HOP + 1, 2 * HOP - 1, 2 * HOP, 2 * HOP + 1, 3 * HOP, L]
    samples = [base[i % len(base)] for i in range(300)]
    samples[255], samples[256], samples[257] = base[1], base[-1], base[3]
    wav = torch.from_numpy(make_wave(300, L / 16000, 903))
    assert wav.shape[1] == L
    want = _wave_oracle(sd, wav, samples)
    m = _model(WAVE_ARGS, sd)
    got = m.enhance_wave(_nan_past(wav, samples).cuda(), lengths=samples).cpu()
    m.check_errors()
    print(f"enhance_wave B300: worst rel_err {max(check_rows(got, want, samples, TOL)):.2e}")


# ------------------------------------------------------------------------------------------------ 6. enhance(X, lengths=)
@pytest.mark.parametrize("model", ["plus", "fullsubnet"])
def test_enhance_lengths_with_nan_and_inf_past_each_clip(model):
    """The fused cIRM epilogue (fsnp_apply_cirm_lengths) with harsh weights (the +-9.9 clamp of decompress_cIRM is hit) and NaN / Inf
    in X past each length: row b equals apply_cirm(oracle mask of the clip, the clip) and is exactly 0 past it."""
    if model == "plus":
        args, sd, cls = dict(DEFAULT_MODEL_ARGS), make_state_dict(41, "harsh"), FullSubNet_Plus
        min_len = max(args["kersize"]) - args["look_ahead"]
    else:
        args, sd, cls = dict(FULLSUBNET_MODEL_ARGS), make_state_dict_fullsubnet(14, "harsh"), FullSubNet
        min_len = 1
    sd = dict(sd)
    sd["sb_model.fc_output_layer.weight"] = sd["sb_model.fc_output_layer.weight"] * (40 if model == "plus" else 10)   # beyond the clamp
    T = 130
    lengths = edge_lengths(T, args["look_ahead"], min_len, edges=(8, 32, 64, 128))
    mag, real, imag = make_inputs(len(lengths), (T - 1) * HOP / 16000, 950)
    assert mag.shape[-1] == T
    X = torch.complex(real[:, 0], imag[:, 0]).contiguous()
    if model == "plus":
        masks = _plus_oracle(sd, args, (mag, real, imag), lengths)
    else:
        masks = _fsn_oracle(sd, (mag,), lengths)
    want = [fsnp_torch.apply_cirm(masks[b], X[b:b + 1, :, :n]) for b, n in enumerate(lengths)]
    assert max(float(w.abs().max()) for w in masks) >= 9.9                  # the clamp is reached
    bad = X.clone()
    for b, n in enumerate(lengths):
        if n < T:
            bad[b, :, n:] = complex(float("nan"), float("inf"))
            bad[b, 1::2, n:] = complex(float("-inf"), 1e30)
    m = _model(args, sd, cls)
    got = m.enhance(bad.cuda(), lengths=lengths).cpu()
    m.check_errors()
    assert torch.isfinite(torch.view_as_real(got)).all()
    errs = check_rows(torch.view_as_real(got).permute(0, 3, 1, 2), [torch.view_as_real(w).permute(0, 3, 1, 2) for w in want],
                      lengths, TOL)
    print(f"enhance {model}: worst rel_err {max(errs):.2e}")


# ------------------------------------------------------------------------------------------------ 7. enhance_wave at STFT edges
@pytest.mark.parametrize("model", ["plus", "fullsubnet"])
def test_enhance_wave_lengths_at_stft_edges(model):
    """Sample counts at the reflection edge (257: the reflected index reaches 0), at multiples of the hop +- 1 and at the buffer
    (max), NaN past each clip: row b equals enhance_wave of the clip alone, 0 past it."""
    L = 64 * HOP + 3
    if model == "plus":
        sd, cls, args = make_state_dict(41, "harsh", attention="SE"), FullSubNet_Plus, WAVE_ARGS
        samples = [257, 258, 511, 512, 513, 767, 768, 769, 16000, 16383, 16384, 16385, L]
    else:
        sd, cls, args = make_state_dict_fullsubnet(13, "harsh"), FullSubNet, FULLSUBNET_MODEL_ARGS
        samples = [257, 511, 512, 769, 16384, L]
    wav = torch.from_numpy(make_wave(len(samples), L / 16000, 904))
    assert wav.shape[1] == L
    want = _wave_oracle(sd, wav, samples, fullsubnet=model == "fullsubnet")
    m = _model(dict(args), sd, cls)
    got = m.enhance_wave(_nan_past(wav, samples).cuda(), lengths=samples).cpu()
    m.check_errors()
    print(f"enhance_wave {model}: worst rel_err {max(check_rows(got, want, samples, TOL)):.2e}")

"""GPU tests of the windowed whole-clip call (include/ext/fsnp_windowed.h): enhance_wave_windowed against the float
restatement of its contract (tests/_windowed_util.py: oracle.fsnp_torch.enhance_wave per window, merged in float64), bit identity with
enhance_wave where no clip needs a second window, the PCM formats, the round-trip hook on both row-chunk edges and past 2^31 elements,
and the refusals of the C entry point.

Default geometry (n_fft 512, hop 256); W = 4096, V = 1024 (17 frames per full window) unless stated.

The ragged batches run on a FullSubNet+ with the "SE" attention.  With the default "TSSE" attention (kernel sizes 3, 5, 10, look_ahead 2)
a clip needs 8 frames - 1792 samples - in the reference and in the oracle alike (attention_model.py:86 fails inside Conv1d below that), so
the 700-sample clip and the 1025-sample last window of the 4097-sample clip, the smallest a last window can be at V = 1024, are no
input that model has an answer for; test_short_windows_follow_the_models_own_floor pins that refusal, and the TSSE model runs a ragged
batch whose windows it accepts."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from fullsubnet_plus_amd import FullSubNet, FullSubNet_Plus, _call, _lib, window_count
from fullsubnet_plus_amd.synthetic import DEFAULT_MODEL_ARGS, FULLSUBNET_MODEL_ARGS, make_state_dict_fullsubnet, make_wave
from oracle.weights import make_state_dict
from tests import _pcm_util
from tests._util import rel_err
from tests._windowed_util import oracle_windowed, window_plan

pytestmark = pytest.mark.gpu
TOL = 1e-3                   # the suite's golden / oracle tolerance (tests/test_gpu_lengths.py)
W, V = 4096, 1024
SE_ARGS = dict(DEFAULT_MODEL_ARGS, channel_attention_model="SE")
RAGGED = [10000, 4096, 4097, 700]          # K = 3, 1, 2, 1; windows of 4096, 4096, 1808 | 4096 | 4096, 1025 | 700 samples


def _build(cls, args, sd):
    m = cls(**args)
    m.load_state_dict(sd, strict=True)
    m = m.to("cuda").eval()
    m.batch_mode = "full"
    return m


@functools.lru_cache(maxsize=None)
def _plus():
    sd = make_state_dict(41, "harsh")
    return sd, _build(FullSubNet_Plus, DEFAULT_MODEL_ARGS, sd)


@functools.lru_cache(maxsize=None)
def _plus_se():
    sd = make_state_dict(41, "harsh", attention="SE")
    return sd, _build(FullSubNet_Plus, SE_ARGS, sd)


@functools.lru_cache(maxsize=None)
def _ragged_case():
    """The ragged batch, 1e3 written past each length, and each row's own oracle (computed once, shared by the tests below)."""
    sd, _ = _plus_se()
    wav = torch.from_numpy(make_wave(len(RAGGED), max(RAGGED) / 16000, 611))
    assert wav.shape[1] == max(RAGGED)
    padded = wav.clone()
    for b, n in enumerate(RAGGED):
        padded[b, n:] = 1e3
    want = [oracle_windowed(sd, wav[b, :n], W, V, channel_attention_model="SE") for b, n in enumerate(RAGGED)]
    return padded, want


def _check_rows(got, want, lengths, tol=TOL):
    got = got.cpu()
    assert not torch.isnan(got).any()
    errs = [rel_err(got[b, :n].numpy(), want[b]) for b, n in enumerate(lengths)]
    print("rel_err per row:", ["%.2e" % e for e in errs])
    for b, n in enumerate(lengths):
        assert torch.count_nonzero(got[b, n:]) == 0, f"row {b}: samples past its length {n} are not 0"
    assert max(errs) < tol, errs
    return errs


# ------------------------------------------------------------------------------------------------ 1. one clip, FullSubNet+
@pytest.mark.parametrize("overlap", [1024, 2048], ids=["v1024", "v2048_hann"])
def test_one_clip_of_three_windows_matches_oracle(overlap):
    """L = 10 000: at V = 1024 three windows, the last 3856 long; V = 2048 = W / 2 is the reference's Hann case (four windows)."""
    sd, m = _plus()
    L = 10000
    assert [n for _, n in window_plan(L, W, 1024)] == [4096, 4096, 3856] and window_count(L, W, overlap) == (3 if overlap == 1024 else 4)
    wav = torch.from_numpy(make_wave(1, L / 16000, 600))
    got = m.enhance_wave_windowed(wav.cuda(), W, overlap)
    assert got.shape == wav.shape and got.dtype == torch.float32
    _check_rows(got, [oracle_windowed(sd, wav[0], W, overlap)], [L])


# ------------------------------------------------------------------------------------------------ 2., 3. ragged batches
@pytest.mark.parametrize("max_batch", [32, 3, 1], ids=["one_forward", "forwards_of_3_3_1", "one_window_each"])
def test_ragged_batch_matches_each_rows_oracle(max_batch):
    """lengths = [10000, 4096, 4097, 700] in one forward of seven windows, in forwards of 3, 3 and 1 windows that cross the clips'
    boundaries, and one window at a time: every row against its own oracle, exact zeros past each length, whatever lies there."""
    _, m = _plus_se()
    padded, want = _ragged_case()
    assert [window_count(n, W, V) for n in RAGGED] == [3, 1, 2, 1] and window_plan(4097, W, V)[-1] == (3072, 1025)
    got = m.enhance_wave_windowed(padded.cuda(), W, V, lengths=RAGGED, max_batch=max_batch)
    _check_rows(got, want, RAGGED)


def test_ragged_batch_on_the_tsse_model():
    """The headline model on a ragged batch whose windows all have the 8 frames its attention needs (last windows of 1808, 1792, 1800)."""
    sd, m = _plus()
    lengths = [10000, 4096, 4864, 1800]
    wav = torch.from_numpy(make_wave(4, max(lengths) / 16000, 612))
    padded = wav.clone()
    for b, n in enumerate(lengths):
        padded[b, n:] = 1e3
    got = m.enhance_wave_windowed(padded.cuda(), W, V, lengths=torch.tensor(lengths))
    _check_rows(got, [oracle_windowed(sd, wav[b, :n], W, V) for b, n in enumerate(lengths)], lengths)


def test_short_windows_follow_the_models_own_floor():
    """TSSE (kernels 3, 5, 10; look_ahead 2): a window below 8 frames in a forward of mixed lengths is refused up front, by name."""
    _, m = _plus()
    wav = torch.from_numpy(make_wave(4, max(RAGGED) / 16000, 611)).cuda()
    ok = m.enhance_wave(wav[:, :4096])
    with pytest.raises(_lib.FsnpError, match="fsnp_enhance_wave_windowed.*too few frames") as e:
        m.enhance_wave_windowed(wav, W, V, lengths=RAGGED)
    assert e.value.code == 2
    assert torch.equal(m.enhance_wave(wav[:, :4096]), ok)
    m.check_errors()


# ------------------------------------------------------------------------------------------------ 4. K = 1 everywhere
def test_single_window_clips_are_enhance_wave_bit_for_bit():
    _, m = _plus()
    wav = torch.from_numpy(make_wave(2, 4096 / 16000, 613)).cuda()
    assert torch.equal(m.enhance_wave_windowed(wav, W, V, lengths=[4096, 4096]), m.enhance_wave(wav, lengths=[4096, 4096]))
    assert torch.equal(m.enhance_wave_windowed(wav, W, V), m.enhance_wave(wav))
    _, se = _plus_se()
    wav3 = torch.from_numpy(make_wave(3, 4096 / 16000, 614)).cuda()
    lengths = [3000, 4096, 700]
    wav3[0, 3000:] = 1e3
    wav3[2, 700:] = float("nan")
    assert torch.equal(se.enhance_wave_windowed(wav3, W, V, lengths=lengths), se.enhance_wave(wav3, lengths=lengths))


# ------------------------------------------------------------------------------------------------ 5. the original FullSubNet
def test_fullsubnet_three_windows_match_oracle():
    sd = make_state_dict_fullsubnet(13, "harsh")
    m = _build(FullSubNet, dict(FULLSUBNET_MODEL_ARGS), sd)
    L = 10000
    wav = torch.from_numpy(make_wave(1, L / 16000, 615))
    got = m.enhance_wave_windowed(wav.cuda(), W, V)
    _check_rows(got, [oracle_windowed(sd, wav[0], W, V, fullsubnet=True)], [L])


# ------------------------------------------------------------------------------------------------ 6. PCM
def test_pcm_in_place_and_out_formats():
    _, m = _plus()
    L = 10000
    x = make_wave(1, L / 16000, 616)[0]
    # one int16 channel of an interleaved stereo buffer, read where it lies
    stereo = torch.zeros((L, 2), dtype=torch.int16)
    stereo[:, 0] = torch.from_numpy(np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16))
    stereo[:, 1] = 12345
    stereo = stereo.cuda()
    ch = stereo.t()[0:1]
    assert ch.stride(1) == 2 and ch.dtype == torch.int16
    f32 = m.enhance_wave_windowed(ch, W, V, out_format="f32")
    assert torch.equal(f32, m.enhance_wave_windowed(ch.float() / 32768, W, V))          # int16 in is s.float() / 32768, bit for bit
    s16 = m.enhance_wave_windowed(ch, W, V)                                             # None follows the input: "s16"
    want, _ = _pcm_util.quantise_rows(f32.cpu().numpy())
    assert s16.dtype == torch.int16 and np.array_equal(s16.cpu().numpy(), want)
    # a ragged batch scaled to saturate: clipped counts per row, nothing counted past a length
    lengths = [10000, 6000]
    loud = torch.from_numpy(make_wave(2, L / 16000, 617) * 30.0).cuda()
    loud[1, 6000:] = 1e3
    ref = m.enhance_wave_windowed(loud, W, V, lengths=lengths).cpu().numpy()
    clipped = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    got = m.enhance_wave_windowed(loud, W, V, lengths=lengths, out_format="s16", clipped=clipped)
    want, counts = _pcm_util.quantise_rows(ref, lengths)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(clipped.cpu().numpy(), counts) and counts.min() > 0
    # the reference CLI's peak normalisation over each clip's own merged samples
    peak = m.enhance_wave_windowed(loud, W, V, lengths=lengths, out_format="s16_peak", clipped=clipped)
    assert np.array_equal(peak.cpu().numpy(), _pcm_util.peak_rows(ref, lengths)) and clipped.cpu().tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ 7. the round-trip hook
@pytest.mark.parametrize("dtype", [torch.float32, torch.int16], ids=["f32", "s16"])
def test_roundtrip_crosses_both_row_chunk_edges(dtype):
    """400 clips of 600 - 900 samples at W = 512, V = 256: more clips than one merge launch takes, and 1000 windows in one forward, more
    than three pad launches take.  The plan and the two kernels alone give the input back, bit for bit."""
    _, m = _plus()
    rng = np.random.default_rng(7)
    B, cols = 400, 900
    lengths = rng.integers(600, cols + 1, size=B)
    lengths[:3] = (600, 900, 769)
    assert B > 309 and 3 * 309 < sum(window_count(int(n), 512, 256) for n in lengths) <= 1000      # (4096 - 384) / 12 rows per launch
    if dtype == torch.int16:
        x = torch.from_numpy(rng.integers(-32768, 32768, size=(B, cols)).astype(np.int16))
    else:
        x = torch.from_numpy((rng.standard_normal((B, cols)) * 10.0 ** rng.integers(-6, 6, size=(B, cols))).astype(np.float32))
    want = x.clone()
    for b, n in enumerate(lengths):
        want[b, n:] = 0
        x[b, n:] = 77
    got = m.debug_window_roundtrip(x.cuda(), 512, 256, lengths=lengths.tolist(), max_batch=1000)
    assert got.dtype == dtype and torch.equal(got.cpu(), want)
    got = m.debug_window_roundtrip(x.cuda(), 512, 256, lengths=lengths.tolist(), max_batch=7)
    assert torch.equal(got.cpu(), want)


def test_roundtrip_of_a_long_clip_past_2_31_elements():
    """One int16 clip of 5 000 000 samples at W = 65 536, V = 8192 (88 windows, forwards of 32), read as one channel of a 480-channel
    interleaved buffer: its last samples lie 2.4e9 elements into the buffer, so a 32-bit element index would wrap."""
    _, m = _plus()
    L, channels = 5_000_000, 480
    assert (L - 1) * channels > 2 ** 31 and window_count(L, 65536, 8192) == 88
    x = torch.from_numpy(np.random.default_rng(8).integers(-32768, 32768, size=L).astype(np.int16)).cuda()
    buf = torch.empty((L, channels), dtype=torch.int16, device="cuda")
    buf[:, 0] = x
    ch = buf.t()[0:1]
    assert ch.stride(1) == channels
    got = m.debug_window_roundtrip(ch, 65536, 8192)
    assert got.dtype == torch.int16 and torch.equal(got[0], x)
    del buf


# ------------------------------------------------------------------------------------------------ 8. refusals of the C entry point
def _c_call(m, wav, window, overlap, max_batch=32, lengths=None):
    """fsnp_enhance_wave_windowed itself, past the Python checks -> (code, message)"""
    lib = _lib.load()
    out = torch.empty_like(wav)
    samples = None if lengths is None else (ctypes.c_int32 * len(lengths))(*lengths)
    rc = _call.enqueue(lib.fsnp_enhance_wave_windowed, wav.device, m._handle, wav.data_ptr(), _lib.SAMPLE_F32, wav.stride(0), 1, out.data_ptr(),
                       _lib.SAMPLE_F32, out.stride(0), 1, samples, wav.shape[0], wav.shape[1], window, overlap, max_batch, None)
    return rc, _lib.last_error()


def test_c_level_refusals_enqueue_nothing():
    _, m = _plus()
    wav = torch.from_numpy(make_wave(1, 10000 / 16000, 618)).cuda()
    ok = m.enhance_wave(wav)
    for args, what in (((W, 255), "overlap 255 outside"), ((W, 2049), "overlap 2049 outside"), ((W, V, 0), "max_batch 0")):
        rc, msg = _c_call(m, wav, *args)
        assert rc == 2 and "fsnp_enhance_wave_windowed" in msg and what in msg, (rc, msg)
    rc, msg = _c_call(m, wav[:, :200], W, V)
    assert rc == 2 and "fsnp_enhance_wave_windowed" in msg and "200 samples" in msg, (rc, msg)
    rc, msg = _c_call(m, wav, W, V, lengths=[200])
    assert rc == 2 and "clip 0: 200 samples" in msg, (rc, msg)
    assert torch.equal(m.enhance_wave(wav), ok)                          # nothing of the refused calls was left behind
    m.check_errors()


def test_models_the_lengths_path_refuses_run_plans_of_equal_windows():
    """subband_num = 2 (ECA): refused, by name, when a planned forward holds windows of different lengths - and only then."""
    args = dict(DEFAULT_MODEL_ARGS, channel_attention_model="ECA", subband_num=2)
    sd = make_state_dict(0, "default", attention="ECA")
    m = _build(FullSubNet_Plus, args, sd)
    wav = torch.from_numpy(make_wave(1, 10000 / 16000, 619))
    with pytest.raises(_lib.FsnpError, match="fsnp_enhance_wave_windowed.*subband_num") as e:
        m.enhance_wave_windowed(wav.cuda(), W, V)                        # 4096, 4096, 3856 in one forward
    assert e.value.code == 2
    equal = wav[:, :W + (W - V)]                                         # two full windows
    got = m.enhance_wave_windowed(equal.cuda(), W, V)
    _check_rows(got, [oracle_windowed(sd, equal[0], W, V, channel_attention_model="ECA", subband_num=2)], [equal.shape[1]])
    got = m.enhance_wave_windowed(wav.cuda(), W, V, max_batch=1)         # one window per forward: nothing is ragged
    _check_rows(got, [oracle_windowed(sd, wav[0], W, V, channel_attention_model="ECA", subband_num=2)], [10000])
    tcn = _build(FullSubNet_Plus, dict(DEFAULT_MODEL_ARGS, sequence_model="TCN"), make_state_dict(0, "default", sequence_model="TCN"))
    with pytest.raises(_lib.FsnpError, match="fsnp_enhance_wave_windowed.*TCN"):
        tcn.enhance_wave_windowed(wav.cuda(), W, V)

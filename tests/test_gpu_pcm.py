"""GPU tests of 16-bit PCM at the boundary of the waveform path and of wave sessions (include/fsnp_pcm.h).

Every comparison is exact (torch.equal / np.array_equal): an int16 input must give what the fp32 call gives for x.float() / 32768, and
every int16 output is a pure function (tests/_pcm_util.py) of the fp32 output the library already produces, so there is no tolerance to
choose.  What the fp32 results themselves are worth is the business of the existing wave tests; the models are theirs."""
import ctypes

import numpy as np
import pytest
import torch

from fullsubnet_plus_amd import FullSubNet, FullSubNet_Plus, _lib
from oracle.ref_loader import DEFAULT_MODEL_ARGS, FULLSUBNET_MODEL_ARGS
from oracle.weights import make_state_dict, make_state_dict_fullsubnet
from tests._pcm_util import crafted, peak_rows, peak_s16, quantise_rows
from tests._util import Golden

pytestmark = pytest.mark.gpu
HOP = 256
WAVE_ARGS = dict(DEFAULT_MODEL_ARGS, channel_attention_model="SE")       # as tests/test_gpu_stft_geometry.py: SE takes any clip the STFT takes

_models = {}


def _model(name):
    """the models of the existing wave tests, one of each per process"""
    if name not in _models:
        if name == "plus":
            cls, args, sd = FullSubNet_Plus, WAVE_ARGS, make_state_dict(41, "harsh", attention="SE")
        elif name == "fullsubnet":
            cls, args, sd = FullSubNet, FULLSUBNET_MODEL_ARGS, make_state_dict_fullsubnet(13, "harsh")
        elif name == "session":      # tests/test_gpu_wave_stream.py: a cumulative norm, as a session demands
            cls, args, sd = FullSubNet, dict(FULLSUBNET_MODEL_ARGS, norm_type="cumulative_layer_norm"), make_state_dict_fullsubnet(31, "default")
        else:                        # "f161": tests/test_gpu_stft_geometry.py _f161, run at hop 80
            g = Golden("fsn_b3_t18_la1_nb10_f161_tanh")
            cls, args, sd = FullSubNet, dict(g.args, norm_type="cumulative_layer_norm"), g.state_dict()
        m = cls(**args)
        m.load_state_dict(sd, strict=True)
        m = m.to("cuda").eval()
        m.batch_mode, m.error_check = "full", "sync"
        if name == "f161":
            m.hop_length = 80
        _models[name] = m
    return _models[name]


def _pcm(shape, seed):
    """seeded int16 samples over the whole range, with both ends of it and 0 in every row"""
    x = torch.from_numpy(np.random.RandomState(seed).randint(-32768, 32768, size=shape).astype(np.int16))
    x[:, 3], x[:, 4], x[:, 5] = -32768, 32767, 0
    return x


def _odd(x):
    """x [B, n] int16 (CPU) -> the same values on the GPU as buf[:, 1:] of a [B, n + 1] buffer: rows start at odd element offsets (2-byte
    aligned only) with a row stride that is odd when n is even"""
    buf = torch.full((x.shape[0], x.shape[1] + 1), 12345, dtype=torch.int16, device="cuda")
    buf[:, 1:] = x.cuda()
    view = buf[:, 1:]
    assert view.storage_offset() % 2 == 1 and view.stride() == (x.shape[1] + 1, 1) and view.data_ptr() % 4 == 2
    return view


def _eq16(got, want, what):
    assert got.dtype == torch.int16 and got.is_cuda, what
    assert np.array_equal(got.cpu().numpy(), want), (what, int((got.cpu().numpy() != want).sum()))


# ------------------------------------------------------------------------------------------------ 1. the conversion hook
def _convert(m, v, samples, fmt):
    """fsnp_debug_pcm_convert of v [rows, n] (CPU fp32) -> (int16 [rows, n], clipped int32 [rows]) on the CPU"""
    lib = m._ensure_handle(torch.device("cuda", torch.cuda.current_device()))
    rows, n = v.shape
    x = v.contiguous().cuda()
    out = torch.full((rows, n), 777, dtype=torch.int16, device="cuda")
    clipped = torch.full((rows,), -5, dtype=torch.int32, device="cuda")
    cnt = None if samples is None else (ctypes.c_int32 * rows)(*samples)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.fsnp_debug_pcm_convert(m._handle, x.data_ptr(), out.data_ptr(), rows, n, cnt, fmt, clipped.data_ptr(),
                                          ctypes.c_void_p(stream)), "fsnp_debug_pcm_convert")
    torch.cuda.synchronize()
    return out.cpu().numpy(), clipped.cpu().numpy()


def test_conversion_hook_on_crafted_values():
    """Ties, the two ends of the range, infinities, NaN and a denormal through exactly the store of the overlap-add kernels."""
    m = _model("fullsubnet")
    c, q, _ = crafted()
    rng = np.random.RandomState(5)
    v = rng.uniform(-1.2, 1.2, size=(2, 70)).astype(np.float32)
    v[0, 20:20 + c.size] = c                       # row 0: inside the row
    v[1, 33 - c.size:33] = c                       # row 1: right in front of its end ...
    v[1, 40:40 + c.size] = c                       # ... and behind it, where nothing may be read into the result
    samples = [70, 33]
    got, clipped = _convert(m, torch.from_numpy(v), samples, _lib.SAMPLE_S16)
    want, counts = quantise_rows(v, samples)
    assert np.array_equal(want[0, 20:20 + c.size], q)
    assert np.array_equal(got, want) and np.array_equal(clipped, counts) and counts.min() > 0
    assert not got[1, 33:].any()
    # the peak format: finite values (numpy's own tail turns a NaN or an infinity into a NaN peak)
    f = np.where(np.isfinite(v), v, np.float32(0.5)).astype(np.float32)
    f[0, 69] = -1.25                               # a negative peak, in the row's last sample
    got, clipped = _convert(m, torch.from_numpy(f), samples, _lib.SAMPLE_S16_PEAK)
    assert np.array_equal(got, peak_rows(f, samples)) and not clipped.any()
    assert got[0, 69] == -26213 and not got[1, 33:].any()
    # an all-zero row next to one that is not
    z = f.copy()
    z[1] = 0.0
    got, _ = _convert(m, torch.from_numpy(z), None, _lib.SAMPLE_S16_PEAK)
    assert np.array_equal(got, peak_rows(z)) and not got[1].any()


def test_peak_reduction_across_workgroups():
    """[1, 5000]: 20 workgroups fold into one row's maximum, which sits in the last element."""
    m = _model("fullsubnet")
    v = np.random.RandomState(6).uniform(-0.5, 0.5, size=(1, 5000)).astype(np.float32)
    v[0, 4999] = 0.75
    got, _ = _convert(m, torch.from_numpy(v), None, _lib.SAMPLE_S16_PEAK)
    assert np.array_equal(got[0], peak_s16(v[0])) and got[0, 4999] == 26213
    got, clipped = _convert(m, torch.from_numpy(v * 3), None, _lib.SAMPLE_S16)
    want, counts = quantise_rows(v * 3)
    assert np.array_equal(got, want) and np.array_equal(clipped, counts) and counts[0] > 1000


# ------------------------------------------------------------------------------------------------ 2. / 3. whole clips
def _whole_clip(m, x, lengths, what):
    """(a) - (d) of one int16 batch x [B, n] (CPU) handed over as an odd-offset view"""
    B, n = x.shape
    xv = _odd(x)
    xf = x.float().cuda() / 32768
    ref = m.enhance_wave(xf, lengths)
    lens = lengths if lengths is not None else [n] * B
    # (a) fp32 out of int16 in: the fp32 call's bits
    got = m.enhance_wave(xv, lengths, out_format="f32")
    assert got.dtype == torch.float32 and torch.equal(got, ref), what
    # (b) int16 out (the default for int16 in), with the clipped counts
    want, counts = quantise_rows(ref.cpu().numpy(), lens)
    clipped = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    _eq16(m.enhance_wave(xv, lengths, clipped=clipped), want, what + " s16")
    assert np.array_equal(clipped.cpu().numpy(), counts), (what, clipped.tolist(), counts.tolist())
    _eq16(m.enhance_wave(xv, lengths, out_format="s16"), want, what + " s16, no counts")
    # (c) the reference CLI's tail over each row's own samples, 0 behind them; nothing clips
    clipped.fill_(-1)
    _eq16(m.enhance_wave(xv, lengths, out_format="s16_peak", clipped=clipped), peak_rows(ref.cpu().numpy(), lens), what + " s16_peak")
    assert not clipped.any()
    # (d) fp32 in, int16 out
    clipped.fill_(-1)
    _eq16(m.enhance_wave(xf, lengths, out_format="s16", clipped=clipped), want, what + " fp32 in")
    assert np.array_equal(clipped.cpu().numpy(), counts)
    for b in range(B):
        assert not want[b, lens[b]:].any() and torch.count_nonzero(ref[b, lens[b]:]) == 0
    m.check_errors()
    return ref, want, counts


@pytest.mark.parametrize("name", ["plus", "fullsubnet"])
def test_whole_clip_default_geometry(name):
    """B = 3 clips of 257 (the shortest the reflect padding allows), 1000 (no multiple of the hop) and 1279 (odd) samples."""
    m = _model(name)
    _, want, counts = _whole_clip(m, _pcm((3, 1280), 21), [257, 1000, 1279], f"{name} lengths")
    print(f"{name}: clipped per row {counts.tolist()}, |q| max {np.abs(want.astype(np.int32)).max()}")
    _whole_clip(m, _pcm((2, 1000), 22), None, f"{name} B=2 L=1000")


def test_whole_clip_off_default_geometry():
    """161 bins: n_fft = 320 at hop 80 (the overlap-add's general path: up to four frames per sample), B = 1, L = 403."""
    m = _model("f161")
    x = _pcm((1, 403), 23)
    _whole_clip(m, x, None, "f161 hop 80")
    _whole_clip(m, x, [403], "f161 hop 80 lengths")


# ------------------------------------------------------------------------------------------------ 4. interleaved input
@pytest.mark.parametrize("dtype", [torch.int16, torch.float32])
def test_interleaved_input_is_read_in_place(dtype):
    """Three channels of an [n, 3] buffer as its transposed view (sample step 3, row stride 1)."""
    m = _model("fullsubnet")
    x = _pcm((3, 1000), 24)
    lengths = [1000, 257, 999]
    planar = x.cuda() if dtype == torch.int16 else x.float().cuda() / 32768
    inter = planar.t().contiguous().t()
    assert inter.stride() == (1, 3) and torch.equal(inter, planar)
    for fmt in ("f32", "s16", "s16_peak"):
        assert torch.equal(m.enhance_wave(inter, lengths, out_format=fmt), m.enhance_wave(planar, lengths, out_format=fmt)), fmt
    assert torch.equal(m.enhance_wave(inter), m.enhance_wave(planar))
    spec = m.stft(x.float().cuda() / 32768)
    got = m.stft(inter)
    assert got.shape == spec.shape and got.stride() == spec.stride() and torch.equal(got, spec)
    assert torch.equal(m.stft(_odd(x)), spec)
    m.check_errors()


# ------------------------------------------------------------------------------------------------ 5. / 6. wave sessions
def _blocks(lengths, sizes):
    """push by push (n, counts): block sizes `sizes` (the last one repeats) until every clip is through; slot 1 takes half a block on odd
    pushes, slot 2 sits every third push out"""
    left, k, out = list(lengths), 0, []
    while any(left):
        n = sizes[min(k, len(sizes) - 1)]
        ask = [n, n // 2 if k % 2 else n, 0 if k % 3 == 1 else n][:len(left)]
        counts = [min(a, l) for a, l in zip(ask, left)]
        left = [l - c for l, c in zip(left, counts)]
        out.append((n, counts))
        k += 1
    return out


def _feed(clips, pos, n, counts, as_float):
    """the [S, n] input of one push: counts[b] samples of clip b from pos[b] on, and behind them what must never be read"""
    S = len(clips)
    x = torch.full((S, n), float("nan")) if as_float else torch.full((S, n), 12345, dtype=torch.int16)
    for b in range(S):
        blk = clips[b][pos[b]:pos[b] + counts[b]]
        x[b, :counts[b]] = blk.float() / 32768 if as_float else blk
    return x.cuda()


def _session_pair(m, S, max_samples, live, clips, plan, swap_at=None, interleave=False):
    """An int16 session and an fp32 session of the same model through the same pushes and a finish."""
    with m.open_wave_stream(S, max_samples=max_samples, live=live) as wa, m.open_wave_stream(S, max_samples=max_samples, live=live) as wb:
        pos = [0] * S
        for k, (n, counts) in enumerate(plan):
            xa, xb = _feed(clips, pos, n, counts, False), _feed(clips, pos, n, counts, True)
            if interleave:
                xa, xb = xa.t().contiguous().t(), xb.t().contiguous().t()
                assert xa.stride() == (1, S) and xb.stride() == (1, S)
            ref = wb.push(xb, counts)
            as_f32 = k % 4 == 3
            got = wa.push(xa, counts, out_format="f32" if as_f32 else None)
            if as_f32:      # fp32 out of an int16 push: the fp32 session's bits
                assert got.dtype == torch.float32 and torch.equal(got, ref), k
            else:
                _eq16(got, quantise_rows(ref.cpu().numpy())[0], f"push {k} n={n} counts={counts}")
            for b in range(S):
                assert torch.count_nonzero(got[b, counts[b]:]) == 0 and torch.count_nonzero(ref[b, counts[b]:]) == 0, (k, b)
                pos[b] += counts[b]
            if k == swap_at:      # the records are fp32 whatever the pushes' formats: the states are the same bytes, and they move
                assert wa.state_bytes == wb.state_bytes
                for b in range(S):
                    assert torch.equal(wa.state(b), wb.state(b)), b
                wb.load_state(0, wa.state(0))
                assert wb.samples(0) == wa.samples(0) == pos[0]
        assert pos == [c.numel() for c in clips] and [wa.samples(b) for b in range(S)] == pos
        fin = wb.finish()
        _eq16(wa.finish(out_format="s16"), quantise_rows(fin.cpu().numpy())[0], "finish")
        assert torch.count_nonzero(fin) > 0
        # 7. nothing moved: a float push after all of that, on the session that ran the PCM calls, against the fp32-only session
        x = clips[0][:max_samples].float().cuda().repeat(S, 1) / 32768
        for _ in range(2):      # (twice: a clip needs more than n_fft / 2 samples to be finished)
            assert torch.equal(wa.push(x), wb.push(x))
        assert torch.equal(wa.finish(), wb.finish())
        m.check_errors()


def test_default_wave_session():
    """3 slots, blocks of 1, 255, 256, 257 and 300 samples with idle and partial slots, clips of 1279, 1000 and 700 samples."""
    m = _model("session")
    lengths = [1279, 1000, 700]
    x = _pcm((3, 1279), 25)
    clips = [x[b, :lengths[b]] for b in range(3)]
    plan = _blocks(lengths, [1, 255, 256, 257, 300])
    assert any(0 in c for _, c in plan) and any(0 < c[1] < n for n, c in plan) and len(plan) >= 6
    _session_pair(m, 3, 300, False, clips, plan, swap_at=len(plan) // 2)


def test_live_wave_session():
    """1 slot, six pushes of one hop, then finish; and two slots fed from one interleaved buffer (sample step 2)."""
    m = _model("session")
    x = _pcm((2, 6 * HOP), 26)
    _session_pair(m, 1, HOP, True, [x[0]], [(HOP, [HOP])] * 6, swap_at=3)
    _session_pair(m, 2, HOP, True, [x[0], x[1]], [(HOP, [HOP, HOP])] * 6, interleave=True)


# ------------------------------------------------------------------------------------------------ 7. nothing moved, and refusals
def test_fp32_calls_keep_their_bits_after_pcm_calls():
    m = _model("plus")
    x = _pcm((2, 1000), 27)
    xf = x.float().cuda() / 32768
    before, before_len = m.enhance_wave(xf), m.enhance_wave(xf, [1000, 300])
    for fmt in ("s16", "s16_peak", "f32"):
        m.enhance_wave(_odd(x), [1000, 300], out_format=fmt)
        m.enhance_wave(x.cuda(), out_format=fmt)
    assert torch.equal(m.enhance_wave(xf), before) and torch.equal(m.enhance_wave(xf, [1000, 300]), before_len)
    assert before.dtype == torch.float32 and m.enhance_wave(xf, out_format="f32").dtype == torch.float32
    m.check_errors()


def test_c_refusals_name_the_reason_before_anything_is_enqueued():
    m = _model("session")
    lib = m._ensure_handle(torch.device("cuda", torch.cuda.current_device()))
    x = _pcm((1, 1000), 28).cuda()
    out = torch.zeros((1, 1000), dtype=torch.int16, device="cuda")
    h, s = m._handle, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def refused(rc, code, *words):
        err = lib.fsnp_last_error().decode()
        assert rc == code and all(w in err for w in words), (rc, err)

    call = lambda ifmt, istep, ofmt, ostep, wav=x.data_ptr(), o=out.data_ptr(): lib.fsnp_enhance_wave_pcm(
        h, wav, ifmt, 1000, istep, o, ofmt, 1000, ostep, None, 1, 1000, None, s)
    refused(call(3, 1, 1, 1), 2, "fsnp_enhance_wave_pcm", "unknown", "input")
    refused(call(1, 1, -1, 1), 2, "unknown", "output")
    refused(call(2, 1, 1, 1), 2, "FSNP_SAMPLE_S16_PEAK", "input")
    refused(call(1, 0, 1, 1), 2, "step", "input")
    refused(call(1, 1, 1, 0), 2, "step", "output")
    refused(call(1, 1, 1, 1, wav=None), 1, "null")
    refused(call(1, 1, 1, 1, o=None), 1, "null")
    spec = torch.zeros((1, 4, 257, 2), device="cuda")
    refused(lib.fsnp_stft_pcm(h, x.data_ptr(), 2, 1000, 1, spec.data_ptr(), 1, 1000, s), 2, "fsnp_stft_pcm", "FSNP_SAMPLE_S16_PEAK")
    refused(lib.fsnp_stft_pcm(h, x.data_ptr(), 1, 1000, 0, spec.data_ptr(), 1, 1000, s), 2, "step")
    refused(lib.fsnp_stft_pcm(h, None, 1, 1000, 1, spec.data_ptr(), 1, 1000, s), 1, "null")
    with m.open_wave_stream(1, max_samples=HOP) as ws:
        st = ws._st
        push = lambda ifmt, istep, ofmt, ostep, wav=x.data_ptr(), o=out.data_ptr(): lib.fsnp_wave_stream_push_pcm(
            st, wav, ifmt, 1000, istep, None, o, ofmt, 1000, ostep, HOP, s)
        refused(push(1, 1, 2, 1), 2, "fsnp_wave_stream_push_pcm", "FSNP_SAMPLE_S16_PEAK", "no peak")
        refused(push(2, 1, 1, 1), 2, "FSNP_SAMPLE_S16_PEAK")
        refused(push(7, 1, 1, 1), 2, "unknown")
        refused(push(1, 0, 1, 1), 2, "step")
        refused(push(1, 1, 1, -2), 2, "step")
        refused(push(1, 1, 1, 1, wav=None), 1, "null")
        refused(push(1, 1, 1, 1, o=None), 1, "null")
        fin = lambda ofmt, ostep, o=out.data_ptr(): lib.fsnp_wave_stream_finish_pcm(st, None, 0, o, ofmt, 1000, ostep, s)
        refused(fin(2, 1), 2, "fsnp_wave_stream_finish_pcm", "FSNP_SAMPLE_S16_PEAK", "no peak")
        refused(fin(5, 1), 2, "unknown")
        refused(fin(1, 0), 2, "step")
        refused(fin(1, 1, o=None), 1, "null")
        assert ws.samples(0) == 0
        with pytest.raises(ValueError, match="no peak"):
            ws.push(x[:, :HOP], out_format="s16_peak")
    with pytest.raises(ValueError, match="out_format"):
        m.enhance_wave(x, out_format="u8")
    with pytest.raises(ValueError, match="clipped"):
        m.enhance_wave(x, clipped=torch.zeros(1, dtype=torch.int64, device="cuda"))
    torch.cuda.synchronize()
    assert torch.count_nonzero(out) == 0
    m.check_errors()

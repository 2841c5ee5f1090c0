"""GPU tests of the waveform path at any n_fft and hop length (include/fsnp_stft_geometry.h, model.hop_length): stft / istft against
torch on the CPU, enhance_wave (with and without lengths=) and wave sessions (default and live) against the torch-CPU oracle composed at
the same geometry (stft -> model -> cIRM -> istft, tests/_wave_geometry_util.py oracle_enhance_wave), and the default geometry bit for bit
against a model whose hop_length was never assigned.  The clip lengths are those of the host restatement: the shortest legal clip
(n_fft / 2 + 1), one below, at and one above a multiple of the hop, and one in the middle of a hop.  Measured errors are printed."""
import pytest
import torch

from fullsubnet_plus_amd import FullSubNet, FullSubNet_Plus, _lib
from oracle import fsnp_torch
from oracle.ref_loader import DEFAULT_MODEL_ARGS, FULLSUBNET_MODEL_ARGS
from oracle.weights import make_state_dict, make_state_dict_fullsubnet, make_wave
from tests._stream_util import stream_kwargs
from tests._util import Golden, check_rows, fullsubnet_oracle_kwargs, oracle_kwargs
from tests._wave_geometry_util import clip_lengths, oracle_enhance_wave
from tests._wave_stream_util import random_schedule, schedule, wave_clip

pytestmark = pytest.mark.gpu
TOL = 1e-3                   # the suite's golden / oracle tolerance (tests/test_gpu_parity.py)
torch.set_num_threads(16)

WAVE_ARGS = dict(DEFAULT_MODEL_ARGS, channel_attention_model="SE")       # as tests/test_gpu_lengths_edges.py: SE takes any clip the STFT takes


def _model(cls, args, sd, error_check="sync"):
    m = cls(**args)
    m.load_state_dict(sd, strict=True)
    m = m.to("cuda").eval()
    m.batch_mode = "full"
    m.error_check = error_check
    return m


def _rel(got, want):
    return float((got - want).abs().max() / want.abs().max())


# ------------------------------------------------------------------------------------------------ 4. stft / istft against torch
_plus_models = {}


def _plus(num_freqs):
    """one FullSubNet+ per bin count, shared by the cases of this file that only run its transforms"""
    if num_freqs not in _plus_models:
        _plus_models[num_freqs] = _model(FullSubNet_Plus, dict(DEFAULT_MODEL_ARGS, num_freqs=num_freqs), make_state_dict(0, num_freqs=num_freqs))
    return _plus_models[num_freqs]


@pytest.mark.parametrize("num_freqs,hop", [(161, 160), (161, 80), (161, 40), (257, 128), (257, 64), (33, 8), (33, 12), (101, 52)])
def test_stft_istft_vs_torch_at_any_hop(num_freqs, hop):
    """fsnp_stft / fsnp_istft at (n_fft, hop) vs torch.stft / torch.istft on the CPU: shape and strides as torch gives them, the transform,
    the round trip and the inverse of a random spectrum under 1e-5 relative (the bound of test_stft_istft_vs_torch).  (101, 52): the rows
    of the forward DFT matrix are padded (n_fft = 200 is no multiple of the GEMM's k-tile) and the hop does not divide n_fft."""
    n_fft, B = 2 * (num_freqs - 1), 3
    m = _plus(num_freqs)
    m.hop_length = hop
    try:
        for L in clip_lengths(n_fft, hop):
            if 2 * hop == n_fft and L == 5 * hop - 1:
                # the one case where the reference itself is ill-conditioned: the last sample is divided by one tiny w^2, and torch's own
                # fp32 is 2.3e-5 off its fp64 there (every other case: at most 4.7e-7)
                continue
            wav = torch.from_numpy(make_wave(B, L / 16000.0, 400 + L))
            assert wav.shape == (B, L)
            want = fsnp_torch.stft(wav, n_fft, hop, n_fft)
            got = m.stft(wav.cuda())
            assert got.shape == want.shape == (B, num_freqs, 1 + L // hop) and got.stride() == want.stride()
            e_stft = _rel(got.cpu(), want)
            e_rt = _rel(m.istft(got, L).cpu(), wav)
            rng = torch.Generator().manual_seed(L)
            spec = torch.complex(torch.randn(want.shape, generator=rng), torch.randn(want.shape, generator=rng))
            e_istft = _rel(m.istft(spec.cuda(), L).cpu(), fsnp_torch.istft(spec, L, n_fft, hop, n_fft))
            print(f"F={num_freqs} hop={hop} L={L}: stft {e_stft:.2e} round trip {e_rt:.2e} istft {e_istft:.2e}")
            assert e_stft < 1e-5 and e_rt < 1e-5 and e_istft < 1e-5, (L, e_stft, e_rt, e_istft)
        with pytest.raises(RuntimeError, match="reflect padding"):
            m.stft(torch.zeros(1, n_fft // 2, device="cuda"))
    finally:
        m.hop_length = num_freqs - 1
    assert f"n_fft={n_fft} hop_length={num_freqs - 1}" in m.dump_config()


# ------------------------------------------------------------------------------------------------ 5. the default geometry untouched
def test_assigning_the_default_hop_changes_no_bit():
    """stft, istft, enhance_wave and wave sessions (default and live, their state records included) of a model whose hop_length was assigned
    its default value against the same calls on a model that never had it assigned."""
    sd = make_state_dict(41, "harsh", attention="SE")
    a, b = _model(FullSubNet_Plus, WAVE_ARGS, sd), _model(FullSubNet_Plus, WAVE_ARGS, sd)
    b.hop_length = 256
    assert "_hop_length" not in a.__dict__
    wav = torch.from_numpy(make_wave(3, 0.25, 77)).cuda()
    L = wav.shape[1]
    Xa, Xb = a.stft(wav), b.stft(wav)
    assert "n_fft=512 hop_length=256" in a.dump_config() and "n_fft=512 hop_length=256" in b.dump_config()
    assert torch.equal(Xa, Xb) and torch.equal(a.istft(Xa, L), b.istft(Xb, L))
    assert torch.equal(a.enhance_wave(wav), b.enhance_wave(wav))
    lens = [257, 1279, L]
    assert torch.equal(a.enhance_wave(wav, lengths=lens), b.enhance_wave(wav, lengths=lens))
    args = dict(FULLSUBNET_MODEL_ARGS, norm_type="cumulative_layer_norm")
    sdf = make_state_dict_fullsubnet(31, "default")
    fa, fb = _model(FullSubNet, args, sdf), _model(FullSubNet, args, sdf)
    fb.hop_length = 256
    clip = wave_clip(5 * 256 + 77, 2001).cuda()
    for live in (False, True):
        with fa.open_wave_stream(2, max_samples=256, live=live) as wa, fb.open_wave_stream(2, max_samples=256, live=live) as wb:
            assert wa.state_bytes == wb.state_bytes and wa.delay == wb.delay == 4 * 256 and wa.hop_length == wb.hop_length == 256
            pos = 0
            for c in schedule(clip.numel(), 255):             # (idle pushes included)
                x = torch.zeros(2, 256, device="cuda")
                x[0, :c] = clip[pos:pos + c]
                assert torch.equal(wa.push(x, [c, 0]), wb.push(x, [c, 0])), (live, pos)
                pos += c
            assert torch.equal(wa.state(0), wb.state(0))
            assert torch.equal(wa.finish(), wb.finish())


# ------------------------------------------------------------------------------------------------ 6. enhance_wave against the composed oracle
def _nan_past(wav, samples):
    padded = wav.clone()
    for b, n in enumerate(samples):
        padded[b, n:] = float("nan")
    return padded


@pytest.mark.parametrize("model,num_freqs,hop", [("plus", 257, 128), ("plus", 161, 80), ("fullsubnet", 161, 40)])
def test_enhance_wave_at_any_hop_against_the_composed_oracle(model, num_freqs, hop):
    """fsnp_enhance_wave at (n_fft, hop): B = 3 x 0.25 s against stft -> model -> cIRM -> istft of torch on the CPU, the two-step form
    istft(enhance(stft(x))) within 1e-5 of the one call, and a ragged batch (NaN past each clip) whose sample counts sit at the reflection
    edge, around a multiple of the hop and at the buffer's end: row b is the clip alone, exactly 0 past it."""
    n_fft = 2 * (num_freqs - 1)
    if model == "plus":
        args, sd, cls = dict(WAVE_ARGS, num_freqs=num_freqs), make_state_dict(41, "harsh", num_freqs=num_freqs, attention="SE"), FullSubNet_Plus
        oracle = lambda w: oracle_enhance_wave(sd, w, num_freqs, hop, **oracle_kwargs(args))
    else:
        args, sd, cls = dict(FULLSUBNET_MODEL_ARGS, num_freqs=num_freqs), make_state_dict_fullsubnet(13, "harsh", num_freqs=num_freqs), FullSubNet
        oracle = lambda w: oracle_enhance_wave(sd, w, num_freqs, hop, fullsubnet=True, **fullsubnet_oracle_kwargs(args))
    m = _model(cls, args, sd)
    m.hop_length = hop
    wav = torch.from_numpy(make_wave(3, 0.25, 500))
    L = wav.shape[1]
    want = oracle(wav)
    got = m.enhance_wave(wav.cuda())
    m.check_errors()
    err = _rel(got.cpu(), want)
    two_step = m.istft(m.enhance(m.stft(wav.cuda())), L)
    e2 = _rel(two_step, got)
    print(f"enhance_wave {model} F={num_freqs} hop={hop}: rel err {err:.2e}, two-step form vs one call {e2:.2e}")
    assert err < TOL and e2 < 1e-5, (err, e2)
    # clips of different lengths in one batch
    samples = [n_fft // 2 + 1, 5 * hop - 1, 5 * hop, 5 * hop + 1, L]
    wav5 = torch.from_numpy(make_wave(5, L / 16000.0, 904))
    assert wav5.shape == (5, L)
    want_rows = [oracle(wav5[b:b + 1, :n]) for b, n in enumerate(samples)]
    got5 = m.enhance_wave(_nan_past(wav5, samples).cuda(), lengths=samples).cpu()
    m.check_errors()
    print(f"enhance_wave lengths {model} F={num_freqs} hop={hop}: worst rel err {max(check_rows(got5, want_rows, samples, TOL)):.2e}")
    # reserve() sizes the waveform area for this hop: the same call again allocates nothing new and gives the same bits
    m.reserve(3, 1 + L // hop, max_samples=L)
    assert torch.equal(m.enhance_wave(wav.cuda()), got)


# ------------------------------------------------------------------------------------------------ 7. wave sessions
def _f161():
    """the arguments of the offline-norm fixture fsn_b3_t18_la1_nb10_f161_tanh with a cumulative norm, as tests/test_gpu_stream_live.py"""
    g = Golden("fsn_b3_t18_la1_nb10_f161_tanh")
    return dict(g.args, norm_type="cumulative_layer_norm"), g.state_dict()


def _drive(ws, clips, schedules):
    """clips[b] [L_b] (CPU), schedules[b]: samples of slot b push by push (idle pushes pad the shorter ones) -> per slot the pushed
    columns in order (CPU).  The unread input holds NaN; everything past counts[b] must come back exactly 0."""
    S = ws.slots
    npush = max(len(s) for s in schedules)
    pos, got = [0] * S, [[] for _ in range(S)]
    for k in range(npush):
        counts = [schedules[b][k] if k < len(schedules[b]) else 0 for b in range(S)]
        n = max(max(counts), 1)
        x = torch.full((S, n), float("nan"))
        for b in range(S):
            x[b, :counts[b]] = clips[b][pos[b]:pos[b] + counts[b]]
            pos[b] += counts[b]
        out = ws.push(x.cuda(), counts).cpu()
        assert out.shape == (S, n)
        for b in range(S):
            assert torch.count_nonzero(out[b, counts[b]:]) == 0 and not torch.isnan(out[b]).any(), (k, b)
            got[b].append(out[b, :counts[b]])
    assert [ws.samples(b) for b in range(S)] == [c.numel() for c in clips]
    return [torch.cat(g) for g in got]


def _check(name, got, want, D):
    """got [L + D] of one slot (pushes, then finish), want [L]: the first D samples exactly 0, the rest the whole-clip waveform"""
    assert got.shape == (want.numel() + D,), (name, got.shape, want.shape)
    assert torch.count_nonzero(got[:D]) == 0, name
    err = _rel(got[D:], want)
    print(f"{name}: rel err {err:.3e}")
    assert err < TOL, (name, err)


def _alternating(L, hop):
    """pushes of hop - 1 and hop + 1 samples in turn, with an idle push after the first"""
    out, left, k = [], L, 0
    while left:
        c = min(left, hop - 1 if k % 2 == 0 else hop + 1)
        out.append(c)
        left -= c
        k += 1
        if k == 1:
            out.append(0)
    return out


@pytest.mark.parametrize("live", [False, True])
@pytest.mark.parametrize("hop", [80, 40])
def test_wave_sessions_at_any_hop_against_the_composed_oracle(hop, live):
    """F = 161 (n_fft 320), look_ahead 1, hop 80 and 40, default and live sessions.  Slots 0 - 2 take the same 9 hop + 77 clip in one push,
    in pushes of 160 and on a seeded random schedule with idle pushes, and finish together; slots 3 - 7 take one clip each of the lengths
    of the host restatement in pushes of hop - 1 / hop + 1 and are finished on calls of their own (up to n_fft / (2 hop) frames of a clip
    are only made there).  All outputs of a slot, then its finish: D = n_fft + look_ahead * hop zeros, then the oracle's waveform."""
    args, sd = _f161()
    n_fft, la = 320, args["look_ahead"]
    lengths = clip_lengths(n_fft, hop)
    long = lengths[-1]
    clips = [wave_clip(long, 2001)] * 3 + [wave_clip(L, 2100 + i) for i, L in enumerate(lengths)]
    sched = [[long], schedule(long, 160), random_schedule(long, 11, 3 * hop)] + [_alternating(L, hop) for L in lengths]
    kw = stream_kwargs(args)
    want = {id(c): oracle_enhance_wave(sd, c.unsqueeze(0), 161, hop, fullsubnet=True, **kw)[0] for c in clips}
    m = _model(FullSubNet, args, sd, "deferred")
    m.hop_length = hop
    with m.open_wave_stream(8, max_samples=long, live=live) as ws:
        m.hop_length = 160                                   # a session keeps the hop it was opened with
        D = ws.delay
        assert D == n_fft + la * hop and ws.hop_length == hop and ws.live == live
        got = _drive(ws, clips, sched)
        fins = {}
        fin = ws.finish([0, 1, 2]).cpu()
        assert fin.shape == (8, D) and torch.count_nonzero(fin[3:]) == 0
        for b in range(3):
            fins[b] = fin[b]
        for b in range(3, 8):
            assert ws.samples(b) == lengths[b - 3]
            fin = ws.finish([b]).cpu()
            assert torch.count_nonzero(fin[:b]) == 0 and torch.count_nonzero(fin[b + 1:]) == 0
            fins[b] = fin[b]
        m.check_errors()
        for b in range(8):
            assert ws.samples(b) == 0 and torch.count_nonzero(ws.state(b)) == 0, f"slot {b} is not zeroed after finish"
    for b in range(8):
        _check(f"{'live' if live else 'default'} hop={hop} slot {b} ({clips[b].numel()} samples)", torch.cat([got[b], fins[b]]), want[id(clips[b])], D)


def test_a_call_moves_mid_clip_from_a_default_to_a_live_session_at_hop_40():
    args, sd = _f161()
    hop, L = 40, 9 * 40 + 77
    clip = wave_clip(L, 2301)
    want = oracle_enhance_wave(sd, clip.unsqueeze(0), 161, hop, fullsubnet=True, **stream_kwargs(args))[0]
    m = _model(FullSubNet, args, sd, "deferred")
    m.hop_length = hop
    cut = 5 * hop + 13                                       # partial sums of three frames and a part-filled fifo travel with the call
    with m.open_wave_stream(1, max_samples=cut) as w1, m.open_wave_stream(2, max_samples=L - cut, live=True) as w2:
        assert w1.state_bytes == w2.state_bytes and not w1.live and w2.live
        first = w1.push(clip[:cut].unsqueeze(0).cuda())[0].cpu()
        w2.load_state(1, w1.state(0))
        assert w2.samples(1) == cut
        x = torch.full((2, L - cut), float("nan"))
        x[1] = clip[cut:]
        moved = w2.push(x.cuda(), [0, L - cut])[1].cpu()
        fin = w2.finish([1])[1].cpu()
        m.check_errors()
        _check("default -> live migration at hop 40", torch.cat([first, moved, fin]), want, w2.delay)


def test_a_live_session_whose_finish_needs_more_than_16_rows_is_refused_at_creation():
    args, sd = _f161()
    m = _model(FullSubNet, dict(args, look_ahead=13), sd, "deferred")
    m.hop_length = 40                                        # a finish can take ceil(320 / 80) + 13 = 17 frames
    with pytest.raises(_lib.FsnpError, match=r"finishing a clip takes up to .* 17 frames .* at most 16") as e:
        m.open_wave_stream(1, max_samples=40, live=True)
    assert e.value.code == 2
    with m.open_wave_stream(1, max_samples=40) as ws:        # a default session takes it
        assert ws.delay == 320 + 13 * 40
    m.hop_length = 80                                        # 2 + 13 frames: a live session again
    with m.open_wave_stream(1, max_samples=80, live=True) as ws:
        assert ws.delay == 320 + 13 * 80 and ws.hop_length == 80


# ------------------------------------------------------------------------------------------------ 8. one set of whole-clip kernels
# A batch of equal clips is the batch of clips of different lengths whose lengths are all equal: the whole-clip waveform path has one
# kernel body per step, and a call without lengths= runs it with the one length every row has.  The one thing that is NOT a function of
# the sample count is the number of frames the overlap-add sums: fsnp_istft sums every frame it is given.
@pytest.mark.parametrize("hop,T", [(80, 8), (160, 5)])
def test_istft_sums_every_frame_it_is_given(hop, T):
    """fsnp_istft takes any frames with (frames - 1) hop + n_fft >= length + n_fft / 2, so more than the 1 + length / hop of the clip's
    own STFT: the spare frames still reach into the clip's last samples, as in torch.istft(..., length=).  [2, 161, T] random spectra,
    length 200 (3 frames at hop 80, 2 at hop 160 - the two-frame branch of the default geometry - would do) against torch on the CPU
    under the 1e-5 of test_stft_istft_vs_torch_at_any_hop.  An overlap-add over the clip's own frames alone is 8e-2 off."""
    L, n_fft = 200, 320
    assert T > 1 + L // hop
    rng = torch.Generator().manual_seed(hop)
    spec = torch.complex(torch.randn((2, 161, T), generator=rng), torch.randn((2, 161, T), generator=rng))
    want = fsnp_torch.istft(spec, L, n_fft, hop, n_fft)
    m = _plus(161)
    m.hop_length = hop
    try:
        got = m.istft(spec.cuda(), L).cpu()
    finally:
        m.hop_length = 160
    err = _rel(got, want)
    print(f"istft of {T} frames at hop {hop} into {L} samples: rel err {err:.2e}")
    assert got.shape == want.shape == (2, L) and err < 1e-5, err


@pytest.mark.parametrize("hop", [160, 80])
def test_a_batch_of_equal_clips_is_the_ragged_batch_with_equal_lengths_bit_for_bit(hop):
    """B = 3 x 4000 samples at F = 161: enhance_wave(w) against enhance_wave(w, lengths=[4000] * 3) as fp32, as int16 with the clipped
    counts and peak-normalised, and enhance(X) against enhance(X, lengths=[T] * 3)."""
    m = _model(FullSubNet_Plus, dict(WAVE_ARGS, num_freqs=161), make_state_dict(41, "harsh", num_freqs=161, attention="SE"))
    m.hop_length = hop
    wav = torch.from_numpy(make_wave(3, 0.25, 611)).cuda()
    L = wav.shape[1]
    assert L == 4000
    for fmt in ("f32", "s16", "s16_peak"):
        ca, cb = (torch.full((3,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
        counts = fmt == "s16"
        a = m.enhance_wave(wav, out_format=fmt, clipped=ca if counts else None)
        b = m.enhance_wave(wav, lengths=[L] * 3, out_format=fmt, clipped=cb if counts else None)
        m.check_errors()
        assert a.dtype == b.dtype == (torch.float32 if fmt == "f32" else torch.int16) and a.shape == b.shape == (3, L)
        assert torch.count_nonzero(a) > 0 and torch.equal(a, b), fmt
        if counts:
            print(f"hop {hop}: clipped samples per row {ca.tolist()}")
            assert (ca >= 0).all() and torch.equal(ca, cb)
    X = m.stft(wav)
    T = X.shape[-1]
    assert T == 1 + L // hop
    assert torch.equal(m.enhance(X), m.enhance(X, lengths=[T] * 3))
    m.check_errors()


def _row_errs(got, want, rows=(0, 255, 256)):
    """worst relative error of the whole batch and of each row of `rows` against that row's own maximum"""
    return [_rel(got, want)] + [_rel(got[r], want[r]) for r in rows]


def test_equal_clips_past_the_256_rows_of_one_launch():
    """The launchers walk a batch 256 rows per launch, with or without lengths: B = 257 puts row 256 into a launch of its own.  The
    cIRM epilogue at [257, 3, 4] against oracle.fsnp_torch.apply_cirm, stft and istft of 257 x 400 samples against torch on the CPU; the
    whole batch and rows 0, 255 and 256 each.  Bounds: 1e-5 for the transforms, as test_stft_istft_vs_torch_at_any_hop; 1e-5 for the
    epilogue: a mask value near 0 goes through log((K - v) / (K + v)) of an argument near 1, where three fp32 roundings (2^-24 each)
    times K = 10 leave up to 2e-6 absolute in the decompressed mask of either side, on values of the order of 1."""
    B = 257
    m = _plus(161)
    rng = torch.Generator().manual_seed(257)
    mask = torch.randn((B, 2, 3, 4), generator=rng)
    X = torch.complex(torch.randn((B, 3, 4), generator=rng), torch.randn((B, 3, 4), generator=rng))
    got = m._apply_cirm(mask.cuda(), X.cuda()).cpu()
    errs = _row_errs(torch.view_as_real(got), torch.view_as_real(fsnp_torch.apply_cirm(mask, X)))
    print("apply_cirm B257: rel err of all rows, row 0, row 255, row 256:", " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) < 1e-5, errs
    L, n_fft, hop = 400, 320, 160
    wav = torch.from_numpy(make_wave(B, L / 16000.0, 257))
    assert wav.shape == (B, L) and not torch.equal(wav[255], wav[256])
    want = fsnp_torch.stft(wav, n_fft, hop, n_fft)
    got = m.stft(wav.cuda()).cpu()
    assert got.shape == want.shape == (B, 161, 1 + L // hop)
    errs = _row_errs(torch.view_as_real(got), torch.view_as_real(want))
    print("stft B257: rel err of all rows, row 0, row 255, row 256:", " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) < 1e-5, errs
    spec = torch.complex(torch.randn(want.shape, generator=rng), torch.randn(want.shape, generator=rng))
    errs = _row_errs(m.istft(spec.cuda(), L).cpu(), fsnp_torch.istft(spec, L, n_fft, hop, n_fft))
    print("istft B257: rel err of all rows, row 0, row 255, row 256:", " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) < 1e-5, errs

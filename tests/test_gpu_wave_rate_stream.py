"""GPU tests of rate sessions (include/fsnp_wave_rate_stream.h, FullSubNet.open_wave_stream(..., sample_rate=R)).

All push outputs of a clip at rate R followed by its finish() output are L + D_R samples: the first D_R exactly 0, the rest the whole-clip
enhance_wave(clip, sample_rate=R) of that clip alone.  Two references, neither of them the code under test: bit for bit, the composition
of public calls the header names (model.resample -> a model-rate wave session pushed ready(P + c) - ready(P) samples per call ->
model.resample); and, at the bar of the wave-session tests (1e-3 of max |want|), the torch-CPU oracle composed with the float64 converter
of tests/_resample_util.py.  Model and geometry are those of tests/test_gpu_wave_stream.py; clips are about 9 hops at the model's rate."""
import functools

import numpy as np
import pytest
import torch

from fullsubnet_plus_amd import FullSubNet, _lib
from fullsubnet_plus_amd.stream import WaveRateStream, WaveStream
from oracle import fsnp_torch
from oracle.ref_loader import FULLSUBNET_MODEL_ARGS
from oracle.weights import make_state_dict_fullsubnet
from tests._pcm_util import quantise_rows
from tests._resample_util import plan, resample64
from tests._stream_util import stream_kwargs
from tests._wave_rate_stream_util import rate_delay, ready, total
from tests._wave_stream_util import random_schedule, schedule, wave_clip

pytestmark = pytest.mark.gpu
TOL = 1e-3
F, HOP, M, DM = 257, 256, 16000, 1024
RATES = [48000, 44100, 8000]
ARGS = dict(FULLSUBNET_MODEL_ARGS, norm_type="cumulative_layer_norm")
torch.set_num_threads(16)


@functools.lru_cache(maxsize=None)
def _sd(seed=41):
    return make_state_dict_fullsubnet(seed, "default")


def _model():
    m = FullSubNet(**ARGS)
    m.load_state_dict(_sd(), strict=True)
    m = m.to("cuda").eval()
    m.batch_mode = "full"
    m.error_check = "deferred"
    return m


def _clip(rate, model_samples=9 * HOP + 77, seed=2301):
    up, down, _ = plan(rate, M)
    return wave_clip(model_samples * down // up, seed + rate % 97)


@functools.lru_cache(maxsize=None)
def _oracle(rate, model_samples=9 * HOP + 77, seed=2301):
    """the whole-clip oracle at rate R of _clip(rate, ...): resample64 -> fsnp_torch.enhance_wave -> resample64, cut to the clip's length"""
    clip = _clip(rate, model_samples, seed)
    x = torch.from_numpy(resample64(clip.numpy(), rate, M)[0]).float()
    e = fsnp_torch.enhance_wave(_sd(), x.unsqueeze(0), fullsubnet=True, **stream_kwargs(ARGS))[0]
    return torch.from_numpy(resample64(e.numpy(), M, rate)[0][:clip.numel()]).float()


def _err(got, want):
    return float((got - want).abs().max() / want.abs().max())


def _push_all(ws, clips, schedules):
    """clips[b]: [L_b] CPU (None = the slot stays idle); schedules[b]: samples of slot b push by push (padded with idle pushes to the
    longest).  -> per slot the pushed columns in order (CPU), and the per-push counts.  The unread input holds NaN; everything past
    counts[b] must come back exactly 0."""
    S = ws.slots
    npush = max(len(s) for s in schedules if s is not None)
    pos, got, calls = [0] * S, [[] for _ in range(S)], []
    for k in range(npush):
        counts = [0 if schedules[b] is None or k >= len(schedules[b]) else schedules[b][k] for b in range(S)]
        n = max(max(counts), 1)
        x = torch.full((S, n), float("nan"))
        for b in range(S):
            if counts[b]:
                x[b, :counts[b]] = clips[b][pos[b]:pos[b] + counts[b]]
                pos[b] += counts[b]
        out = ws.push(x.cuda(), counts).cpu()
        assert out.shape == (S, n)
        for b in range(S):
            assert torch.count_nonzero(out[b, counts[b]:]) == 0 and not torch.isnan(out[b]).any(), (k, b)
            got[b].append(out[b, :counts[b]])
        calls.append(counts)
    for b in range(S):
        assert ws.samples(b) == (0 if clips[b] is None else clips[b].numel())
    return [torch.cat(g) for g in got], calls


def _check(name, got, want, D):
    assert got.shape == (want.numel() + D,), (name, got.shape, want.shape)
    assert torch.count_nonzero(got[:D]) == 0, name
    err = _err(got[D:], want)
    print(f"{name}: rel err {err:.3e}")
    assert err < TOL, (name, err)


def _schedules(L, rate, seed):
    block = rate // 100
    return [schedule(L, block), schedule(L, 3 * block + 1, idle_every=2), random_schedule(L, seed, 4 * block)]


@functools.lru_cache(maxsize=None)
def _streamed(rate, live):
    """one clip in three slots of a rate session on three schedules -> (outputs [3][L + D_R], the composition of public calls [3][L + D_R])"""
    up, down, half = plan(rate, M)
    clip = _clip(rate)
    L = clip.numel()
    sched = _schedules(L, rate, 17)
    m = _model()
    with m.open_wave_stream(3, max_samples=max(max(s) for s in sched), live=live, sample_rate=rate) as rs:
        assert isinstance(rs, WaveRateStream) and rs.sample_rate == rate and rs.live == live
        D = rs.delay
        assert D == rate_delay(DM, up, down, half) and rs.model_delay == DM
        assert rs.model_max_samples == max(rs.max_samples * up // down + 1, -(-half // down))
        got, calls = _push_all(rs, [clip] * 3, sched)
        fin = rs.finish().cpu()
        m.check_errors()
        assert fin.shape == (3, D) and [rs.samples(b) for b in range(3)] == [0, 0, 0]
        got = [torch.cat([got[b], fin[b]]) for b in range(3)]
        model_max = rs.model_max_samples
    # the composition: the whole clip converted once, a model-rate session of the same kind fed what each call completes
    x_m = m.resample(clip.unsqueeze(0).cuda(), rate, M)[0]
    n_m = total(L, up, down)
    assert x_m.shape == (n_m,)
    with m.open_wave_stream(3, max_samples=model_max, live=live) as ws:
        assert type(ws) is WaveStream and ws.delay == DM
        P, pos, outs = [0] * 3, [0] * 3, [[] for _ in range(3)]
        for counts in calls + ["remainder"]:
            if counts == "remainder":
                cm = [n_m - pos[b] for b in range(3)]
            else:
                cm = [ready(P[b] + counts[b], up, down, half) - ready(P[b], up, down, half) for b in range(3)]
                P = [P[b] + counts[b] for b in range(3)]
            n = max(max(cm), 1)
            x = torch.full((3, n), float("nan"), device="cuda")
            for b in range(3):
                x[b, :cm[b]] = x_m[pos[b]:pos[b] + cm[b]]
            o = ws.push(x, cm)
            for b in range(3):
                outs[b].append(o[b, :cm[b]])
                pos[b] += cm[b]
        assert pos == [n_m] * 3 and P == [L] * 3
        fin_m = ws.finish()
        m.check_errors()
    want = []
    for b in range(3):
        e = torch.cat(outs[b] + [fin_m[b]])[DM:]
        assert e.shape == (n_m,)
        back = m.resample(e.unsqueeze(0), M, rate)[0][:L].cpu()
        want.append(torch.cat([torch.zeros(D), back]))
    return got, want, D


# ------------------------------------------------------------------------------------------------ 1. the composition of public calls
@pytest.mark.parametrize("live", [True, False])
@pytest.mark.parametrize("rate", RATES)
def test_a_rate_session_is_bit_for_bit_the_composition_of_public_calls(rate, live):
    got, want, D = _streamed(rate, live)
    for b in range(3):
        assert got[b].shape == want[b].shape
        diff = (got[b] != want[b]).nonzero().flatten()
        assert torch.equal(got[b], want[b]), (rate, live, b, diff[:8].tolist(), diff.numel())


# ------------------------------------------------------------------------------------------------ 2. the oracle
@pytest.mark.parametrize("live", [True, False])
@pytest.mark.parametrize("rate", RATES)
def test_a_rate_session_against_the_oracle(rate, live):
    got, _, D = _streamed(rate, live)
    want = _oracle(rate)
    for b, nm in enumerate(("10 ms blocks", "30 ms + 1 blocks", "random schedule")):
        _check(f"{rate} Hz live={live} {nm}", got[b], want, D)


# ------------------------------------------------------------------------------------------------ 3. chunk sizes and unread input
def test_chunk_sizes_around_the_histories_and_the_delay():
    """48 kHz (input history 192, enhanced history 64, delay 3264): pushes of 1 sample (mostly no model-rate sample per push) for the first
    400 samples and then 10 ms blocks; pushes of 100 (shorter than the input history); a first push longer than the delay, then pushes of
    500.  _push_all fills the unread input with NaN and checks that the columns past counts[b] are exactly 0."""
    rate = 48000
    clip, want = _clip(rate), _oracle(rate)
    L = clip.numel()
    sched = [[1] * 400 + schedule(L - 400, 480), schedule(L, 100), [3300] + schedule(L - 3300, 500)]
    m = _model()
    with m.open_wave_stream(3, max_samples=3300, sample_rate=rate) as rs:
        D = rs.delay
        assert D == 3264 < 3300
        got, _ = _push_all(rs, [clip] * 3, sched)
        assert torch.count_nonzero(got[2][3264:3300]) > 0                  # the first push already returns audio
        fin = rs.finish().cpu()
        m.check_errors()
    for b, nm in enumerate(("1 sample x 400, then 10 ms", "pushes of 100", "3300, then 500")):
        _check(f"48 kHz {nm}", torch.cat([got[b], fin[b]]), want, D)


# ------------------------------------------------------------------------------------------------ 4. both ends of the clip
def test_clip_ends_at_48_khz():
    """One slot per length: model-rate lengths n_fft / 2 + 1 (the shortest clip; shorter than the delay), 5 hop - 1, 5 hop, 5 hop + 1,
    expressed at 48 kHz (total(L) = ceil(L / 3)); each slot finished in a call of its own, which must leave the others' states bit for
    bit.  A clip one sample too short is refused at finish and the session stays usable."""
    rate = 48000
    targets = [HOP + 1, 5 * HOP - 1, 5 * HOP, 5 * HOP + 1]
    lengths = [3 * targets[0] - 2, 3 * targets[1], 3 * targets[2] - 1, 3 * targets[3] - 2]
    assert [total(L, 1, 3) for L in lengths] == targets
    m = _model()
    with m.open_wave_stream(4, max_samples=481, sample_rate=rate) as rs:
        D = rs.delay
        assert lengths[0] < D
        clips = [_clip(rate, t, 2400 + b)[:L] for b, (t, L) in enumerate(zip(targets, lengths))]
        sched = [schedule(L, 479 if b % 2 else 481) for b, L in enumerate(lengths)]
        got, _ = _push_all(rs, clips, sched)
        fins = []
        for b in range(4):
            others = [rs.state(o) for o in range(4) if o != b]
            fins.append(rs.finish([b]).cpu())
            assert rs.samples(b) == 0
            assert torch.count_nonzero(fins[-1][[o for o in range(4) if o != b]]) == 0
            for st, o in zip(others, [o for o in range(4) if o != b]):
                assert torch.equal(st, rs.state(o)), (b, o)
        # one sample too short: 768 samples are 256 at the model's rate
        short = _clip(rate, HOP + 1, 2400)[:3 * HOP]
        rs.push(short[:481].repeat(4, 1).cuda(), [481, 0, 0, 0])
        rs.push(short[481:].repeat(4, 1).cuda(), [768 - 481, 0, 0, 0])
        with pytest.raises(_lib.FsnpError, match="reflect padding") as e:
            rs.finish([0])
        assert e.value.code == 2 and rs.samples(0) == 768
        out = rs.push(short[:1].repeat(4, 1).cuda(), [1, 0, 0, 0])            # still usable: one more sample makes it a clip
        assert out.shape == (4, 1) and rs.samples(0) == 769
        last = rs.finish([0]).cpu()
        m.check_errors()
        assert torch.isfinite(last).all() and torch.count_nonzero(last[0]) > 0 and torch.count_nonzero(last[1:]) == 0
    for b, (t, L) in enumerate(zip(targets, lengths)):
        x = torch.from_numpy(resample64(clips[b].numpy(), rate, M)[0]).float()
        e = fsnp_torch.enhance_wave(_sd(), x.unsqueeze(0), fullsubnet=True, **stream_kwargs(ARGS))[0]
        want = torch.from_numpy(resample64(e.numpy(), M, rate)[0][:L]).float()
        _check(f"48 kHz, {L} samples ({t} at the model's rate)", torch.cat([got[b], fins[b][b]]), want, D)


# ------------------------------------------------------------------------------------------------ 5. PCM
def test_pcm_in_and_out_and_an_interleaved_view():
    """int16 in gives the bits of the fp32 push of x / 32768; int16 out is quantise_rows of the fp32 output; a two-channel interleaved
    buffer is read in place."""
    rate = 44100
    clip = _clip(rate)
    L = clip.numel()
    pcm = torch.from_numpy(quantise_rows(clip.numpy()[None] * 0.9)[0][0])
    assert pcm.dtype == torch.int16
    scheds = [schedule(L, 441), schedule(L, 300)]
    m = _model()
    runs = []
    with m.open_wave_stream(2, max_samples=441, live=True, sample_rate=rate) as rs:
        D = rs.delay
        inter = torch.zeros((2, 441, 2), dtype=torch.int16, device="cuda")       # channel 0 is the stream, channel 1 must never reach it
        # the same two schedules four times over: fp32 in / fp32 out, int16 / fp32, int16 / int16, an interleaved int16 view / fp32
        for mode in ("f32", "s16 in", "s16", "interleaved"):
            pos, rows = [0, 0], [[], []]
            for k in range(max(len(v) for v in scheds)):
                counts = [v[k] if k < len(v) else 0 for v in scheds]
                n = max(max(counts), 1)
                a = torch.zeros((2, n), dtype=torch.int16)
                for b in range(2):
                    a[b, :counts[b]] = pcm[pos[b]:pos[b] + counts[b]]
                    pos[b] += counts[b]
                if mode == "f32":
                    o = rs.push((a.float() / 32768.0).cuda(), counts)
                elif mode == "s16 in":
                    o = rs.push(a.cuda(), counts, out_format="f32")
                elif mode == "s16":
                    o = rs.push(a.cuda(), counts)
                else:
                    inter[:, :, 1] = 12345
                    inter[:, :n, 0] = a.cuda()
                    o = rs.push(inter[:, :n, 0], counts, out_format="f32")
                assert o.dtype == (torch.int16 if mode == "s16" else torch.float32)
                for b in range(2):
                    assert torch.count_nonzero(o[b, counts[b]:]) == 0
                    rows[b].append(o[b, :counts[b]].cpu())
            fin = rs.finish(out_format="s16" if mode == "s16" else "f32").cpu()
            runs.append(torch.stack([torch.cat(rows[b] + [fin[b]]) for b in range(2)]))
        m.check_errors()
    f32, s16in, s16, inter_out = runs
    assert f32.shape == (2, L + D) and torch.count_nonzero(f32[:, D:]) > 0
    assert torch.equal(f32, s16in) and torch.equal(f32, inter_out)
    assert s16.dtype == torch.int16 and np.array_equal(s16.numpy(), quantise_rows(f32.numpy())[0])


# ------------------------------------------------------------------------------------------------ 6. state
def test_a_slot_moves_between_slots_sessions_and_kinds_and_a_record_of_another_pair_is_refused():
    rate = 48000
    clip, want = _clip(rate), _oracle(rate)
    L = clip.numel()
    cut = 5 * 480 + 7
    m = _model()
    with m.open_wave_stream(2, max_samples=480, live=True, sample_rate=rate) as a, \
            m.open_wave_stream(3, max_samples=960, live=False, sample_rate=rate) as b, \
            m.open_wave_stream(1, max_samples=441, live=True, sample_rate=44100) as other:
        D = a.delay
        with m.open_wave_stream(1, max_samples=160, live=True) as plain:
            assert a.state_bytes == b.state_bytes == other.state_bytes + 4 * (192 - 176) > plain.state_bytes
        head, _ = _push_all(a, [clip[:cut], None], [schedule(cut, 480), None])
        st = a.state(0)
        # a 48 kHz record in a 44.1 kHz session: the histories differ in size, so the Python layer refuses its length; a record of the
        # right length that names 1 : 3 (the 44.1 kHz session's own, its pair rewritten) is refused by the library, nothing loaded
        with pytest.raises(ValueError, match="bytes"):
            other.load_state(0, st)
        other.load_state(0, other.state(0))                                  # an empty record (count 0, no pair yet) loads
        other.push(torch.from_numpy(resample64(clip[:1323].numpy(), rate, 44100)[0][:441]).float().unsqueeze(0).cuda())
        own = other.state(0)
        tail = own[-16:].view(torch.int32)                                   # rate record [.. | count int64 | up | down]: 960 + 16 bytes at 44.1 kHz
        assert tail.tolist() == [441, 0, 160, 441]
        forged = own.clone()
        forged[-8:] = torch.tensor([1, 3], dtype=torch.int32).view(torch.uint8).cuda()
        with pytest.raises(_lib.FsnpError, match="ratio 1 : 3") as e:
            other.load_state(0, forged)
        assert e.value.code == 2 and other.samples(0) == 441 and torch.equal(other.state(0), own)
        other.load_state(0, own)
        a.load_state(1, st)                                                  # to another slot of the live session ...
        b.load_state(2, st)                                                  # ... and to a default session
        assert a.samples(1) == cut == b.samples(2)
        rest = clip[cut:]
        sa, sb = schedule(L - cut, 480), schedule(L - cut, 960)
        pos, ta = 0, []
        for c in sa:
            x = torch.full((2, max(c, 1)), float("nan"))
            x[1, :c] = rest[pos:pos + c]
            ta.append(a.push(x.cuda(), [0, c])[1, :c].cpu())
            pos += c
        pos, tb = 0, []
        for c in sb:
            x = torch.full((3, max(c, 1)), float("nan"))
            x[2, :c] = rest[pos:pos + c]
            tb.append(b.push(x.cuda(), [0, 0, c])[2, :c].cpu())
            pos += c
        fa, fb = a.finish([1]).cpu()[1], b.finish([2]).cpu()[2]
        m.check_errors()
    _check("48 kHz, moved to another slot", torch.cat([head[0]] + ta + [fa]), want, D)
    _check("48 kHz, moved live -> default", torch.cat([head[0]] + tb + [fb]), want, D)


def test_a_live_session_refuses_a_push_size_by_its_model_rate_count_and_says_both():
    """20000 samples at 48 kHz are up to 6667 at the model's rate, 27 frames per call: a live session runs 16.  The default session takes it."""
    m = _model()
    with pytest.raises(_lib.FsnpError, match=r"max_samples 20000 at 48000 Hz is up to 6667 samples per call") as e:
        m.open_wave_stream(1, max_samples=20000, live=True, sample_rate=48000)
    assert e.value.code == 2 and "fsnp_wave_rate_stream_create_live" in str(e.value) and "16" in str(e.value)
    with m.open_wave_stream(1, max_samples=20000, sample_rate=48000) as rs:
        assert rs.model_max_samples == 6667 and not rs.live


# ------------------------------------------------------------------------------------------------ 7. the model's own rate
def test_the_models_own_rate_is_the_session_it_has_always_been():
    clip = wave_clip(5 * HOP + 3, 2500)
    m = _model()
    outs, sizes = [], []
    for kw in ({}, {"sample_rate": None}, {"sample_rate": 16000}, {"sample_rate": np.int64(16000)}):
        with m.open_wave_stream(2, max_samples=160, live=True, **kw) as ws:
            assert type(ws) is WaveStream and not hasattr(ws, "model_delay")
            got, _ = _push_all(ws, [clip, clip], [schedule(clip.numel(), 160), schedule(clip.numel(), 97)])
            outs.append(torch.cat([torch.stack([torch.cat([g, f]) for g, f in zip(got, ws.finish().cpu())])]))
            sizes.append(ws.state_bytes)
    m.check_errors()
    assert all(torch.equal(outs[0], o) for o in outs[1:]) and len(set(sizes)) == 1
    with pytest.raises(_lib.FsnpError, match="fsnp_wave_stream_create") as e:           # the C entry point refuses the model's own rate
        WaveRateStream(m, 1, 160, torch.device("cuda", torch.cuda.current_device()), live=False, sample_rate=16000)
    assert e.value.code == 2

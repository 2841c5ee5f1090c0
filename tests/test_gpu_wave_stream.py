"""GPU tests of wave sessions of the original FullSubNet (include/fsnp_wave_stream.h, FullSubNet.open_wave_stream).

All push outputs of a clip followed by its finish() output are L + D samples, D = (2 + look_ahead) hop: the first D exactly 0, the rest the
whole-clip enhance_wave of that clip alone.  Every comparison is against the torch-CPU oracle fsnp_torch.enhance_wave(..., fullsubnet=True)
(never against the code under test), error max|got - want| / max|want| as test_enhance_wave_vs_oracle, bar 1e-3 (BASELINE.json north_star);
the measured errors are printed."""
import re
import time

import pytest
import torch

from fullsubnet_plus_amd import FullSubNet, _lib
from oracle import fsnp_torch
from oracle.make_golden import make_spec
from oracle.ref_loader import FULLSUBNET_MODEL_ARGS
from oracle.weights import make_state_dict_fullsubnet, make_wave
from tests._stream_util import stream_kwargs
from tests._wave_stream_util import random_schedule, schedule, wave_clip

pytestmark = pytest.mark.gpu
TOL = 1e-3
F, HOP = 257, 256
torch.set_num_threads(16)


def _model(args, sd, error_check="deferred"):
    m = FullSubNet(**args)
    m.load_state_dict(sd, strict=True)
    m = m.to("cuda").eval()
    m.batch_mode = "full"
    m.error_check = error_check
    return m


def _args(norm_type="cumulative_layer_norm", **kw):
    return dict(FULLSUBNET_MODEL_ARGS, norm_type=norm_type, **kw)


def _oracle(sd, clip, args):
    return fsnp_torch.enhance_wave(sd, clip.unsqueeze(0), fullsubnet=True, **stream_kwargs(args))[0]


def _err(got, want):
    return float((got - want).abs().max() / want.abs().max())


def _push_all(ws, clips, schedules):
    """clips[b]: [L_b] CPU (None = the slot stays idle); schedules[b]: samples of slot b push by push (padded with idle pushes to the longest).
    -> per slot the pushed columns in order (CPU).  The unread input holds NaN; everything past counts[b] must come back exactly 0."""
    S = ws.slots
    npush = max(len(s) for s in schedules if s is not None)
    pos, got = [0] * S, [[] for _ in range(S)]
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
    for b in range(S):
        assert ws.samples(b) == (0 if clips[b] is None else clips[b].numel())
    return [torch.cat(g) for g in got]


def _check(name, got, want, D):
    """got [L + D] of one slot (pushes, then finish), want [L]: the first D samples exactly 0, the rest the whole-clip waveform"""
    assert got.shape == (want.numel() + D,), (name, got.shape, want.shape)
    assert torch.count_nonzero(got[:D]) == 0, name
    err = _err(got[D:], want)
    print(f"{name}: rel err {err:.3e}")
    assert err < TOL, (name, err)
    return err


# ------------------------------------------------------------------------------------------------ chunking invariance
@pytest.mark.parametrize("norm_type,look_ahead", [("cumulative_layer_norm", 2), ("cumulative_laplace_norm", 0)])
def test_chunking_invariance_against_the_oracle(norm_type, look_ahead):
    """Three slots, the same clip of 9 hop + 77 samples: in one push, in pushes of 160, and on a seeded random schedule with idle pushes."""
    args, L = _args(norm_type, look_ahead=look_ahead), 9 * HOP + 77
    sd = make_state_dict_fullsubnet(31, "default")
    clip = wave_clip(L, 2001)
    want = _oracle(sd, clip, args)
    sched = [[L], schedule(L, 160), random_schedule(L, 11, 3 * HOP)]
    m = _model(args, sd)
    with m.open_wave_stream(3, max_samples=L) as ws:
        D = ws.delay
        assert D == (2 + look_ahead) * HOP and ws.max_samples == L
        got = _push_all(ws, [clip] * 3, sched)
        fin = ws.finish().cpu()
        m.check_errors()
        assert fin.shape == (3, D) and [ws.samples(b) for b in range(3)] == [0, 0, 0]
    for b, nm in enumerate(("one push", "pushes of 160", "random schedule")):
        _check(f"{norm_type} look_ahead={look_ahead} {nm}", torch.cat([got[b], fin[b]]), want, D)


@pytest.mark.parametrize("live", [False, True])
@pytest.mark.parametrize("look_ahead", [1, 4])
def test_ring_shorter_equal_and_longer_than_a_push(look_ahead, live):
    """The wave counterpart of the spectrum sessions' test of this name.  One clip of 8 hop + 33 samples in three slots of a session of
    6 frames per push: pushes of hop (none, two, then one frame per push: the ring is longer than a push at look_ahead 4, as long at 1),
    of 4 hop (as long at 4, shorter at 1) and of 5 hop + 3, whose first push holds steps without a frame and steps with one in the same
    call (the first frame row the overlap-add reads is row look_ahead: j0 = 1 with 4 enhanced frames, j0 = 4 with 1).  Idle pushes in
    between, then finish()."""
    args, L = _args("cumulative_layer_norm", look_ahead=look_ahead), 8 * HOP + 33
    sd = make_state_dict_fullsubnet(38, "default")
    clip = wave_clip(L, 2701)
    want = _oracle(sd, clip, args)
    sizes = [HOP, 4 * HOP, 5 * HOP + 3]
    m = _model(args, sd)
    with m.open_wave_stream(3, max_samples=5 * HOP + 3, live=live) as ws:
        D = ws.delay
        assert D == (2 + look_ahead) * HOP and ws.live == live
        got = _push_all(ws, [clip] * 3, [schedule(L, c) for c in sizes])
        fin = ws.finish().cpu()
        m.check_errors()
    for b in range(3):
        _check(f"look_ahead {look_ahead}, live {live}, pushes of {sizes[b]}", torch.cat([got[b], fin[b]]), want, D)


# ------------------------------------------------------------------------------------------------ both ends of the clip
def test_clip_ends():
    """One slot per length around the frame grid (the shortest clip a whole-clip call takes, exact multiples of hop, one sample either side);
    pushes of hop - 1 and hop + 1 samples, different per slot in every push; each slot finished on a call of its own, which must leave the
    others' state bit for bit.  Lengths below D are here on purpose: most of their audio comes out of finish()."""
    args = _args("cumulative_layer_norm")
    sd = make_state_dict_fullsubnet(32, "default")
    lengths = [HOP + 1, 2 * HOP, 5 * HOP - 1, 5 * HOP, 5 * HOP + 1]
    clips = [wave_clip(L, 2100 + b) for b, L in enumerate(lengths)]
    sched = []
    for b, L in enumerate(lengths):
        s, left = [], L
        while left:
            c = min(left, HOP - 1 if (len(s) + b) % 2 else HOP + 1)
            s.append(c)
            left -= c
        sched.append(s)
    m = _model(args, sd)
    with m.open_wave_stream(5, max_samples=HOP + 1) as ws:
        D = ws.delay
        got = _push_all(ws, clips, sched)
        fins = []
        for b in range(5):
            others = [ws.state(o) for o in range(5) if o != b]
            out = ws.finish([b]).cpu()
            assert torch.count_nonzero(out[[o for o in range(5) if o != b]]) == 0
            assert all(torch.equal(s, ws.state(o)) for s, o in zip(others, [o for o in range(5) if o != b])), b
            assert ws.samples(b) == 0 and torch.count_nonzero(ws.state(b)) == 0
            fins.append(out[b])
        m.check_errors()
    for b, L in enumerate(lengths):
        _check(f"clip of {L} samples", torch.cat([got[b], fins[b]]), _oracle(sd, clips[b], args), D)


# ------------------------------------------------------------------------------------------------ slot counts
@pytest.mark.parametrize("slots", [1, 3, 33])
def test_slot_counts(slots):
    """Each slot its own 4-hop clip, a few slots idle throughout, two pushes of different counts per slot, then finish()."""
    args, L = _args("cumulative_layer_norm"), 4 * HOP
    sd = make_state_dict_fullsubnet(33, "default")
    idle = {b for b in range(slots) if slots > 2 and b % 7 == 2}
    clips = [None if b in idle else wave_clip(L, 2200 + b) for b in range(slots)]
    sched = [None if b in idle else [HOP + 17 * (b % 5), L - HOP - 17 * (b % 5)] for b in range(slots)]
    m = _model(args, sd)
    with m.open_wave_stream(slots, max_samples=L) as ws:
        D = ws.delay
        got = _push_all(ws, clips, sched)
        for b in idle:
            assert ws.samples(b) == 0 and torch.count_nonzero(ws.state(b)) == 0
        fin = ws.finish().cpu()
        m.check_errors()
    errs = []
    for b in range(slots):
        if b in idle:
            assert torch.count_nonzero(fin[b]) == 0 and got[b].numel() == 0
            continue
        full = torch.cat([got[b], fin[b]])
        assert torch.count_nonzero(full[:D]) == 0
        errs.append(_err(full[D:], _oracle(sd, clips[b], args)))
    print(f"S = {slots}: max rel err over {len(errs)} active slots {max(errs):.3e}")
    assert max(errs) < TOL, errs


# ------------------------------------------------------------------------------------------------ independence, reset, migration
def test_slots_are_independent_reset_starts_a_fresh_clip_and_state_migrates():
    args = _args("cumulative_laplace_norm")
    sd = make_state_dict_fullsubnet(34, "default")
    m = _model(args, sd)
    L = 5 * HOP + 40
    a, b = wave_clip(L, 2301), wave_clip(L, 2302)
    x = torch.stack([a, b, a]).cuda()
    c1, c2 = 2 * HOP + 9, 3 * HOP + 31

    def run(neighbours):
        """slot 1 is fed c1 + c2 samples; its neighbours are idle / active / reset in between -> (slot 1's outputs, its state)"""
        on = neighbours != "idle"
        with m.open_wave_stream(3, max_samples=c2) as ws:
            o1 = ws.push(x[:, :c1].contiguous(), [c1 if on else 0, c1, 300 if on else 0])
            before = ws.state(1)
            ws.push(x[:, :700].contiguous(), [700 if on else 0, 0, 0])              # counts[1] = 0: untouched, bit for bit
            assert torch.equal(ws.state(1), before)
            if neighbours == "reset":
                ws.reset([0, 2])
            o2 = ws.push(x[:, c1:c1 + c2].contiguous(), [c2 if on else 0, c2, 0])
            return torch.cat([o1[1, :c1], o2[1, :c2]]).clone(), ws.state(1).clone()

    ref_out, ref_state = run("idle")
    for nb in ("active", "reset"):
        out, state = run(nb)
        assert torch.equal(out, ref_out) and torch.equal(state, ref_state), nb
    # migration: slot 2 of a session of 4 continues bit-identically as slot 0 of a session of 2
    x4 = a.expand(4, -1).contiguous().cuda()
    with m.open_wave_stream(4, max_samples=c2) as w4, m.open_wave_stream(2, max_samples=c2) as w2:
        first = w4.push(x4[:, :c1].contiguous(), [0, 0, c1, 0])[2, :c1]
        blob = w4.state(2)
        assert blob.dtype == torch.uint8 and blob.numel() == w4.state_bytes == w2.state_bytes
        stay = w4.push(x4[:, c1:c1 + c2].contiguous(), [0, 0, c2, 0])[2]
        w2.load_state(0, blob)
        assert w2.samples(0) == c1
        moved = w2.push(x4[:2, c1:c1 + c2].contiguous(), [c2, 0])[0]
        assert torch.equal(moved, stay) and torch.equal(w2.state(0), w4.state(2)) and w2.samples(0) == c1 + c2 == L
        fin = w2.finish([0])[0]
        assert torch.equal(fin, w4.finish([2])[2])
        D = w2.delay
    _check("migrated stream", torch.cat([first, moved, fin]).cpu(), _oracle(sd, a, args), D)
    # reset of one slot mid-stream: it equals a fresh clip, its neighbour's bits stay
    with m.open_wave_stream(2, max_samples=L) as ws:
        ws.push(x[:2, :c1].contiguous())
        keep = ws.state(1)
        ws.reset([0])
        assert ws.samples(0) == 0 and ws.samples(1) == c1 and torch.equal(ws.state(1), keep)
        fresh = ws.push(x[:2].contiguous(), [L, 0])[0].cpu()
        fin = ws.finish([0])[0].cpu()
    m.check_errors()
    _check("slot reset mid-stream, then a fresh clip", torch.cat([fresh, fin]), _oracle(sd, a, args), D)


# ------------------------------------------------------------------------------------------------ serving properties
def _sleep_cycles_for(seconds):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    torch.cuda._sleep(20_000_000)
    torch.cuda.synchronize()
    return int(seconds / ((time.perf_counter() - t0) / 20_000_000))


def _ws_bytes(m):
    return int(re.search(r"workspace=(\d+) bytes", m.dump_config()).group(1))


def test_pushes_and_finish_never_synchronise_nor_grow():
    args = _args("cumulative_layer_norm")
    m = _model(args, make_state_dict_fullsubnet(35, "default"))
    x = torch.from_numpy(make_wave(8, 3 * HOP / 16000.0, 2401)).cuda()
    with m.open_wave_stream(8, max_samples=3 * HOP) as ws:
        ws.push(x)
        torch.cuda.synchronize()
        wsb, mem = _ws_bytes(m), torch.cuda.memory_allocated()
        ticks = _sleep_cycles_for(1.5)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            torch.cuda._sleep(ticks)
        t0 = time.perf_counter()
        counts = [768, 300, 0, 768, 1, 768, 768, 200]
        a = ws.push(x, counts)
        counts[0] = 1                                          # the caller may reuse its buffer as soon as the call returns
        b = ws.push(x[:, :HOP].contiguous())
        c = ws.finish([0, 3])
        host_s = time.perf_counter() - t0
        still_running = not side.query()
        torch.cuda.synchronize()
        m.check_errors()
        assert still_running and host_s < 0.5, (still_running, host_s)
        assert _ws_bytes(m) == wsb
        assert 0 <= torch.cuda.memory_allocated() - mem - (a.numel() + b.numel() + c.numel()) * 4 < 2048      # the outputs, nothing else
        assert [ws.samples(i) for i in range(8)] == [0, 1324, 1024, 0, 1025, 1792, 1792, 1224]


def test_nothing_else_moved():
    """The whole-clip forward and a mag-stream push give the same bits before, during and after a wave session on the same model."""
    args = _args("cumulative_layer_norm")
    m = _model(args, make_state_dict_fullsubnet(36, "default"), "sync")
    x = make_spec(3, 40, 811)[0].cuda()
    wav = wave_clip(3 * HOP, 2501).expand(2, -1).contiguous().cuda()

    def mag_push():
        with m.open_stream(3, max_chunk=8) as st:
            return st.push(x[..., :8].contiguous(), [8, 0, 3]), st.state(0)

    before, plan, (pb, sb) = m(x), m.describe_plan(3), mag_push()
    with m.open_wave_stream(2, max_samples=3 * HOP) as ws:
        ws.push(wav, [3 * HOP, 100])
        during, (pd, sd_) = m(x), mag_push()
        ws.finish([0])
    after, (pa, sa) = m(x), mag_push()
    assert torch.equal(before, during) and torch.equal(before, after) and m.describe_plan(3) == plan
    assert torch.equal(pb, pd) and torch.equal(pb, pa) and torch.equal(sb, sd_) and torch.equal(sb, sa)


def test_refusals_and_weight_edits():
    args = _args("cumulative_layer_norm")
    sd = make_state_dict_fullsubnet(37, "default")
    m = _model(args, sd, "sync")
    L = 8 * HOP + 5
    clip = wave_clip(L, 2601)
    x = torch.stack([clip, clip]).cuda()
    with m.open_wave_stream(2, max_samples=HOP) as ws:
        with pytest.raises(_lib.FsnpError, match=r"slot 1: count 201") as e:
            ws.push(x[:, :200].contiguous(), [200, 201])
        assert e.value.code == 2
        with pytest.raises(_lib.FsnpError, match=r"slot 0: count -1"):
            ws.push(x[:, :200].contiguous(), [-1, 2])
        with pytest.raises(_lib.FsnpError, match="max_samples"):
            ws.push(x[:, :HOP + 1].contiguous())
        assert ws.samples(0) == 0 and ws.samples(1) == 0            # nothing was enqueued
        ws.push(x[:, :HOP].contiguous(), [HOP, 0])
        with pytest.raises(_lib.FsnpError, match=r"slot 0 holds 256 samples") as e:
            ws.finish([0])
        assert e.value.code == 2 and ws.samples(0) == HOP
        with pytest.raises(_lib.FsnpError, match=r"slot 0 holds 256 samples"):
            ws.finish()
        assert ws.samples(0) == HOP
        assert torch.count_nonzero(ws.finish([1])) == 0            # an empty slot: a row of zeros
    # a .data edit between two pushes is noticed and re-packed before the next result
    first = 5 * HOP                                                # 5 frames, look_ahead 2: the masks of frames 0 .. 2 are the old weights'
    with m.open_wave_stream(1, max_samples=first) as ws:
        D = ws.delay
        o1 = ws.push(clip[None, :first].cuda())
        with torch.no_grad():
            m.sb_model.fc_output_layer.weight.data.mul_(2.0)
            m.sb_model.fc_output_layer.bias.data.mul_(2.0)
        o2 = ws.push(clip[None, first:].cuda())
        assert ws.samples(0) == L
        o3 = ws.finish()
    got = torch.cat([o1[0], o2[0], o3[0]]).cpu()
    sd2 = dict(sd)
    sd2["sb_model.fc_output_layer.weight"] = sd["sb_model.fc_output_layer.weight"] * 2.0
    sd2["sb_model.fc_output_layer.bias"] = sd["sb_model.fc_output_layer.bias"] * 2.0
    w1, w2 = _oracle(sd, clip, args), _oracle(sd2, clip, args)
    # sample i needs the masks of frames i / hop and i / hop + 1: below 2 hop the old weights' alone, from 3 hop on the edited ones' alone
    assert torch.count_nonzero(got[:D]) == 0
    e1 = float((got[D:D + 2 * HOP] - w1[:2 * HOP]).abs().max() / w1.abs().max())
    e2 = float((got[D + 3 * HOP:] - w2[3 * HOP:]).abs().max() / w2.abs().max())
    print(f"weight edit between pushes: before {e1:.3e}, after (edited weights) {e2:.3e}")
    assert e1 < TOL and e2 < TOL


def test_deferred_enhance_wave_answers_a_flagged_weight_edit_like_forward():
    """error_check="deferred": the enhance_wave after a .data edit runs on the OLD weights and is flagged; the next one warns, re-packs and
    returns the edited weights' waveform, as forward and the pushes do (it used to raise code 6)."""
    args = _args("cumulative_layer_norm")
    sd = make_state_dict_fullsubnet(37, "default")
    m = _model(args, sd)
    assert m.error_check == "deferred"
    clip = wave_clip(8 * HOP + 5, 2601)
    x = clip[None].cuda()
    m.enhance_wave(x)
    with torch.no_grad():
        m.sb_model.fc_output_layer.weight.data.mul_(2.0)
        m.sb_model.fc_output_layer.bias.data.mul_(2.0)
    m.enhance_wave(x)                                              # the flagged call
    torch.cuda.synchronize()
    with pytest.warns(RuntimeWarning, match="through .data"):
        got = m.enhance_wave(x)
    sd2 = dict(sd)
    sd2["sb_model.fc_output_layer.weight"] = sd["sb_model.fc_output_layer.weight"] * 2.0
    sd2["sb_model.fc_output_layer.bias"] = sd["sb_model.fc_output_layer.bias"] * 2.0
    err = _err(got[0].cpu(), _oracle(sd2, clip, args))
    print(f"deferred enhance_wave after a weight edit: rel err (edited weights) {err:.3e}")
    assert err < TOL, err
    m.refresh_weights()
    assert torch.equal(m.enhance_wave(x), got)
    m.check_errors()

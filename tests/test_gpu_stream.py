"""GPU tests of stream sessions of the original FullSubNet (include/fsnp_stream.h, FullSubNet.open_stream).

A clip pushed in any chunking, followed by look_ahead zero frames, must give - after dropping the first look_ahead columns - the whole-clip
mask of that clip alone.  Every comparison is against the reference's golden vectors or the torch-CPU oracle (never against the code under
test), tolerance 1e-3 rel (BASELINE.json north_star); the measured errors are printed."""
import re
import time

import numpy as np
import pytest
import torch

from fullsubnet_plus_amd import FullSubNet, _lib
from oracle import fsnp_torch
from oracle.make_golden import make_spec
from oracle.ref_loader import FULLSUBNET_MODEL_ARGS
from oracle.weights import make_state_dict_fullsubnet
from tests._stream_util import stream_kwargs
from tests._util import Golden, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-3
F = 257
torch.set_num_threads(16)


def _model(args, sd, error_check="sync"):
    m = FullSubNet(**args)
    m.load_state_dict(sd, strict=True)
    m = m.to("cuda").eval()
    m.batch_mode = "full"
    m.error_check = error_check
    return m


def _args(norm_type="cumulative_layer_norm", **kw):
    return dict(FULLSUBNET_MODEL_ARGS, norm_type=norm_type, **kw)


def _feed(stream, clips, schedules, la, nan_tail=True):
    """clips[b]: [1, 1, F, T_b] CPU (None = the slot stays idle); schedules[b]: chunk sizes of slot b, push by push (0 = idle in that push;
    all schedules equally long, sum = T_b).  Then the tail.  -> per slot [2, F, T_b + la] (CPU): the pushed columns in order; checks that
    everything past counts[b] is exactly 0 although the unread input holds NaN."""
    S = stream.slots
    npush = max(len(s) for s in schedules if s is not None)
    pos = [0] * S
    got = [[] for _ in range(S)]
    for k in range(npush):
        counts = [0 if schedules[b] is None else schedules[b][k] for b in range(S)]
        n = max(max(counts), 1)
        x = torch.full((S, 1, F, n), float("nan") if nan_tail else 0.0)
        for b in range(S):
            if counts[b]:
                x[b, ..., :counts[b]] = clips[b][0, ..., pos[b]:pos[b] + counts[b]]
                pos[b] += counts[b]
        out = stream.push(x.cuda(), counts).cpu()
        assert out.shape == (S, 2, F, n)
        for b in range(S):
            assert torch.count_nonzero(out[b, ..., counts[b]:]) == 0 and not torch.isnan(out[b]).any(), (k, b)
            got[b].append(out[b, ..., :counts[b]])
    if la:
        active = [b for b in range(S) if schedules[b] is not None]
        out = stream.tail(active).cpu()
        for b in active:
            got[b].append(out[b])
    return [torch.cat(g, dim=-1) if g else None for g in got]


def _check(name, got, want, la):
    """got [2, F, T + la] of one slot, want [2, F, T]: the first la columns exactly 0, the rest the whole-clip mask."""
    assert got.shape[-1] == want.shape[-1] + la, (got.shape, want.shape)
    assert torch.count_nonzero(got[..., :la]) == 0
    err = rel_err(got[..., la:].numpy(), np.asarray(want))
    print(f"{name}: rel err {err:.3e}")
    assert err < TOL, (name, err)
    return err


# ------------------------------------------------------------------------------------------------ the reference's golden vectors
def test_golden_cum_layer_in_chunks():
    g = Golden("fsn_b1_t30_cum_layer")
    m = _model(g.args, g.state_dict())
    mag = g.inputs()[0]
    with m.open_stream(1, max_chunk=16) as st:
        got = _feed(st, [mag], [[7, 1, 12, 10]], 2)
        assert st.frames(0) == 32
    _check("fsn_b1_t30_cum_layer (7, 1, 12, 10) + tail", got[0], g.arrays["out"][0], 2)


def test_golden_cum_laplace_three_slots_three_chunkings():
    g = Golden("fsn_b3_t18_cum_laplace")
    m = _model(g.args, g.state_dict())
    mag = g.inputs()[0]
    sched = [[18, 0, 0, 0, 0], [1, 5, 0, 6, 6], [4, 4, 4, 4, 2]]
    with m.open_stream(3, max_chunk=18) as st:
        got = _feed(st, [mag[b:b + 1] for b in range(3)], sched, 2)
    for b in range(3):
        _check(f"fsn_b3_t18_cum_laplace slot {b} {sched[b]}", got[b], g.arrays["full"][b], 2)


# ------------------------------------------------------------------------------------------------ chunking invariance
@pytest.mark.parametrize("norm_type", ["cumulative_layer_norm", "cumulative_laplace_norm"])
def test_chunking_invariance(norm_type):
    """Three slots, the same 120-frame clip: all at once, one frame per push, and a seeded random schedule with idle pushes."""
    args, T = _args(norm_type), 120
    sd = make_state_dict_fullsubnet(21, "default")
    mag = make_spec(1, T, 301)[0]
    want = fsnp_torch.forward_fullsubnet_full(sd, mag, **stream_kwargs(args))[0]
    rng = np.random.RandomState(7)
    rnd, left = [], T
    while left:
        c = 0 if rng.rand() < 0.3 else int(min(left, rng.randint(1, 9)))
        rnd.append(c)
        left -= c
    npush = max(T, len(rnd))
    sched = [[T] + [0] * (npush - 1), [1] * T + [0] * (npush - T), rnd + [0] * (npush - len(rnd))]
    m = _model(args, sd, "deferred")
    with m.open_stream(3, max_chunk=T) as st:
        got = _feed(st, [mag] * 3, sched, args["look_ahead"])
        m.check_errors()
    for b, nm in enumerate(("all at once", "n = 1", "random schedule")):
        _check(f"{norm_type} {nm}", got[b], want, args["look_ahead"])


def test_long_stream_error_does_not_grow():
    """One slot, 10 s (626 frames) in chunks of 4: the error over the last 100 frames is under the bar like that over the first 100."""
    args, T = _args("cumulative_layer_norm"), 626
    sd = make_state_dict_fullsubnet(22, "default")
    mag = make_spec(1, T, 302)[0]
    want = fsnp_torch.forward_fullsubnet_full(sd, mag, **stream_kwargs(args))[0].numpy()
    m = _model(args, sd, "deferred")
    with m.open_stream(1, max_chunk=4) as st:
        got = _feed(st, [mag], [[4] * 156 + [2]], 2)[0][..., 2:].numpy()
        m.check_errors()
    scale = np.abs(want).max()
    first, last = np.abs(got[..., :100] - want[..., :100]).max() / scale, np.abs(got[..., -100:] - want[..., -100:]).max() / scale
    print(f"long stream: rel err first 100 frames {first:.3e}, last 100 frames {last:.3e}, whole {rel_err(got, want):.3e}")
    assert first < TOL and last < TOL and rel_err(got, want) < TOL


# ------------------------------------------------------------------------------------------------ tile and round edges
@pytest.mark.parametrize("slots", [1, 2, 32, 33, 64])
def test_tile_and_round_edges(slots):
    """S * 257 rows below, at and above multiples of 32, more tiles than CUs (two rounds); each slot its own clip, a few slots idle, two
    pushes of different counts per slot (tiles that straddle two slots end at different steps)."""
    args = _args("cumulative_layer_norm")
    sd = make_state_dict_fullsubnet(23, "default")
    idle = {b for b in range(slots) if slots > 2 and b % 7 == 3}
    c1 = [0 if b in idle else 1 + b % 3 for b in range(slots)]
    c2 = [0 if b in idle else 3 - b % 2 for b in range(slots)]
    clips = [None if b in idle else make_spec(1, c1[b] + c2[b], 400 + b)[0] for b in range(slots)]
    sched = [None if b in idle else [c1[b], c2[b]] for b in range(slots)]
    m = _model(args, sd, "deferred")
    with m.open_stream(slots, max_chunk=4) as st:
        got = _feed(st, clips, sched, 2)
        m.check_errors()
        for b in idle:
            assert st.frames(b) == 0 and torch.count_nonzero(st.state(b)) == 0
    errs = []
    for b in range(slots):
        if b in idle:
            continue
        want = fsnp_torch.forward_fullsubnet_full(sd, clips[b], **stream_kwargs(args))[0]
        assert torch.count_nonzero(got[b][..., :2]) == 0
        errs.append(rel_err(got[b][..., 2:].numpy(), want.numpy()))
    print(f"S = {slots}: max rel err over {len(errs)} active slots {max(errs):.3e}")
    assert max(errs) < TOL, errs


# ------------------------------------------------------------------------------------------------ independence, reset, migration
@pytest.mark.parametrize("sb_hidden,fb_neighbors", [(256, 0), (384, 5), (256, 5)])
def test_other_row_tile_sizes(sb_hidden, fb_neighbors):
    """The other instantiations of the streaming row-tile kernel (csrc/lstm.hip lstm2_fc_stream_kernel): sb_model_hidden_size 256, and
    fb_num_neighbors 5 (42 sub-band inputs: K = 64), at S = 2 with pushes of different counts per slot."""
    args = _args("cumulative_laplace_norm", sb_model_hidden_size=sb_hidden, fb_num_neighbors=fb_neighbors)
    sd = make_state_dict_fullsubnet(29, "default", sb_hidden=sb_hidden, fb_num_neighbors=fb_neighbors)
    clips = [make_spec(1, 9, 450 + b)[0] for b in range(2)]
    m = _model(args, sd)
    with m.open_stream(2, max_chunk=4) as st:
        got = _feed(st, clips, [[1, 4, 1, 3], [4, 0, 2, 3]], 2)
        m.check_errors()
    for b in range(2):
        want = fsnp_torch.forward_fullsubnet_full(sd, clips[b], **stream_kwargs(args))[0]
        _check(f"sb hidden {sb_hidden}, fb neighbours {fb_neighbors}, slot {b}", got[b], want, 2)


def test_slots_are_independent_and_reset_starts_a_fresh_clip():
    args = _args("cumulative_laplace_norm")
    sd = make_state_dict_fullsubnet(24, "default")
    m = _model(args, sd, "deferred")
    a, b = make_spec(1, 12, 501)[0], make_spec(1, 12, 502)[0]
    x = torch.cat([a, b, a], dim=0).cuda()                     # slots 0 and 2 get the same clip

    def run(neighbours):
        """slot 1 is fed 5 + 7 frames; its neighbours are idle / active / reset in between -> (slot 1's outputs, its state)"""
        with m.open_stream(3, max_chunk=8) as st:
            o1 = st.push(x[..., :5].contiguous(), [5 if neighbours != "idle" else 0, 5, 3 if neighbours != "idle" else 0])
            before = st.state(1)
            st.push(x[..., :4].contiguous(), [4 if neighbours != "idle" else 0, 0, 0])       # counts[1] = 0: untouched, bit for bit
            assert torch.equal(st.state(1), before)
            if neighbours == "reset":
                st.reset([0, 2])
            o2 = st.push(x[..., 5:12].contiguous(), [7 if neighbours != "idle" else 0, 7, 0])
            return torch.cat([o1[1], o2[1, ..., :7]], dim=-1).clone(), st.state(1).clone()

    ref_out, ref_state = run("idle")
    for nb in ("active", "reset"):
        out, state = run(nb)
        assert torch.equal(out, ref_out) and torch.equal(state, ref_state), nb
    # reset of one slot mid-stream: it equals a fresh clip, its neighbour's bits stay
    with m.open_stream(2, max_chunk=12) as st:
        st.push(x[:2, ..., :6].contiguous())
        keep = st.state(1)
        st.reset([0])
        assert st.frames(0) == 0 and st.frames(1) == 6 and torch.equal(st.state(1), keep)
        fresh = st.push(x[:2].contiguous(), [12, 0])[0].cpu()
        tail = st.tail([0])[0].cpu()
    m.check_errors()
    want = fsnp_torch.forward_fullsubnet_full(sd, a, **stream_kwargs(args))[0]
    _check("slot reset mid-stream, then a fresh clip", torch.cat([fresh, tail], dim=-1), want, 2)


def test_state_migrates_between_sessions():
    """state() of slot 2 of one session, loaded into slot 0 of a session of another size, continues bit-identically."""
    args = _args("cumulative_layer_norm")
    sd = make_state_dict_fullsubnet(25, "default")
    m = _model(args, sd, "deferred")
    clip = make_spec(1, 14, 601)[0]
    x4 = clip.expand(4, -1, -1, -1).contiguous().cuda()
    with m.open_stream(4, max_chunk=8) as st4, m.open_stream(2, max_chunk=8) as st2:
        first = st4.push(x4[..., :6].contiguous(), [0, 0, 6, 0])[2]
        blob = st4.state(2)
        assert blob.dtype == torch.uint8 and blob.numel() == st4.state_bytes == st2.state_bytes
        stay = st4.push(x4[..., 6:].contiguous(), [0, 0, 8, 0])[2]
        st2.load_state(0, blob)
        assert st2.frames(0) == 6
        moved = st2.push(x4[:2, ..., 6:].contiguous(), [8, 0])[0]
        assert torch.equal(moved, stay) and torch.equal(st2.state(0), st4.state(2)) and st2.frames(0) == 14
        tail = st2.tail([0])[0]
    m.check_errors()
    want = fsnp_torch.forward_fullsubnet_full(sd, clip, **stream_kwargs(args))[0]
    _check("migrated stream", torch.cat([first, moved, tail], dim=-1).cpu(), want, 2)


# ------------------------------------------------------------------------------------------------ serving properties
def _sleep_cycles_for(seconds):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    torch.cuda._sleep(20_000_000)
    torch.cuda.synchronize()
    return int(seconds / ((time.perf_counter() - t0) / 20_000_000))


def _ws_bytes(m):
    return int(re.search(r"workspace=(\d+) bytes", m.dump_config()).group(1))


def test_pushes_never_synchronise_nor_grow():
    args = _args("cumulative_layer_norm")
    m = _model(args, make_state_dict_fullsubnet(26, "default"), "deferred")
    x = make_spec(8, 8, 701)[0].cuda()
    with m.open_stream(8, max_chunk=8) as st:
        st.push(x)
        torch.cuda.synchronize()
        ws, mem = _ws_bytes(m), torch.cuda.memory_allocated()
        ticks = _sleep_cycles_for(1.5)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            torch.cuda._sleep(ticks)
        t0 = time.perf_counter()
        counts = [8, 3, 0, 8, 1, 8, 8, 2]
        a = st.push(x, counts)
        counts[0] = 1                                          # the caller may reuse its buffer as soon as the call returns
        b = st.push(x[..., :4].contiguous())
        st.reset([2])
        host_s = time.perf_counter() - t0
        still_running = not side.query()
        torch.cuda.synchronize()
        m.check_errors()
        assert still_running and host_s < 0.5, (still_running, host_s)
        assert _ws_bytes(m) == ws
        assert 0 <= torch.cuda.memory_allocated() - mem - (a.numel() + b.numel()) * 4 < 2048      # the two outputs, nothing else
        assert [st.frames(i) for i in range(8)] == [20, 15, 0, 20, 13, 20, 20, 14]


def test_whole_clip_forward_is_untouched_by_a_session():
    args = _args("cumulative_layer_norm")
    m = _model(args, make_state_dict_fullsubnet(27, "default"))
    x = make_spec(3, 40, 801)[0].cuda()
    before, plan = m(x), m.describe_plan(3)
    with m.open_stream(5, max_chunk=8) as st:
        st.push(x[..., :8].repeat(2, 1, 1, 1)[:5].contiguous(), [8, 0, 3, 8, 1])
        during = m(x)
    after = m(x)
    assert torch.equal(before, during) and torch.equal(before, after) and m.describe_plan(3) == plan


def test_refusals_and_weight_edits():
    args = _args("cumulative_layer_norm")
    sd = make_state_dict_fullsubnet(28, "default")
    m = _model(args, sd)
    x = make_spec(2, 6, 901)[0].cuda()
    with m.open_stream(2, max_chunk=4) as st:
        with pytest.raises(_lib.FsnpError, match=r"slot 1: count 5") as e:
            st.push(x[..., :4].contiguous(), [4, 5])
        assert e.value.code == 2
        with pytest.raises(_lib.FsnpError, match=r"slot 0: count -1"):
            st.push(x[..., :4].contiguous(), [-1, 2])
        with pytest.raises(_lib.FsnpError, match="max_chunk"):
            st.push(x)
        assert st.frames(0) == 0 and st.frames(1) == 0            # nothing was enqueued
    props = torch.cuda.get_device_properties(0)
    with pytest.raises(_lib.FsnpError, match="slots") as e:
        m.open_stream(32 * (props.multi_processor_count // 16) + 1)
    assert e.value.code == 2
    # a .data edit between two pushes is noticed and re-packed before the next result
    clip = make_spec(1, 6, 902)[0]
    with m.open_stream(1, max_chunk=4) as st:
        o1 = st.push(clip[..., :4].contiguous().cuda())
        with torch.no_grad():
            m.sb_model.fc_output_layer.weight.data.mul_(2.0)
            m.sb_model.fc_output_layer.bias.data.mul_(2.0)
        o2 = st.push(torch.cat([clip[..., 4:], torch.zeros(1, 1, F, 2)], dim=-1).cuda())
        assert st.frames(0) == 8
    sd2 = dict(sd)
    sd2["sb_model.fc_output_layer.weight"] = sd["sb_model.fc_output_layer.weight"] * 2.0
    sd2["sb_model.fc_output_layer.bias"] = sd["sb_model.fc_output_layer.bias"] * 2.0
    w1 = fsnp_torch.forward_fullsubnet_full(sd, clip, **stream_kwargs(args))[0]
    w2 = fsnp_torch.forward_fullsubnet_full(sd2, clip, **stream_kwargs(args))[0]
    e1, e2 = rel_err(o1[0, ..., 2:].cpu().numpy(), w1[..., :2].numpy()), rel_err(o2[0].cpu().numpy(), w2[..., 2:].numpy())
    print(f"weight edit between pushes: before {e1:.3e}, after (edited weights) {e2:.3e}")
    assert e1 < TOL and e2 < TOL


def test_deferred_weight_edit_is_answered_by_the_push_after_the_flagged_one():
    """The error_check="deferred" twin of the weight-edit case above.  Nothing waits for the weight watch: the push after a .data edit runs
    on the OLD weights and is flagged (its output is not asserted); the push after that one is told, warns, re-packs and - like every
    push from then on - returns the edited weights' masks."""
    args = _args("cumulative_layer_norm")
    sd = make_state_dict_fullsubnet(28, "default")
    m = _model(args, sd, "deferred")
    clip = make_spec(1, 6, 902)[0]
    with m.open_stream(1, max_chunk=4) as st:
        o1 = st.push(clip[..., :2].contiguous().cuda())
        with torch.no_grad():
            m.sb_model.fc_output_layer.weight.data.mul_(2.0)
            m.sb_model.fc_output_layer.bias.data.mul_(2.0)
        st.push(clip[..., 2:4].contiguous().cuda())                # the flagged push
        torch.cuda.synchronize()
        with pytest.warns(RuntimeWarning, match="through .data"):
            o3 = st.push(torch.cat([clip[..., 4:], torch.zeros(1, 1, F, 2)], dim=-1).cuda())
        assert st.frames(0) == 8
        m.check_errors()
    sd2 = dict(sd)
    sd2["sb_model.fc_output_layer.weight"] = sd["sb_model.fc_output_layer.weight"] * 2.0
    sd2["sb_model.fc_output_layer.bias"] = sd["sb_model.fc_output_layer.bias"] * 2.0
    w2 = fsnp_torch.forward_fullsubnet_full(sd2, clip, **stream_kwargs(args))[0]
    assert torch.count_nonzero(o1) == 0                             # steps 0 and 1: look_ahead 2
    err = rel_err(o3[0].cpu().numpy(), w2[..., 2:].numpy())         # steps 4 .. 7: the masks of frames 2 .. 5
    print(f"deferred weight edit: after the warning (edited weights) {err:.3e}")
    assert err < TOL, err

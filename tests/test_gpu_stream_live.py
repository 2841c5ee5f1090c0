"""GPU tests of LIVE stream sessions (include/fsnp_stream_live.h, open_stream(..., live=True) / open_wave_stream(..., live=True)): the
per-step column-split kernels of csrc/lstm_step.hip behind the session interface of include/fsnp_stream.h.

The contract is the default session's: a clip pushed in any chunking, followed by look_ahead zero frames, gives - after dropping the first
look_ahead columns - the whole-clip mask of that clip alone.  Every comparison is against the reference's golden vectors or the torch-CPU
oracle (never against the code under test, and never against a default session), tolerance 1e-3 rel (BASELINE.json north_star); the
measured errors are printed.  Bit-for-bit comparisons are between two runs of the live path itself (independence, migration)."""
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
from tests._wave_stream_util import random_schedule, schedule, wave_clip
from tests.test_gpu_wave_stream import _check as _check_wave
from tests.test_gpu_wave_stream import _oracle as _oracle_wave
from tests.test_gpu_wave_stream import _push_all as _push_all_wave

pytestmark = pytest.mark.gpu
TOL = 1e-3
HOP = 256
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


def _feed(stream, clips, schedules, la, F=257):
    """clips[b]: [1, 1, F, T_b] CPU (None = the slot stays idle); schedules[b]: chunk sizes of slot b, push by push (0 = idle in that push).
    Then the tail.  -> per slot [2, F, T_b + la] (CPU).  The unread input holds NaN; everything past counts[b] must come back exactly 0."""
    S = stream.slots
    npush = max(len(s) for s in schedules if s is not None)
    pos = [0] * S
    got = [[] for _ in range(S)]
    for k in range(npush):
        counts = [0 if schedules[b] is None or k >= len(schedules[b]) else schedules[b][k] for b in range(S)]
        n = max(max(counts), 1)
        x = torch.full((S, 1, F, n), float("nan"))
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
    m = _model(g.args, g.state_dict(), "sync")
    mag = g.inputs()[0]
    with m.open_stream(1, max_chunk=16, live=True) as st:
        assert st.live is True
        got = _feed(st, [mag], [[7, 1, 12, 10]], 2)
        assert st.frames(0) == 32
    _check("live fsn_b1_t30_cum_layer (7, 1, 12, 10) + tail", got[0], g.arrays["out"][0], 2)


def test_golden_cum_laplace_three_slots_three_schedules():
    g = Golden("fsn_b3_t18_cum_laplace")
    m = _model(g.args, g.state_dict(), "sync")
    mag = g.inputs()[0]
    sched = [[1] * 18, [1, 5, 0, 6, 6] + [0] * 13, [4, 0, 4, 0, 4, 4, 0, 2] + [0] * 10]      # n = 1 throughout; idle pushes mixed in
    with m.open_stream(3, max_chunk=16, live=True) as st:
        got = _feed(st, [mag[b:b + 1] for b in range(3)], sched, 2)
    for b in range(3):
        _check(f"live fsn_b3_t18_cum_laplace slot {b}", got[b], g.arrays["full"][b], 2)


def test_f161_neighbors_10_look_ahead_1_tanh_against_the_oracle():
    """The arguments of the offline-norm fixture fsn_b3_t18_la1_nb10_f161_tanh with a cumulative norm: F = 161 (6 row tiles, the last one a
    single row), 21 + 1 sub-band inputs, look_ahead 1, Tanh on the output."""
    g = Golden("fsn_b3_t18_la1_nb10_f161_tanh")
    args = dict(g.args, norm_type="cumulative_layer_norm")
    sd = g.state_dict()
    mag = g.inputs()[0]
    assert mag.shape == (3, 1, 161, 18)
    sched = [[1] * 18, [3, 0, 5, 4, 6] + [0] * 13, [16, 2] + [0] * 16]
    m = _model(args, sd)
    with m.open_stream(3, max_chunk=16, live=True) as st:
        got = _feed(st, [mag[b:b + 1] for b in range(3)], sched, 1, F=161)
        m.check_errors()
    for b in range(3):
        want = fsnp_torch.forward_fullsubnet_full(sd, mag[b:b + 1], **stream_kwargs(args))[0]
        _check(f"live F=161 nb=10 la=1 tanh slot {b}", got[b], want, 1)


# ------------------------------------------------------------------------------------------------ tile and slice edges
@pytest.mark.parametrize("slots", [1, 2, 33])
def test_tile_and_slice_edges(slots):
    """S * 257 rows = 8 x 32 + 1, 16 x 32 + 2, 265 x 32 + 1; each slot its own clip, slots b % 7 == 3 idle at S = 33, two pushes of different
    counts per slot (tiles that straddle two slots end at different steps; the full-band row count crosses 8 and 16)."""
    args = _args("cumulative_layer_norm")
    sd = make_state_dict_fullsubnet(23, "default")
    idle = {b for b in range(slots) if slots > 2 and b % 7 == 3}
    c1 = [0 if b in idle else 1 + b % 3 for b in range(slots)]
    c2 = [0 if b in idle else 3 - b % 2 for b in range(slots)]
    clips = [None if b in idle else make_spec(1, c1[b] + c2[b], 400 + b)[0] for b in range(slots)]
    sched = [None if b in idle else [c1[b], c2[b]] for b in range(slots)]
    m = _model(args, sd)
    with m.open_stream(slots, max_chunk=4, live=True) as st:
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
    print(f"live S = {slots}: max rel err over {len(errs)} active slots {max(errs):.3e}")
    assert max(errs) < TOL, errs


@pytest.mark.parametrize("sb_hidden,fb_hidden", [(256, 512), (384, 300)])
def test_other_hidden_sizes(sb_hidden, fb_hidden):
    """sb_model_hidden_size 256 (16 column slices of 16 units) and fb_model_hidden_size 300 (38 slices of 8 units, the last one half
    empty; K = 557 and 600 are no multiples of the k-loop's stride) at S = 2."""
    args = _args("cumulative_laplace_norm", sb_model_hidden_size=sb_hidden, fb_model_hidden_size=fb_hidden)
    sd = make_state_dict_fullsubnet(29, "default", fb_hidden=fb_hidden, sb_hidden=sb_hidden)
    clips = [make_spec(1, 9, 450 + b)[0] for b in range(2)]
    m = _model(args, sd)
    with m.open_stream(2, max_chunk=4, live=True) as st:
        got = _feed(st, clips, [[1, 4, 1, 3], [4, 0, 2, 3]], 2)
        m.check_errors()
    for b in range(2):
        want = fsnp_torch.forward_fullsubnet_full(sd, clips[b], **stream_kwargs(args))[0]
        _check(f"live sb hidden {sb_hidden}, fb hidden {fb_hidden}, slot {b}", got[b], want, 2)


# ------------------------------------------------------------------------------------------------ independence, migration
def test_slots_are_independent_of_their_neighbours():
    args = _args("cumulative_laplace_norm")
    sd = make_state_dict_fullsubnet(24, "default")
    m = _model(args, sd)
    a, b = make_spec(1, 12, 501)[0], make_spec(1, 12, 502)[0]
    x = torch.cat([a, b, a], dim=0).cuda()

    def run(neighbours):
        """slot 1 is fed 5 + 7 frames; its neighbours are idle / active / reset in between -> (slot 1's outputs, its state)"""
        with m.open_stream(3, max_chunk=8, live=True) as st:
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
    m.check_errors()
    want = fsnp_torch.forward_fullsubnet_full(sd, b, **stream_kwargs(args))[0]
    err = rel_err(ref_out[..., 2:].cpu().numpy(), want[..., :10].numpy())
    print(f"live independence: slot 1 against the oracle, rel err {err:.3e}")
    assert err < TOL


@pytest.mark.parametrize("first_live", [False, True])
def test_state_migrates_between_the_two_modes(first_live):
    """6 frames in a session of one mode, state(), 8 frames + tail in a session of the other mode: the whole clip within tolerance."""
    args = _args("cumulative_layer_norm")
    sd = make_state_dict_fullsubnet(25, "default")
    m = _model(args, sd)
    clip = make_spec(1, 14, 601)[0]
    x = clip.cuda()
    with m.open_stream(1, max_chunk=8, live=first_live) as s1, m.open_stream(2, max_chunk=8, live=not first_live) as s2:
        assert s1.live is first_live and s2.live is (not first_live) and s1.state_bytes == s2.state_bytes
        first = s1.push(x[..., :6].contiguous())[0]
        s2.load_state(1, s1.state(0))
        assert s2.frames(1) == 6
        x2 = torch.cat([torch.full_like(x[..., 6:], float("nan")), x[..., 6:]], dim=0).contiguous()
        moved = s2.push(x2, [0, 8])[1]
        tail = s2.tail([1])[1]
        assert s2.frames(1) == 16 and s2.frames(0) == 0
    m.check_errors()
    want = fsnp_torch.forward_fullsubnet_full(sd, clip, **stream_kwargs(args))[0]
    _check(f"{'live -> default' if first_live else 'default -> live'} migration", torch.cat([first, moved, tail], dim=-1).cpu(), want, 2)


def test_state_migrates_between_live_sessions_bit_for_bit():
    """state() of slot 2 of a live session of 4 slots, loaded into slot 0 of a live session of 2 slots, continues bit-identically."""
    args = _args("cumulative_layer_norm")
    sd = make_state_dict_fullsubnet(25, "default")
    m = _model(args, sd)
    clip = make_spec(1, 14, 601)[0]
    x4 = clip.expand(4, -1, -1, -1).contiguous().cuda()
    with m.open_stream(4, max_chunk=8, live=True) as st4, m.open_stream(2, max_chunk=8, live=True) as st2:
        first = st4.push(x4[..., :6].contiguous(), [0, 0, 6, 0])[2]
        blob = st4.state(2)
        stay = st4.push(x4[..., 6:].contiguous(), [0, 0, 8, 0])[2]
        st2.load_state(0, blob)
        assert st2.frames(0) == 6
        moved = st2.push(x4[:2, ..., 6:].contiguous(), [8, 0])[0]
        assert torch.equal(moved, stay) and torch.equal(st2.state(0), st4.state(2)) and st2.frames(0) == 14
        tail = st2.tail([0])[0]
    m.check_errors()
    want = fsnp_torch.forward_fullsubnet_full(sd, clip, **stream_kwargs(args))[0]
    _check("live -> live migration", torch.cat([first, moved, tail], dim=-1).cpu(), want, 2)


# ------------------------------------------------------------------------------------------------ refusals, the other paths untouched
def test_refusals_and_the_other_paths_stay_bit_identical():
    args = _args("cumulative_layer_norm")
    m = _model(args, make_state_dict_fullsubnet(27, "default"), "sync")
    with pytest.raises(_lib.FsnpError, match=r"max_chunk 17 > 16") as e:
        m.open_stream(1, max_chunk=17, live=True)
    assert e.value.code == 2
    with pytest.raises(_lib.FsnpError, match=r"max_chunk 17 > 16") as e:
        m.open_wave_stream(1, max_samples=16 * HOP, live=True)          # 17 frames per push
    assert e.value.code == 2
    x = make_spec(3, 24, 801)[0].cuda()
    counts = [8, 3, 8]

    def default_session():
        with m.open_stream(3, max_chunk=8) as st:
            assert st.live is False
            return st.push(x[..., :8].contiguous(), counts).clone(), [st.state(b).clone() for b in range(3)]

    fwd_before, plan = m(x), m.describe_plan(3)
    def_before = default_session()
    with m.open_stream(2, max_chunk=16, live=True) as live, m.open_stream(3, max_chunk=8) as beside:
        assert live.live is True and beside.live is False
        live.push(x[:2, ..., :3].contiguous(), [3, 1])
        fwd_during = m(x)
        def_during = beside.push(x[..., :8].contiguous(), counts).clone(), [beside.state(b).clone() for b in range(3)]
        with pytest.raises(_lib.FsnpError, match="max_chunk"):
            live.push(x[:2, ..., :17].contiguous())
        with pytest.raises(_lib.FsnpError, match=r"slot 1: count 4") as e:
            live.push(x[:2, ..., :3].contiguous(), [3, 4])
        assert e.value.code == 2 and live.frames(0) == 3 and live.frames(1) == 1
    fwd_after = m(x)
    def_after = default_session()
    assert torch.equal(fwd_before, fwd_during) and torch.equal(fwd_before, fwd_after) and m.describe_plan(3) == plan
    for got in (def_during, def_after):
        assert torch.equal(got[0], def_before[0]) and all(torch.equal(p, q) for p, q in zip(got[1], def_before[1]))


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
    m = _model(args, make_state_dict_fullsubnet(26, "default"))
    x = make_spec(8, 8, 701)[0].cuda()
    with m.open_stream(8, max_chunk=8, live=True) as st:
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


# ------------------------------------------------------------------------------------------------ waveforms
@pytest.mark.parametrize("blocks", ["hop", "uneven"])
def test_live_wave_session_against_the_oracle(blocks):
    """Two slots, clips of 5 hop + 1 and 3 hop samples, one hop per push at most (max_samples = hop: 3 frames per push with the tail),
    then finish(): the oracle's enhance_wave of each clip, `delay` samples late."""
    args = _args("cumulative_layer_norm")
    sd = make_state_dict_fullsubnet(33, "default")
    lengths = [5 * HOP + 1, 3 * HOP]
    clips = [wave_clip(L, 2100 + i) for i, L in enumerate(lengths)]
    sched = ([schedule(L, HOP) for L in lengths] if blocks == "hop" else [schedule(lengths[0], 97), random_schedule(lengths[1], 12, HOP)])
    m = _model(args, sd)
    with m.open_wave_stream(2, max_samples=HOP, live=True) as ws:
        assert ws.live is True
        D = ws.delay
        got = _push_all_wave(ws, clips, sched)
        fin = ws.finish().cpu()
        m.check_errors()
    for b in range(2):
        _check_wave(f"live wave, blocks {blocks}, slot {b} ({lengths[b]} samples)", torch.cat([got[b], fin[b]]), _oracle_wave(sd, clips[b], args), D)

"""GPU tests of spectrum sessions of the original FullSubNet (include/fsnp_spec_stream.h, FullSubNet.open_spec_stream).

A clip of noisy STFT frames pushed in any chunking, followed by look_ahead zero frames, must give [look_ahead columns of exactly 0 | the
whole-clip enhanced frames of that clip alone].  Every comparison is against the torch-CPU oracle apply_cirm(forward_fullsubnet_full(sd,
|X|), X), never against the code under test; the error is max |got - want| / max |want| under 1e-3, as test_fullsubnet_enhance_epilogue
judges the whole-clip enhance().  Default sizes (the streaming kernels exist for them only): F = 257 is one bin past a 256-thread block.
The measured errors are printed."""
import functools
import gc
import re

import pytest
import torch

from fullsubnet_plus_amd import FullSubNet, _lib
from oracle.ref_loader import FULLSUBNET_MODEL_ARGS
from oracle.weights import make_state_dict_fullsubnet
from tests._spec_stream_util import crel_err, oracle_enhance, spec_clip
from tests._stream_util import stream_kwargs

pytestmark = pytest.mark.gpu
TOL = 1e-3
F = 257
NAN = complex(float("nan"), float("nan"))
SCHEDULES = [[18, 0, 0, 0, 0], [1, 5, 0, 6, 6], [4, 4, 4, 4, 2]]
torch.set_num_threads(16)


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_behind():
    """models and sessions of this module are gone from the GPU before the next module measures its own allocations"""
    yield
    gc.collect()


def _refused(fn, match, code=2):
    """fn() must fail with an FsnpError of `code` whose message matches; the exception (and the frames it holds) does not outlive the call"""
    try:
        fn()
    except _lib.FsnpError as e:
        assert e.code == code and re.search(match, str(e)), (e.code, str(e))
    else:
        raise AssertionError(f"no FsnpError (expected one matching {match!r})")


def _args(norm_type="cumulative_layer_norm", **kw):
    return dict(FULLSUBNET_MODEL_ARGS, norm_type=norm_type, **kw)


def _model(args, sd, error_check="deferred"):
    m = FullSubNet(**args)
    m.load_state_dict(sd, strict=True)
    m = m.to("cuda").eval()
    m.batch_mode = "full"
    m.error_check = error_check
    return m


@functools.lru_cache(maxsize=None)
def _case(norm_type, look_ahead, wseed, batch, frames, seed):
    """-> (args, state dict, clips [batch, F, frames] complex64 CPU, the oracle's enhanced clips): computed once, shared, never written to"""
    args = _args(norm_type, look_ahead=look_ahead)
    sd = make_state_dict_fullsubnet(wseed, "default")
    X = spec_clip(batch, frames, seed)
    return args, sd, X, oracle_enhance(sd, X, **stream_kwargs(args))


def _upload(x):
    """a CPU tensor with its strides (torch.stft's order: bins fastest) onto the GPU"""
    g = torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device="cuda")
    g.copy_(x)
    assert g.stride() == x.stride()
    return g


def _feed(ss, clips, schedules, la, max_chunk=None):
    """clips [S, F, T] complex CPU; schedules[b]: chunk sizes of slot b, push by push (0 = idle in that push; sum = T; a step longer than
    max_chunk goes as several pushes).  Then tail([b]) slot by slot.  -> [S, F, T + la] (CPU): the pushed columns in order.  The unread
    input columns hold NaN; everything past counts[b] must come back as exactly 0."""
    S = ss.slots
    pos, got = [0] * S, [[] for _ in range(S)]
    for k in range(len(schedules[0])):
        left = [schedules[b][k] for b in range(S)]
        while True:
            counts = [min(v, max_chunk or v) for v in left]
            n = max(max(counts), 1)
            x = torch.full((S, n, F), NAN, dtype=torch.complex64).transpose(1, 2)
            for b in range(S):
                x[b, :, :counts[b]] = clips[b, :, pos[b]:pos[b] + counts[b]]
                pos[b] += counts[b]
            out = ss.push(_upload(x), counts).cpu()
            assert out.shape == (S, F, n) and out.dtype == torch.complex64
            for b in range(S):
                assert torch.count_nonzero(out[b, :, counts[b]:]) == 0 and not torch.isnan(torch.view_as_real(out[b])).any(), (k, b)
                got[b].append(out[b, :, :counts[b]])
            left = [v - c for v, c in zip(left, counts)]
            if not any(left):
                break
    for b in range(S):
        out = ss.tail([b]).cpu()
        assert out.shape == (S, F, la)
        assert all(torch.count_nonzero(out[o]) == 0 for o in range(S) if o != b)
        got[b].append(out[b])
    return torch.stack([torch.cat(g, dim=-1) for g in got])


def _check(name, got, want, la):
    """got [F, T + la] of one slot, want [F, T]: the first la columns exactly 0, the rest the oracle's enhanced frames"""
    assert got.shape[-1] == want.shape[-1] + la, (got.shape, want.shape)
    assert torch.count_nonzero(got[:, :la]) == 0, name
    err = crel_err(got[:, la:], want)
    print(f"{name}: rel err {err:.3e}")
    assert err < TOL, (name, err)


@pytest.mark.parametrize("norm_type", ["cumulative_layer_norm", "cumulative_laplace_norm"])
def test_three_slots_three_chunkings(norm_type):
    args, sd, X, want = _case(norm_type, 2, 31, 3, 18, 1101)
    m = _model(args, sd)
    with m.open_spec_stream(3, max_chunk=18) as ss:
        assert not ss.live
        got = _feed(ss, X, SCHEDULES, 2)
        assert [ss.frames(b) for b in range(3)] == [20, 20, 20]
        m.check_errors()
    for b in range(3):
        _check(f"{norm_type} slot {b} {SCHEDULES[b]}", got[b], want[b], 2)


@pytest.mark.parametrize("look_ahead", [0, 1, 4])
def test_ring_shorter_equal_and_longer_than_a_push(look_ahead):
    """Slots fed in chunks of 1, look_ahead and look_ahead + 1 frames in the same pushes: the ring longer than a push, as long, shorter
    (it wraps at frame counts that are no multiple of look_ahead), the empty ring, and rows with different counts in one push."""
    T, la = 12, look_ahead
    args, sd, X, want = _case("cumulative_layer_norm", la, 32, 1, T, 1102)
    sizes = [1, max(la, 1), la + 1]
    sched = [[c] * (T // c) + ([T % c] if T % c else []) for c in sizes]
    sched = [s + [0] * (T - len(s)) for s in sched]
    m = _model(args, sd)
    with m.open_stream(1, max_chunk=1) as mag:
        mag_bytes = mag.state_bytes
    with m.open_spec_stream(3, max_chunk=max(la + 1, 4)) as ss:
        assert ss.state_bytes == mag_bytes + (la * F * 8 + 15) // 16 * 16      # the mag record, then the ring (empty for look_ahead 0)
        got = _feed(ss, X.expand(3, -1, -1), sched, la)
        m.check_errors()
    for b in range(3):
        _check(f"look_ahead {la}, chunks of {sizes[b]}", got[b], want[0], la)


def test_output_through_a_view_of_a_time_major_buffer():
    args, sd, X, want = _case("cumulative_layer_norm", 2, 31, 3, 18, 1101)
    m = _model(args, sd)
    with m.open_spec_stream(3, max_chunk=20) as ss:
        x = torch.cat([X, torch.zeros(3, F, 2, dtype=torch.complex64)], dim=-1)
        buf = torch.full((3, 20, F), NAN, dtype=torch.complex64, device="cuda")
        out = ss.push(_upload(x), out=buf.transpose(1, 2))
        assert out.data_ptr() == buf.data_ptr() and out.stride() == (20 * F, 1, F)
        m.check_errors()
        # a default output is laid out the same way: bins fastest, as torch.stft and torch.istft have it
        ss.reset()
        again = ss.push(_upload(x))
        assert again.stride() == (20 * F, 1, F) and torch.equal(again, out)
    for b in range(3):
        _check(f"[S, n, F] buffer through its [S, F, n] view, slot {b}", buf[b].cpu().T, want[b], 2)


def test_a_push_of_no_frames_leaves_the_record_untouched():
    args, sd, X, want = _case("cumulative_layer_norm", 2, 31, 3, 18, 1101)
    m = _model(args, sd)
    with m.open_spec_stream(2, max_chunk=8) as ss:
        first = ss.push(_upload(X[:2, :, :5]))
        before = [ss.state(b) for b in range(2)]
        x = torch.full((2, 4, F), NAN, dtype=torch.complex64).transpose(1, 2)
        out = ss.push(_upload(x), [0, 0])                          # nobody is fed
        assert torch.count_nonzero(out) == 0 and not torch.isnan(torch.view_as_real(out)).any()
        assert all(torch.equal(ss.state(b), before[b]) for b in range(2))
        x[0, :, :3] = X[0, :, 5:8]
        out = ss.push(_upload(x), [3, 0])                          # slot 1 idles beside an active slot
        assert torch.count_nonzero(out[1]) == 0 and torch.equal(ss.state(1), before[1]) and not torch.equal(ss.state(0), before[0])
        assert [ss.frames(b) for b in range(2)] == [8, 5]
        m.check_errors()
    got = torch.cat([first[0], out[0, :, :3]], dim=-1).cpu()
    _check("slot 0 around the idle pushes", got, want[0][:, :6], 2)


@pytest.mark.parametrize("norm_type", ["cumulative_layer_norm", "cumulative_laplace_norm"])
def test_live_session(norm_type):
    args, sd, X, want = _case(norm_type, 2, 31, 3, 18, 1101)
    m = _model(args, sd)
    with m.open_spec_stream(3, max_chunk=6, live=True) as ss:
        assert ss.live
        got = _feed(ss, X, SCHEDULES, 2, max_chunk=6)
        m.check_errors()
    for b in range(3):
        _check(f"live {norm_type} slot {b} {SCHEDULES[b]}", got[b], want[b], 2)
    _refused(lambda: m.open_spec_stream(1, max_chunk=17, live=True), r"fsnp_spec_stream_create_live: max_chunk 17 > 16")


def test_state_migrates_from_a_default_to_a_live_session():
    args, sd, X, want = _case("cumulative_layer_norm", 2, 31, 3, 18, 1101)
    m = _model(args, sd)
    with m.open_spec_stream(3, max_chunk=9) as dflt, m.open_spec_stream(2, max_chunk=9, live=True) as live, \
            m.open_stream(1, max_chunk=4) as mag:
        counts = [0, 0, 9]
        first = dflt.push(_upload(X[:, :, :9]), counts)[2]
        blob = dflt.state(2)
        assert blob.dtype == torch.uint8 and blob.numel() == dflt.state_bytes == live.state_bytes
        live.load_state(1, blob)
        assert live.frames(1) == 9 and torch.equal(live.state(1), blob)
        rest = live.push(_upload(X[1:, :, 9:]), [0, 9])[1]
        tail = live.tail([1])[1]
        # a mag-session record is another record: refused by its size
        assert mag.state_bytes == dflt.state_bytes - 2 * F * 8
        with pytest.raises(ValueError, match=f"{dflt.state_bytes} bytes"):
            dflt.load_state(0, mag.state(0))
        with pytest.raises(ValueError, match=f"{mag.state_bytes} bytes"):
            mag.load_state(0, blob)
        m.check_errors()
    _check("half in a default session, half in a live one", torch.cat([first, rest, tail], dim=-1).cpu(), want[2], 2)


def test_a_weight_edit_between_pushes_is_answered_with_the_record_put_back():
    """error_check="sync": the push after a .data edit first runs on the old weights, is flagged, and runs again on the edited ones from the
    slot's record as it was - frame count and waiting spectra included: its first two columns are frames 2 and 3 out of the ring."""
    args = _args("cumulative_layer_norm")
    sd = make_state_dict_fullsubnet(28, "default")
    m = _model(args, sd, "sync")
    X = spec_clip(1, 6, 1103)
    kw = stream_kwargs(args)
    with m.open_spec_stream(1, max_chunk=4) as ss:
        o1 = ss.push(_upload(X[:, :, :4]))
        with torch.no_grad():
            m.sb_model.fc_output_layer.weight.data.mul_(2.0)
            m.sb_model.fc_output_layer.bias.data.mul_(2.0)
        o2 = ss.push(_upload(torch.cat([X[:, :, 4:], torch.zeros(1, F, 2, dtype=torch.complex64)], dim=-1)))
        assert ss.frames(0) == 8
    sd2 = dict(sd)
    sd2["sb_model.fc_output_layer.weight"] = sd["sb_model.fc_output_layer.weight"] * 2.0
    sd2["sb_model.fc_output_layer.bias"] = sd["sb_model.fc_output_layer.bias"] * 2.0
    w1, w2 = oracle_enhance(sd, X, **kw)[0], oracle_enhance(sd2, X, **kw)[0]
    assert torch.count_nonzero(o1[0, :, :2]) == 0
    e1, e2 = crel_err(o1[0, :, 2:].cpu(), w1[:, :2]), crel_err(o2[0].cpu(), w2[:, 2:])
    print(f"weight edit between pushes: before {e1:.3e}, after (edited weights) {e2:.3e}")
    assert e1 < TOL and e2 < TOL

"""GPU tests of the device-side weight hand-over (include/fsnp_device_weights.h, model.weight_upload): the blob the pack kernels build is
BYTE for byte the blob the host packer builds from the same weights - for every golden fixture's configuration - so every output is
bit-identical, a re-commit packs in place, and the ordering / lifetime promises of the two new entry points hold.  No tolerance
anywhere: the yardstick is the host path, which is the code in front of this feature."""
import ctypes

import numpy as np
import pytest
import torch

from fullsubnet_plus_amd import FullSubNet, FullSubNet_Plus, _lib
from oracle.make_golden import make_spec
from oracle.ref_loader import DEFAULT_MODEL_ARGS, FULLSUBNET_MODEL_ARGS
from oracle.weights import make_state_dict, make_state_dict_fullsubnet
from tests._util import Golden, golden_names

pytestmark = pytest.mark.gpu
torch.set_num_threads(16)


def _device():
    return torch.device("cuda", torch.cuda.current_device())


def _model(cls, args, sd, upload, **attrs):
    m = cls(**args)
    m.load_state_dict(sd, strict=True)
    m = m.to("cuda").eval()
    m.weight_upload = upload
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def _blob_of(handle):
    lib = _lib.load()
    need = ctypes.c_int64()
    _lib.check(lib.fsnp_debug_weight_blob(handle, None, 0, ctypes.byref(need)), "fsnp_debug_weight_blob")
    buf = np.empty(need.value, np.uint8)
    _lib.check(lib.fsnp_debug_weight_blob(handle, buf.ctypes.data, need.value, None), "fsnp_debug_weight_blob")
    return buf


def _stats_of(handle):
    out = (ctypes.c_int64 * 4)()
    _lib.check(_lib.load().fsnp_debug_commit_stats(handle, ctypes.byref(out)), "fsnp_debug_commit_stats")
    return list(out)


def _same_bytes(a, b):
    if a.shape != b.shape:
        return False
    bad = np.flatnonzero(a != b)
    if bad.size:
        print(f"{bad.size} bytes differ, first at float {bad[0] // 4} of {a.size // 4}")
    return bad.size == 0


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------------ every golden fixture, both models
@pytest.mark.parametrize("name", golden_names("plus") + golden_names("fullsubnet"))
def test_fixture_blob_and_output_are_identical(name):
    g = Golden(name)
    cls = FullSubNet if g.is_fullsubnet else FullSubNet_Plus
    sd = g.state_dict()
    dev = _device()
    host, devm = _model(cls, g.args, sd, "host"), _model(cls, g.args, sd, "device")
    host._ensure_handle(dev)                      # commit without a forward
    devm._ensure_handle(dev)
    sh, sdv = _stats_of(host._handle), _stats_of(devm._handle)
    print(f"{name}: host path copied {sh[1]} bytes up; device path {sdv[3]} kernels, {sdv[1]} bytes up, {sdv[2]} bytes down")
    assert sh[0] == 0 and sdv[0] == 1 and sdv[2] == 0 and sdv[3] > 0
    assert _same_bytes(_blob_of(host._handle), _blob_of(devm._handle))
    ins = [t[:5, ..., :30].cuda() for t in g.inputs()[:1 if g.is_fullsubnet else 3]]      # (FullSubNet takes the magnitude alone)
    with torch.no_grad():
        assert _bits(host(*ins)) == _bits(devm(*ins))


# ------------------------------------------------------------------------------------------------ re-commit in place
def test_recommit_packs_into_the_existing_allocation():
    lib = _lib.load()
    mag, real, imag = [t.cuda() for t in make_spec(2, 12, 5)]
    sd_a, sd_b = make_state_dict(1, "default"), make_state_dict(2, "harsh")
    m = _model(FullSubNet_Plus, DEFAULT_MODEL_ARGS, sd_a, "device", batch_mode="full")
    with torch.no_grad():
        first = m(mag, real, imag)
        addr = lib.fsnp_debug_weight_blob_ptr(m._handle)
        m.load_state_dict(sd_b, strict=True)
        second = m(mag, real, imag)
        fresh = _model(FullSubNet_Plus, DEFAULT_MODEL_ARGS, sd_b, "host", batch_mode="full")
        want = fresh(mag, real, imag)
    st = _stats_of(m._handle)
    assert st[0] == 1 and st[2] == 0 and st[1] < 4096, st           # (up: the unfold multiplicities only)
    assert lib.fsnp_debug_weight_blob_ptr(m._handle) == addr and addr
    assert _same_bytes(_blob_of(m._handle), _blob_of(fresh._handle))
    assert _bits(second) == _bits(want) and _bits(first) != _bits(second)


def test_data_edit_is_repacked_through_the_device_path():
    """An edit through .data bumps no pointer and no version: the weight watch notices it, the forward re-packs and re-runs."""
    mag, real, imag = [t.cuda() for t in make_spec(1, 10, 7)]
    m = _model(FullSubNet_Plus, DEFAULT_MODEL_ARGS, make_state_dict(3, "default"), "auto", error_check="sync")
    with torch.no_grad():
        before = m(mag, real, imag)
        key = m._weights_key()
        m.sb_model.fc_output_layer.bias.data.add_(0.25)
        m.fb_model.sequence_model[0].conv1x1.weight.data.mul_(1.5)
        assert m._weights_key() == key
        after = m(mag, real, imag)
        sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        want = _model(FullSubNet_Plus, DEFAULT_MODEL_ARGS, sd, "host")(mag, real, imag)
    st = _stats_of(m._handle)
    assert st[0] == 1 and st[2] == 0, st
    assert _bits(after) == _bits(want) and _bits(after) != _bits(before)


# ------------------------------------------------------------------------------------------------ an open stream session
def test_open_stream_session_across_a_weight_change():
    args = dict(FULLSUBNET_MODEL_ARGS, norm_type="cumulative_layer_norm")
    sd_a, sd_b = make_state_dict_fullsubnet(1, "default"), make_state_dict_fullsubnet(2, "harsh")
    F = args.get("num_freqs", 257)
    x = make_spec(2, 8, 11)[0].cuda()             # [2, 1, F, 8]
    assert x.shape == (2, 1, F, 8)
    m = _model(FullSubNet, args, sd_a, "device", batch_mode="full", error_check="sync")
    with m.open_stream(2, max_chunk=4) as st:
        st.push(x[..., :4])
        states = [st.state(b).clone() for b in range(2)]
        m.load_state_dict(sd_b, strict=True)
        got = st.push(x[..., 4:])
        stats = _stats_of(m._handle)
    fresh = _model(FullSubNet, args, sd_b, "host", batch_mode="full", error_check="sync")
    with fresh.open_stream(2, max_chunk=4) as st:
        for b in range(2):
            st.load_state(b, states[b])
        want = st.push(x[..., 4:])
    assert stats[0] == 1 and stats[2] == 0, stats
    assert torch.count_nonzero(got) > 0 and _bits(got) == _bits(want)


# ------------------------------------------------------------------------------------------------ the C ABI itself
class _Raw:
    """A handle of the default FullSubNet+ driven through ctypes, and its state dict on the GPU."""

    def __init__(self, sd):
        self.lib = _lib.load()
        cfg = FullSubNet_Plus(**DEFAULT_MODEL_ARGS)._config()
        self.h = ctypes.c_void_p()
        _lib.check(self.lib.fsnp_create(ctypes.byref(cfg), ctypes.byref(self.h)), "fsnp_create")
        self.names = []
        for i in range(self.lib.fsnp_num_weights(self.h)):
            name, numel = ctypes.c_char_p(), ctypes.c_int64()
            _lib.check(self.lib.fsnp_weight_info(self.h, i, ctypes.byref(name), ctypes.byref(numel)), "fsnp_weight_info")
            self.names.append(name.value.decode())
        self.cpu = {k: sd[k].detach().to(torch.float32).contiguous() for k in self.names}
        self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.keep = []

    def readers(self, ins):
        """One call of every kind of blob reader on the CURRENT stream: the forward (full mode), the sub-band model alone, and the two
        stage calls on the magnitude -> their outputs."""
        B, _, F, T = ins[0].shape
        out = torch.empty((B, 2, F, T), device="cuda")
        strides = (ctypes.c_int64 * 3 * 3)()
        for i, t in enumerate(ins):
            strides[i][0], strides[i][1], strides[i][2] = t.stride(0), t.stride(2), t.stride(3)
        _lib.check(self.lib.fsnp_forward(self.h, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), ctypes.byref(strides),
                                         out.data_ptr(), B, T, _lib.MODE_FULL, 0, B, self.stream), "fsnp_forward")
        st1 = (ctypes.c_int64 * 3)(ins[0].stride(0), ins[0].stride(2), ins[0].stride(3))
        att, fb = torch.empty((B, F, T), device="cuda"), torch.empty((B, F, T), device="cuda")
        _lib.check(self.lib.fsnp_channel_attention(self.h, 0, ins[0].data_ptr(), ctypes.byref(st1), att.data_ptr(), B, T, self.stream),
                   "fsnp_channel_attention")
        _lib.check(self.lib.fsnp_fullband_model(self.h, 1, ins[0].data_ptr(), ctypes.byref(st1), fb.data_ptr(), B, T, self.stream),
                   "fsnp_fullband_model")
        x = torch.linspace(-1, 1, 40 * 6 * 34, device="cuda").reshape(40, 6, 34).contiguous()      # (31 sub-band + 3 full-band inputs)
        sb = torch.empty((40, 2, 6), device="cuda")
        _lib.check(self.lib.fsnp_lstm2_fc(self.h, x.data_ptr(), sb.data_ptr(), 40, 6, self.stream), "fsnp_lstm2_fc")
        return out, att, fb, sb

    def host(self, name, numel=None):
        t = self.cpu[name]
        return self.lib.fsnp_set_weight(self.h, name.encode(), t.data_ptr(), t.numel() if numel is None else numel)

    def device(self, name, numel=None, scribble=False, stream=None):
        t = self.cpu[name].cuda()
        if stream is not None:
            self.keep.append(t)                   # (the copy runs on a stream torch's allocator knows nothing of)
        rc = self.lib.fsnp_set_weight_device(self.h, name.encode(), t.data_ptr(), t.numel() if numel is None else numel,
                                             self.stream if stream is None else ctypes.c_void_p(stream.cuda_stream))
        if scribble:
            t.fill_(float("nan"))                 # in stream order behind the hand-over: the arena must hold its own copy
        return rc

    def close(self):
        self.lib.fsnp_destroy(self.h)


@pytest.fixture(scope="module")
def default_sd():
    return make_state_dict(4, "default")


@pytest.fixture(scope="module")
def host_blob(default_sd):
    r = _Raw(default_sd)
    for n in r.names:
        assert r.host(n) == 0
    _lib.check(r.lib.fsnp_commit_weights(r.h), "fsnp_commit_weights")
    assert _stats_of(r.h)[0] == 0
    blob = _blob_of(r.h)
    r.close()
    return blob


def test_mixed_handover_takes_the_host_path(default_sd, host_blob):
    r = _Raw(default_sd)
    for i, n in enumerate(r.names):
        assert (r.host(n) if i % 2 else r.device(n)) == 0
    _lib.check(r.lib.fsnp_commit_weights_on(r.h, r.stream), "fsnp_commit_weights_on")
    st = _stats_of(r.h)
    assert st[0] == 0 and st[2] == sum(4 * r.cpu[n].numel() for n in r.names[0::2]) and st[3] == 0, st
    assert _same_bytes(_blob_of(r.h), host_blob)
    r.close()
    # plain fsnp_commit_weights after a device-only hand-over: everything comes down, the host packs
    r = _Raw(default_sd)
    for n in r.names:
        assert r.device(n) == 0
    _lib.check(r.lib.fsnp_commit_weights(r.h), "fsnp_commit_weights")
    st = _stats_of(r.h)
    assert st[0] == 0 and st[2] == sum(4 * t.numel() for t in r.cpu.values()), st
    assert _same_bytes(_blob_of(r.h), host_blob)
    # ... and the same handle packs on the device when asked to: its arena still holds every tensor
    _lib.check(r.lib.fsnp_commit_weights_on(r.h, r.stream), "fsnp_commit_weights_on")
    assert _stats_of(r.h)[0] == 1 and _stats_of(r.h)[2] == 0
    assert _same_bytes(_blob_of(r.h), host_blob)
    r.close()


def test_errors_are_the_host_setters(default_sd):
    r = _Raw(default_sd)
    lib, first = r.lib, r.names[0]
    assert lib.fsnp_commit_weights_on(r.h, r.stream) == 2
    on = _lib.last_error()
    assert lib.fsnp_commit_weights(r.h) == 2
    assert on == _lib.last_error() == f"missing key in state_dict: {first}"
    x = torch.zeros(8, device="cuda")
    assert lib.fsnp_set_weight_device(r.h, b"no.such.tensor", x.data_ptr(), 8, r.stream) == 2
    dev_msg = _lib.last_error()
    assert lib.fsnp_set_weight(r.h, b"no.such.tensor", r.cpu[first].data_ptr(), 8) == 2
    assert dev_msg == _lib.last_error() == "unexpected key in state_dict: no.such.tensor"
    wrong = r.cpu[first].numel() - 1
    assert r.device(first, numel=wrong) == 2
    dev_msg = _lib.last_error()
    assert r.host(first, numel=wrong) == 2
    assert dev_msg == _lib.last_error() and dev_msg.startswith(f"size mismatch for {first}: expected {wrong + 1} elements, got {wrong}")
    for n in r.names[:-1]:
        assert r.device(n) == 0
    assert lib.fsnp_commit_weights_on(r.h, r.stream) == 2
    assert _lib.last_error() == f"missing key in state_dict: {r.names[-1]}"
    r.close()


def test_source_tensors_may_be_overwritten_right_after_the_handover(default_sd, host_blob):
    r = _Raw(default_sd)
    for n in r.names:
        assert r.device(n, scribble=True) == 0
    _lib.check(r.lib.fsnp_commit_weights_on(r.h, r.stream), "fsnp_commit_weights_on")
    st = _stats_of(r.h)
    assert st[0] == 1 and st[2] == 0, st
    assert _same_bytes(_blob_of(r.h), host_blob)
    r.close()


def test_readers_on_another_stream_wait_for_a_pack_on_a_side_stream(default_sd):
    """fsnp_commit_weights_on returns with the pack enqueued.  The hand-over runs on two side streams that are kept busy, the commit on
    one of them; the forward, the sub-band model and the two stage calls then go to the current stream AT ONCE.  Each must wait for
    the pack on the device - a reader that did not would run while the side stream is still busy and read a blob that is not
    written yet - and give, bit for bit, what a handle packed on the host and read on one stream gives."""
    ins = [t.cuda() for t in make_spec(2, 12, 5)]
    ref = _Raw(default_sd)
    for n in ref.names:
        assert ref.host(n) == 0
    _lib.check(ref.lib.fsnp_commit_weights(ref.h), "fsnp_commit_weights")
    want = [_bits(t) for t in ref.readers(ins)]
    ref.close()
    r = _Raw(default_sd)
    side = [torch.cuda.Stream(), torch.cuda.Stream()]
    busy = torch.full((8192, 8192), 1e-4, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side[0]):
        for _ in range(24):                       # some hundred milliseconds in front of the hand-over
            busy = busy @ busy
    for i, n in enumerate(r.names):
        assert r.device(n, stream=side[i % 2]) == 0
    _lib.check(r.lib.fsnp_commit_weights_on(r.h, ctypes.c_void_p(side[0].cuda_stream)), "fsnp_commit_weights_on")
    assert not side[0].query(), "the side stream finished before the readers were enqueued: the test showed nothing"
    got = [_bits(t) for t in r.readers(ins)]
    torch.cuda.synchronize()
    assert _stats_of(r.h)[0] == 1
    for name, g, w in zip(("forward", "channel_attention", "fullband_model", "lstm2_fc"), got, want):
        assert g == w, name
    r.close()

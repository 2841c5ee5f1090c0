"""CPU tests of the device-side weight hand-over (include/fsnp_device_weights.h): the bindings, the argument checks that touch no
device, the Python chooser - and every weight image's layout.  fsnp_debug_pack_emulate walks an image on the host through the very
functions the device pack kernels run (csrc/weight_layouts.h); it is compared byte for byte

  * with the packers this tree had BEFORE the layouts moved into that header: tests/golden/pack_digests.json holds the SHA-256 of what
    each of them wrote for the sources of _values() below (integer arithmetic, so the same on every numpy).  How it was recorded:
    libfsnp_hip.so was built at commit f4848bd ("Run wave sessions on the spectrum ring push; share slot helpers"), the last one with
    the per-kernel packers fsnp::lstm_pack_weights, lstm_pack_weights_bf16ih, lstm16_pack_weights, lstm16_pack_weights_bf16ih,
    gru_pack_weights, lstm_coop_pack_weights, lstm_coopn_pack_weights, lstm_hp_pack_weights, lstm_hpw_pack_weights,
    lstm_coopw_pack_weights, lstm_fbv_pack_weights and lstm_generic_pack_weights; tools/record_pack_digests.py called each of them
    through ctypes (they are exported under their C++ names) on case_sources() of every rnn_cases() entry - four-slot matrices, for the
    GRU image spread() of the [3H] tensors, for the bf16 row-tile image bias_ih_l0 + bias_hh_l0 as its fifth source - and wrote the
    digests.  The file cannot be regenerated from this tree (those packers are gone): it is a recorded result, like the golden vectors;
  * with the fsnp_debug_*_pack hooks, where one exists.  Hook and emulation now run the same functions, so this says nothing about a
    layout by itself: it ties the emulation to the hooks' argument handling, and through them to the INDEPENDENT numpy restatements
    of the MFMA fragment layouts in tests/test_host.py (test_lstm_pack_matches_mfma_fragment_emulation,
    test_lstm_coop_pack_matches_mfma_fragment_emulation and the hpw / coopw / fbv kernel restatements), which read the hooks' output;
  * with a plain numpy restatement for what the old commit built inline (GRU spread, summed biases, TCN operands, GroupNorm fold)."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from fullsubnet_plus_amd import FullSubNet_Plus, _lib
from oracle.ref_loader import DEFAULT_MODEL_ARGS

HERE = os.path.dirname(os.path.abspath(__file__))
(ROWTILE, ROWTILE_BF, HALF, HALF_BF, GRU, KSPLIT, COOPN, HP, HPW, COOPW, FBV, GENERIC, BIAS, SPREAD, PADMAT, TRANSPOSE, FOLDW,
 FOLDC) = range(18)
SIZES = [(384, 33, 40), (256, 33, 40), (384, 64, 64), (512, 33, 40)]


def _values(seed, n):
    """n reproducible floats in [-0.5, 0.5): a multiplicative hash of the index, exact in integer arithmetic."""
    i = np.arange(n, dtype=np.uint64)
    x = (i * np.uint64(2654435761) + np.uint64(seed * 40503 + 12345)) % np.uint64(1 << 32)
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(1103515245)) % np.uint64(1 << 32)
    return ((x >> np.uint64(8)).astype(np.float64) / float(1 << 24) - 0.5).astype(np.float32)


def rnn_sources(H, NIN, gates=4, seed=1):
    """weight_ih_l0, weight_hh_l0, weight_ih_l1, weight_hh_l1, bias_ih_l0, bias_hh_l0, bias_ih_l1, bias_hh_l1 of nn.LSTM / nn.GRU"""
    shapes = [(gates * H, NIN), (gates * H, H), (gates * H, H), (gates * H, H)] + [(gates * H,)] * 4
    return [_values(seed + 7 * i, int(np.prod(s))).reshape(s) for i, s in enumerate(shapes)]


def emulate(kind, sizes, sources, expect=0):
    lib = _lib.load()
    sz = (ctypes.c_int32 * len(sizes))(*sizes)
    srcs = [np.ascontiguousarray(s, dtype=np.float32) for s in sources]
    ptrs = (ctypes.c_void_p * len(srcs))(*[s.ctypes.data for s in srcs])
    nums = (ctypes.c_int64 * len(srcs))(*[s.size for s in srcs])
    # the image's size comes back in the message of a call that asks for the wrong one
    rc = lib.fsnp_debug_pack_emulate(kind, sz, len(sizes), ptrs, nums, len(srcs), np.zeros(1, np.float32).ctypes.data, -1)
    msg = _lib.last_error()
    if "need" not in msg:
        assert rc == expect and rc != 0, (rc, msg)
        return None
    n = int(msg.split("need")[1].split()[0])
    out = np.full(n, np.float32(np.nan))          # (every float must be written)
    rc = lib.fsnp_debug_pack_emulate(kind, sz, len(sizes), ptrs, nums, len(srcs), out.ctypes.data, n)
    assert rc == expect, (rc, _lib.last_error())
    return out


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def spread(src, H, hidden):
    """[3H][cols] of a GRU -> the four-slot [4H][cols]: r, z, then n in slot 2 (input matrices) or 3 (hidden matrices)"""
    dst = np.zeros((4 * H, src.shape[1]), np.float32)
    dst[:2 * H] = src[:2 * H]
    dst[(3 if hidden else 2) * H:(4 if hidden else 3) * H] = src[2 * H:]
    return dst


# (id, kind, sizes) of every recurrent image the old packers wrote; the id is the key of the recorded digest
def rnn_cases():
    cases = []
    for H, NIN, KX in SIZES:
        if H in (384, 256):
            for nw in (4, 12) if H == 384 else (4,):
                cases.append((f"rowtile-{H}-{NIN}-{KX}-nw{nw}", ROWTILE, (H, NIN, KX, nw)))
            cases.append((f"half-{H}-{NIN}-{KX}", HALF, (H, NIN, KX)))
            cases.append((f"hp-{H}-{NIN}-{KX}", HP, (H, NIN, KX)))
            cases.append((f"hpw-{H}-{NIN}-{KX}", HPW, (H, NIN, KX)))
        if H == 384:
            cases.append((f"coopw-{H}-{NIN}-{KX}", COOPW, (H, NIN, KX)))
            cases.append((f"gru-{H}-{NIN}-{KX}", GRU, (H, NIN, KX, 4, 1)))
        for units in (8, 16, 32, 64):
            cases.append((f"ksplit-{H}-{NIN}-{KX}-u{units}", KSPLIT, (H, NIN, KX, units)))
        cases.append((f"coopn-{H}-{NIN}-{KX}", COOPN, (H, NIN, KX)))
    for nw in (4, 12):
        cases.append((f"rowtile_bf-384-33-40-nw{nw}", ROWTILE_BF, (384, 33, 40, nw)))
    cases.append(("half_bf-384-33-40", HALF_BF, (384, 33, 40)))
    for units in (8, 16, 32):
        cases.append((f"fullband-ksplit-512-257-264-u{units}", KSPLIT, (512, 257, 264, units)))
    cases.append(("fullband-fbv-512-257", FBV, (512, 257)))
    cases.append(("fullband-generic-512-257", GENERIC, (512, 257)))
    cases.append(("generic-320-33", GENERIC, (320, 33)))
    cases.append(("generic-190-35", GENERIC, (190, 35)))
    return cases


def case_sources(kind, sizes):
    gru = len(sizes) > 4 and sizes[4] == 1
    return rnn_sources(sizes[0], sizes[1], 3 if gru else 4, seed=sizes[0] + sizes[1])


with open(os.path.join(HERE, "golden", "pack_digests.json")) as _f:
    DIGESTS = json.load(_f)


def test_new_symbols_are_bound_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.fsnp_abi_version() == 13 == _lib.ABI_VERSION
    for name in ("fsnp_set_weight_device", "fsnp_commit_weights_on"):
        assert name in _lib.DEVICE_WEIGHTS_SYMBOLS and hasattr(lib, name)
    for name in ("fsnp_debug_weight_blob", "fsnp_debug_weight_blob_ptr", "fsnp_debug_commit_stats", "fsnp_debug_pack_emulate"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    header = open(os.path.join(os.path.dirname(HERE), "include", "fsnp_device_weights.h")).read()
    for name in _lib.DEVICE_WEIGHTS_SYMBOLS:
        assert name + "(" in header
    assert '#include "fsnp_device_weights.h"' in open(os.path.join(os.path.dirname(HERE), "include", "fsnp.h")).read()


def test_null_arguments_return_1_without_a_device():
    lib = _lib.load()
    x = np.zeros(4, np.float32)
    fake = ctypes.c_void_p(8)          # never dereferenced: the null check comes first
    assert lib.fsnp_set_weight_device(None, b"a", x.ctypes.data, 4, None) == 1
    assert "null argument" in _lib.last_error()
    assert lib.fsnp_set_weight_device(fake, None, x.ctypes.data, 4, None) == 1
    assert lib.fsnp_set_weight_device(fake, b"a", None, 4, None) == 1
    assert lib.fsnp_commit_weights_on(None, None) == 1
    out = (ctypes.c_int64 * 4)()
    assert lib.fsnp_debug_commit_stats(None, ctypes.byref(out)) == 1
    assert lib.fsnp_debug_weight_blob(None, None, 0, None) == 1
    assert lib.fsnp_debug_weight_blob_ptr(None) is None


@pytest.mark.parametrize("cid,kind,sizes", rnn_cases(), ids=[c[0] for c in rnn_cases()])
def test_recurrent_images_equal_the_packers_they_replace(cid, kind, sizes):
    got = emulate(kind, sizes, case_sources(kind, sizes))
    assert not np.isnan(got).any()
    assert digest(got) == DIGESTS[cid], cid


@pytest.mark.parametrize("H,NIN,KX", [(384, 33, 40), (256, 33, 40), (384, 64, 64)])
def test_emulation_equals_the_debug_pack_hooks(H, NIN, KX):
    """The hooks take four-slot matrices and no biases, the emulation the reference's eight tensors: the same image either way (the
    bridge to tests/test_host.py's independent fragment emulations - see the module docstring; no layout check of its own)."""
    lib = _lib.load()
    src = rnn_sources(H, NIN, seed=5)
    w = [s.ctypes.data for s in src[:4]]

    def hook(fn, kind, sizes, *lead):
        want = emulate(kind, sizes, src)
        got = np.full(want.size, np.float32(np.nan))
        assert getattr(lib, fn)(*lead, *w, got.ctypes.data, got.size) == 0, _lib.last_error()
        assert got.tobytes() == want.tobytes(), fn
    hook("fsnp_debug_lstm_pack", ROWTILE, (H, NIN, KX, 4), H, NIN, KX, 4)
    for units in (8, 16, 32, 64):
        hook("fsnp_debug_lstm_coop_pack", KSPLIT, (H, NIN, KX, units), H, NIN, KX, units)
    hook("fsnp_debug_lstm_hpw_pack", HPW, (H, NIN, KX), H, NIN, KX)
    if H == 384:
        hook("fsnp_debug_lstm_coopw_pack", COOPW, (H, NIN, KX), H, NIN, KX)


def test_bf16_variants_round_to_nearest_even():
    """The bf16 k-steps of W_ih1: every half word is the RNE rounding of its source, ties included."""
    H, NIN, KX = 384, 33, 40
    src = rnn_sources(H, NIN, seed=9)
    wih1 = src[2].copy()
    bits = wih1.view(np.uint32)
    bits[0, :8] = [0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0xBF808000, 0xBF818000, 0x00008000, 0x7F7F8000]   # ties, near ties
    src[2] = wih1
    want16 = ((bits.astype(np.uint64) + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint16)
    got = emulate(HALF_BF, (H, NIN, KX), src).view(np.uint16).reshape(4, -1, 24, 64, 8)      # [wave][k-group][tile][lane][8]
    kg = (KX + 15) // 16 + 2 * (H // 16)
    # row 0 = gate 0, unit 0: wave 0, tile 0, lane 0 holds k = 0..7 of step 0; lane 16 holds k = 8..15
    assert got[0, kg, 0, 0].tolist() == want16[0, :8].tolist()
    assert got[0, kg, 0, 16].tolist() == want16[0, 8:16].tolist()
    got = emulate(ROWTILE_BF, (H, NIN, KX, 4), src).view(np.uint16).reshape(4, -1, 12, 64, 8)
    kg = KX // 8 + 2 * (H // 8)
    assert got[0, kg, 0, 0].tolist() == want16[0, :8].tolist()
    assert got[0, kg, 0, 32].tolist() == want16[0, 8:16].tolist()


@pytest.mark.parametrize("H,NIN", [(384, 33), (190, 35)])
def test_gru_spread_and_summed_biases(H, NIN):
    src = rnn_sources(H, NIN, gates=3, seed=3)
    for m in range(4):
        got = emulate(SPREAD, (H, NIN, 0, m, 1), src).reshape(4 * H, -1)
        assert got.tobytes() == spread(src[m], H, hidden=bool(m & 1)).tobytes(), m
    got = emulate(BIAS, (H, 0, 0, 0, 1), src).reshape(2, 4 * H)
    for l in range(2):
        bi, bh = src[4 + 2 * l], src[5 + 2 * l]
        want = np.concatenate([bi[:2 * H] + bh[:2 * H], bi[2 * H:], bh[2 * H:]])
        assert got[l].tobytes() == want.tobytes()
    lstm = rnn_sources(H, NIN, seed=4)
    got = emulate(BIAS, (H,), lstm).reshape(2, 4 * H)
    for l in range(2):
        assert got[l].tobytes() == (lstm[4 + 2 * l] + lstm[5 + 2 * l]).tobytes()
    for m in range(4):          # an LSTM's matrices already have four slots
        assert emulate(SPREAD, (H, NIN, 0, m, 0), lstm).tobytes() == lstm[m].tobytes()


def test_gru_image_is_cut_from_the_spread_matrices():
    """The GRU image from the reference's [3H] tensors equals the recorded image the old packer cut from the four-slot matrices -
    and an image of another kind (the K-split one a GRU model also runs on) agrees with the same image of the spread matrices."""
    H, NIN, KX = 384, 33, 40
    src = rnn_sources(H, NIN, gates=3, seed=H + NIN)
    four = [spread(src[m], H, hidden=bool(m & 1)) for m in range(4)] + [np.zeros(4 * H, np.float32)] * 4
    for kind, sizes in ((KSPLIT, (H, NIN, KX, 16)), (COOPN, (H, NIN, KX)), (GENERIC, (H, NIN))):
        a = emulate(kind, tuple(sizes) + (0,) * (4 - len(sizes)) + (1,), src)
        b = emulate(kind, sizes, four)
        assert a.tobytes() == b.tobytes(), kind


@pytest.mark.parametrize("cin", [257, 34])
def test_tcn_operands_and_groupnorm_fold(cin):
    CH = 384
    up = lambda v, a: (v + a - 1) // a * a
    N1P, K1P, N2P, K2P = up(CH, 384), up(cin, 16), up(cin, 384), up(CH, 16)
    w1 = _values(1, CH * cin).reshape(CH, cin)
    w2 = _values(2, cin * CH).reshape(cin, CH)
    g2, be2, sb2 = _values(3, CH) + 1.0, _values(4, CH), _values(5, cin)
    dw = _values(6, CH * 3).reshape(CH, 3)

    def padded(m, NP, KP):
        o = np.zeros((NP, KP), np.float32)
        o[:m.shape[0], :m.shape[1]] = m
        return o
    assert emulate(PADMAT, (CH, cin, N1P, K1P), [w1]).tobytes() == padded(w1, N1P, K1P).tobytes()
    assert emulate(PADMAT, (cin, CH, N2P, K2P), [w2]).tobytes() == padded(w2, N2P, K2P).tobytes()
    assert emulate(PADMAT, (1, cin, 1, N2P), [sb2]).tobytes() == padded(sb2[None], 1, N2P).tobytes()       # a bias: a padded copy
    assert emulate(PADMAT, (1, CH, 1, CH), [g2]).tobytes() == g2.tobytes()                                 # a plain copy
    assert emulate(TRANSPOSE, (CH, 3), [dw]).tobytes() == np.ascontiguousarray(dw.T).tobytes()             # tap major
    fc1 = _values(7, 128 * cin).reshape(128, cin)
    assert emulate(TRANSPOSE, (128, cin), [fc1]).tobytes() == np.ascontiguousarray(fc1.T).tobytes()        # SE fc1 / fc2
    # GroupNorm 2 folded into the sconv GEMM: W[n][k] gamma[k] in fp64, and per row c1 = bias + sum_k beta_k W[n][k],
    # c2 = sum_k gamma_k W[n][k], fp64 sums in k order
    w2d = w2.astype(np.float64)
    want = padded((w2d * g2.astype(np.float64)[None]).astype(np.float32), N2P, K2P)
    assert emulate(FOLDW, (cin, CH, N2P, K2P), [w2, g2]).tobytes() == want.tobytes()
    s1, s2 = sb2.astype(np.float64), np.zeros(cin)
    for k in range(CH):
        s1 = s1 + np.float64(be2[k]) * w2d[:, k]
        s2 = s2 + np.float64(g2[k]) * w2d[:, k]
    for which, s in ((0, s1), (1, s2)):
        want = np.zeros(N2P, np.float32)
        want[:cin] = s.astype(np.float32)
        assert emulate(FOLDC, (cin, CH, N2P, which), [w2, g2, be2, sb2]).tobytes() == want.tobytes(), which


def test_emulation_refuses_what_would_read_outside_a_tensor():
    H, NIN, KX = 384, 33, 40
    src = rnn_sources(H, NIN)
    short = list(src)
    short[1] = src[1].reshape(-1)[:-1]                     # weight_hh_l0 one element short
    emulate(COOPN, (H, NIN, KX), short, expect=3)
    assert "outside its tensor" in _lib.last_error()
    short = list(src)
    short[0] = src[0].reshape(-1)[:4 * H * (NIN - 1)]      # as if it had one input fewer
    emulate(ROWTILE, (H, NIN, KX, 4), short, expect=3)
    emulate(ROWTILE, (H, NIN, KX, 5), src, expect=2)       # 384 hidden units do not split over 5 waves
    emulate(FBV, (384, 33), src, expect=2)
    emulate(FOLDC, (34, 384, 384, 0), [np.zeros(34 * 384, np.float32), np.zeros(384, np.float32), np.zeros(383, np.float32),
                                       np.zeros(34, np.float32)], expect=2)


def test_python_chooser_on_cpu_parameters():
    """weight_upload: CPU parameters take the host setter under "auto"; "device" refuses them; anything else is an error."""
    model = FullSubNet_Plus(**DEFAULT_MODEL_ARGS)
    assert model.weight_upload == "auto"
    dev = torch.device("cuda", 0)
    plan = model._upload_plan(dev)
    assert plan and all(where == "host" for _, _, where in plan)
    assert [n for n, _, _ in plan] == list(model.state_dict().keys())
    model.weight_upload = "device"
    with pytest.raises(RuntimeError, match="weight_upload=\"device\".*not on"):
        model._upload_plan(dev)
    model.weight_upload = "host"
    assert all(where == "host" for _, _, where in model._upload_plan(dev))
    model.weight_upload = "gpu"
    with pytest.raises(ValueError, match="weight_upload"):
        model._upload_plan(dev)

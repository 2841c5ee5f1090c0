"""GPU tests of the sample-rate converter and of enhance_wave at other sample rates (include/fsnp_resample.h).

One comparison has a tolerance: the kernel against the float64 oracle of tests/_resample_util.py run on the library's own fp32 taps.
Its bound is computed per output sample by the oracle - (K + 1) 2^-24 S + 1e-37 for a K-term fmaf chain from 0.0f whose terms sum
to S in magnitude - so nothing is tuned.  Every other comparison is exact: an int16 input is x.float() / 32768, an int16 output is a
pure function (tests/_pcm_util.py) of the fp32 output, a fused call is the composition of the free-standing calls, a row of a batch is
that clip alone.  The models are those of tests/test_gpu_pcm.py; model clips are 2000 - 3000 samples at 16 kHz."""
import ctypes
import re

import numpy as np
import pytest
import torch

from fullsubnet_plus_amd import FullSubNet, _lib, resample_length
from oracle.ref_loader import FULLSUBNET_MODEL_ARGS
from oracle.weights import make_state_dict_fullsubnet
from tests._pcm_util import crafted, peak_rows, quantise_rows
from tests._resample_util import PAIRS, fma_chain_bound, out_length, plan, resample64
from tests.test_gpu_pcm import _model, _odd, _pcm

pytestmark = pytest.mark.gpu
BLOCK = 256          # kResampleBlock (csrc/resample.h): outputs per workgroup


def _fresh():
    """a model of its own for a test that counts the handle's tables or watches its io area"""
    m = FullSubNet(**FULLSUBNET_MODEL_ARGS)
    m.load_state_dict(make_state_dict_fullsubnet(13, "harsh"), strict=True)
    m = m.to("cuda").eval()
    m.batch_mode, m.error_check = "full", "sync"
    return m


def _lib_taps(pair):
    _, _, half = plan(*pair)
    buf = np.zeros(2 * half + 1, dtype=np.float32)
    assert _lib.load().fsnp_resample_taps(pair[0], pair[1], buf.ctypes.data, buf.size) == 0, _lib.last_error()
    return buf.astype(np.float64)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ------------------------------------------------------------------------------------------------ 1. the kernel against the oracle
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_kernel_against_oracle(pair):
    """n = 1 and 5 are clips shorter than the filter; the others put n_out below, at and above one and two workgroups' outputs."""
    m = _model("fullsubnet")
    taps = _lib_taps(pair)
    sizes = {1, 5, 64, 1000}
    for target in (BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK - 1, 2 * BLOCK, 2 * BLOCK + 1):
        n = next(n for n in range(1, 8 * BLOCK) if out_length(n, *pair) >= target)      # (an up-sampling pair steps over some counts)
        sizes.add(n)
    worst = 0.0
    for n in sorted(sizes):
        x = np.random.RandomState(1000 + n).uniform(-1.0, 1.0, size=n).astype(np.float32)
        got = m.resample(torch.from_numpy(x)[None].cuda(), *pair)
        want, S, K = resample64(x, *pair, taps=taps)
        assert got.shape == (1, want.size) and got.dtype == torch.float32, (n, got.shape)
        err = np.abs(got[0].cpu().numpy().astype(np.float64) - want)
        bound = fma_chain_bound(S, K)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (pair, n, int(np.argmax(err / bound)), float((err / bound).max()))
    print(f"{pair}: sizes {sorted(sizes)}, worst error / bound = {worst:.3f}")
    m.check_errors()


# ------------------------------------------------------------------------------------------------ 2. int16 in
def test_int16_input_is_the_fp32_call():
    m = _model("fullsubnet")
    x = _pcm((3, 1001), 51)
    xf = x.float().cuda() / 32768
    for pair in ((48000, 16000), (16000, 44100)):
        ref = m.resample(xf, *pair)
        got = m.resample(_odd(x), *pair, out_format="f32")      # rows at odd element offsets
        assert got.dtype == torch.float32 and torch.equal(got, ref), pair
        # one channel of a 3-channel interleaved buffer, read in place (sample step 3)
        inter = torch.full((1001, 3), 999, dtype=torch.int16, device="cuda")
        inter[:, 1] = x[0].cuda()
        chan = inter[:, 1].unsqueeze(0)
        assert chan.stride(1) == 3
        assert torch.equal(m.resample(chan, *pair, out_format="f32"), ref[0:1]), pair
        fchan = (inter.float() / 32768)[:, 1].unsqueeze(0)
        assert fchan.stride(1) == 3 and torch.equal(m.resample(fchan, *pair), ref[0:1]), pair
    m.check_errors()


# ------------------------------------------------------------------------------------------------ 3. int16 out
def _int16_out(m, x, pair, lengths, what):
    """"s16" with its counts and "s16_peak" of one input against the fp32 call's result"""
    B = x.shape[0]
    lens = None if lengths is None else [out_length(n, *pair) for n in lengths]
    yf = m.resample(x, *pair, lengths=lengths, out_format="f32").cpu().numpy()
    want, counts = quantise_rows(yf, lens)
    clipped = torch.full((B,), -3, dtype=torch.int32, device="cuda")
    got = m.resample(x, *pair, lengths=lengths, out_format="s16", clipped=clipped)
    assert got.dtype == torch.int16 and np.array_equal(got.cpu().numpy(), want), what
    assert np.array_equal(clipped.cpu().numpy(), counts), (what, clipped.tolist(), counts.tolist())
    return yf, counts, lens


def test_int16_output_of_crafted_rows():
    m = _model("fullsubnet")
    c, q, _ = crafted()
    rng = np.random.RandomState(52)
    v = rng.uniform(-1.2, 1.2, size=(2, 600)).astype(np.float32)
    v[0, 300:300 + c.size] = c
    v[1, 400 - c.size:400] = c                     # right in front of the row's end ...
    v[1, 450:450 + c.size] = c                     # ... and behind it
    x = torch.from_numpy(v).cuda()
    # equal rates: the conversion alone, ties and both ends of the range included
    yf, counts, _ = _int16_out(m, x, (16000, 16000), [600, 400], "copy")
    assert np.array_equal(yf[0], v[0], equal_nan=True) and counts.min() > 0
    got = m.resample(x, 16000, 16000, out_format="s16").cpu().numpy()
    assert np.array_equal(got[0, 300:300 + c.size], q)
    # through a filter: infinities and NaN spread over the filter's reach and count as clipped, the rest saturates here and there
    yf, counts, _ = _int16_out(m, x, (48000, 16000), [600, 400], "48 k -> 16 k")
    assert np.isnan(yf).any() and counts.min() > 0
    _int16_out(m, x, (16000, 48000), None, "16 k -> 48 k")
    # the peak format: finite rows (numpy's own tail turns a NaN into a NaN peak), louder than full scale; nothing clips
    f = torch.from_numpy(rng.uniform(-3.0, 3.0, size=(2, 600)).astype(np.float32)).cuda()
    for pair, lengths in (((16000, 16000), [600, 400]), ((48000, 16000), [600, 400]), ((16000, 44100), None)):
        lens = None if lengths is None else [out_length(n, *pair) for n in lengths]
        yf = m.resample(f, *pair, lengths=lengths, out_format="f32").cpu().numpy()
        clipped = torch.full((2,), -3, dtype=torch.int32, device="cuda")
        got = m.resample(f, *pair, lengths=lengths, out_format="s16_peak", clipped=clipped)
        assert got.dtype == torch.int16 and np.array_equal(got.cpu().numpy(), peak_rows(yf, lens)), pair
        assert not clipped.any() and np.abs(got.cpu().numpy().astype(np.int32)).max() == 26213
    m.check_errors()


# ------------------------------------------------------------------------------------------------ 4. lengths
@pytest.mark.parametrize("pair", [(48000, 16000), (16000, 44100)], ids=lambda p: f"{p[0]}-{p[1]}")
def test_rows_of_a_batch_are_the_clips_alone(pair):
    m = _model("fullsubnet")
    n = 1000
    lengths = [n, 1, 257]
    x = torch.from_numpy(np.random.RandomState(53).uniform(-1, 1, size=(3, n)).astype(np.float32))
    for b in range(3):
        x[b, lengths[b]:] = float("nan")            # what must never be read
    xg = x.cuda()
    got = m.resample(xg, *pair, lengths=lengths)
    assert got.shape == (3, out_length(n, *pair))
    got16 = m.resample(xg, *pair, lengths=lengths, out_format="s16")
    for b in range(3):
        alone = m.resample(xg[b:b + 1, :lengths[b]], *pair)
        n_out = out_length(lengths[b], *pair)
        assert alone.shape == (1, n_out) and torch.equal(_bits(got[b, :n_out]), _bits(alone[0])), (pair, b)
        assert not torch.isnan(got[b]).any() and torch.count_nonzero(got[b, n_out:]) == 0, (pair, b)
        assert torch.count_nonzero(got16[b, n_out:]) == 0
    assert np.array_equal(got16.cpu().numpy(), quantise_rows(got.cpu().numpy())[0])
    m.check_errors()


# ------------------------------------------------------------------------------------------------ 5. equal rates
def test_equal_rates_are_a_bit_exact_copy():
    m = _model("fullsubnet")
    xi = _pcm((2, 777), 54)
    xf = torch.from_numpy(np.random.RandomState(55).uniform(-1.5, 1.5, size=(2, 777)).astype(np.float32))
    xf[0, 5], xf[1, 6] = float("nan"), float("inf")
    xf_g = xf.cuda()
    for rate in (16000, 44100):
        got = m.resample(xf_g, rate, rate)                                    # f32 -> f32
        assert got.dtype == torch.float32 and torch.equal(_bits(got), _bits(xf_g))
        want, counts = quantise_rows(xf.numpy())                              # f32 -> s16
        clipped = torch.zeros(2, dtype=torch.int32, device="cuda")
        assert np.array_equal(m.resample(xf_g, rate, rate, out_format="s16", clipped=clipped).cpu().numpy(), want)
        assert np.array_equal(clipped.cpu().numpy(), counts)
        got = m.resample(_odd(xi), rate, rate, out_format="f32")              # s16 -> f32
        assert torch.equal(got, xi.float().cuda() / 32768)
        got = m.resample(_odd(xi), rate, rate)                                # s16 -> s16
        assert got.dtype == torch.int16 and torch.equal(got.cpu(), xi)
        fin = torch.nan_to_num(xf, nan=0.25, posinf=-1.5).cuda()
        assert np.array_equal(m.resample(fin, rate, rate, out_format="s16_peak").cpu().numpy(), peak_rows(fin.cpu().numpy()))
        assert np.array_equal(m.resample(xi.cuda(), rate, rate, out_format="s16_peak").cpu().numpy(),
                              peak_rows((xi.float() / 32768).numpy()))
    m.check_errors()


# ------------------------------------------------------------------------------------------------ 6. enhance_wave at another rate
def _composed(m, x, R, lengths=None):
    """resample(enhance_wave(resample(x, R, M)), M, R)[:, :L] - with lengths, each row composed alone and 0 behind it"""
    M, L = m.sample_rate, x.shape[1]
    if lengths is None:
        return m.resample(m.enhance_wave(m.resample(x, R, M)), M, R)[:, :L].contiguous()
    out = torch.zeros(x.shape, dtype=torch.float32, device=x.device)
    for b, n in enumerate(lengths):
        out[b, :n] = _composed(m, x[b:b + 1, :n].contiguous(), R)[0]
    return out


def _rate_case(R):
    """B = 2 clips at R: L samples that are 2500 (44.1 kHz: 2501) at 16 kHz, the second row one sample short of 2000 there"""
    L = resample_length(2500, 16000, R) + (1 if R == 44100 else 0)      # 7500 / 6892 / 1250 samples
    lengths = [L, resample_length(2000, 16000, R) - 1]
    xi = _pcm((2, L), 60 + R // 1000)
    return L, lengths, xi, xi.float().cuda() / 32768


@pytest.mark.parametrize("R", [48000, 44100, 8000])
@pytest.mark.parametrize("name", ["plus", "fullsubnet"])
def test_enhance_wave_at_another_rate(name, R):
    m = _model(name)
    L, lengths, xi, x = _rate_case(R)
    # fp32, whole rows: the composition of the free-standing calls, bit for bit
    ref = _composed(m, x, R)
    got = m.enhance_wave(x, sample_rate=R)
    assert got.shape == (2, L) and got.dtype == torch.float32 and torch.equal(got, ref), (name, R)
    # per-row lengths (test_enhance_wave_lengths_rows_composed_alone has the fp32 comparison): 0 behind a row's own samples
    got_len = m.enhance_wave(x, lengths, sample_rate=R)
    assert torch.count_nonzero(got_len[1, lengths[1]:]) == 0 and torch.count_nonzero(got_len[1, :lengths[1]]) > 0
    # int16 out is a function of the fp32 result
    for lens, fp in ((None, got), (lengths, got_len)):
        want, counts = quantise_rows(fp.cpu().numpy(), lens)
        clipped = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        out = m.enhance_wave(x, lens, out_format="s16", clipped=clipped, sample_rate=R)
        assert out.dtype == torch.int16 and np.array_equal(out.cpu().numpy(), want), (name, R, lens)
        assert np.array_equal(clipped.cpu().numpy(), counts)
        out = m.enhance_wave(x, lens, out_format="s16_peak", clipped=clipped, sample_rate=R)
        assert np.array_equal(out.cpu().numpy(), peak_rows(fp.cpu().numpy(), lens)) and not clipped.any(), (name, R, lens)
    # int16 in (odd offsets; int16 out by default), and a strided input read in place
    assert torch.equal(m.enhance_wave(_odd(xi), sample_rate=R, out_format="f32"), got)
    assert np.array_equal(m.enhance_wave(_odd(xi), lengths, sample_rate=R).cpu().numpy(), quantise_rows(got_len.cpu().numpy(), lengths)[0])
    inter = x.t().contiguous().t()
    assert inter.stride() == (1, 2) and torch.equal(m.enhance_wave(inter, sample_rate=R), got)
    m.check_errors()


@pytest.mark.parametrize("R", [48000, 44100, 8000])
@pytest.mark.parametrize("name", ["plus", "fullsubnet"])
def test_enhance_wave_lengths_rows_composed_alone(name, R):
    """With lengths, torch.equal with each row composed ALONE: resample(enhance_wave(resample(x[b:b+1, :n_b], R, 16000)), 16000, R)[:, :n_b].

    The model is not bit-identical between batch sizes (at 16 kHz, no conversion anywhere, enhance_wave(x)[0:1] and enhance_wave(x[0:1])
    differ by 7e-6 at max |y| 8.5: the sub-band planner gives B = 1 and B = 2 different kernels), so one batch over the rows misses this
    by 4e-6 ... 1.1e-5; fsnp_enhance_wave_rate therefore runs the rows of a lengths call one clip at a time."""
    m = _model(name)
    L, lengths, xi, x = _rate_case(R)
    got = m.enhance_wave(x, lengths, sample_rate=R)
    ref = _composed(m, x, R, lengths)
    for b, n in enumerate(lengths):
        print(f"{name} {R} row {b}: max |fused - alone| = {float((got[b, :n] - ref[b, :n]).abs().max()):.3e}, "
              f"max |y| = {float(ref[b, :n].abs().max()):.3e}")
    assert torch.equal(got, ref), (name, R)


# ------------------------------------------------------------------------------------------------ 7. the default path did not move
@pytest.mark.parametrize("name", ["plus", "fullsubnet"])
def test_default_rate_calls_are_the_plain_call(name):
    m = _model(name)
    x = _pcm((2, 2500), 70).float().cuda() / 32768
    plain, plain_len = m.enhance_wave(x), m.enhance_wave(x, [2500, 2000])
    assert torch.equal(m.enhance_wave(x, sample_rate=None), plain) and torch.equal(m.enhance_wave(x, sample_rate=16000), plain)
    assert torch.equal(m.enhance_wave(x, [2500, 2000], sample_rate=16000), plain_len)
    try:
        m.sample_rate = 8000
        assert torch.equal(m.enhance_wave(x, sample_rate=8000), plain) and torch.equal(m.enhance_wave(x), plain)
    finally:
        m.sample_rate = 16000
    m.enhance_wave(x, sample_rate=48000)
    assert torch.equal(m.enhance_wave(x), plain) and torch.equal(m.enhance_wave(x, [2500, 2000]), plain_len)
    m.check_errors()


# ------------------------------------------------------------------------------------------------ 8. reserve
def _io_area(m):
    size, addr, tables = re.search(r"waveform io area: (\d+) bytes at (\S+); resample tables: (\d+) of 8", m.dump_config()).groups()
    return int(size), addr, int(tables)


def test_reserved_calls_leave_the_io_area_alone():
    m = _fresh()
    B, L = 3, 9000                                   # 3000 samples at 16 kHz
    x = _pcm((B, L), 80)
    m.reserve(B, 1 + 3000 // m.hop_length, max_samples=L, sample_rate=48000)
    torch.cuda.synchronize()
    area = _io_area(m)
    assert area[0] > B * L * 4 and area[2] == 2
    for fmt in ("f32", "s16", "s16_peak"):
        m.enhance_wave(x.cuda(), out_format=fmt, sample_rate=48000)
        m.enhance_wave(x.float().cuda() / 32768, [L, 5000, 801], out_format=fmt, sample_rate=48000)
    torch.cuda.synchronize()
    assert _io_area(m) == area
    m.check_errors()


# ------------------------------------------------------------------------------------------------ 9. refusals with a handle
def test_refusals_leave_the_handle_usable():
    m = _fresh()
    x = _pcm((1, 3000), 81).float().cuda() / 32768
    before = m.enhance_wave(x)
    # a clip too short at the model's rate: 768 samples at 48 kHz are 256 at 16 kHz, n_fft / 2
    with pytest.raises(_lib.FsnpError, match="model's rate") as e:
        m.enhance_wave(x[:, :768], sample_rate=48000)
    assert e.value.code == 2
    with pytest.raises(_lib.FsnpError, match="model's rate") as e:
        m.enhance_wave(torch.cat([x, x]), [3000, 768], sample_rate=48000)
    assert e.value.code == 2
    # FSNP_SAMPLE_S16_PEAK as an input format
    lib, h = _lib.load(), m._handle
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.zeros((1, 3000), dtype=torch.int16, device="cuda")
    xi = _pcm((1, 3000), 82).cuda()
    assert lib.fsnp_resample_pcm(h, xi.data_ptr(), 2, 3000, 1, out.data_ptr(), 1, 3000, 1, None, 1, 3000, 48000, 16000, None, s) == 2
    assert "FSNP_SAMPLE_S16_PEAK" in _lib.last_error() and "fsnp_resample_pcm" in _lib.last_error()
    assert lib.fsnp_enhance_wave_rate(h, xi.data_ptr(), 2, 3000, 1, out.data_ptr(), 1, 3000, 1, None, 1, 3000, None, 48000, 16000, s) == 2
    assert "FSNP_SAMPLE_S16_PEAK" in _lib.last_error() and "fsnp_enhance_wave_rate" in _lib.last_error()
    torch.cuda.synchronize()
    assert torch.count_nonzero(out) == 0
    # the ninth distinct pair
    pairs = [(16000, r) for r in (8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 88200, 96000)]
    while _io_area(m)[2] < 8:
        tables = _io_area(m)[2]
        m.resample(x, *pairs.pop(0))
        assert _io_area(m)[2] in (tables, tables + 1)
    with pytest.raises(_lib.FsnpError, match="8") as e:
        m.resample(x, 192000, 16000)
    assert e.value.code == 2 and _io_area(m)[2] == 8
    with pytest.raises(_lib.FsnpError, match="pairs") as e:
        m.enhance_wave(x.repeat(1, 2), sample_rate=192000)          # (500 samples at the model's rate: long enough)
    assert e.value.code == 2 and _io_area(m)[2] == 8
    # still usable: the default call's bits, a pair it holds, and equal rates (no table)
    assert torch.equal(m.enhance_wave(x), before)
    assert m.resample(x, 16000, 8000).shape == (1, 1500) and torch.equal(m.resample(x, 192000, 192000), x)
    m.check_errors()

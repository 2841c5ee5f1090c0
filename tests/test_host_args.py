"""The argument helpers of fullsubnet_plus_amd._args that every waveform entry point and session shares, on CPU and `meta` tensors:
no GPU, no library.  (What they feed is compared with the kernels' results in tests/test_gpu_pcm.py and tests/test_gpu_resample.py.)"""
import pytest
import torch

from fullsubnet_plus_amd import _args, _lib


def _meta(shape, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device="meta")


# ------------------------------------------------------------------------------------------------ require_cuda
@pytest.mark.parametrize("tensor", [torch.zeros(2, 3), _meta((2, 3)), torch.zeros(2, dtype=torch.int16)], ids=["cpu", "meta", "cpu_int16"])
def test_require_cuda_refuses_in_one_wording(tensor):
    with pytest.raises(RuntimeError) as e:
        _args.require_cuda(tensor)
    assert "runs on MI355X (HIP) only" in str(e.value) and "no CPU fallback" in str(e.value)


def test_require_cuda_reads_nothing_but_is_cuda():
    class OnDevice:
        is_cuda = True
    assert _args.require_cuda(OnDevice()) is None


# ------------------------------------------------------------------------------------------------ other_rate
def test_other_rate():
    assert _args.other_rate(None, 16000, "f") is None
    assert _args.other_rate(16000, 16000, "f") is None
    assert _args.other_rate(48000, 16000, "f") == 48000 and type(_args.other_rate(48000, 16000, "f")) is int
    assert _args.other_rate(16000, 8000, "f") == 16000
    for bad in (0, -1, 44100.0, "48k", True):
        with pytest.raises(ValueError, match="f: a sample rate"):
            _args.other_rate(bad, 16000, "f")
    with pytest.raises(ValueError, match="640"):       # both directions are planned: 16000 -> 44101 has up = 44101
        _args.other_rate(44101, 16000, "f")


# ------------------------------------------------------------------------------------------------ reads_in_place / f32_rows / pcm_input
@pytest.mark.parametrize("make", [torch.zeros, _meta], ids=["cpu", "meta"])
def test_route_and_conversion_of_every_input_kind(make):
    S16, F32 = _lib.SAMPLE_S16, _lib.SAMPLE_F32
    f32, s16, f64 = make((2, 8)), make((2, 8), dtype=torch.int16), make((2, 8), dtype=torch.float64)
    inter = make((2, 8, 2), dtype=torch.int16)[:, :, 1]                 # one channel of an interleaved buffer: step 2
    cases = [  # tensor, goes to the PCM entry points?, what pcm_input returns after the tensor
        (f32, False, (F32, 8, 1)), (s16, True, (S16, 8, 1)), (f64, False, (F32, 8, 1)), (inter, True, (S16, 16, 2)),
        (make((2, 8, 3))[:, :, 0], True, (F32, 24, 3)),                  # strided fp32 is read where it lies
        (make((2, 1)).expand(2, 8), True, (F32, 8, 1)),                  # step 0: the one copy pcm_input makes
        (make((2, 1), dtype=torch.int16).expand(2, 8), True, (S16, 8, 1)),
        (make((2, 1, 3))[:, :, 0], False, (F32, 3, 3)),                  # one sample per row: no step to speak of
    ]
    for t, in_place, (fmt, row, step) in cases:
        assert _args.reads_in_place(t) is in_place, (t.dtype, t.stride())
        x, got_fmt, got_row, got_step = _args.pcm_input(t)
        assert (got_fmt, got_row, got_step) == (fmt, row, step), (t.dtype, t.stride())
        assert x.dtype == (torch.int16 if fmt == S16 else torch.float32) and x.shape == t.shape and got_step >= 1
        assert (x is t) == (t.dtype != torch.float64 and (t.shape[1] == 1 or t.stride(1) >= 1))       # nothing is copied otherwise
        rows = _args.f32_rows(t)
        assert rows.dtype == torch.float32 and rows.shape == t.shape and rows.stride(1) == 1
    assert _args.f32_rows(f32) is f32


def test_pcm_input_keeps_the_samples():
    t = torch.arange(16, dtype=torch.float64).reshape(2, 8)
    assert torch.equal(_args.pcm_input(t)[0], t.float())
    e = torch.tensor([[3], [5]], dtype=torch.int16).expand(2, 4)
    assert torch.equal(_args.pcm_input(e)[0], e) and _args.pcm_input(e)[0].is_contiguous()


# ------------------------------------------------------------------------------------------------ output_format
def test_output_format():
    F32, S16, PEAK = _lib.SAMPLE_F32, _lib.SAMPLE_S16, _lib.SAMPLE_S16_PEAK
    assert _args.output_format(None, torch.float32, "f") == (F32, torch.float32)
    assert _args.output_format(None, torch.float64, "f") == (F32, torch.float32)
    assert _args.output_format(None, torch.int16, "f") == (S16, torch.int16)
    assert _args.output_format("f32", torch.int16, "f") == (F32, torch.float32)
    assert _args.output_format("s16", torch.float32, "f") == (S16, torch.int16)
    assert _args.output_format("s16_peak", torch.float32, "f") == (PEAK, torch.int16)
    assert _args.output_format("s16", torch.float32, "f", peak=False) == (S16, torch.int16)
    with pytest.raises(ValueError, match=r"enhance_wave: out_format 'u8' is none of None, 'f32', 's16', 's16_peak'$"):
        _args.output_format("u8", torch.float32, "enhance_wave")
    with pytest.raises(ValueError, match=r"WaveStream.push: out_format 'u8' is none of None, 'f32', 's16'$"):
        _args.output_format("u8", torch.float32, "WaveStream.push", peak=False)
    with pytest.raises(ValueError, match=r"WaveStream.finish: out_format 's16_peak' is none of None, 'f32', 's16' \(a stream has no peak"):
        _args.output_format("s16_peak", torch.float32, "WaveStream.finish", peak=False)


# ------------------------------------------------------------------------------------------------ clipped_pointer
def test_clipped_pointer():
    dev = torch.device("cuda", 0)
    assert _args.clipped_pointer(None, 2, dev, "f") is None
    for bad in (torch.zeros(2, dtype=torch.int32), _meta((2,), torch.int32)):                 # not on the GPU
        with pytest.raises(ValueError, match=r"f: clipped must be a contiguous torch.int32 tensor \[2\] on cuda:0"):
            _args.clipped_pointer(bad, 2, dev, "f")

    class Clipped:            # what the helper reads of a tensor, with one property wrong at a time
        def __init__(self, **kw):
            self.is_cuda, self.device, self.dtype, self.shape, self._contiguous = True, dev, torch.int32, (2,), True
            self.__dict__.update(kw)

        def is_contiguous(self):
            return self._contiguous

        def data_ptr(self):
            return 4096
    assert _args.clipped_pointer(Clipped(), 2, dev, "f") == 4096
    for wrong in (dict(device=torch.device("cuda", 1)), dict(dtype=torch.int64), dict(shape=(3,)), dict(shape=(2, 1)), dict(_contiguous=False)):
        with pytest.raises(ValueError, match="clipped must be"):
            _args.clipped_pointer(Clipped(**wrong), 2, dev, "f")

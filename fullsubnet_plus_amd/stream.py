"""Stream sessions of the original FullSubNet (include/fsnp_stream.h): chunked forwards that carry their state.

    stream = model.open_stream(slots=8, max_chunk=16)
    mask = stream.push(noisy_mag)            # [8, 1, F, n] -> [8, 2, F, n]; column j = cIRM of frame P + j - look_ahead
    ...
    mask = stream.tail()                     # look_ahead zero frames: the masks of the last look_ahead frames

and the same for waveforms (include/fsnp_wave_stream.h): samples in, samples out at the fixed delay n_fft + look_ahead * hop_length.

    wave = model.open_wave_stream(slots=8, max_samples=4096)
    out = wave.push(block)                   # [8, n] -> [8, n]; column j = enhanced sample P + j - wave.delay (0 before the clip's start)
    ...
    out = wave.finish()                      # [8, wave.delay]: the clips' last samples; the slots are reset

and for samples at another rate than the model's (include/fsnp_wave_rate_stream.h): the same session between two streaming converters.

    wave = model.open_wave_stream(slots=1, max_samples=480, live=True, sample_rate=48000)
    out = wave.push(block)                   # [1, 480] at 48 kHz -> [1, 480] at 48 kHz, wave.delay = 3264 samples (68 ms) late

and for a caller who owns the STFT (include/fsnp_spec_stream.h): noisy complex frames in, enhanced complex frames out, look_ahead late.

    spec = model.open_spec_stream(slots=8, max_chunk=16)
    enh = spec.push(noisy_complex)           # [8, F, n] complex64 -> [8, F, n]; column j = enhanced frame P + j - look_ahead
    ...
    enh = spec.tail()                        # look_ahead zero frames: the last look_ahead enhanced frames

and, for either model, live audio in the cross-faded windows of enhance_wave_windowed (include/session/fsnp_window_stream.h): the only
online form FullSubNet+ has.

    win = plus.open_window_stream(slots=8, window=32000, overlap=4000, max_samples=160)
    out = win.push(block)                    # [8, n] -> [8, n]; column j = merged sample P + j - win.delay, win.delay = window
    ...
    out = win.finish()                       # [8, window]: the clips' last samples; the slots are reset

The first three take live=True (include/fsnp_stream_live.h): the session mode for a few streams fed one hop at a time, on per-step kernels that
fill the chip at one slot.  Same interface, same state records; max_chunk <= 16.
"""
import ctypes
import gc
import numbers

import torch

from . import _call, _lib, _policy
from ._args import _host_lengths, clipped_pointer, output_format, pcm_input, require_cuda

PLUS_REASON = ("FullSubNet+ cannot be streamed exactly: its full-band TCN blocks are not causal and normalise with GroupNorm(1, C) over "
               "the whole clip, and TSSE pools over all of time; stream the original FullSubNet (fullsubnet_plus_amd.FullSubNet) with a "
               "cumulative norm")


def refusal(model):
    """Why `model` (a FullSubNet) cannot be streamed, or None.  Decided from the constructor arguments alone: no GPU is touched."""
    if model.norm_type not in ("cumulative_laplace_norm", "cumulative_layer_norm"):
        return (f"norm_type {model.norm_type!r} needs the whole clip's total; streaming needs cumulative_laplace_norm or "
                "cumulative_layer_norm")
    if model.sequence_model != "LSTM":
        return f"sequence_model {model.sequence_model!r} is not built for streaming (LSTM only)"
    nin = (model.sb_num_neighbors * 2 + 1) + (model.fb_num_neighbors * 2 + 1)
    if model.sb_model_hidden_size not in (256, 384) or nin > 64:
        return (f"sb_model_hidden_size {model.sb_model_hidden_size} with {nin} sub-band inputs is outside the row-tile kernel "
                "(hidden 256 / 384, <= 64 inputs): not built for streaming")
    return None


def spec_refusal(model):
    """Why `model` (a FullSubNet) cannot stream spectra, or None: refusal(), and the cIRM epilogue's output_size.  No GPU is touched."""
    why = refusal(model)
    if why is not None:
        return why
    if model.output_size != 2:
        return f"the cIRM epilogue needs output_size = 2 (this model: {model.output_size})"
    return None


def wave_refusal(model):
    """Why `model` (a FullSubNet) cannot stream waveforms, or None: spec_refusal(), and the rules of include/fsnp_stft_geometry.h for the
    model's hop_length (what its setter refuses: here only a default hop num_freqs - 1 that is no multiple of 4).  No GPU is touched."""
    why = spec_refusal(model)
    if why is not None:
        return why
    return hop_refusal(model.num_freqs, model.hop_length)


def hop_refusal(num_freqs, hop):
    """Why the waveform path of a model of `num_freqs` bins cannot run at hop length `hop`, or None (include/fsnp_stft_geometry.h:
    n_fft = 2 (num_freqs - 1), n_fft / 8 <= hop <= n_fft / 2, hop % 4 == 0).  Arithmetic only."""
    if num_freqs < 3:
        return f"the waveform path needs num_freqs >= 3 (n_fft = 2 (num_freqs - 1)); this model: {num_freqs}"
    n_fft = 2 * (num_freqs - 1)
    if isinstance(hop, bool) or not isinstance(hop, numbers.Integral):
        return f"hop_length must be an integer number of samples, got {hop!r}"
    if hop <= 0 or 2 * hop > n_fft or 8 * hop < n_fft:
        return (f"hop_length {hop} outside [n_fft / 8, n_fft / 2] = [{(n_fft + 7) // 8}, {n_fft // 2}] (n_fft = 2 (num_freqs - 1) = {n_fft}): "
                "above it frames no longer cover the clip's tail, below it is outside what the waveform path is built for")
    if hop % 4:
        return (f"hop_length {hop} is not a multiple of 4: the forward DFT GEMM reads frame t at float t * hop_length of the padded signal "
                "as 16-byte vectors")
    return None


def _slot_array(slots):
    """None (every slot) or slot indices -> (ctypes int32 array or None, count)"""
    if slots is None:
        return None, 0
    vals = [int(v) for v in slots]
    return (ctypes.c_int32 * max(len(vals), 1))(*vals), len(vals)


class _Session:
    """What Stream, WaveStream and SpecStream share: the C session behind the symbols `_prefix`_*, its lifetime, the slots' state records, and the
    model's error policy (_policy) around every call that enqueues work.  `live` is the subclass's to set."""
    _prefix = _opener = None         # "fsnp_stream" / "fsnp_wave_stream" / "fsnp_spec_stream"; the FullSubNet method that opens one, for messages

    def __init__(self, model, slots, limit, device, live):
        # A model dropped through a reference cycle (a kept traceback is enough) keeps its handle until a cyclic collection finds it,
        # and destroying a handle waits for the device (hipFree).  Opening a session allocates and waits anyway, so the young
        # generations are collected here - what the interpreter does by itself every few hundred allocations, never the whole heap -
        # and no such finaliser is left to run inside one of this session's pushes, which never wait.
        gc.collect(1)
        self.model, self.slots, self.device, self.look_ahead = model, int(slots), device, model.look_ahead
        lib = self._lib = model._ensure_handle(device)
        self._owner = model._hip.handle.value
        for name in ("destroy", "reset", "get_state", "set_state", "state_bytes"):
            setattr(self, "_" + name, getattr(lib, f"{self._prefix}_{name}"))
        sp = ctypes.c_void_p()
        _call.call(getattr(lib, self._create_symbol(live)), device, model._hip.handle, self.slots, int(limit), *self._create_extra(), ctypes.byref(sp), stream=False)
        self._st, self._backup = sp, None
        self.state_bytes = int(self._state_bytes(sp))

    # ------------------------------------------------------------------ plumbing
    def _create_symbol(self, live):
        return f"{self._prefix}_create_live" if live else f"{self._prefix}_create"

    def _create_extra(self):
        """what the session's create call takes between its limit and its out pointer"""
        return ()

    def _session(self):
        if self._st is None:
            raise RuntimeError("this stream is closed")
        h = self.model._hip.handle
        if h is None or h.value != self._owner:
            raise RuntimeError(f"the model's HIP handle was re-created (device change or copy) since {self._opener}: open a new stream")
        return self._st

    def close(self):
        st, self._st = self._st, None
        h = self.model._hip.handle
        if st is not None and h is not None and h.value == self._owner:      # (a destroyed handle took nothing of the session with it)
            _call.enqueue(self._destroy, self.device, st, stream=False)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _guarded(self, fn, out, *args):
        """fn(*args, hip_stream) -> rc enqueues one library call that fills `out`.  Under error_check="sync" a call that the weight watch
        flags ran on the OLD weights and has advanced the states: they are put back to what it started from before it runs again."""
        model, device, what = self.model, self.device, fn.__name__

        def run():
            _policy.enqueue_retrying_stale(lambda: _call.enqueue(fn, device, *args), model._stale_weights_noticed, what)
            return out
        if model.error_check != "sync":      # a live push is host time: "deferred" is this one call, with nothing built around it
            return run()
        # only watched parameters can be flagged (an unwatched model registers none with fsnp_watch_weights), so a session without
        # save / restore never sees the code that would run its push twice
        watched = model.__dict__.get("_fsnp_watched", False)
        return _policy.run_checked(run, what, sync=True, wait_and_poll=self._wait_and_poll, repack=model._repack,
                                   save=self._save_states if watched else None, restore=self._restore_states if watched else None)

    def _wait_and_poll(self):
        torch.cuda.current_stream(self.device).synchronize()
        return self._lib.fsnp_poll_errors(self.model._handle)

    def _save_states(self):
        if self._backup is None:
            self._backup = torch.empty((self.slots, self.state_bytes), dtype=torch.uint8, device=self.device)
        for b in range(self.slots):
            _call.call(self._get_state, self.device, self._st, b, self._backup[b].data_ptr())

    def _restore_states(self):
        for b in range(self.slots):
            _call.call(self._set_state, self.device, self._st, b, self._backup[b].data_ptr())

    def _counter(self, name, slot):
        st = self._session()
        v = ctypes.c_int64()
        _call.call(getattr(self._lib, f"{self._prefix}_{name}"), self.device, st, int(slot), ctypes.byref(v), stream=False)
        return int(v.value)

    # ------------------------------------------------------------------ the slots' state
    def reset(self, slots=None):
        """Stream-ordered zeroing of the state of `slots` (None: all): the next push starts a fresh clip there."""
        st = self._session()
        arr, num = _slot_array(slots)
        _call.call(self._reset, self.device, st, arr, num)

    def state(self, slot):
        """-> torch.uint8 CUDA tensor [state_bytes]: the slot's whole state (kernel-independent layout: the session's header, include/fsnp_stream.h,
        include/fsnp_wave_stream.h or include/fsnp_spec_stream.h)."""
        st = self._session()
        buf = torch.empty(self.state_bytes, dtype=torch.uint8, device=self.device)
        _call.call(self._get_state, self.device, st, int(slot), buf.data_ptr())
        return buf

    def load_state(self, slot, tensor):
        """Load what state() of a slot of any session of a model of the same sizes returned."""
        st = self._session()
        if tensor.dtype != torch.uint8 or tensor.numel() != self.state_bytes:
            raise ValueError(f"load_state: expected a torch.uint8 tensor of {self.state_bytes} bytes, got {tensor.dtype} x {tensor.numel()}")
        t = tensor.to(self.device).contiguous()
        _call.call(self._set_state, self.device, st, int(slot), t.data_ptr())


class _FrameSession(_Session):
    """What the two sessions fed in frames share (Stream, SpecStream: both have max_chunk and num_freqs)."""

    def _tail(self, slots, dtype, lead_in, lead_out):
        """push() of look_ahead all-zero frames lead_in + (look_ahead,) into `slots` (None: all); lead_out + (0,) for look_ahead = 0"""
        la = self.look_ahead
        if la == 0:
            return torch.zeros(lead_out + (0,), dtype=dtype, device=self.device)
        if la > self.max_chunk:
            raise ValueError(f"tail: look_ahead {la} > max_chunk {self.max_chunk}")
        zeros = torch.zeros(lead_in + (la,), dtype=dtype, device=self.device)
        counts = None if slots is None else [la if b in set(int(v) for v in slots) else 0 for b in range(self.slots)]
        return self.push(zeros, counts)

    def frames(self, slot):
        """Frames pushed into `slot` since its last reset (host-side count; after load_state the first call waits for that copy)."""
        return self._counter("frames", slot)


class Stream(_FrameSession):
    """`slots` independent live streams on one FullSubNet.  Open one through FullSubNet.open_stream, which refuses a model that cannot be
    streamed before any GPU is touched.  Everything runs on the current CUDA stream; a push
    allocates nothing but its output tensor and never synchronises (under the model's error_check="sync" it then waits and polls, as
    forward does)."""
    _prefix, _opener = "fsnp_stream", "open_stream"

    def __init__(self, model, slots, max_chunk, device, live=False):
        super().__init__(model, slots, max_chunk, device, live)
        self.max_chunk, self.num_freqs = int(max_chunk), model.num_freqs
        self.live = bool(self._lib.fsnp_stream_is_live(self._st))      # what the library made, not what was asked for

    def push(self, noisy_mag, counts=None):
        """noisy_mag [slots, 1, F, n] fp32 CUDA tensor (any strides), n <= max_chunk; counts: None (n frames for every slot) or frames
        per slot (a Python sequence or a CPU integer tensor, 0 <= counts[b] <= n; input past counts[b] is never read) -> [slots, 2, F, n]:
        column j < counts[b] of slot b is the model's output of step P + j (the cIRM of frame P + j - look_ahead; exactly 0 while
        P + j < look_ahead), columns >= counts[b] are exactly 0."""
        st = self._session()
        assert noisy_mag.dim() == 4 and noisy_mag.shape[1] == 1, f"{self.model.__class__.__name__} takes the mag feature as inputs."
        S, _, F, n = noisy_mag.shape
        assert S == self.slots, f"expected {self.slots} slots, got {S}"
        assert F == self.num_freqs, f"expected {self.num_freqs} frequency bins, got {F}"
        require_cuda(noisy_mag)
        assert noisy_mag.device == self.device
        x = noisy_mag if noisy_mag.dtype == torch.float32 else noisy_mag.float()
        cnt = None if counts is None else _host_lengths(counts, S, "Stream.push")
        sb, _, sf, stt = x.stride()
        strides = (ctypes.c_int64 * 3)(sb, sf, stt)
        out = torch.empty((S, 2, F, n), dtype=torch.float32, device=self.device)
        return self._guarded(self._lib.fsnp_stream_push, out, st, x.data_ptr(), ctypes.byref(strides), cnt, out.data_ptr(), n)

    def tail(self, slots=None):
        """Push look_ahead all-zero frames (the reference's own pad) into `slots` (None: all): the masks of the last look_ahead frames.
        -> [slots, 2, F, look_ahead] (an empty tensor for look_ahead = 0)."""
        return self._tail(slots, torch.float32, (self.slots, 1, self.num_freqs), (self.slots, 2, self.num_freqs))


class WaveStream(_Session):
    """`slots` independent live audio streams on one FullSubNet (open one through FullSubNet.open_wave_stream, which refuses a model that
    cannot stream waveforms before any GPU is touched): blocks of samples in, the same number of
    enhanced samples out, `delay` = n_fft + look_ahead * hop_length samples late ((2 + look_ahead) * hop_length in the default geometry).
    `hop_length` is the model's when the session was opened; later assignments to model.hop_length do not touch the session.  All push outputs of a clip followed by its finish() output,
    without the first `delay` samples, are enhance_wave() of that clip alone, whatever the block sizes.  Everything runs on the current
    CUDA stream; a push allocates nothing but its output tensor and never synchronises (under the model's error_check="sync" it then
    waits and polls, as forward does).  load_state takes what state() of a slot of any wave session of a model of the same sizes
    returned and is a migration call here: it waits once for the copy, to learn the slot's sample count."""
    _prefix, _opener = "fsnp_wave_stream", "open_wave_stream"
    _f32_calls = True                # the session has fp32 entry points next to the _pcm ones

    def __init__(self, model, slots, max_samples, device, live=False):
        self.hop_length = self.hop = int(model.hop_length)       # (the C session is created from the handle's hop: _ensure_handle set it)
        super().__init__(model, slots, max_samples, device, live)
        self.max_samples = int(max_samples)
        self.delay, self.live = int(getattr(self._lib, f"{self._prefix}_delay")(self._st)), bool(live)

    def push(self, wav, counts=None, out_format=None):
        """wav [slots, n] CUDA tensor, n <= max_samples; counts: None (n samples for every slot) or samples per
        slot (a Python sequence or a CPU integer tensor, 0 <= counts[b] <= n; input past counts[b] is never read) -> [slots, n]: column
        j < counts[b] of slot b is enhanced sample P + j - delay of its clip (exactly 0 while P + j < delay), columns >= counts[b] are
        exactly 0.

        PCM (include/fsnp_pcm.h): wav is fp32 or torch.int16 (full scale: what wav.float() / 32768 gives, bit for bit) at any strides -
        the [slots, n] view of a channel-interleaved socket buffer is read in place.  out_format: None (follow the input: float -> fp32,
        int16 -> "s16"), "f32" or "s16" (int16, round half to even, saturating).  The session's state is fp32 whatever the formats, so
        PCM and fp32 pushes mix freely."""
        ofmt, out_dtype = output_format(out_format, wav.dtype, "WaveStream.push", peak=False)
        st = self._session()
        assert wav.dim() == 2, "WaveStream.push takes [slots, n] samples"
        S, n = wav.shape
        assert S == self.slots, f"expected {self.slots} slots, got {S}"
        require_cuda(wav)
        assert wav.device == self.device
        x, ifmt, row, step = pcm_input(wav)
        cnt = None if counts is None else _host_lengths(counts, S, "WaveStream.push")
        out = torch.empty((S, n), dtype=out_dtype, device=self.device)
        if self._f32_calls and ifmt == ofmt == _lib.SAMPLE_F32 and (n == 1 or step == 1):
            return self._guarded(self._lib.fsnp_wave_stream_push, out, st, x.data_ptr(), row, cnt, out.data_ptr(), n, n)
        return self._guarded(getattr(self._lib, f"{self._prefix}_push_pcm"), out, st, x.data_ptr(), ifmt, row, step, cnt, out.data_ptr(), ofmt,
                             n, 1, n)

    def finish(self, slots=None, out_format=None):
        """End the clips of `slots` (None: all) -> [slots, delay]: each clip's last `delay` samples (exactly 0 where the clip is shorter);
        rows of slots not listed, and of slots that hold no samples, are exactly 0.  The finished slots are reset: their next push starts
        a fresh clip.  A slot that holds 1 .. n_fft / 2 samples is refused, as enhance_wave refuses such a clip.  out_format: None or
        "f32" (fp32), or "s16" (int16, as push)."""
        ofmt, out_dtype = output_format(out_format, torch.float32, "WaveStream.finish", peak=False)
        st = self._session()
        arr, num = _slot_array(slots)
        out = torch.empty((self.slots, self.delay), dtype=out_dtype, device=self.device)
        if self._f32_calls and ofmt == _lib.SAMPLE_F32:
            return self._guarded(self._lib.fsnp_wave_stream_finish, out, st, arr, num, out.data_ptr(), self.delay)
        return self._guarded(getattr(self._lib, f"{self._prefix}_finish_pcm"), out, st, arr, num, out.data_ptr(), ofmt, self.delay, 1)

    def samples(self, slot):
        """Samples pushed into `slot` since its last reset or finish (host-side count)."""
        return self._counter("samples", slot)


class WaveRateStream(WaveStream):
    """A WaveStream whose samples arrive, and leave, at `sample_rate` instead of the model's (include/fsnp_wave_rate_stream.h; open one
    through FullSubNet.open_wave_stream(..., sample_rate=R)): a wave session at model.sample_rate between two streaming converters, the
    filter of enhance_wave(..., sample_rate=R) run push by push on the device.  Same interface as WaveStream - int16 and strided input,
    out_format, counts, finish, state / load_state, samples, the model's error policy; `max_samples`, `delay` and samples() count at
    `sample_rate`.  `delay` = ceil((model_delay * down + 2 half + 1) / up) - 1, the smallest at which every push returns as many
    samples as it took (3264 samples = 68 ms at 48 kHz against the model's 64 ms, at n_fft 512, hop 256, look_ahead 2).
    `model_max_samples` and `model_delay` are the inner session's.  All push outputs of a clip followed by finish(), without the first
    `delay` samples, are enhance_wave(clip, sample_rate=sample_rate) of that clip alone, whatever the block sizes.  A state loads into
    a session of the same rate pair only."""
    _prefix, _opener = "fsnp_wave_rate_stream", "open_wave_stream"
    _f32_calls = False               # one push and one finish: fp32 is FSNP_SAMPLE_F32 of the _pcm calls

    def __init__(self, model, slots, max_samples, device, live=False, sample_rate=None):
        self.sample_rate, self.model_rate = int(sample_rate), int(model.sample_rate)
        super().__init__(model, slots, max_samples, device, live)
        self.model_delay = int(self._lib.fsnp_wave_rate_stream_model_delay(self._st))
        self.model_max_samples = int(self._lib.fsnp_wave_rate_stream_model_max_samples(self._st))

    def _create_extra(self):
        return (self.sample_rate, self.model_rate)


class SpecStream(_FrameSession):
    """`slots` independent live streams on one FullSubNet for a caller who owns the STFT (open one through FullSubNet.open_spec_stream,
    which refuses a model that cannot be streamed before any GPU is touched): noisy complex64 frames in, as many enhanced frames out,
    look_ahead frames late.  The noisy frames wait for their masks inside the slot's state, so state() / load_state move a call whole.
    All push outputs of a clip followed by its tail() output, without the first look_ahead columns, are enhance() of that clip alone,
    whatever the chunking.  Everything runs on the current CUDA stream; a push allocates nothing but its output tensor and never
    synchronises (under the model's error_check="sync" it then waits and polls, as forward does)."""
    _prefix, _opener = "fsnp_spec_stream", "open_spec_stream"

    def __init__(self, model, slots, max_chunk, device, live=False):
        super().__init__(model, slots, max_chunk, device, live)
        self.max_chunk, self.num_freqs, self.live = int(max_chunk), model.num_freqs, bool(live)

    def push(self, noisy_complex, counts=None, out=None):
        """noisy_complex [slots, F, n] complex64 CUDA tensor (any strides: torch.stft's output as it is), n <= max_chunk; counts: None
        (n frames for every slot) or frames per slot (a Python sequence or a CPU integer tensor, 0 <= counts[b] <= n; input past
        counts[b] is never read) -> [slots, F, n] complex64: column j < counts[b] of slot b is the enhanced frame P + j - look_ahead
        (exactly 0 while P + j < look_ahead), columns >= counts[b] are exactly 0.  out: None (a new tensor in torch.stft's memory order,
        bins fastest) or a [slots, F, n] complex64 CUDA tensor of any strides that does not overlap the input."""
        st = self._session()
        assert noisy_complex.dim() == 3 and noisy_complex.is_complex(), "SpecStream.push takes [slots, F, n] complex frames"
        S, F, n = noisy_complex.shape
        assert S == self.slots, f"expected {self.slots} slots, got {S}"
        assert F == self.num_freqs, f"expected {self.num_freqs} frequency bins, got {F}"
        require_cuda(noisy_complex)
        assert noisy_complex.device == self.device
        x = noisy_complex if noisy_complex.dtype == torch.complex64 else noisy_complex.to(torch.complex64)
        x = x.resolve_conj()
        cnt = None if counts is None else _host_lengths(counts, S, "SpecStream.push")
        if out is None:
            out = torch.empty((S, n, F), dtype=torch.complex64, device=self.device).transpose(1, 2)
        else:
            assert out.shape == x.shape and out.dtype == torch.complex64 and out.device == self.device and not out.is_conj(), \
                f"out must be a [{S}, {F}, {n}] complex64 tensor on {self.device}"
        strides = (ctypes.c_int64 * 3)(*x.stride())
        out_strides = (ctypes.c_int64 * 3)(*out.stride())
        return self._guarded(self._lib.fsnp_spec_stream_push, out, st, x.data_ptr(), ctypes.byref(strides), cnt, out.data_ptr(),
                             ctypes.byref(out_strides), n)

    def tail(self, slots=None):
        """Push look_ahead all-zero frames (the reference's own pad) into `slots` (None: all): the last look_ahead enhanced frames.
        -> [slots, F, look_ahead] (an empty tensor for look_ahead = 0)."""
        return self._tail(slots, torch.complex64, (self.slots, self.num_freqs), (self.slots, self.num_freqs))


class WindowStream(_Session):
    """`slots` independent live audio streams on either model, enhanced in the overlapping, cross-faded windows of enhance_wave_windowed
    (include/session/fsnp_window_stream.h; open one through model.open_window_stream): blocks of samples in, the same
    number of samples out, `delay` = `window` samples late.  A window runs through the model in the push that completes it (window k
    at k (window - overlap) + window samples), up to `max_batch` windows of all slots per forward; most pushes complete none and
    only move samples.  All push outputs of a clip followed by its finish() output, without the first `delay` samples, are
    enhance_wave_windowed(clip, window, overlap) of that clip alone, whatever the block sizes - bit for bit when both run one window
    per forward (max_batch=1).  Everything runs on the current CUDA stream; a push allocates nothing but its output tensor and never
    synchronises (under the model's error_check="sync" it then waits and polls, as forward does).  load_state takes what state() of a
    slot of any window session of the same window and overlap returned; it waits once for the copy, to learn the slot's sample count."""
    _prefix, _opener = "fsnp_window_stream", "open_window_stream"
    _copy = False                    # _debug.debug_open_window_stream_copy: the test hook's session, whose forwards copy

    def __init__(self, model, slots, window, overlap, max_samples, max_batch, device):
        self.window, self.overlap, self.max_samples, self.max_batch = window, overlap, max_samples, max_batch
        self.hop_length = int(model.hop_length)                  # (kept, as a WaveStream keeps it: later assignments do not touch the session)
        super().__init__(model, slots, window, device, False)
        self.delay = int(self._lib.fsnp_window_stream_delay(self._st))

    def _create_symbol(self, live):
        return "fsnp_debug_window_stream_create_copy" if self._copy else "fsnp_window_stream_create"

    def _create_extra(self):
        return (self.overlap, self.max_samples, self.max_batch)

    def _guarded(self, fn, out, *args):
        if self._copy:               # no model runs: nothing of the model's error policy applies
            _lib.check(_call.enqueue(fn, self.device, *args), fn.__name__)
            return out
        return super()._guarded(fn, out, *args)

    def push(self, wav, counts=None, out_format=None, clipped=None):
        """wav [slots, n] CUDA tensor, fp32 or torch.int16 at any strides (read in place), n <= max_samples; counts: None (n samples
        for every slot) or samples per slot (a Python sequence or a CPU integer tensor, 0 <= counts[b] <= n; input past counts[b] is
        never read) -> [slots, n]: column j < counts[b] of slot b is merged sample P + j - delay of its clip (exactly 0 while
        P + j < delay), columns >= counts[b] are exactly 0.  out_format: None (follow the input: float -> fp32, int16 -> "s16"), "f32"
        or "s16"; clipped: optional int32 CUDA tensor [slots], overwritten with each row's saturated or NaN samples ("s16" only)."""
        what = "WindowStream.push"
        ofmt, out_dtype = output_format(out_format, wav.dtype, what, peak=False)
        st = self._session()
        assert wav.dim() == 2, "WindowStream.push takes [slots, n] samples"
        S, n = wav.shape
        assert S == self.slots, f"expected {self.slots} slots, got {S}"
        require_cuda(wav)
        assert wav.device == self.device
        x, ifmt, row, step = pcm_input(wav)
        cnt = None if counts is None else _host_lengths(counts, S, what)
        clip = clipped_pointer(clipped, S, self.device, what)
        out = torch.empty((S, n), dtype=out_dtype, device=self.device)
        return self._guarded(self._lib.fsnp_window_stream_push_pcm, out, st, x.data_ptr(), ifmt, row, step, cnt, out.data_ptr(), ofmt, n, 1, n,
                             clip)

    def finish(self, slots=None, out_format=None, clipped=None):
        """End the clips of `slots` (None: all) -> [slots, delay]: each clip's last `delay` merged samples (exactly 0 where the clip is
        shorter), after running the clip's last window if the pushes have not; rows of slots not listed, and of slots that hold no
        samples, are exactly 0.  The finished slots are reset.  Refused, with every slot untouched, for a slot whose whole clip the
        model does not accept (1 .. n_fft / 2 samples; for the TSSE attention fewer than its 8 frames).  out_format: None or "f32",
        or "s16"; clipped as in push."""
        what = "WindowStream.finish"
        ofmt, out_dtype = output_format(out_format, torch.float32, what, peak=False)
        st = self._session()
        arr, num = _slot_array(slots)
        clip = clipped_pointer(clipped, self.slots, self.device, what)
        out = torch.empty((self.slots, self.delay), dtype=out_dtype, device=self.device)
        return self._guarded(self._lib.fsnp_window_stream_finish_pcm, out, st, arr, num, out.data_ptr(), ofmt, self.delay, 1, clip)

    def samples(self, slot):
        """Samples pushed into `slot` since its last reset or finish (host-side count)."""
        return self._counter("samples", slot)

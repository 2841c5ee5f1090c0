"""Torch-CPU restatement of the wave-session contract (include/fsnp_wave_stream.h) for ONE slot, and helpers of its tests.

TorchWaveStream.push(x [c]) returns c samples, `delay` = (2 + look_ahead) * hop samples late; finish() returns the last `delay`.  It is
built on TorchStream (the mag-session contract) and holds what a wave session carries: the newest n_fft + 1 input samples, the reflect
padding at both ends of the clip, the spectra that wait look_ahead frames for their masks, the overlap-add tail with torch.istft's
window-envelope division, and the finished samples that are not due yet.  It works in the dtype of the weights it is given."""
import numpy as np
import torch

from oracle import fsnp_torch
from oracle.weights import make_wave
from tests._stream_util import TorchStream


class TorchWaveStream:
    def __init__(self, p, **kw):
        self.ts = TorchStream(p, **kw)
        self.dtype, self.la, self.F = self.ts.dtype, kw["look_ahead"], self.ts.F
        self.hop, self.n_fft = self.F - 1, 2 * (self.F - 1)
        self.delay = (2 + self.la) * self.hop
        w32 = torch.hann_window(self.n_fft)                              # the oracle's window (fsnp_torch.stft / istft)
        self.window = w32.to(self.dtype)
        self.wsq = (w32 * w32)                                           # torch.istft forms its window envelope in the WINDOW's dtype
        self.reset()

    def reset(self):
        self.ts.reset()
        self.P = 0                                                       # samples received
        self.carry = torch.zeros(self.n_fft + 1, dtype=self.dtype)       # samples P - (n_fft + 1) .. P - 1 (0 before the clip)
        self.frames = 0                                                  # STFT frames made = steps of the model
        self.ring = []                                                   # spectra waiting for their masks (at most look_ahead + 1)
        self.tail = None                                                 # second half of the newest enhanced frame
        self.fifo = torch.zeros(0, dtype=self.dtype)                     # finished samples [sent, done)
        self.sent = 0

    # ---- one step of the model: the mask it returns belongs to frame step - look_ahead
    def _step(self, spec):
        mag = (spec.abs() if spec is not None else torch.zeros(self.F, dtype=self.dtype)).reshape(1, 1, self.F, 1)
        mask = self.ts.push(mag)
        if spec is not None:
            self.ring.append(spec)
        step, self.frames = self.frames, self.frames + 1
        if step < self.la:
            assert torch.count_nonzero(mask) == 0
            return
        x = self.ring.pop(0).reshape(1, self.F, 1)
        enh = fsnp_torch.apply_cirm(mask, x).reshape(self.F)
        fr = torch.fft.irfft(enh, n=self.n_fft) * self.window
        if self.tail is not None:                                        # frames g - 1 and g finish samples [(g - 1) hop, g hop)
            den = (self.wsq[self.hop:] + self.wsq[:self.hop]).to(self.dtype)
            self.fifo = torch.cat([self.fifo, (self.tail + fr[:self.hop]) / den])
        self.tail = fr[self.hop:]

    def _frame(self, t, buf, first, end=None):
        """STFT frame t from buf, whose element 0 is sample `first`; end: the clip's length (reflect there) or None"""
        idx = ((t - 1) * self.hop + torch.arange(self.n_fft)).abs()      # torch "reflect" at the clip's start
        if end is not None:
            idx = torch.where(idx >= end, 2 * (end - 1) - idx, idx)
        assert int(idx.min()) >= max(first, 0) and int(idx.max()) - first < buf.numel()
        return torch.fft.rfft(buf[idx - first] * self.window)

    @torch.no_grad()
    def push(self, x):
        """x [c] -> [c]: sample j is enhanced sample P + j - delay, exactly 0 while that is negative"""
        c = x.numel()
        if c == 0:
            return torch.zeros(0, dtype=self.dtype)
        buf, first = torch.cat([self.carry, x.to(self.dtype)]), self.P - (self.n_fft + 1)
        total = self.P + c
        complete = 0 if total <= self.hop else total // self.hop         # frame t needs (t + 1) hop samples, frame 0 hop + 1
        for t in range(self.frames, complete):
            self._step(self._frame(t, buf, first))
        self.carry, self.P = buf[-(self.n_fft + 1):].clone(), total
        due = max(0, total - self.delay) - self.sent
        assert 0 <= due <= c and due <= self.fifo.numel(), "the delay is too short for this push"
        out = torch.zeros(c, dtype=self.dtype)
        if due:
            out[c - due:] = self.fifo[:due]
        self.fifo, self.sent = self.fifo[due:], self.sent + due
        assert self.fifo.numel() <= self.hop
        return out

    @torch.no_grad()
    def finish(self):
        """-> [delay]: enhanced samples L - delay .. L - 1 (0 where negative); the slot is reset"""
        L = self.P
        out = torch.zeros(self.delay, dtype=self.dtype)
        if L == 0:
            return out
        if L <= self.hop:
            raise ValueError(f"{L} samples: a clip needs more than n_fft/2 = {self.hop} (reflect padding)")
        last = L // self.hop
        assert self.frames == last
        self._step(self._frame(last, self.carry, L - (self.n_fft + 1), end=L))
        for _ in range(self.la):                                         # the reference's look_ahead zero frames
            self._step(None)
        assert not self.ring
        r = L - last * self.hop                                          # behind (T - 1) hop only the last frame counts
        den = self.wsq[self.hop:self.hop + r].to(self.dtype)
        self.fifo = torch.cat([self.fifo, torch.where(den > 1e-11, self.tail[:r] / den, torch.zeros_like(den))])
        assert self.sent + self.fifo.numel() == L and self.fifo.numel() == min(L, self.delay)
        out[self.delay - self.fifo.numel():] = self.fifo
        self.reset()
        return out


def wave_clip(samples, seed):
    """[samples] fp32 seeded audio (oracle.weights.make_wave)"""
    w = make_wave(1, samples / 16000.0, seed)
    assert w.shape == (1, samples), w.shape
    return torch.from_numpy(w[0])


def schedule(total, chunk, idle_every=3):
    """chunk sizes that sum to total: `chunk` samples per push, with an idle push (0) after the first and then every idle_every pushes"""
    out, left = [], total
    while left:
        c = min(chunk, left)
        out.append(c)
        left -= c
        if len(out) % (idle_every + 1) == 1:
            out.append(0)
    return out


def random_schedule(total, seed, biggest):
    rng, out, left = np.random.RandomState(seed), [0], total
    while left:
        c = 0 if rng.rand() < 0.25 else int(min(left, rng.randint(1, biggest + 1)))
        out.append(c)
        left -= c
    return out

"""Helpers of the STFT-geometry tests (include/fsnp_stft_geometry.h): the wave-session contract restated in torch on the CPU for ONE slot
at ANY hop length, and the whole-clip oracle composed at a given geometry.

TorchWaveStreamAt generalises tests/_wave_stream_util.py TorchWaveStream (hop = n_fft / 2) and keeps the two lengths apart that coincide
there: `hop`, the distance between frames, and `half` = n_fft / 2, the reflect padding and the distance from a frame's start to its centre.
push(x [c]) returns c samples, `delay` = n_fft + look_ahead * hop samples late; finish() returns the last `delay`.  What it carries is what
a slot's record holds: the newest n_fft + 1 input samples, the spectra that wait look_ahead frames for their masks, the partial
overlap-add sums of the n_fft - hop samples behind the finished ones, and at most hop finished samples that are not due yet (both
asserted).  It works in the dtype of the weights it is given."""
import torch

from oracle import fsnp_torch
from tests._stream_util import TorchStream


def frames_held(P, hop, half):
    """STFT frames that P samples complete: frame t needs t * hop + half samples, frame 0 half + 1 (it reflects wav[1 .. half])"""
    return 0 if P <= half else (P - half) // hop + 1


def clip_lengths(n_fft, hop):
    """the clip lengths of the geometry tests: the shortest legal clip, around a multiple of the hop, and one in the middle of a hop"""
    return [n_fft // 2 + 1, 5 * hop - 1, 5 * hop, 5 * hop + 1, 9 * hop + 77]


class TorchWaveStreamAt:
    def __init__(self, p, hop, **kw):
        self.ts = TorchStream(p, **kw)
        self.dtype, self.la, self.F = self.ts.dtype, kw["look_ahead"], self.ts.F
        self.n_fft, self.hop = 2 * (self.F - 1), int(hop)
        self.half = self.n_fft // 2
        assert self.n_fft <= 8 * self.hop and 2 * self.hop <= self.n_fft
        self.delay = self.n_fft + self.la * self.hop
        w32 = torch.hann_window(self.n_fft)                              # the oracle's window (fsnp_torch.stft / istft)
        self.window = w32.to(self.dtype)
        self.wsq = w32 * w32                                             # torch.istft forms its window envelope in the WINDOW's dtype
        self.reset()

    def reset(self):
        self.ts.reset()
        self.P = 0                                                       # samples received
        self.carry = torch.zeros(self.n_fft + 1, dtype=self.dtype)       # samples P - (n_fft + 1) .. P - 1 (0 before the clip)
        self.frames = 0                                                  # STFT frames made
        self.enh = 0                                                     # enhanced frames overlap-added
        self.ring = []                                                   # spectra waiting for their masks (at most look_ahead + 1)
        self.sums = torch.zeros(self.n_fft - self.hop, dtype=self.dtype)  # partial sums of samples enh * hop - half + q
        self.fifo = torch.zeros(0, dtype=self.dtype)                     # finished samples [sent, done)
        self.sent = 0

    def _envelope(self, first, count, frames):
        """sum of w^2 over the frames t < `frames` that cover samples first .. first + count - 1, added as torch.istft adds them: in the
        window's dtype, frame by frame from the oldest (by descending position inside the window)"""
        p = torch.arange(first, first + count) + self.half               # positions in the centre-padded clip
        den = torch.zeros(count, dtype=self.wsq.dtype)
        for j in reversed(range(-(-self.n_fft // self.hop))):
            k = p % self.hop + j * self.hop
            t = (p - k) // self.hop
            ok = (k < self.n_fft) & (t >= 0) & (t < frames)
            den = den + torch.where(ok, self.wsq[k.clamp(max=self.n_fft - 1)], torch.zeros_like(den))
        return den.to(self.dtype)

    def _finished(self, values, first, frames):
        """values of samples first .. (overlap-add sums) -> the samples >= 0 among them, divided by their envelope"""
        den = self._envelope(first, values.numel(), frames)
        out = torch.where(den > 1e-11, values / den, torch.zeros_like(den))
        return out[max(0, -first):]

    # ---- one step of the model: the mask it returns belongs to frame step - look_ahead
    def _step(self, spec, step):
        mag = (spec.abs() if spec is not None else torch.zeros(self.F, dtype=self.dtype)).reshape(1, 1, self.F, 1)
        mask = self.ts.push(mag)
        if spec is not None:
            self.ring.append(spec)
        if step < self.la:
            assert torch.count_nonzero(mask) == 0
            return
        x = self.ring.pop(0).reshape(1, self.F, 1)
        enh = fsnp_torch.apply_cirm(mask, x).reshape(self.F)
        fr = torch.fft.irfft(enh, n=self.n_fft) * self.window
        e = self.enh                                                     # this frame: samples [e hop - half, e hop + half)
        acc = torch.cat([self.sums, torch.zeros(self.hop, dtype=self.dtype)]) + fr
        # with e + 1 frames the samples below (e + 1) hop - half are finished: every frame that covers them is in
        self.fifo = torch.cat([self.fifo, self._finished(acc[:self.hop], e * self.hop - self.half, e + 1)])
        self.sums, self.enh = acc[self.hop:], e + 1

    def _frame(self, t, buf, first, end=None):
        """STFT frame t from buf, whose element 0 is sample `first`; end: the clip's length (reflect there) or None"""
        idx = (t * self.hop - self.half + torch.arange(self.n_fft)).abs()      # torch "reflect" at the clip's start
        if end is not None:
            idx = torch.where(idx >= end, 2 * (end - 1) - idx, idx)
        assert int(idx.min()) >= max(first, 0) and int(idx.max()) - first < buf.numel(), "the carry is too short for this frame"
        return torch.fft.rfft(buf[idx - first] * self.window)

    @torch.no_grad()
    def push(self, x):
        """x [c] -> [c]: sample j is enhanced sample P + j - delay, exactly 0 while that is negative"""
        c = x.numel()
        if c == 0:
            return torch.zeros(0, dtype=self.dtype)
        buf, first = torch.cat([self.carry, x.to(self.dtype)]), self.P - (self.n_fft + 1)
        total = self.P + c
        for t in range(self.frames, frames_held(total, self.hop, self.half)):
            self._step(self._frame(t, buf, first), t)
            self.frames = t + 1
        self.carry, self.P = buf[-(self.n_fft + 1):].clone(), total
        due = max(0, total - self.delay) - self.sent
        assert 0 <= due <= c and due <= self.fifo.numel(), "the delay is too short for this push"
        out = torch.zeros(c, dtype=self.dtype)
        if due:
            out[c - due:] = self.fifo[:due]
        self.fifo, self.sent = self.fifo[due:], self.sent + due
        assert self.fifo.numel() <= self.hop, "the fifo outgrew hop samples"
        return out

    @torch.no_grad()
    def finish(self):
        """-> [delay]: enhanced samples L - delay .. L - 1 (0 where negative); the slot is reset"""
        L = self.P
        out = torch.zeros(self.delay, dtype=self.dtype)
        if L == 0:
            return out
        if L <= self.half:
            raise ValueError(f"{L} samples: a clip needs more than n_fft/2 = {self.half} (reflect padding)")
        T = 1 + L // self.hop
        assert self.frames == frames_held(L, self.hop, self.half) and 1 <= T - self.frames <= -(-self.half // self.hop)
        self.finish_frames = T - self.frames
        for t in range(self.frames, T):                                  # the clip's last frames, each reflected at its end
            self._step(self._frame(t, self.carry, L - (self.n_fft + 1), end=L), t)
        for j in range(self.la):                                         # the reference's look_ahead zero frames
            self._step(None, T + j)
        assert not self.ring and self.enh == T
        first = T * self.hop - self.half                                 # behind it only the T frames of the clip count
        assert 0 <= L - first <= self.sums.numel()
        self.fifo = torch.cat([self.fifo, self._finished(self.sums[:L - first], first, T)])
        assert self.sent + self.fifo.numel() == L and self.fifo.numel() == min(L, self.delay)
        out[self.delay - self.fifo.numel():] = self.fifo
        self.reset()
        return out


@torch.no_grad()
def oracle_enhance_wave(sd, wav, num_freqs, hop, fullsubnet=False, **kw):
    """fsnp_torch.enhance_wave (inferencer.py:142-158) composed at n_fft = 2 (num_freqs - 1) and `hop`: wav [B, L] -> [B, L], every clip on its
    own as the reference's inferencer runs it (no drop_band)"""
    n_fft = 2 * (num_freqs - 1)
    X = fsnp_torch.stft(wav, n_fft, hop, n_fft)
    if fullsubnet:
        mask = fsnp_torch.forward_fullsubnet_full(sd, X.abs().unsqueeze(1), **kw)
    else:
        mask = fsnp_torch.forward_full(sd, X.abs().unsqueeze(1), X.real.unsqueeze(1), X.imag.unsqueeze(1), **kw)
    return fsnp_torch.istft(fsnp_torch.apply_cirm(mask, X), wav.shape[-1], n_fft, hop, n_fft)

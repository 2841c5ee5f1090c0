"""float64 restatement of the rate-session contract (include/fsnp_wave_rate_stream.h) for ONE slot, and helpers of its tests.

TorchWaveRateStream is a TorchWaveStreamAt (the wave-session contract at the model's rate M, tests/_wave_geometry_util.py) between two
streaming converters written from the header's rules and the filter of tests/_resample_util.py: push(x [c]) at rate R returns c samples
`delay` = D_R late, finish() the last D_R.  What it carries is what a slot's rate record holds - the newest floor(2 half / up) input
samples, the newest ceil(2 half / down) enhanced model-rate samples, the count - and it asserts that no sum ever reaches below them,
that no sum of a push reaches past what has arrived (the delay is long enough), and how many model-rate samples one call makes."""
import numpy as np
import torch

from tests._resample_util import plan, resample64, taps64
from tests._wave_geometry_util import TorchWaveStreamAt, oracle_enhance_wave


def ready(P, up, down, half):
    """model-rate samples whose whole window lies inside the first P input samples"""
    return 0 if P * up <= half else (P * up - half - 1) // down + 1


def total(L, up, down):
    return -(-L * up // down)


def rate_delay(DM, up, down, half):
    return -(-(DM * down + 2 * half + 1) // up) - 1


def _sum(t, step_out, step_in, half, buf, first, m, n):
    """y[m] = sum over 0 <= k < n with |m step_out - k step_in| <= half of t[m step_out - k step_in] buf[k - first]; -> (y, lowest k, highest k)"""
    c = m * step_out
    k0 = max(0, -((half - c) // step_in))
    k1 = min(n - 1, (c + half) // step_in)
    if k1 < k0:
        return 0.0, k0, k1
    assert k0 >= first, f"sample {m} reads input {k0}, the history starts at {first}"
    k = np.arange(k0, k1 + 1)
    return float((t[c - k * step_in + half] * buf[k - first]).sum()), k0, k1


class TorchWaveRateStream:
    def __init__(self, p, hop, rate, model_rate, **kw):
        self.inner = TorchWaveStreamAt(p, hop, **kw)
        self.up, self.down, self.half = plan(rate, model_rate)
        assert plan(model_rate, rate) == (self.down, self.up, self.half)
        self.t_in = self.up * taps64(rate, model_rate)
        self.t_out = self.down * taps64(model_rate, rate)
        self.DM = self.inner.delay
        self.delay = rate_delay(self.DM, self.up, self.down, self.half)
        self.HI, self.HE = 2 * self.half // self.up, -(-2 * self.half // self.down)
        self.n_half = self.inner.half
        self.most_per_push = self.most_at_finish = 0
        self.reset()

    def reset(self):
        self.inner.reset()
        self.P, self.E = 0, 0                                # samples at rate R received, enhanced model-rate samples held
        self.hist_in = np.zeros(self.HI)                     # samples P - HI .. P - 1
        self.hist_e = np.zeros(self.HE)                      # enhanced samples E - HE .. E - 1

    def _ready(self, P):
        return ready(P, self.up, self.down, self.half)

    def _convert_in(self, buf, j0, j1, n):
        out = np.zeros(j1 - j0)
        for j in range(j0, j1):
            out[j - j0], _, k1 = _sum(self.t_in, self.down, self.up, self.half, buf, self.P - self.HI, j, n)
            assert k1 <= n - 1
        return out

    def _inner_push(self, xm, r0):
        """the inner session's output of samples r0 .. of its stream -> the enhanced samples (index - DM >= 0) among them"""
        o = self.inner.push(torch.from_numpy(xm)).numpy() if xm.size else np.zeros(0)
        assert o.shape == xm.shape
        lead = min(max(self.DM - r0, 0), o.size)
        assert not o[:lead].any()
        return o[lead:]

    @torch.no_grad()
    def push(self, x):
        """x [c] float64 -> [c]: sample j is enhanced sample P + j - delay at rate R, exactly 0 while that is negative"""
        x = np.asarray(x, dtype=np.float64)
        c = x.size
        if c == 0:
            return torch.zeros(0, dtype=torch.float64)
        buf = np.concatenate([self.hist_in, x])
        r0, r1 = self._ready(self.P), self._ready(self.P + c)
        assert r1 - r0 <= c * self.up // self.down + 1
        self.most_per_push = max(self.most_per_push, r1 - r0)
        xm = self._convert_in(buf, r0, r1, self.P + c)
        ebuf = np.concatenate([self.hist_e, self._inner_push(xm, r0)])
        efirst, E1 = self.E - self.HE, max(r1 - self.DM, 0)
        assert ebuf.size == E1 - efirst
        out = np.zeros(c)
        for j in range(c):
            m = self.P + j - self.delay
            if m >= 0:
                out[j], _, k1 = _sum(self.t_out, self.up, self.down, self.half, ebuf, efirst, m, E1)
                assert (m * self.up + self.half) // self.down <= E1 - 1, "the delay is too short for this push"
        self.hist_in, self.hist_e, self.P, self.E = buf[-self.HI:].copy(), ebuf[-self.HE:].copy(), self.P + c, E1
        return torch.from_numpy(out)

    @torch.no_grad()
    def finish(self):
        """-> [delay]: enhanced samples L - delay .. L - 1 at rate R (0 where negative); the slot is reset"""
        L = self.P
        out = np.zeros(self.delay)
        if L == 0:
            return torch.from_numpy(out)
        r0, r1 = self._ready(L), total(L, self.up, self.down)
        if r1 <= self.n_half:
            raise ValueError(f"{L} samples are {r1} at the model's rate: a clip needs more than n_fft/2 = {self.n_half} (reflect padding)")
        assert r1 - r0 <= -(-self.half // self.down)
        self.most_at_finish = max(self.most_at_finish, r1 - r0)
        xm = self._convert_in(self.hist_in, r0, r1, L)                       # the input clamped at L - 1
        new_e = self._inner_push(xm, r0)
        last = self.inner.finish().numpy()                                   # inner samples r1 - DM .. r1 - 1
        ebuf = np.concatenate([self.hist_e, new_e, last[max(self.DM - r1, 0):]])
        efirst = self.E - self.HE
        assert ebuf.size == r1 - efirst
        for j in range(self.delay):
            m = L - self.delay + j
            if m >= 0:
                out[j], _, _ = _sum(self.t_out, self.up, self.down, self.half, ebuf, efirst, m, r1)      # the enhanced clip clamped at r1 - 1
        self.reset()
        return torch.from_numpy(out)


@torch.no_grad()
def oracle_rate(sd, clip, rate, model_rate, num_freqs, hop, **kw):
    """the whole-clip oracle at rate R: resample64 -> oracle_enhance_wave at the model's rate -> resample64, cut to the clip's length"""
    x = resample64(clip.numpy(), rate, model_rate)[0]
    e = oracle_enhance_wave(sd, torch.from_numpy(x).to(next(iter(sd.values())).dtype).unsqueeze(0), num_freqs, hop, fullsubnet=True, **kw)[0]
    return torch.from_numpy(resample64(e.double().numpy(), model_rate, rate)[0][:clip.numel()])


def shortest_clip(up, down, n_half):
    """the fewest samples at rate R whose model-rate length total(L) exceeds n_fft / 2"""
    L = 1
    while total(L, up, down) <= n_half:
        L += 1
    return L

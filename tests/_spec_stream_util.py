"""Torch-CPU restatement of the spectrum-session contract (include/fsnp_spec_stream.h) for ONE slot, and helpers of its tests.

TorchSpecStream.push(X [1, F, c] complex) feeds |X| to TorchStream (the mag-session contract), keeps the noisy frames that wait for their
masks in a list, and returns c columns: column j is oracle.fsnp_torch.apply_cirm of the model's output of step P + j and the noisy frame
P + j - look_ahead, exactly 0 + 0i where P + j < look_ahead.  It works in the dtype of the weights it is given."""
import numpy as np
import torch

from oracle import fsnp_torch
from tests._stream_util import TorchStream


class TorchSpecStream:
    def __init__(self, p, **kw):
        self.mag = TorchStream(p, **kw)
        self.la, self.F, self.dtype = self.mag.la, self.mag.F, self.mag.dtype
        self.cdtype = torch.complex128 if self.dtype == torch.float64 else torch.complex64
        self.waiting = []              # noisy frames [1, F] that have no mask yet, oldest first (at most look_ahead)

    @property
    def P(self):
        return self.mag.P

    def reset(self):
        self.mag.reset()
        self.waiting = []

    @torch.no_grad()
    def push(self, X):
        """X [1, F, c] complex -> [1, F, c] complex"""
        c = X.shape[-1]
        out = torch.zeros(1, self.F, c, dtype=self.cdtype)
        if c == 0:
            return out
        X = X.to(self.cdtype)
        P = self.P
        mask = self.mag.push(X.abs().unsqueeze(1))                 # [1, 2, F, c]: step P + j in column j
        frames = self.waiting + [X[..., j] for j in range(c)]      # frames P - len(waiting) ... P + c - 1
        first = P - len(self.waiting)
        for j in range(c):
            g = P + j - self.la
            if g < 0:
                continue
            out[..., j] = fsnp_torch.apply_cirm(mask[..., j:j + 1], frames[g - first].unsqueeze(-1))[..., 0]
        self.waiting = frames[max(len(frames) - self.la, 0):] if self.la else []
        return out

    def tail(self):
        return self.push(torch.zeros(1, self.F, self.la, dtype=self.cdtype))


def spec_clip(batch, frames, seed):
    """[batch, F, frames] complex64 CPU in torch.stft's memory order (bins fastest), from oracle.make_golden.make_spec"""
    from oracle.make_golden import make_spec
    _, re, im = make_spec(batch, frames, seed)
    return torch.complex(re[:, 0], im[:, 0])


def oracle_enhance(sd, X, **kw):
    """The yardstick: apply_cirm(forward_fullsubnet_full(sd, |X|), X) per clip, X [B, F, T] complex -> [B, F, T] complex"""
    return torch.cat([fsnp_torch.apply_cirm(fsnp_torch.forward_fullsubnet_full(sd, X[b:b + 1].abs().unsqueeze(1), **kw), X[b:b + 1])
                      for b in range(X.shape[0])])


def random_schedule(total, seed, biggest):
    """chunk sizes in [0, biggest] that sum to total, about a third of them idle pushes"""
    rng = np.random.RandomState(seed)
    out, left = [], total
    while left:
        c = 0 if rng.rand() < 0.3 else int(min(left, rng.randint(1, biggest + 1)))
        out.append(c)
        left -= c
    return out


def crel_err(got, want):
    """max |got - want| over max |want| of complex tensors"""
    return float((got - want).abs().max() / want.abs().max())

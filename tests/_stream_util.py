"""Torch-CPU restatement of the stream-session contract (include/fsnp_stream.h) for ONE slot, and helpers of the streaming tests.

TorchStream.push(x [1, 1, F, c]) runs steps P .. P+c-1 of the pieces of oracle.fsnp_torch.forward_fullsubnet_full - both cumulative norms as
prefix sums continued from carried sums, both two-layer LSTMs from carried (h, c) - and returns the model's output of those steps, with
exactly 0 where P + j < look_ahead.  It works in the dtype of the weights it is given (the identity test uses fp64)."""
import torch
import torch.nn.functional as Fn

from oracle import fsnp_torch

EPS = fsnp_torch.EPSILON


class TorchStream:
    def __init__(self, p, *, look_ahead, sb_num_neighbors, fb_num_neighbors, norm_type, fb_output_activate_function,
                 sb_output_activate_function, num_groups_in_drop_band=2):
        assert norm_type in ("cumulative_laplace_norm", "cumulative_layer_norm")
        self.p, self.la, self.nsb, self.nfb, self.norm_type = p, look_ahead, sb_num_neighbors, fb_num_neighbors, norm_type
        self.fb_act, self.sb_act = fb_output_activate_function, sb_output_activate_function
        self.dtype = p["fb_model.sequence_model.weight_hh_l0"].dtype
        self.F = p["fb_model.sequence_model.weight_ih_l0"].shape[1]
        self.reset()

    def reset(self):
        z = lambda *s: torch.zeros(*s, dtype=self.dtype)
        CH = self.p["fb_model.sequence_model.weight_hh_l0"].shape[1]
        H = self.p["sb_model.sequence_model.weight_hh_l0"].shape[1]
        self.P = 0
        self.fb_hc = (z(2, 1, CH), z(2, 1, CH))
        self.sb_hc = (z(2, self.F, H), z(2, self.F, H))
        self.fb_sums = (z(1), z(1))                    # running sum, sum of squares of the full-band input
        self.sb_sums = (z(self.F), z(self.F))          # the same per sub-band sequence

    def _norm(self, y, sums, rows):
        """y [N, rows, c]: normalise with the prefix statistics continued from `sums` ([N] each); entry count of step t = rows (P + t + 1)."""
        c = y.shape[-1]
        count = (torch.arange(self.P + 1, self.P + c + 1, dtype=self.dtype) * rows).reshape(1, c)
        cum = sums[0].unsqueeze(1) + torch.cumsum(y.sum(dim=1), dim=-1)
        cum_pow = sums[1].unsqueeze(1) + torch.cumsum(torch.square(y).sum(dim=1), dim=-1)
        new = (cum[:, -1].clone(), cum_pow[:, -1].clone())
        mean = cum / count
        if self.norm_type == "cumulative_laplace_norm":
            return y / (mean.unsqueeze(1) + EPS), new
        var = (cum_pow - 2 * mean * cum) / count + mean.pow(2)
        return (y - mean.unsqueeze(1)) / torch.sqrt(var + EPS).unsqueeze(1), new

    def _lstm(self, x, prefix, hc, act):
        flat = [self.p[f"{prefix}.sequence_model.{nm}_l{layer}"] for layer in (0, 1) for nm in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        o, h, c = torch.lstm(x.permute(0, 2, 1).contiguous(), hc, flat, True, 2, 0.0, False, False, True)
        o = Fn.linear(o, self.p[prefix + ".fc_output_layer.weight"], self.p[prefix + ".fc_output_layer.bias"])
        return fsnp_torch._activation(o, act).permute(0, 2, 1).contiguous(), (h, c)

    @torch.no_grad()
    def push(self, x):
        """x [1, 1, F, c] -> [1, 2, F, c]"""
        c, F = x.shape[-1], self.F
        if c == 0:
            return torch.zeros(1, 2, F, 0, dtype=self.dtype)
        mag = x.to(self.dtype)
        fb_in, self.fb_sums = self._norm(mag.reshape(1, F, c), self.fb_sums, F)
        fb_out, self.fb_hc = self._lstm(fb_in, "fb_model", self.fb_hc, self.fb_act)
        nfb, nsb = 2 * self.nfb + 1, 2 * self.nsb + 1
        fb_unf = fsnp_torch.unfold(fb_out.reshape(1, 1, F, c), self.nfb).reshape(1, F, nfb, c)
        mag_unf = fsnp_torch.unfold(mag, self.nsb).reshape(1, F, nsb, c)
        sb_in, self.sb_sums = self._norm(torch.cat([mag_unf, fb_unf], dim=2).reshape(F, nsb + nfb, c), self.sb_sums, nsb + nfb)
        mask, self.sb_hc = self._lstm(sb_in, "sb_model", self.sb_hc, self.sb_act)
        out = mask.reshape(1, F, 2, c).permute(0, 2, 1, 3).contiguous()
        warm = max(0, min(c, self.la - self.P))
        out[..., :warm] = 0
        self.P += c
        return out


def stream_kwargs(args):
    """The oracle's keyword arguments out of a FullSubNet constructor-argument dict."""
    return {k: args[k] for k in ("look_ahead", "sb_num_neighbors", "fb_num_neighbors", "norm_type", "num_groups_in_drop_band",
                                 "fb_output_activate_function", "sb_output_activate_function")}


def chunked(total, chunks):
    """[(start, count)] of a clip of `total` frames cut as `chunks` (their sum must be total)."""
    assert sum(chunks) == total, (chunks, total)
    out, s = [], 0
    for c in chunks:
        out.append((s, c))
        s += c
    return out

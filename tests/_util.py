"""Shared helpers for the tests: golden-fixture loading and input regeneration."""
import json
import os

import numpy as np
import torch

from oracle.make_golden import make_spec
from oracle.weights import make_inputs, make_state_dict, make_state_dict_fullsubnet

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_names(model="plus"):
    """Fixtures of FullSubNet+ ("plus") or of the original FullSubNet ("fullsubnet", files fsn_*)."""
    names = sorted(f[:-4] for f in os.listdir(GOLDEN_DIR) if f.endswith(".npz"))
    return [n for n in names if n.startswith("fsn_") == (model == "fullsubnet")]


class Golden:
    def __init__(self, name):
        self.name = name
        z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
        self.arrays = {k: z[k] for k in z.files if k != "meta"}
        self.meta = json.loads(bytes(z["meta"]).decode())
        self.args = self.meta["args"]
        self.sub = self.meta.get("subsample_f", 1)

    @property
    def is_fullsubnet(self):
        return self.meta.get("model") == "fullsubnet"

    def state_dict(self):
        if self.is_fullsubnet:
            return make_state_dict_fullsubnet(self.meta["wseed"], self.meta["profile"],
                                              sequence_model=self.args.get("sequence_model", "LSTM"),
                                              fb_num_neighbors=self.args.get("fb_num_neighbors", 0),
                                              num_freqs=self.args.get("num_freqs", 257),
                                              sb_num_neighbors=self.args.get("sb_num_neighbors", 15),
                                              fb_hidden=self.args.get("fb_model_hidden_size", 512),
                                              sb_hidden=self.args.get("sb_model_hidden_size", 384))
        return make_state_dict(self.meta["wseed"], self.meta["profile"],
                               attention=self.args.get("channel_attention_model", "TSSE"),
                               sequence_model=self.args.get("sequence_model", "LSTM"),
                               fb_num_neighbors=self.args.get("fb_num_neighbors", 0),
                               num_freqs=self.args.get("num_freqs", 257),
                               sb_num_neighbors=self.args.get("sb_num_neighbors", 15),
                               kersize=tuple(self.args.get("kersize", (3, 5, 10))),
                               sb_hidden=self.args.get("sb_model_hidden_size", 384),
                               output_size=self.args.get("output_size", 2))

    def inputs(self):
        inp = self.meta["inp"]
        if "mag" in self.arrays:             # fsn_* stft fixtures keep the magnitude itself, [B,1,F,T]
            m = torch.from_numpy(self.arrays["mag"][:, 0].transpose(0, 2, 1).copy()).permute(0, 2, 1).unsqueeze(1)
            return m, None, None
        if "X" in self.arrays:
            X = torch.from_numpy(self.arrays["X"].transpose(0, 2, 1).copy()).permute(0, 2, 1)  # stft strides
            return X.abs().unsqueeze(1), X.real.unsqueeze(1), X.imag.unsqueeze(1)
        if inp["kind"] == "stft":
            return make_inputs(inp["B"], inp["t"], inp["seed"])
        return make_spec(inp["B"], inp["t"], inp["seed"], self.args.get("num_freqs", 257))

    def fwd_kwargs(self):
        a = self.args
        if self.is_fullsubnet:
            return {k: a[k] for k in ("look_ahead", "sb_num_neighbors", "fb_num_neighbors", "norm_type",
                                      "num_groups_in_drop_band", "fb_output_activate_function",
                                      "sb_output_activate_function")}
        return dict(look_ahead=a["look_ahead"], sb_num_neighbors=a["sb_num_neighbors"],
                    fb_num_neighbors=a["fb_num_neighbors"], norm_type=a["norm_type"],
                    num_groups_in_drop_band=a["num_groups_in_drop_band"],
                    channel_attention_model=a.get("channel_attention_model", "TSSE"),
                    subband_num=a.get("subband_num", 1),
                    fb_output_activate_function=a.get("fb_output_activate_function", "ReLU"),
                    sb_output_activate_function=a.get("sb_output_activate_function", False),
                    output_size=a.get("output_size", 2))


def reference_facts():
    """tests/golden/reference/facts.json: what oracle/make_golden.py main_reference_facts recorded about the reference (its config
    digest, [model.args], parameter trees and unfold digests), so the checks against it run where the reference is not mounted."""
    with open(os.path.join(GOLDEN_DIR, "reference", "facts.json")) as f:
        return json.load(f)


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ------------------------------------------------------------------------------------------------ stage-level comparison
STAGE_TAGS = ("att_mag", "att_real", "att_imag", "fb_mag", "fb_real", "fb_imag")
STAGE_CAPS = {"att": 2e-5, "fb": 2e-4}       # what the suite already asserts at these stages (test_stages_vs_reference, the submodule test)


def plane_errs(got, want):
    """got, want [B, F, T'] -> (errs, where): errs[b] = max|got[b] - want[b]| / max|want[b]| over utterance b's OWN plane (a quiet clip
    cannot hide behind a loud one of the same batch), where[b] = (bin, frame) of its worst element.  A non-finite element of `got` is
    an infinite error at that element."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and got.ndim == 3, (got.shape, want.shape)
    errs, where = [], []
    for g, w in zip(got, want):
        d = np.abs(g - w)
        d[~np.isfinite(d)] = np.inf
        k = int(np.argmax(d))
        errs.append(float(d.flat[k] / max(np.abs(w).max(), 1e-30)))
        where.append(tuple(int(i) for i in np.unravel_index(k, d.shape)))
    return errs, where


def mask_errs(got, want):
    """got, want [B, output_size, Fo, T] -> plane_errs of each utterance's own [output_size, Fo, T] block (reshaped to one plane of
    Fo * output_size rows): (errs, where) with where[b] = (bin, output, frame)."""
    got, want = np.asarray(got), np.asarray(want)
    B, O, Fo, T = want.shape
    errs, where = plane_errs(got.transpose(0, 2, 1, 3).reshape(B, Fo * O, T), want.transpose(0, 2, 1, 3).reshape(B, Fo * O, T))
    return errs, [(r // O, r % O, t) for r, t in where]


def spec_dc(batch, frames, seed, num_freqs=257, dc=0.6):
    """oracle.make_golden.make_spec's recipe (same envelope, same [B][T][F] complex64 layout, same return) with real / imag planes that
    have a mean: re = env * (dc + N(0, 1)), im = env * (-dc + N(0, 1)).  The two Laplace norms divide by a plane's (running) mean; on
    make_spec's zero-mean real / imag planes that mean is a cancelled sum and the float32 oracle itself is off by up to 7.7e-4 of the
    plane (cumulative_laplace_norm, B = 2, T = 38), which is no yardstick.  With dc = 0.6 it stays at or below 3.5e-7."""
    rng = np.random.Generator(np.random.PCG64(20_000 + seed))
    env = (0.05 + rng.random(size=(batch, frames, 1))) * (0.2 + rng.random(size=(batch, 1, num_freqs)))
    re = (env * (dc + rng.standard_normal(size=(batch, frames, num_freqs)))).astype(np.float32)
    im = (env * (-dc + rng.standard_normal(size=(batch, frames, num_freqs)))).astype(np.float32)
    X = torch.complex(torch.from_numpy(re), torch.from_numpy(im)).permute(0, 2, 1)  # [B,F,T], strides (T*F,1,F)
    return X.abs().unsqueeze(1), X.real.unsqueeze(1), X.imag.unsqueeze(1)


def reflect_pad_bins(x, pad):
    """[B, 1, F, T] -> [B, 1, F + pad, T]: `pad` reflected rows behind the last bin (row F + k = row F - 2 - k), fullsubnet_plus.py:148.
    Looked up when oracle_frontend runs, so a test may replace it."""
    return torch.nn.functional.pad(x, [0, 0, 0, pad], mode="reflect")


@torch.no_grad()
def oracle_frontend(sd, ins, args, dtype=torch.float64):
    """The front end of fsnp_torch.forward alone (pad by look_ahead, NORMS[norm_type], the attention of channel_attention_model),
    evaluated in `dtype` with the attention weights and the inputs cast to it: ins = (mag, real, imag) [B, 1, F, T], None for a branch
    that is not wanted -> {"att_<tag>": [B, F, T + look_ahead], "gate_<tag>": [B, F]}.  With subband_num > 1 the magnitude branch is
    regrouped as fsnp_torch.forward does it (reflect-pad the bins, view as [(F + pad) / sn channels][sn T'], gate the channels, keep
    the first F rows): the gate of bin f is then the gate of channel f // sn.  The oracle's functions are looked up when called."""
    from oracle import fsnp_torch
    p = {k: v.to(dtype) for k, v in sd.items() if k.startswith("channel_attention")}
    kind, la, sn = args.get("channel_attention_model", "TSSE"), args["look_ahead"], args.get("subband_num", 1)
    out = {}
    for tag, x in zip(("mag", "real", "imag"), ins):
        if x is None:
            continue
        x = torch.nn.functional.pad(x.to(dtype), [0, la])
        B, _, F, T = x.shape
        prefix = "channel_attention" + ("" if tag == "mag" else "_" + tag)
        xn = fsnp_torch.NORMS[args["norm_type"]](x)
        if tag == "mag" and sn != 1:                                 # oracle/fsnp_torch.py forward, fullsubnet_plus.py:146-153
            pad_num = sn - F % sn
            xin = reflect_pad_bins(xn, pad_num).reshape(B, (F + pad_num) // sn, T * sn)
            g = fsnp_torch.attention_gate(xin, p, prefix, kind)
            att = (xin * g.unsqueeze(2)).reshape(B, F + pad_num, T)[:, :F, :]
            gate = g.repeat_interleave(sn, dim=1)[:, :F]
        else:
            xin = xn.reshape(B, F, T)
            gate = fsnp_torch.attention_gate(xin, p, prefix, kind)
            att = xin * gate.unsqueeze(2)
        out["att_" + tag], out["gate_" + tag] = att, gate
    return out


@torch.no_grad()
def oracle_stages(sd, ins, args, dtype=torch.float64):
    """The attention and full-band stages of fsnp_torch.forward alone (no sub-band model), evaluated in `dtype` with the state dict and
    the inputs cast to it: ins = (mag, real, imag) [B, 1, F, T] -> {tag: [B, F, T + look_ahead]} for the tags of STAGE_TAGS."""
    from oracle import fsnp_torch
    p = {k: v.to(dtype) for k, v in sd.items() if k.startswith("fb_model")}
    front = oracle_frontend(sd, ins, args, dtype)
    out = {}
    for tag in ("mag", "real", "imag"):
        if "att_" + tag not in front:
            continue
        att = front["att_" + tag]
        out["att_" + tag] = att
        out["fb_" + tag] = fsnp_torch.fb_sequence_model(att, p, "fb_model" + ("" if tag == "mag" else "_" + tag),
                                                        args["fb_output_activate_function"])
    return out


FRONTEND_K, FRONTEND_FLOOR = 8, 2.0 ** -23


def frontend_bound(e32, k=FRONTEND_K):
    """What tests/test_gpu_frontend.py allows plane_errs(hip, oracle64) of one att_* plane or one gate_* vector, given e32 =
    plane_errs(oracle32, oracle64) of the same: k times the float32 oracle's own error (floored at one fp32 spacing of the plane's
    maximum), never beyond STAGE_CAPS["att"].  The figures of test_gpu_stages.py at this stage and of fullband_lstm_bound."""
    return min(k * max(e32, FRONTEND_FLOOR), STAGE_CAPS["att"])


FB_LSTM_K, FB_LSTM_CAP, FB_LSTM_FLOOR = 8, 2e-5, 2.0 ** -23


def fullband_lstm_bound(e32, k=FB_LSTM_K):
    """What tests/test_gpu_fullband_lstm.py allows plane_errs(hip, oracle64) of one fb_mag plane of the original FullSubNet, given e32 =
    plane_errs(oracle32, oracle64) of that plane: k times the float32 oracle's own error (floored at one fp32 spacing of the plane's
    maximum, below which e32 is luck), never beyond what the suite asserts of every recurrent kernel in dense mode."""
    return min(k * max(e32, FB_LSTM_FLOOR), FB_LSTM_CAP)


@torch.no_grad()
def oracle_fullband_fullsubnet(sd, mag, args, dtype=torch.float64):
    """The full-band stage of fsnp_torch.forward_fullsubnet alone (pad by look_ahead, norm, the two-layer recurrent fb_model, Linear,
    activation), evaluated in `dtype` with the fb_model.* weights and the input cast to it: mag [B, 1, F, T] ->
    {"fb_mag": [B, F, T + look_ahead]}."""
    from oracle import fsnp_torch
    p = {k: v.to(dtype) for k, v in sd.items() if k.startswith("fb_model.")}
    x = torch.nn.functional.pad(mag.to(dtype), [0, args["look_ahead"]])
    B, C, F, T = x.shape
    assert C == 1
    fb_input = fsnp_torch.NORMS[args["norm_type"]](x).reshape(B, F, T)
    return {"fb_mag": fsnp_torch.lstm2_fc(fb_input, p, "fb_model", args["fb_output_activate_function"])}


@torch.no_grad()
def oracle_subband(sd, stages, args, dtype, drop_band=False, record=None):
    """The sub-band half of fsnp_torch.forward / forward_fullsubnet alone (oracle/fsnp_torch.py: unfold with reflect padding,
    concatenate, normalise over the concatenated tensor, drop bands, lstm2_fc or the TCN sub-band model, reshape, look-ahead trim),
    evaluated in `dtype` with the sub-band weights cast to it.  stages = {att_mag, fb_mag[, fb_real, fb_imag]}, each
    [B, F, T + look_ahead] (the original FullSubNet has one fb branch and the padded magnitude as att_mag)
    -> mask [B', output_size, Fo, T].  The oracle's functions are looked up when called, so a test may replace one; record: a dict that
    receives "sb_input", the sub-band model's input [B' * Fo, features, T + look_ahead]."""
    from oracle import fsnp_torch
    p = {k: v.to(dtype) for k, v in sd.items() if k.startswith("sb_model")}
    att = stages["att_mag"].to(dtype)
    fbs = [stages[tag].to(dtype) for tag in ("fb_mag", "fb_real", "fb_imag") if tag in stages]
    B, F, T = att.shape
    la, nsbn, nfbn, out_size = args["look_ahead"], args["sb_num_neighbors"], args["fb_num_neighbors"], args.get("output_size", 2)
    nsb, nfb = 2 * nsbn + 1, 2 * nfbn + 1
    parts = [fsnp_torch.unfold(att.reshape(B, 1, F, T), nsbn).reshape(B, F, nsb, T)]
    parts += [fsnp_torch.unfold(o.reshape(B, 1, F, T), nfbn).reshape(B, F, nfb, T) for o in fbs]
    sb_input = fsnp_torch.NORMS[args["norm_type"]](torch.cat(parts, dim=2))
    Fo = F
    if drop_band:
        sb_input = fsnp_torch.drop_band(sb_input.permute(0, 2, 1, 3), args["num_groups_in_drop_band"])
        Fo = sb_input.shape[2]
        sb_input = sb_input.permute(0, 2, 1, 3)
    sb_input = sb_input.reshape(sb_input.shape[0] * Fo, nsb + len(fbs) * nfb, T)
    if record is not None:
        record["sb_input"] = sb_input
    act = args.get("sb_output_activate_function", False)
    if "sb_model.sequence_model.0.conv1x1.weight" in p:
        sb_mask = fsnp_torch.fb_sequence_model(sb_input, p, "sb_model", act).contiguous()
    else:
        sb_mask = fsnp_torch.lstm2_fc(sb_input, p, "sb_model", act)
    sb_mask = sb_mask.reshape(-1, Fo, out_size, T).permute(0, 2, 1, 3).contiguous()
    return sb_mask[:, :, :, la:]


# ------------------------------------------------------------------------------------------------ clips of different lengths
def edge_lengths(T, look_ahead, min_len, edges=(8, 32, 64, 128, 256), extra=()):
    """Clip lengths L (frames) that put L + look_ahead - the frames a clip's per-utterance reductions end at - one below, at and one
    above every edge (a multiple of a kernel's sub-tile, row tile or chunk) that fits in [min_len, T], plus min_len, T and `extra`
    (kept where they fit).  Sorted, without repeats."""
    out = {min_len, T}
    for e in edges:
        for d in (-1, 0, 1):
            out.add(e + d - look_ahead)
    out.update(extra)
    return sorted(L for L in out if min_len <= L <= T)


def garbage_tails(ts, lengths, seed):
    """Contiguous copies of [B, 1, F, T] tensors with huge values and NaN at frames >= lengths[b]."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for t in ts:
        t = t.contiguous().clone()
        for b, n in enumerate(lengths):
            if n < t.shape[-1]:
                tail = t[b, :, :, n:]
                tail.copy_(torch.randn(tail.shape, generator=g) * 1e6)
                tail[..., 0, 0] = float("nan")
        out.append(t)
    return out


def oracle_kwargs(args):
    """fsnp_torch.forward / forward_full keyword arguments of a FullSubNet+ model's arguments."""
    return dict(look_ahead=args["look_ahead"], sb_num_neighbors=args["sb_num_neighbors"], fb_num_neighbors=args["fb_num_neighbors"],
                norm_type=args["norm_type"], num_groups_in_drop_band=args["num_groups_in_drop_band"],
                channel_attention_model=args.get("channel_attention_model", "TSSE"), subband_num=args.get("subband_num", 1),
                fb_output_activate_function=args["fb_output_activate_function"],
                sb_output_activate_function=args["sb_output_activate_function"], output_size=args.get("output_size", 2))


def fullsubnet_oracle_kwargs(args):
    """fsnp_torch.forward_fullsubnet_full keyword arguments of an original FullSubNet's model arguments."""
    return {k: args[k] for k in ("look_ahead", "sb_num_neighbors", "fb_num_neighbors", "norm_type", "num_groups_in_drop_band",
                                 "fb_output_activate_function", "sb_output_activate_function")}


def oracle_rows(fn, ts, lengths):
    """Row b of each [B, ...] tensor in ts trimmed to its lengths[b] (last axis) and passed through fn, one call per distinct length
    (the rows of one length stacked: every reduction of a "full" forward is per utterance) -> list of [1, ...] results, row by row."""
    by_len = {}
    for b, n in enumerate(lengths):
        by_len.setdefault(int(n), []).append(b)
    rows = [None] * len(lengths)
    for n, bs in by_len.items():
        out = fn(*[t[bs][..., :n] for t in ts])
        for i, b in enumerate(bs):
            rows[b] = out[i:i + 1]
    return rows


def check_rows(got, want_rows, lengths, tol):
    """got [B, ..., T] (CPU); want_rows[b] = the reference's [1, ..., lengths[b]].  Per row: rel_err on the clip < tol, exactly 0 past it,
    no NaN anywhere.  Returns the per-row errors."""
    assert not torch.isnan(got).any()
    errs = []
    for b, n in enumerate(lengths):
        errs.append(rel_err(got[b:b + 1, ..., :n].numpy(), want_rows[b].numpy()))
        assert torch.count_nonzero(got[b, ..., n:]) == 0, f"row {b}: frames past its length {n} are not 0"
    assert max(errs) < tol, (max(errs), int(np.argmax(errs)), errs)
    return errs

"""CPU checks of the reference, the case table and the metric of tests/test_gpu_frontend.py.  Nothing here needs a GPU.

1. The gate split of fsnp_torch.attention (attention = x * attention_gate) returns the bits the unsplit function returned, for the four
   attention kinds, and tests/_util.py oracle_frontend is the front half of fsnp_torch.forward (subband_num > 1 included).

2. Yardstick: for every case of tests/_frontend_cases.py and its actual inputs, the float32 oracle's own error e32 on every att_* plane
   and every gate_* vector satisfies max(e32, 2**-23) <= 2e-5 / 8: the GPU test's bound min(8 * max(e32, 2**-23), 2e-5) is never the cap
   alone for a clean float32 implementation.  (The Laplace-norm cases use tests/_util.py spec_dc for that reason.)

3. Coverage: over all cases the restated launch formulas take every value csrc/frontend.hip distinguishes.

4. Would the metric fail on a subtly wrong kernel?  The faults a front-end kernel could plausibly have are emulated inside the oracle in
   float64 (fsnp_torch.attention_gate, an entry of fsnp_torch.NORMS or tests/_util.py reflect_pad_bins replaced), each on a small
   shape that has the feature.  Each must exceed 32 * max(e32, 2**-23) - four times the GPU test's margin - on at least one plane or
   gate of every utterance it touches.  Next to it stands the fault's rel_err on the final mask in float64 (the faulty front end, then
   the clean full-band stacks and tests/_util.py oracle_subband, which test_host_subband_metric.py pins to fsnp_torch.forward_full),
   normalised by the batch's maximum as the end-to-end tests do.  Measured (default | harsh weights; B = 2, T = 38 unless FAULTS says
   otherwise), and asserted by side of the end-to-end 1e-3 where the figure is more than three times away from it:
     gaussian_biased_std                  1.2e-05 | 3.2e-07   let through
     tsse_large_pool_misses_last_frame    8.0e-05 | 3.1e-04   let through
     tsse_large_mean_one_frame_too_many   1.0e-04 | 4.9e-04   let through
     cumlayer_frame20_stale_md            1.6e-03 | 9.6e-05   let through with the harsh weights
     eca_last_bin_reads_itself            3.7e-03 | 5.8e-04   let through with the harsh weights
     fc1_sums_F_minus_1_inputs            2.4e-03 | 1.6e-04   let through with the harsh weights
     cbam_max_misses_last_real_frame      6.2e-03 | 2.5e-03   seen
     subband_reflect_off_by_one           7.6e-03 | 1.6e-03   seen
     offline_count_includes_padding       7.3e-02 | 1.1e-02   seen
     cumlaplace_count_late_from_256       5.6e-04 | 8.0e-05   let through (B = 1, 257 frames)
   So the 1e-3 of the end-to-end tests lets seven of the ten through under at least one weight profile; at the stage every one of them
   is beyond 32 x the yardstick on every utterance it touches.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from oracle import fsnp_torch
from tests import _frontend_cases as fc
from tests import _util
from tests._util import FRONTEND_FLOOR, STAGE_CAPS, oracle_frontend, oracle_kwargs, oracle_subband, plane_errs

K, TOL_END_TO_END = 8, 1e-3
LA = fc.LA
torch.set_num_threads(min(16, torch.get_num_threads()))


# ------------------------------------------------------------------------------------------------ 1. the split and the pin
def _attention_before_the_split(x, p, prefix, kind):
    """fsnp_torch.attention as it stood before attention_gate was cut out of it."""
    if kind == "TSSE":
        C = x.shape[1]
        feats = []
        for nm in ("smallConv1d", "middleConv1d", "largeConv1d"):
            y = Fn.conv1d(x, p[f"{prefix}.{nm}.0.weight"], p[f"{prefix}.{nm}.0.bias"], groups=C)
            feats.append(torch.relu(y.mean(dim=2, keepdim=True)))
        feature = torch.cat(feats, dim=2)
        squeeze = Fn.linear(feature, p[f"{prefix}.feature_concate_fc.weight"], p[f"{prefix}.feature_concate_fc.bias"])[..., 0]
        h = torch.relu(Fn.linear(squeeze, p[f"{prefix}.fc1.weight"], p[f"{prefix}.fc1.bias"]))
        gate = torch.sigmoid(Fn.linear(h, p[f"{prefix}.fc2.weight"], p[f"{prefix}.fc2.bias"]))
        return x * gate.unsqueeze(2)
    if kind == "SE":
        sq = x.mean(dim=2)
        h = torch.relu(Fn.linear(sq, p[f"{prefix}.fc1.weight"], p[f"{prefix}.fc1.bias"]))
        gate = torch.sigmoid(Fn.linear(h, p[f"{prefix}.fc2.weight"], p[f"{prefix}.fc2.bias"]))
        return x * gate.unsqueeze(2)
    if kind == "CBAM":
        h = torch.relu(Fn.linear(x.mean(dim=2), p[f"{prefix}.fc1.weight"], p[f"{prefix}.fc1.bias"])) + \
            torch.relu(Fn.linear(x.max(dim=2)[0], p[f"{prefix}.fc1.weight"], p[f"{prefix}.fc1.bias"]))
        gate = torch.sigmoid(Fn.linear(h, p[f"{prefix}.fc2.weight"], p[f"{prefix}.fc2.bias"]))
        return x * gate.unsqueeze(2)
    y = x.mean(dim=2, keepdim=True)
    y = Fn.conv1d(y.transpose(-1, -2), p[f"{prefix}.conv.weight"], padding=1).transpose(-1, -2)
    return x * torch.sigmoid(y)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("kind", fc.ATTENTIONS)
def test_gate_split_returns_the_bits_of_the_unsplit_attention(kind, dtype):
    from oracle.weights import make_state_dict
    for F, T in ((33, 12), (257, 40)):
        sd = {k: v.to(dtype) for k, v in make_state_dict(3, "harsh", attention=kind, num_freqs=F).items() if k.startswith("channel_attention")}
        x = torch.randn(3, F, T, dtype=dtype, generator=torch.Generator().manual_seed(F))
        for prefix in ("channel_attention", "channel_attention_imag"):
            want = _attention_before_the_split(x, sd, prefix, kind)
            got = fsnp_torch.attention(x, sd, prefix, kind)
            gate = fsnp_torch.attention_gate(x, sd, prefix, kind)
            assert gate.shape == (3, F) and torch.equal(got, want) and torch.equal(x * gate.unsqueeze(2), want)


@pytest.mark.parametrize("over", [dict(), dict(channel_attention_model="ECA", subband_num=2), dict(channel_attention_model="ECA", subband_num=3),
                                  dict(channel_attention_model="CBAM", norm_type="cumulative_layer_norm")], ids=lambda o: "_".join(map(str, o.values())) or "default")
def test_oracle_frontend_is_the_front_half_of_the_oracle_forward(over):
    from oracle.make_golden import make_spec
    from oracle.ref_loader import DEFAULT_MODEL_ARGS
    from tests._subband_cases import plus_state_dict
    args = dict(DEFAULT_MODEL_ARGS, num_freqs=33, **over)
    sd = plus_state_dict(3, "harsh", args)
    ins = make_spec(2, 12, 17, 33)
    st = {}
    fsnp_torch.forward(sd, *ins, apply_drop_band=False, stages=st, **oracle_kwargs(args))
    got = oracle_frontend(sd, ins, args, torch.float32)
    for tag in fc.BRANCHES:
        assert torch.equal(got["att_" + tag], st["att_" + tag]), tag
    only_mag = oracle_frontend(sd, (ins[0], None, None), args, torch.float32)
    assert sorted(only_mag) == ["att_mag", "gate_mag"] and torch.equal(only_mag["att_mag"], got["att_mag"])
    sn = args["subband_num"]
    g = got["gate_mag"]
    assert g.shape == (2, 33) and all(torch.equal(g[:, k], g[:, k - k % sn]) for k in range(33))


# ------------------------------------------------------------------------------------------------ 2. the yardstick of every case
_SD, _ORACLE = {}, {}


def _state_dict(c):
    key = fc.model_key(c)
    if key not in _SD:
        _SD.clear()                                                          # (cases arrive grouped by model: keep one)
        _SD[key] = fc.case_state_dict(c)
    return _SD[key]


def _case_e32(c):
    """The case's yardstick; cases that differ only in how the clips are batched share one evaluation."""
    key = (fc.model_key(c), c["kind"], c["inputs"], c["seed"], c["T"], tuple(c["lengths"]) if c["lengths"] else c["B"], c["route"] == "complex")
    if key not in _ORACLE:
        sd, ins = _state_dict(c), fc.case_inputs(c)
        _ORACLE[key] = fc.yardstick(fc.case_oracle(c, sd, ins, torch.float64), fc.case_oracle(c, sd, ins, torch.float32))
    return _ORACLE[key]


GROUPS = sorted({(c["section"], c["kind"], c["att"], c["profile"]) for c in fc.CASES.values()})


@pytest.mark.parametrize("section,kind,att,profile", GROUPS)
def test_float32_oracle_times_the_margin_stays_under_the_cap(section, kind, att, profile):
    cases = sorted(fc.cases_of(section, kind=kind, att=att, profile=profile), key=lambda c: (str(fc.model_key(c)), c["name"]))
    assert cases
    worst = (0.0, None)
    for c in cases:
        if kind == "identity":
            continue                                                         # (bit equality with the input: no yardstick)
        for i, e in enumerate(_case_e32(c)):
            for tag, v in e.items():
                worst = max(worst, (v, f"{c['name']} clip {i} {tag}"))
                assert max(v, FRONTEND_FLOOR) <= STAGE_CAPS["att"] / K, (c["name"], i, tag, v)
    _ORACLE.clear()
    print(f"{section} {kind} {att} {profile}: worst e32 {worst[0]:.2e} ({worst[1]})")


# ------------------------------------------------------------------------------------------------ 3. coverage of the launch arithmetic
def test_cases_cross_every_edge_of_the_launch_arithmetic():
    seen = {}
    for c in fc.CASES.values():
        assert set(c["why"]) <= set(fc.case_formulas(c)), c["name"]
        assert all(fc.case_formulas(c)[k] == v for k, v in c["why"].items()), c["name"]
        for k, v in fc.case_formulas(c).items():
            seen.setdefault(k, set()).add(v)
    assert seen["ns1_capped_by_lds"] == {True, False}
    assert {"F>=1024", "Fr/16"} <= seen["ns2_decided_by"]
    assert any(fc.ns2(c["F"]) == 1 and fc.ns2_decided_by(c["F"]) == why for why in ("F>=1024", "Fr/16") for c in fc.CASES.values() if c["att"] != "ECA")
    assert all(any(fc.ns2(c["F"]) == 1 and fc.case_formulas(c).get("ns2_decided_by") == why for c in fc.CASES.values()) for why in ("F>=1024", "Fr/16"))
    assert max(seen["ns2"]) > 1
    assert 256 in seen["fsum_threads"] and 512 in seen["fsum_threads"] and any(t % 64 == 0 and 256 < t < 512 for t in seen["fsum_threads"])
    assert seen["fsum_passes"] >= {1, 2, 3}                                   # (F = 513 / 515: two passes; F = 1025: three)
    assert seen["fsum_rows"] == {4, 8, 16, 32}
    assert seen["scan_chunk"] == {1, 2, 3}
    assert seen["lds_optin"] == {True, False}
    assert {fc.gate_lds_bytes(440), fc.gate_lds_bytes(441)} == {65120, 65712} <= seen["lds_bytes"]
    assert {(True,), (False,), (False, True)} <= seen["edge_overlap"]
    assert seen["clip_of_kmax_frames"] == {True, False}
    assert seen["conv_with_k1"] == {True, False}
    assert seen["f_fast"] == {True, False}
    assert seen["subband_whole_group"] == {True, False} and seen["subband_pad"] == {1, 2, 3}
    assert seen["gate_passes"] == {1, 2}
    # ... and per kernel: f_fast both ways on the real and on the complex repack, the ragged fsum rows under a cumulative norm
    fwd = [c for c in fc.CASES.values() if c["kind"] == "forward"]
    assert {c["route"] for c in fwd} == {"f", "t", "complex"}
    assert {fc.fsum_rows(c["B"]) for c in fwd if c["lengths"] and c["norm"] in fc.CUMULATIVE} == {4, 8, 16, 32}
    assert any(c["att"] == "CBAM" and c["lengths"] for c in fwd)
    # the restated reflection is torch's (fullsubnet_plus.py:148)
    x = torch.arange(7.0).reshape(1, 1, 7, 1)
    assert _util.reflect_pad_bins(x, 3).flatten().tolist() == [float(fc.reflected_row(7, r)) for r in range(10)]


# ------------------------------------------------------------------------------------------------ 4. emulated faults
def faulty_gate(fault):
    """A replacement of fsnp_torch.attention_gate (same operations in the same order) with one emulated fault, or none."""
    def gate(x, p, prefix, kind):
        T = x.shape[2]
        if kind == "TSSE":
            C = x.shape[1]
            feats = []
            for nm in ("smallConv1d", "middleConv1d", "largeConv1d"):
                w, b = p[f"{prefix}.{nm}.0.weight"], p[f"{prefix}.{nm}.0.bias"]
                if nm == "largeConv1d" and fault == "tsse_large_pool_misses_last_frame":
                    x0 = x.clone()
                    x0[:, :, T - 1] = 0                                       # the last tap's window sum stops one frame early
                    m = Fn.conv1d(x0, w, b, groups=C).mean(dim=2, keepdim=True)
                elif nm == "largeConv1d" and fault == "tsse_large_mean_one_frame_too_many":
                    y = Fn.conv1d(x, w, None, groups=C)
                    m = y.sum(dim=2, keepdim=True) / (y.shape[2] + 1) + b[None, :, None]
                else:
                    m = Fn.conv1d(x, w, b, groups=C).mean(dim=2, keepdim=True)
                feats.append(torch.relu(m))
            feature = torch.cat(feats, dim=2)
            squeeze = Fn.linear(feature, p[f"{prefix}.feature_concate_fc.weight"], p[f"{prefix}.feature_concate_fc.bias"])[..., 0]
            h = torch.relu(Fn.linear(squeeze, p[f"{prefix}.fc1.weight"], p[f"{prefix}.fc1.bias"]))
            return torch.sigmoid(Fn.linear(h, p[f"{prefix}.fc2.weight"], p[f"{prefix}.fc2.bias"]))
        if kind in ("SE", "CBAM"):
            w1, b1 = p[f"{prefix}.fc1.weight"], p[f"{prefix}.fc1.bias"]

            def fc1(v):
                if fault == "fc1_sums_F_minus_1_inputs":
                    return torch.relu(Fn.linear(v[:, :-1], w1[:, :-1], b1))
                return torch.relu(Fn.linear(v, w1, b1))
            h = fc1(x.mean(dim=2))
            if kind == "CBAM":
                xm = x
                if fault == "cbam_max_misses_last_real_frame":
                    xm = torch.cat([x[:, :, :T - LA - 1], x[:, :, T - LA:]], dim=2)
                h = h + fc1(xm.max(dim=2)[0])
            return torch.sigmoid(Fn.linear(h, p[f"{prefix}.fc2.weight"], p[f"{prefix}.fc2.bias"]))
        y = x.mean(dim=2, keepdim=True)
        if fault == "eca_last_bin_reads_itself":
            yp = torch.cat([torch.zeros_like(y[:, :1]), y, y[:, -1:]], dim=1)
            y = Fn.conv1d(yp.transpose(-1, -2), p[f"{prefix}.conv.weight"]).transpose(-1, -2)
        else:
            y = Fn.conv1d(y.transpose(-1, -2), p[f"{prefix}.conv.weight"], padding=1).transpose(-1, -2)
        return torch.sigmoid(y)[..., 0]
    return gate


def _gaussian_biased_std(x):
    mu = torch.mean(x, dim=(1, 2, 3), keepdim=True)
    return (x - mu) / (torch.std(x, dim=(1, 2, 3), keepdim=True, unbiased=False) + 1e-5)


def _cumlayer_frame20_stale(x):
    y, count = fsnp_torch._cum_stats(x)
    cum = torch.cumsum(y.sum(dim=1), dim=-1)
    cum_pow = torch.cumsum(torch.square(y).sum(dim=1), dim=-1)
    mean = cum / count
    std = torch.sqrt((cum_pow - 2 * mean * cum) / count + mean.pow(2) + fsnp_torch.EPSILON)
    mean[:, 20], std[:, 20] = mean[:, 19].clone(), std[:, 19].clone()
    return ((y - mean.unsqueeze(1)) / std.unsqueeze(1)).reshape(x.shape)


def _cumlaplace_count_late_from_256(x):
    y, count = fsnp_torch._cum_stats(x)
    count = count.clone()
    count[:, 256:] -= x.shape[2]
    mean = (torch.cumsum(y.sum(dim=1), dim=-1) / count).unsqueeze(1)
    return (y / (mean + fsnp_torch.EPSILON)).reshape(x.shape)


def _offline_laplace_counting_the_buffer(buffer_frames):
    def norm(x):
        return x / (x.sum(dim=(1, 2, 3), keepdim=True) / (x.shape[2] * buffer_frames) + 1e-5)
    return norm


def _reflect_off_by_one(x, pad):
    """row F + k = row F - 1 - k (2 F - 1 - row) instead of row F - 2 - k (2 (F - 1) - row)."""
    return torch.cat([x, x.flip(2)[:, :, :pad]], dim=2)


# name -> (what to replace, case arguments, utterances touched, branches touched, does the end-to-end 1e-3 let it through with the default /
# the harsh weights - None where the measured figure is within three times of 1e-3)
FAULTS = {
    "gaussian_biased_std": (("norm", "offline_gaussian_norm", _gaussian_biased_std), dict(norm="offline_gaussian_norm"), (0, 1), fc.BRANCHES, (True, True)),
    "tsse_large_pool_misses_last_frame": (("gate",), dict(norm="cumulative_layer_norm"), (0, 1), fc.BRANCHES, (True, True)),
    "cumlayer_frame20_stale_md": (("norm", "cumulative_layer_norm", _cumlayer_frame20_stale), dict(norm="cumulative_layer_norm"), (0, 1), fc.BRANCHES, (None, True)),
    "tsse_large_mean_one_frame_too_many": (("gate",), dict(norm="cumulative_layer_norm"), (0, 1), fc.BRANCHES, (True, None)),
    "eca_last_bin_reads_itself": (("gate",), dict(att="ECA", norm="offline_gaussian_norm"), (0, 1), fc.BRANCHES, (False, None)),
    "cbam_max_misses_last_real_frame": (("gate",), dict(att="CBAM", norm="cumulative_layer_norm"), (0, 1), fc.BRANCHES, (False, None)),
    "subband_reflect_off_by_one": (("reflect",), dict(att="ECA", sn=2, norm="offline_gaussian_norm"), (0, 1), ("mag",), (False, None)),
    "cumlaplace_count_late_from_256": (("norm", "cumulative_laplace_norm", _cumlaplace_count_late_from_256),
                                       dict(norm="cumulative_laplace_norm", B=1, T=257), (0,), fc.BRANCHES, (None, True)),
    "offline_count_includes_padding": (("norm", "offline_laplace_norm", _offline_laplace_counting_the_buffer(38 + LA)),
                                       dict(norm="offline_laplace_norm", att="SE", lengths=[29, 38]), (0,), fc.BRANCHES, (False, False)),
    "fc1_sums_F_minus_1_inputs": (("gate",), dict(att="SE", norm="offline_gaussian_norm"), (0, 1), fc.BRANCHES, (None, True)),
}


def test_restated_gate_without_a_fault_is_the_oracles_gate():
    from oracle.weights import make_state_dict
    x = torch.randn(2, 257, 40, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    for kind in fc.ATTENTIONS:
        p = {k: v.double() for k, v in make_state_dict(21, "harsh", attention=kind).items() if k.startswith("channel_attention")}
        assert torch.equal(faulty_gate(None)(x, p, "channel_attention_real", kind), fsnp_torch.attention_gate(x, p, "channel_attention_real", kind))


def _mask(c, sd, rows):
    """The final mask in float64 of each clip alone, from its att_* planes: the clean full-band stacks, then oracle_subband."""
    args = fc.model_args(c)
    p = {k: v.double() for k, v in sd.items() if k.startswith("fb_model")}
    out = []
    for r in rows:
        st = {"att_mag": torch.from_numpy(r["att_mag"])[None]}
        for b in fc.BRANCHES:
            st["fb_" + b] = fsnp_torch.fb_sequence_model(torch.from_numpy(r["att_" + b])[None], p, "fb_model" + ("" if b == "mag" else "_" + b),
                                                         args["fb_output_activate_function"])
        out.append(oracle_subband(sd, st, args, torch.float64).numpy())
    return out


@pytest.mark.parametrize("profile", fc.PROFILES)
@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_emulated_frontend_fault_is_caught_at_the_stage(fault, profile, monkeypatch):
    what, over, utts, branches, passes_end_to_end = FAULTS[fault]
    c = fc.make_case("X_" + fault, {}, **{"profile": profile, "T": 40 - LA, "seed": 38, **over})
    sd, ins = fc.case_state_dict(c), fc.case_inputs(c)
    clean = fc.case_oracle(c, sd, ins, torch.float64)
    e32 = fc.yardstick(clean, fc.case_oracle(c, sd, ins, torch.float32))
    if what[0] == "gate":
        monkeypatch.setattr(fsnp_torch, "attention_gate", faulty_gate(fault))
    elif what[0] == "norm":
        monkeypatch.setitem(fsnp_torch.NORMS, what[1], what[2])
    else:
        monkeypatch.setattr(_util, "reflect_pad_bins", _reflect_off_by_one)
    bad = fc.case_oracle(c, sd, ins, torch.float64)
    monkeypatch.undo()
    for i in range(len(clean)):
        ratios = {t: plane_errs(bad[i][t][None], clean[i][t][None])[0][0] / max(e32[i][t], FRONTEND_FLOOR) for t in fc.TAGS}
        touched = i in utts
        print(f"{fault} {profile} clip {i}: err / max(e32, 2**-23) = " + ", ".join(f"{t} {v:.1f}" for t, v in ratios.items()))
        if touched:
            assert max(ratios.values()) > 32, (fault, profile, i, ratios)
            assert all(max(ratios["att_" + b], ratios["gate_" + b]) > 0 for b in branches), (fault, profile, i, ratios)
        else:
            assert max(ratios.values()) < 1e-6, (fault, profile, i, ratios)          # (another summation order in float64 at most)
        assert all(ratios[g + "_" + b] == 0.0 for g in ("att", "gate") for b in fc.BRANCHES if b not in branches), (fault, profile, i, ratios)
    good_mask, bad_mask = _mask(c, sd, [clean[i] for i in utts]), _mask(c, sd, [bad[i] for i in utts])
    scale = max(np.abs(m).max() for m in good_mask)
    end_to_end = max(np.abs(b - g).max() for b, g in zip(bad_mask, good_mask)) / scale
    print(f"{fault} {profile}: final mask rel_err {end_to_end:.2e} ({'passes' if end_to_end < TOL_END_TO_END else 'fails'} the end-to-end {TOL_END_TO_END})")
    side = passes_end_to_end[fc.PROFILES.index(profile)]
    if side is not None:
        assert (end_to_end < TOL_END_TO_END) == side, (fault, profile, end_to_end)

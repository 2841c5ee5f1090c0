"""GPU tests of the front end (csrc/frontend.hip: repack -> one of four norms -> one of four channel attentions, subband_num > 1, the
gate and apply kernels) at the stage itself, per norm, attention kind and launch edge - not through the final mask, which the sub-band
model shields: the faults tests/test_host_frontend_metric.py emulates move the mask by as little as 1e-5 of a batch's maximum.

A case (tests/_frontend_cases.py) is a whole forward in batch_mode "full" - through forward, forward with lengths= (garbage_tails
inputs: NaN and 1e6 past each clip) or forward_complex - or one call of model.channel_attention{,_real,_imag}; then check_errors() and
read_stage("att_*" | "gate_*").

Reference: tests/_util.py oracle_frontend in float64 (the stage alone: fsnp_torch.attention_gate and the multiply); for ragged batches
the oracle of each clip alone.  Only a clip's own lengths[b] + look_ahead frames are compared, and they must be finite.

Metric and bound: tests/_util.py plane_errs over ONE utterance's plane of ONE branch; a gate is a plane of one frame.  The yardstick e32
is the same metric of the float32 oracle against the float64 oracle on that plane: nothing of the code under test enters it.  Asserted
plane by plane: err <= min(8 * max(e32, 2**-23), 2e-5) (tests/_util.py frontend_bound: the margin, the floor and STAGE_CAPS["att"] the
suite already uses at this stage).  Every case's worst err / max(e32, 2**-23) per group ("att", "gate") goes to frontend_report.json
next to stage_report.json, with the plane, clip, length and (bin, frame).

Paths: the front end has no debug switch; which launch arithmetic a call meets is a function of its shape.  Every case recomputes the
restated formulas (tests/_frontend_cases.py formulas) from the model it built and the tensors it passed and asserts they are what the
table names, so a case cannot pass on a path it did not take.

The routes of section D (F-fastest views, frames-fastest tensors, forward_complex) are each held to the bound; bit equality between
them is NOT asserted (the offline statistics are fp64 atomics in no fixed order); their mutual rel_err goes to the report.

Measured on an MI355X, worst err / max(e32, 2**-23) of a case, over the 605 cases (frontend_report.json):
  per norm        att_*: offline_laplace 0.84 ... 1.79, offline_gaussian 0.80 ... 1.65, cumulative_laplace 0.53 ... 1.81,
                  cumulative_layer 0.69 ... 1.56; gate_*: 0.76 ... 1.25, 0.68 ... 1.30, 0.54 ... 1.46, 0.71 ... 1.45
  per attention   att_*: TSSE 0.63 ... 1.81, SE 0.67 ... 1.55, ECA 0.63 ... 1.56, CBAM 0.53 ... 1.81;
                  gate_*: TSSE 0.68 ... 1.38, SE 0.68 ... 1.14, ECA 0.70 ... 0.95, CBAM 0.54 ... 1.46
  the attention stage alone (no gate to read) 0.59 ... 1.81.
Frames-fastest and F-fastest inputs gave the same bits; forward_complex differed from them by 1.2e-7 ... 2.7e-7 (its magnitude is
hypotf of the float32 parts).  No case needs more than a quarter of the margin and no kernel was changed.
"""
import os

import numpy as np
import pytest
import torch

from fullsubnet_plus_amd import FullSubNet, FullSubNet_Plus
from tests import _frontend_cases as fc
from tests._util import FRONTEND_FLOOR, frontend_bound, garbage_tails, plane_errs, rel_err

pytestmark = pytest.mark.gpu
LA = fc.LA
REPORT = {}

torch.set_num_threads(min(16, os.cpu_count() or 1))


def _record(name, entry):
    """frontend_report.json, written the way (and where) tests/test_gpu_stages.py writes stage_report.json."""
    from tests.test_gpu_parity import _record as record
    record(name, _report=REPORT, _file="frontend_report.json", **entry)


def _strided_cuda(t):
    """To the GPU with the strides kept (make_spec's views are not dense: .cuda() would compact them)."""
    g = torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device="cuda")
    g.copy_(t)
    return g


def _f_fastest(t):
    """[..., F, T] -> the same values on the GPU with bins fastest in memory ([...][T][F] order, like torch.stft's output)."""
    return _strided_cuda(t.transpose(-1, -2).contiguous().transpose(-1, -2))


def _model(c):
    args, sd = fc.model_args(c), fc.case_state_dict(c)
    m = (FullSubNet if c["kind"] == "identity" else FullSubNet_Plus)(**args)
    m.load_state_dict(sd, strict=True)
    m = m.to("cuda").eval()
    m.batch_mode = "full"
    return m, sd


def _routed(ins, route):
    """The same values in the route's memory layout, on the GPU -> (tensors, stride of a bin, stride of a frame)."""
    if route == "t":
        ts = [t.contiguous().cuda() for t in ins]
        assert all(t.is_contiguous() for t in ts)
    else:
        ts = [_strided_cuda(t) for t in ins]
    return ts, ts[0].stride(2), ts[0].stride(3)


def _forward_rows(m, c, ins):
    """The case's forwards -> (rows[i] = {tag: [F, T'_i] or [F, 1]}, what the launches saw: F, B, buffer T', clip T', f_fast)."""
    B, T, F = c["B"], c["T"], c["F"]
    lengths = c["lengths"]
    n = B if lengths is None else len(lengths)
    rows, seen = [None] * n, {"F": m.num_freqs, "B": set(), "buffer": set(), "clips": [], "f_fast": set()}
    for k in range(0, n, B):
        idx = [(k + i) % n for i in range(B)]
        sub = [t[idx] for t in ins]
        if lengths is None:
            lens = [T] * B
            if c["route"] == "complex":
                X = _f_fastest(torch.complex(sub[1], sub[2])[:, 0])               # [B, F, T] complex64 in torch.stft's memory order
                sf, st = X.stride(1), X.stride(2)
                m.forward_complex(X)
            else:
                ts, sf, st = _routed(sub, c["route"])
                m(*ts)
        else:
            lens = [lengths[i] for i in idx]
            ts = [_f_fastest(t) for t in garbage_tails(sub, lens, 9 + k)]        # (garbage_tails makes frames-fastest copies)
            sf, st = ts[0].stride(2), ts[0].stride(3)
            m(*ts, lengths=lens)
        m.check_errors()
        seen["B"].add(len(idx)); seen["buffer"].add(sub[0].shape[-1] + LA); seen["f_fast"].add(fc.f_fast(sf, st))
        st_ = {t: m.read_stage(t, B, T) for t in fc.TAGS}
        for j, i in enumerate(idx):
            if rows[i] is None:
                seen["clips"].append(lens[j] + LA)
                rows[i] = {t: (st_[t][j, :lens[j] + LA].T if t.startswith("att_") else st_[t][j][:, None]).numpy().copy() for t in fc.TAGS}
    return rows, seen


def _stage_rows(m, c, ins):
    rows = [{} for _ in range(c["B"])]
    for b, x in zip(fc.BRANCHES, ins):
        layer = getattr(m, "channel_attention" + ("" if b == "mag" else "_" + b))
        got = layer(x.cuda())
        m.check_errors()
        assert got.shape == x.shape
        got = got.cpu().numpy()
        for i in range(c["B"]):
            rows[i]["att_" + b] = got[i]
    seen = {"F": m.num_freqs, "B": {ins[0].shape[0]}, "buffer": {ins[0].shape[2]}, "clips": [ins[0].shape[2]] * c["B"],
            "f_fast": {fc.f_fast(ins[0].stride(1), ins[0].stride(2))}}
    return rows, seen


def _assert_path(c, m, seen):
    """The formulas of what was actually launched are the case's, and hold what the case is there for."""
    (B,), (buffer,), (ff,) = seen["B"], seen["buffer"], seen["f_fast"]
    stage = c["kind"] == "stage"
    ran = fc.formulas(F=seen["F"], B=B, frames={"buffer": buffer, "clips": tuple(sorted(seen["clips"]))}, norm=getattr(m, "norm_type", c["norm"]),
                      att=None if c["kind"] == "identity" else m.channel_attention_model, kersize=tuple(getattr(m, "kersize", c["kersize"])),
                      sn=getattr(m, "subband_num", 1), f_is_fast=ff, stage=stage)
    want = fc.case_formulas(c)
    assert ran == want, (c["name"], ran, want)
    assert all(ran[k] == v for k, v in c["why"].items()), (c["name"], c["why"], ran)
    return ran


def run_case(c, m, sd):
    """One case against the float64 oracle, plane by plane; -> its rows (for the callers that compare cases with each other)."""
    ins = fc.case_inputs(c)
    want = fc.case_oracle(c, sd, ins, torch.float64)
    e32 = fc.yardstick(want, fc.case_oracle(c, sd, ins, torch.float32))
    rows, seen = (_stage_rows if c["kind"] == "stage" else _forward_rows)(m, c, ins)
    ran = _assert_path(c, m, seen)
    lengths = c["lengths"] or [c["T"]] * c["B"]
    worst, failures = {g: {"ratio": 0.0} for g in sorted({t[:t.index("_")] for t in rows[0]})}, []
    for i, (g_i, w_i) in enumerate(zip(rows, want)):
        for tag in g_i:
            (err,), (where,) = plane_errs(g_i[tag][None], w_i[tag][None])
            grp, bound = tag[:tag.index("_")], frontend_bound(e32[i][tag])
            ratio = err / max(e32[i][tag], FRONTEND_FLOOR)
            if ratio >= worst[grp]["ratio"]:
                worst[grp] = {"ratio": ratio, "err": err, "e32": e32[i][tag], "tag": tag, "clip": i, "length": lengths[i], "bin_frame": list(where)}
            if not err <= bound:
                failures.append((tag, i, lengths[i], where, err, bound, ratio))
    print(f"{c['name']}: " + ", ".join(f"{g} worst {w['ratio']:.2f} x e32" + (f" ({w['err']:.2e} on {w['tag']} of clip {w['clip']}, length "
                                       f"{w['length']}, at {w['bin_frame']})") for g, w in worst.items()))
    _record(c["name"], {"worst": worst, "formulas": {k: (list(v) if isinstance(v, tuple) else v) for k, v in ran.items()},
                        "lengths": c["lengths"], "norm": c["norm"] if c["kind"] == "forward" else None, "attention": c["att"]})
    assert not failures, (c["name"], "(tag, clip, length, (bin, frame), err, bound, err / max(e32, 2**-23))", failures[:12])
    return rows


def _run_group(cases):
    """Cases grouped by model: one model per key, dropped before the next is built."""
    by_key = {}
    for c in cases:
        by_key.setdefault(fc.model_key(c), []).append(c)
    assert by_key
    out = {}
    for group in by_key.values():
        m, sd = _model(group[0])
        for c in group:
            out[c["name"]] = run_case(c, m, sd)
        del m
    return out


# ------------------------------------------------------------------------------------------------ A. whole forwards at F = 257
@pytest.mark.parametrize("profile", fc.PROFILES)
@pytest.mark.parametrize("norm", fc.NORMS)
@pytest.mark.parametrize("att", fc.ATTENTIONS)
def test_norm_x_attention_uniform_and_scan_chunks(att, norm, profile):
    """B = 3 at T' = 31 / 32 / 33 (the repack tile edge); B = 1 at T' = 255 / 256 / 257 / 513 (fe_scan_kernel's chunk 1 -> 2 -> 3)."""
    cases = [c for c in fc.cases_of("A", att=att, norm=norm, profile=profile) if c["lengths"] is None]
    assert len(cases) == (7 if norm in fc.SCAN_NORMS else 3)
    _run_group(cases)


@pytest.mark.parametrize("profile", fc.PROFILES)
@pytest.mark.parametrize("norm", fc.NORMS)
@pytest.mark.parametrize("att", fc.ATTENTIONS)
def test_norm_x_attention_ragged_pool(att, norm, profile):
    """The 140-frame pool at B = 1 / 2 / 4 / 8: fe_fsum_kernel at 4 / 8 / 16 / 32 frames per workgroup with clips ending inside a
    workgroup's frames; the offline counts, the pooled means and CBAM's max must skip the NaN / 1e6 tails."""
    cases = [c for c in fc.cases_of("A", att=att, norm=norm, profile=profile) if c["lengths"] is not None]
    assert [c["B"] for c in cases] == [1, 2, 4, 8]
    _run_group(cases)


# ------------------------------------------------------------------------------------------------ B. TSSE kernel sizes
@pytest.mark.parametrize("profile", fc.PROFILES)
@pytest.mark.parametrize("norm", fc.B_NORMS)
def test_tsse_kernel_sizes(norm, profile):
    cases = fc.cases_of("B", norm=norm, profile=profile)
    assert len(cases) >= 6
    _run_group(cases)


# ------------------------------------------------------------------------------------------------ C. subband_num > 1
@pytest.mark.parametrize("profile", fc.PROFILES)
@pytest.mark.parametrize("norm", fc.C_NORMS)
def test_eca_subband_groups(norm, profile):
    """gate_mag is constant over each group of subband_num bins and equal to the oracle's channel gate (run_case: the oracle repeats
    the channel gate over its bins); gate_real / gate_imag follow the plain ECA."""
    cases = fc.cases_of("C", norm=norm, profile=profile)
    assert len(cases) == 4
    for name, rows in _run_group(cases).items():
        sn, F = fc.CASES[name]["sn"], fc.CASES[name]["F"]
        for r in rows:
            g = r["gate_mag"][:, 0]
            assert all(np.all(g[k:k + sn] == g[k]) for k in range(0, F, sn)), (name, "gate_mag varies inside a group")


# ------------------------------------------------------------------------------------------------ D. input routes
@pytest.mark.parametrize("profile", fc.PROFILES)
@pytest.mark.parametrize("norm", fc.D_NORMS)
def test_input_routes(norm, profile):
    cases = [c for c in fc.cases_of("D", norm=norm, profile=profile) if c["kind"] == "forward"]
    assert len(cases) == 6
    out = _run_group(cases)
    for tp in (33, 129):
        r = {route: out[f"D_route_{route}_{fc._short(norm)}_{profile}_Tp{tp}"] for route in ("f", "t", "complex")}
        mutual = {f"{a}_vs_{b}": max(rel_err(x[t], y[t]) for x, y in zip(r[a], r[b]) for t in fc.TAGS) for a, b in (("f", "t"), ("f", "complex"))}
        _record(f"D_routes_mutual_{fc._short(norm)}_{profile}_Tp{tp}", mutual)


@pytest.mark.parametrize("route", ["f", "t"])
def test_fullsubnet_att_mag_is_the_padded_magnitude_on_either_layout(route):
    for c in fc.cases_of("D", kind="identity", route=route):
        m, _ = _model(c)
        mag = fc.case_inputs(c)[0]
        (x,), sf, st = _routed([mag], route)
        m(x)
        m.check_errors()
        assert fc.f_fast(sf, st) == c["why"]["f_fast"] and m.num_freqs == c["F"]
        att = m.read_stage("att_mag", c["B"], c["T"]).permute(0, 2, 1)
        assert torch.equal(att[:, :, :c["T"]], mag[:, 0]) and torch.count_nonzero(att[:, :, c["T"]:]) == 0, c["name"]
        _record(c["name"], {"bit_equal": True, "f_fast": c["why"]["f_fast"]})


# ------------------------------------------------------------------------------------------------ E. bin counts
@pytest.mark.parametrize("profile", fc.PROFILES)
@pytest.mark.parametrize("F", [161, 441, 515])
def test_forward_at_other_bin_counts(F, profile):
    cases = fc.cases_of("E", kind="forward", F=F, profile=profile)
    assert len(cases) == 4
    _run_group(cases)


@pytest.mark.parametrize("profile", fc.PROFILES)
@pytest.mark.parametrize("F", [33, 440, 441, 513, 515, 1025])
def test_attention_stage_alone_at_bin_counts(F, profile):
    cases = fc.cases_of("E", kind="stage", F=F, profile=profile)
    assert len(cases) == 16
    _run_group(cases)

"""CPU check of the stage-level metric and bound of tests/test_gpu_fullband_lstm.py: would they fail on a subtly wrong full-band LSTM
stage of the original FullSubNet (norm -> two-layer LSTM -> Linear -> activation)?

The faults the K-split kernel (csrc/lstm_coop.hip), the matrix-vector kernel (csrc/lstm_fbv.hip), launch_frontend_mag and
launch_linear_act could plausibly have are emulated in a plain step loop written here (which is fsnp_torch.lstm2_fc when no fault is set:
asserted), evaluated in float32 at B = 2, T = 20 with both weight profiles and compared with the float64 oracle under plane_errs:

  a k tail ignored (input bin 256 = 64 * 4 + 0 never multiplied), a stale image of the three-image h rotation (layer 1 reads h1 of step
  t - 2 at one step), a hand-off of h0 in bf16, the last hidden unit missing from the Linear's k range, the Linear's N tail (output bin
  256) never written, a per-frame statistic counted over one frame too many, a clip normalised with its neighbour's statistics.

Each must put EVERY plane at least 2 x beyond the bound the GPU test asserts (tests/_util.py fullband_lstm_bound), while the clean
float32 oracle stays below CAP / 8.  The end-to-end assertion the suite had for these shapes (the final mask within 1e-3 of the batch's
maximum) is kept on record next to it: the sub-band model attenuates all of the LSTM faults but one below it.

Measured (fb_mag plane error, worst and best plane; mask error), default / harsh weights:
  clean float32 oracle                      5.1e-7 ... 5.9e-7 / 2.0e-7 ... 2.1e-7     5.9e-7 / 3.3e-7
  input bin 256 never multiplied            3.4e-2 ... 1.1e-1 / 1.2e-3 ... 3.3e-3     7.0e-4 / 2.8e-5
  layer 1 reads h1 of step t - 2 once       1.5e-2 ... 1.6e-2 / 4.2e-4 ... 7.0e-4     6.2e-5 / 1.7e-6
  h0 handed over in bf16                    7.6e-4 ... 1.2e-3 / 7.7e-5 ... 8.4e-5     6.2e-6 / 5.3e-7
  hidden unit 511 missing from the Linear   1.0e-2 ... 1.1e-2 / 4.5e-3 ... 4.5e-3     8.9e-5 / 4.0e-5
  output bin 256 zeroed                     0.34 ... 0.42 / 7.6e-2 ... 7.6e-2         2.8e-3 / 7.1e-4
  per-frame count one frame too many        1.5e-1 ... 1.6e-1 / 9.8e-3 ... 1.6e-2     (cumulative_laplace_norm)
  normalised with the neighbour's mean      4.5e-2 ... 4.9e-2 / 3.7e-3 ... 4.2e-3
The closest any fault comes is the bf16 hand-off with "harsh" weights: 7.7e-5, 3.9 x CAP = 2e-5 and 45 x the bound of its plane
(8 x e32 = 1.7e-6).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from oracle import fsnp_torch
from oracle.make_golden import make_spec
from oracle.ref_loader import FULLSUBNET_MODEL_ARGS
from oracle.weights import make_state_dict_fullsubnet
from tests._util import FB_LSTM_CAP, fullband_lstm_bound, oracle_fullband_fullsubnet, oracle_subband, plane_errs, rel_err

B, T = 2, 20
LA = FULLSUBNET_MODEL_ARGS["look_ahead"]
STALE_STEP = 11
MASK_TOL = 1e-3              # what tests/test_gpu_fullsubnet.py asserts of the final mask, of the batch's maximum
# fault -> the weight profiles with which the end-to-end 1e-3 does NOT see it (the table of the module docstring)
LSTM_FAULTS = {"input_bin256_never_multiplied": ("default", "harsh"),
               "layer1_reads_h1_of_step_t_minus_2_once": ("default", "harsh"),
               "h0_handed_over_in_bf16": ("default", "harsh"),
               "hidden_unit_511_missing_from_linear": ("default", "harsh"),
               "output_bin256_zeroed": ("harsh",)}
NORM_FAULTS = ("frame_statistics_count_one_frame_too_many", "clip_normalised_with_neighbours_statistics")
CUM_ARGS = dict(FULLSUBNET_MODEL_ARGS, norm_type="cumulative_laplace_norm")


def faulty_norm(x, norm_type, fault):
    """fsnp_torch.NORMS[norm_type] of the padded x [B, 1, F, T'] with one emulated fault of the statistics, or none."""
    if fault == "clip_normalised_with_neighbours_statistics":
        assert norm_type == "offline_laplace_norm"
        return x / (torch.mean(x, dim=(1, 2, 3), keepdim=True).roll(1, 0) + 1e-5)
    if fault == "frame_statistics_count_one_frame_too_many":
        assert norm_type == "cumulative_laplace_norm"
        y, count = fsnp_torch._cum_stats(x)
        mean = (torch.cumsum(y.sum(dim=1), dim=-1) / (count + x.shape[2])).unsqueeze(1)
        return (y / (mean + fsnp_torch.EPSILON)).reshape(x.shape)
    return fsnp_torch.NORMS[norm_type](x)


def lstm2_fc_steps(x, p, prefix, activation, fault=None):
    """fsnp_torch.lstm2_fc for an LSTM, as a plain step loop (gate order i, f, g, o of torch.nn.LSTM), with one emulated fault, or none.
    x [N, in, T] -> [N, out, T]."""
    w = {(nm, layer): p[f"{prefix}.sequence_model.{nm}_l{layer}"] for nm in ("weight_ih", "weight_hh", "bias_ih", "bias_hh") for layer in (0, 1)}
    N, _, steps = x.shape
    H = w["weight_hh", 0].shape[1]

    def cell(layer, inp, h, c):
        g = inp @ w["weight_ih", layer].T + w["bias_ih", layer] + h @ w["weight_hh", layer].T + w["bias_hh", layer]
        i, f, gg, o = g.chunk(4, dim=1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
        return torch.sigmoid(o) * torch.tanh(c), c

    h0, c0, h1, c1, h1_before = (torch.zeros(N, H, dtype=x.dtype) for _ in range(5))
    seq = []
    for t in range(steps):
        xt = x[:, :, t]
        if fault == "input_bin256_never_multiplied":
            xt = xt.clone()
            xt[:, 256] = 0
        h0, c0 = cell(0, xt, h0, c0)
        if fault == "h0_handed_over_in_bf16":                # the exchange image both of its readers (layer 1 now, layer 0 next step) see
            h0 = h0.bfloat16().to(x.dtype)
        stale = fault == "layer1_reads_h1_of_step_t_minus_2_once" and t == STALE_STEP
        new_h1, c1 = cell(1, h0, h1_before if stale else h1, c1)
        h1_before, h1 = h1, new_h1
        seq.append(h1)
    wl = p[prefix + ".fc_output_layer.weight"]
    if fault == "hidden_unit_511_missing_from_linear":
        wl = wl.clone()
        wl[:, 511] = 0
    o = fsnp_torch._activation(Fn.linear(torch.stack(seq, dim=1), wl, p[prefix + ".fc_output_layer.bias"]), activation).permute(0, 2, 1).contiguous()
    if fault == "output_bin256_zeroed":
        o[:, 256] = 0
    return o


@torch.no_grad()
def faulty_fullband(sd, mag, args, dtype, fault=None):
    """tests/_util.py oracle_fullband_fullsubnet with the step loop above and one emulated fault, or none -> fb_mag [B, F, T + look_ahead]."""
    p = {k: v.to(dtype) for k, v in sd.items() if k.startswith("fb_model.")}
    x = Fn.pad(mag.to(dtype), [0, args["look_ahead"]])
    xn = faulty_norm(x, args["norm_type"], fault).reshape(x.shape[0], x.shape[2], x.shape[3])
    return lstm2_fc_steps(xn, p, "fb_model", args["fb_output_activate_function"], fault)


def _mask(sd, mag, fb_mag, dtype):
    """The final mask behind a given fb_mag plane, [B, 2, F, T]."""
    stages = {"att_mag": Fn.pad(mag[:, 0], [0, LA]), "fb_mag": fb_mag}
    return oracle_subband(sd, stages, FULLSUBNET_MODEL_ARGS, dtype).numpy()


@pytest.fixture(scope="module", params=["default", "harsh"])
def clean(request):
    """(profile, sd, mag, {norm_type: (fb_mag in float64, fb_mag in float32, e32 per plane)}, the clean mask in float64)."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sd = make_state_dict_fullsubnet(21, request.param)
    mag = make_spec(B, T, 4020)[0]
    ref = {}
    for args in (FULLSUBNET_MODEL_ARGS, CUM_ARGS):
        s64, s32 = (oracle_fullband_fullsubnet(sd, mag, args, dt)["fb_mag"] for dt in (torch.float64, torch.float32))
        ref[args["norm_type"]] = (s64, s32, plane_errs(s32.numpy(), s64.numpy())[0])
    return request.param, sd, mag, ref, _mask(sd, mag, ref["offline_laplace_norm"][0], torch.float64)


def test_step_loop_without_a_fault_is_the_oracles_lstm2_fc(clean):
    _, sd, mag, ref, _ = clean
    for args in (FULLSUBNET_MODEL_ARGS, CUM_ARGS):
        got = faulty_fullband(sd, mag, args, torch.float64).numpy()
        want = ref[args["norm_type"]][0].numpy()
        assert got.shape == want.shape == (B, 257, T + LA)
        assert max(plane_errs(got, want)[0]) < 1e-13, plane_errs(got, want)       # float64 rounding in another summation order
    got32 = faulty_fullband(sd, mag, FULLSUBNET_MODEL_ARGS, torch.float32).numpy()
    assert max(plane_errs(got32, ref["offline_laplace_norm"][0].numpy())[0]) < FB_LSTM_CAP / 8


def test_clean_float32_oracle_is_inside_the_cap(clean):
    """The yardstick alone, times the margin, fits under the cap; and the floor 2**-23 does not hide it."""
    profile, sd, mag, ref, mask64 = clean
    for norm_type, (s64, s32, e32) in ref.items():
        print(f"{profile} {norm_type}: float32 oracle vs float64 {e32}")
        assert max(e32) < FB_LSTM_CAP / 8, (profile, norm_type, e32)
        assert all(fullband_lstm_bound(e) < FB_LSTM_CAP for e in e32)
    e = rel_err(_mask(sd, mag, ref["offline_laplace_norm"][1], torch.float32), mask64)
    print(f"{profile}: float32 mask vs float64 {e:.2e}")
    assert e < MASK_TOL / 100


def _check_fault(profile, fault, bad, s64, e32):
    errs, where = plane_errs(bad.numpy(), s64.numpy())
    bounds = [fullband_lstm_bound(e) for e in e32]
    print(f"{profile} {fault}: fb_mag {errs} at {where}; bounds {bounds}; closest {min(e / b for e, b in zip(errs, bounds)):.1f} x its bound")
    for b in range(B):
        assert errs[b] > 2 * bounds[b], (profile, fault, b, errs, where, bounds)


@pytest.mark.parametrize("fault", list(LSTM_FAULTS))
def test_emulated_lstm_fault_exceeds_the_stage_bound_and_passes_the_mask_tolerance(clean, fault):
    profile, sd, mag, ref, mask64 = clean
    s64, _, e32 = ref["offline_laplace_norm"]
    bad = faulty_fullband(sd, mag, FULLSUBNET_MODEL_ARGS, torch.float32, fault)
    _check_fault(profile, fault, bad, s64, e32)
    e = rel_err(_mask(sd, mag, bad, torch.float32), mask64)
    print(f"{profile} {fault}: mask error {e:.2e} of the batch's maximum")
    if profile in LSTM_FAULTS[fault]:
        assert e < MASK_TOL, (profile, fault, e)           # the gap: the end-to-end assertion on the same data does not see it


@pytest.mark.parametrize("fault", NORM_FAULTS)
def test_emulated_statistics_fault_exceeds_the_stage_bound(clean, fault):
    profile, sd, mag, ref, _ = clean
    args = CUM_ARGS if fault == "frame_statistics_count_one_frame_too_many" else FULLSUBNET_MODEL_ARGS
    s64, _, e32 = ref[args["norm_type"]]
    _check_fault(profile, fault, faulty_fullband(sd, mag, args, torch.float32, fault), s64, e32)

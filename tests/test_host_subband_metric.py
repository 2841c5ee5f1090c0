"""CPU checks of the sub-band reference and metric of tests/test_gpu_subband.py.

1. tests/_util.py oracle_subband is pinned: fed the float32 stages a whole oracle forward records, it returns that forward's output
   bit for bit (FullSubNet+, the original FullSubNet, drop band on and off, fb_num_neighbors 0 and 2, LSTM / GRU / TCN sub-band
   models, output_size 3).

2. Would the metric fail on a subtly wrong gather or normalisation?  The faults a per-kernel gather (sb_feature_offset /
   reflect_index, written once per kernel file) or a per-utterance count (per_frame * tpb[b]) could plausibly have are emulated inside
   oracle_subband by replacing fsnp_torch.unfold or one entry of fsnp_torch.NORMS.  Each emulated fault, evaluated in float32 on the
   oracle's own float32 stages,
     - passes the end-to-end check the suite had (rel_err on the mask against the float32 oracle < 1e-3, normalised by the global
       maximum of the batch),
     - exceeds the bound the GPU test asserts per utterance, min(8 * e32, 2e-5), by ten times or more,
   while the clean float32 oracle - the yardstick e32 - stays below 2e-5 / 8.  Profile, T and seed of each fault were chosen on the
   CPU among small shapes; FAULTS states them.  A cumulative norm whose count starts one frame late (frame t divided by F * t) is
   not among them: it doubles the mean at frame 1 whatever the clip's length, and moved the mask by 1.8e-2 of its maximum at
   T = 40 (harsh, cumulative_laplace_norm) - the end-to-end check already sees it at every small shape.
"""
import numpy as np
import pytest
import torch

from oracle import fsnp_torch
from oracle.make_golden import make_spec
from oracle.ref_loader import DEFAULT_MODEL_ARGS, FULLSUBNET_MODEL_ARGS
from oracle.weights import make_state_dict, make_state_dict_fullsubnet
from tests._subband_cases import plus_state_dict
from tests._util import fullsubnet_oracle_kwargs, mask_errs, oracle_kwargs, oracle_subband, rel_err

CAP, K, TOL_END_TO_END = 2e-5, 8, 1e-3


# ------------------------------------------------------------------------------------------------ 1. the pin
PLUS_PINS = {
    "default_full": (dict(), False, 1),
    "default_drop_b3": (dict(), True, 3),
    "three_groups_b4": (dict(num_groups_in_drop_band=3), True, 4),
    "fbn2_drop_b4": (dict(fb_num_neighbors=2), True, 4),
    "fbn2_full_cum_layer": (dict(fb_num_neighbors=2, norm_type="cumulative_layer_norm"), False, 2),
    "gru_gaussian": (dict(sequence_model="GRU", norm_type="offline_gaussian_norm"), False, 2),
    "tcn_cum_laplace": (dict(sequence_model="TCN", norm_type="cumulative_laplace_norm"), False, 1),
    "tcn_drop_b3": (dict(sequence_model="TCN"), True, 3),
    "output3_tanh": (dict(output_size=3, sb_output_activate_function="Tanh"), False, 2),
    "eca_subband2": (dict(channel_attention_model="ECA", subband_num=2), False, 1),
    "sbn7_la0": (dict(sb_num_neighbors=7, look_ahead=0), False, 1),
}


@pytest.mark.parametrize("name", sorted(PLUS_PINS))
def test_oracle_subband_is_the_second_half_of_the_oracle_forward(name):
    over, drop, B = PLUS_PINS[name]
    args = dict(DEFAULT_MODEL_ARGS, num_freqs=33, **over)          # (33 bins: the drop-band tail F % groups != 0 at 2 and 3 groups)
    sd = plus_state_dict(3, "harsh", args)
    ins = make_spec(B, 12, 17, 33)
    st = {}
    want = fsnp_torch.forward(sd, *ins, apply_drop_band=drop, stages=st, **oracle_kwargs(args))
    assert all(st[k].dtype == torch.float32 for k in st)
    got = oracle_subband(sd, {k: st[k] for k in ("att_mag", "fb_mag", "fb_real", "fb_imag")}, args, torch.float32, drop_band=drop)
    assert got.shape == want.shape and torch.equal(got, want)
    wide = oracle_subband(sd, st, args, torch.float64, drop_band=drop)
    assert wide.dtype == torch.float64 and rel_err(got.numpy(), wide.numpy()) < 1e-5


@pytest.mark.parametrize("fbn,drop,B", [(0, False, 1), (0, True, 3), (2, False, 2), (2, True, 4)])
def test_oracle_subband_is_the_second_half_of_the_fullsubnet_oracle_forward(fbn, drop, B):
    args = dict(FULLSUBNET_MODEL_ARGS, num_freqs=33, fb_num_neighbors=fbn)
    sd = make_state_dict_fullsubnet(5, "harsh", num_freqs=33, fb_num_neighbors=fbn)
    mag = make_spec(B, 12, 23, 33)[0]
    st = {}
    want = fsnp_torch.forward_fullsubnet(sd, mag, apply_drop_band=drop, stages=st, **fullsubnet_oracle_kwargs(args))
    att = torch.nn.functional.pad(mag, [0, args["look_ahead"]])[:, 0]          # FullSubNet unfolds the padded magnitude itself
    got = oracle_subband(sd, {"att_mag": att, "fb_mag": st["fb_mag"]}, args, torch.float32, drop_band=drop)
    assert got.shape == want.shape and torch.equal(got, want)


def test_mask_errs_is_per_utterance_and_says_where():
    want = np.zeros((2, 2, 5, 7))
    want[0, 1, 2, 3], want[1, 0, 4, 1] = 100.0, 0.01               # a loud and a quiet utterance
    got = want.copy()
    got[0, 0, 4, 6] += 1.0
    got[1, 1, 3, 5] += 0.001
    errs, where = mask_errs(got, want)
    assert np.allclose(errs, [0.01, 0.1]) and where == [(4, 0, 6), (3, 1, 5)]


# ------------------------------------------------------------------------------------------------ 2. emulated faults
def faulty_unfold(bug):
    """fsnp_torch.unfold with the reflected neighbour of ONE edge bin of the magnitude read from the wrong bin."""
    real = fsnp_torch.unfold

    def unfold(x, n):
        u = real(x, n)                                           # [B, F, C, 2 n + 1, T]
        if n >= 1:
            u = u.clone()
            if bug == "reflect_bin0":                            # neighbour -1 of bin 0: bin 0 instead of bin 1
                u[:, 0, :, n - 1] = x[:, :, 0]
            elif bug == "reflect_last_bin":                      # neighbour F of bin F - 1: bin F - 1 instead of bin F - 2
                u[:, -1, :, n + 1] = x[:, :, -1]
        return u
    return unfold


def offline_laplace_one_frame_too_many(x):
    """offline_laplace_norm whose element count holds one frame more than the clip has."""
    T = x.shape[-1]
    return x / (torch.mean(x, dim=(1, 2, 3), keepdim=True) * T / (T + 1) + 1e-5)


def offline_gaussian_one_frame_too_many(x):
    """offline_gaussian_norm from the sums, with one frame too many in both counts (mean and unbiased variance)."""
    n = x[0].numel() // x.shape[-1] * (x.shape[-1] + 1)
    s, ss = x.sum(dim=(1, 2, 3), keepdim=True), (x * x).sum(dim=(1, 2, 3), keepdim=True)
    mu = s / n
    return (x - mu) / (torch.sqrt((ss - n * mu * mu) / (n - 1)) + 1e-5)


# fault -> (what to replace, profile, T, seed of make_spec(2, T, seed), norm_type)
FAULTS = {
    "reflect_bin0": ("unfold", "harsh", 40, 4040, "offline_laplace_norm"),
    "reflect_last_bin": ("unfold", "harsh", 40, 4040, "offline_laplace_norm"),
    "laplace_count_one_frame_too_many": (offline_laplace_one_frame_too_many, "harsh", 400, 4040, "offline_laplace_norm"),
    "gaussian_count_one_frame_too_many": (offline_gaussian_one_frame_too_many, "harsh", 400, 4040, "offline_gaussian_norm"),
}
_CLEAN = {}


def clean(profile, T, seed, norm):
    """(sd, args, the oracle's own float32 stages, the mask in float64, the mask in float32) - one per shape, shared by its faults."""
    key = (profile, T, seed, norm)
    if key not in _CLEAN:
        torch.set_num_threads(min(16, torch.get_num_threads()))
        args = dict(DEFAULT_MODEL_ARGS, norm_type=norm)
        sd = make_state_dict(21, profile)
        st = {}
        out = fsnp_torch.forward_full(sd, *make_spec(2, T, seed), stages=st, **oracle_kwargs(args))
        st = {k: st[k] for k in ("att_mag", "fb_mag", "fb_real", "fb_imag")}
        w64, w32 = (oracle_subband(sd, st, args, dt).numpy() for dt in (torch.float64, torch.float32))
        assert np.array_equal(w32, out.numpy())
        _CLEAN[key] = (sd, args, st, w64, w32)
    return _CLEAN[key]


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_emulated_subband_fault_passes_end_to_end_and_fails_the_new_metric(fault, monkeypatch):
    what, profile, T, seed, norm = FAULTS[fault]
    sd, args, st, w64, w32 = clean(profile, T, seed, norm)
    if what == "unfold":
        monkeypatch.setattr(fsnp_torch, "unfold", faulty_unfold(fault))
    else:
        monkeypatch.setitem(fsnp_torch.NORMS, norm, what)
    bad = oracle_subband(sd, st, args, torch.float32).numpy()
    end_to_end = rel_err(bad, w32)
    (e32, _), (errs, where) = mask_errs(w32, w64), mask_errs(bad, w64)
    bounds = [min(K * e, CAP) for e in e32]
    print(f"{fault} ({profile}, T = {T}, {norm}): end to end {end_to_end:.2e}; per utterance {errs} at {where}; e32 {e32}; bounds {bounds}")
    assert max(e32) < CAP / K, e32                                # the yardstick alone meets the condition
    assert end_to_end < TOL_END_TO_END, end_to_end                # the check the suite had does not see the fault
    assert max(e / b for e, b in zip(errs, bounds)) >= 10, (errs, bounds)       # the new one does, ten times over


@pytest.mark.parametrize("norm", sorted(fsnp_torch.NORMS))
@pytest.mark.parametrize("profile", ["default", "harsh"])
def test_clean_float32_oracle_is_inside_the_cap(profile, norm):
    """The reference's own fp32 rounding, times the margin K = 8, fits under the cap with every norm and both weight profiles."""
    _, _, _, w64, w32 = clean(profile, 40, 4040, norm)
    e32, where = mask_errs(w32, w64)
    print(f"{profile} {norm}: float32 oracle vs float64 {e32} at {where}")
    assert max(e32) < CAP / K, (e32, where)


# ------------------------------------------------------------------------------------------------ 3. the plans of the GPU cases
def _lib_plan(rows, cus, hidden, gru, coop, costs):
    """fsnp_debug_plan_rows2 (host only, as tests/test_host.py calls it) -> [(kind, rows, tiles, ex, par, rpg)]."""
    import ctypes as ct
    from fullsubnet_plus_amd import _lib
    lib = _lib.load()
    buf = (ct.c_int32 * (8 * 64))()
    arr = (ct.c_double * _lib.NUM_COSTS)(*(list(costs) + [1e9] * (_lib.NUM_COSTS - len(costs)))) if costs else None
    n = lib.fsnp_debug_plan_rows2(rows, cus, hidden, gru, coop, 0.97, 1, arr, buf, 64)
    assert n > 0, lib.fsnp_last_error()
    return [(buf[8 * i], buf[8 * i + 2], buf[8 * i + 3], buf[8 * i + 4], buf[8 * i + 5], buf[8 * i + 6]) for i in range(n)]


def test_written_out_cost_table_is_the_built_in_one():
    from tests._subband_cases import BUILT_IN
    for rows in (161, 257, 384, 514, 771, 1028, 2056, 4112, 8224):
        assert _lib_plan(rows, 256, 384, 0, 1, BUILT_IN) == _lib_plan(rows, 256, 384, 0, 1, None), rows


@pytest.mark.parametrize("name", [n for n, c in __import__("tests._subband_cases", fromlist=["CASES"]).CASES.items() if c["host"]])
def test_gpu_case_states_the_plan_the_host_planner_gives(name):
    from tests._subband_cases import CASES, host_plan
    c = CASES[name]
    assert host_plan(c, _lib_plan) == c["plan"], (name, host_plan(c, _lib_plan))


def test_gpu_cases_cover_every_launch_shape():
    """Every kernel kind, every K-split and wave-owned width, VALU rows 0 / 1 / 2 / 4, several rounds, one-tile launches, ragged last
    tiles, one and two row tiles per three-way group - by the plans the cases state."""
    from tests._subband_cases import CASES
    launches = [(c, p) for c in CASES.values() if c["plan"] for p in c["plan"]]
    assert {p[0] for _, p in launches} == {0, 1, 2, 4, 8, 9}
    assert {p[4] for _, p in launches if p[0] == 1} == {8, 16, 32, 64} and {p[4] for _, p in launches if p[0] == 9} == {32, 64, 96}
    assert {p[3] for _, p in launches if p[0] == 0} == {0, 1, 2, 4} and {p[5] for _, p in launches if p[0] == 2} == {1, 2}
    assert any(p[0] == 0 and c["cus"] and p[2] > 2 * c["cus"] for c, p in launches)              # three rounds of row tiles
    assert any(p[0] == 1 and p[2] == 1 for _, p in launches) and any(p[0] == 1 and p[2] > 1 for _, p in launches)
    assert any(p[0] == 4 and p[1] % 16 == 1 for _, p in launches) and any(p[0] == 0 and p[1] % (32 + p[3]) for _, p in launches)
    assert {c["waves"] for c, p in launches if p[0] == 0} >= {4, 12}
    assert {c["pp"] for c, p in launches if p[0] == 8} == {"hp", "hpw"}

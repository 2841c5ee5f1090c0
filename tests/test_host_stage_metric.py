"""CPU check of the stage-level metric of tests/test_gpu_stages.py: would it fail on a subtly wrong full-band kernel?

The TCN bugs a kernel of csrc/tcn.hip could plausibly have (a dropped output column - the 64-row kernel's VALU column N - 1; a missing
halo frame of the depthwise conv; a GroupNorm count off by one frame; an ignored k tail; one frame of one block's sconv lost) are
emulated inside the oracle by replacing fsnp_torch.tcn_block, at B = 2, T = 140 with both weight profiles.  Each must move every
full-band plane by more than the cap the GPU test asserts (tests/_util.py STAGE_CAPS["fb"] = 2e-4) under plane_errs, while the clean
oracle in float32 - the yardstick the GPU test multiplies by its margin k = 8 - stays below cap / 8.  The stage functions only: no
sub-band LSTM runs here.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from oracle import fsnp_torch
from oracle.make_golden import make_spec
from oracle.ref_loader import DEFAULT_MODEL_ARGS
from oracle.weights import make_state_dict
from tests._util import STAGE_CAPS, STAGE_TAGS, oracle_stages, plane_errs

B, T = 2, 140
BUGS = ("sconv_bin256_dropped_last_block", "sconv_bin256_dropped_every_block", "dwconv_dil9_halo_misses_last_frame",
        "groupnorm1_count_off_by_one_frame", "conv1x1_ignores_bin256", "sconv_frame127_zeroed_block3")


def _group_norm(y, w, b, frames_counted):
    """GroupNorm(1 group) of y [B, C, T] from its sums, with C * frames_counted as the element count."""
    cnt = y.shape[1] * frames_counted
    m = y.sum(dim=(1, 2), keepdim=True) / cnt
    var = (y * y).sum(dim=(1, 2), keepdim=True) / cnt - m * m
    return (y - m) / torch.sqrt(var + 1e-8) * w[None, :, None] + b[None, :, None]


def bugged_tcn_block(bug):
    """A replacement of fsnp_torch.tcn_block (causal_conv.py:96-108, same operations in the same order) with one emulated bug, or none."""
    def block(x, p, prefix, dilation):
        blk = int(prefix.rsplit(".", 1)[1])
        Hc, Tn = p[prefix + ".conv1x1.weight"].shape[0], x.shape[-1]
        xin = x
        if bug == "conv1x1_ignores_bin256":
            xin = x.clone()
            xin[:, 256] = 0
        y = Fn.prelu(Fn.conv1d(xin, p[prefix + ".conv1x1.weight"], p[prefix + ".conv1x1.bias"]), p[prefix + ".prelu1.weight"])
        if bug == "groupnorm1_count_off_by_one_frame":
            y = _group_norm(y, p[prefix + ".norm1.weight"], p[prefix + ".norm1.bias"], Tn + 1)
        else:
            y = Fn.group_norm(y, 1, p[prefix + ".norm1.weight"], p[prefix + ".norm1.bias"], 1e-8)
        dw = p[prefix + ".depthwise_conv.weight"]
        z = Fn.conv1d(y, dw, p[prefix + ".depthwise_conv.bias"], padding=dilation, dilation=dilation, groups=Hc)
        if bug == "dwconv_dil9_halo_misses_last_frame" and dilation == 9:
            z[:, :, Tn - 1 - dilation] -= dw[None, :, 0, 2] * y[:, :, Tn - 1]       # the tap one dilation ahead read 0 there
        z = Fn.group_norm(Fn.prelu(z, p[prefix + ".prelu2.weight"]), 1, p[prefix + ".norm2.weight"], p[prefix + ".norm2.bias"], 1e-8)
        s = Fn.conv1d(z, p[prefix + ".sconv.weight"], p[prefix + ".sconv.bias"])
        if bug == "sconv_bin256_dropped_every_block" or (bug == "sconv_bin256_dropped_last_block" and blk == 7):
            s[:, 256] = 0
        if bug == "sconv_frame127_zeroed_block3" and blk == 3:
            s[:, :, 127] = 0
        return x + s
    return block


@pytest.fixture(scope="module", params=["default", "harsh"])
def clean(request):
    """(profile, sd, ins, the clean stages in float64, the clean stages in float32)."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sd = make_state_dict(21, request.param)
    ins = make_spec(B, T, 77)
    return request.param, sd, ins, oracle_stages(sd, ins, DEFAULT_MODEL_ARGS), oracle_stages(sd, ins, DEFAULT_MODEL_ARGS, torch.float32)


def test_plane_errs_is_per_plane_and_says_where():
    want = np.zeros((2, 5, 7))
    want[0, 1, 2], want[1, 3, 3] = 100.0, 0.01                 # a loud and a quiet utterance
    got = want.copy()
    got[0, 4, 6] += 1.0
    got[1, 0, 5] += 0.001
    errs, where = plane_errs(got, want)
    assert np.allclose(errs, [0.01, 0.1]) and where == [(4, 6), (0, 5)]
    got[1, 2, 2] = np.nan
    errs, where = plane_errs(got, want)
    assert errs[1] == np.inf and where[1] == (2, 2) and np.isclose(errs[0], 0.01)


def test_restated_block_without_a_bug_is_the_oracles_block(clean):
    _, sd, ins, _, _ = clean
    p = {k: v.double() for k, v in sd.items()}
    x = torch.randn(2, 257, 40, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    for blk, dil in ((0, 1), (3, 9)):
        prefix = f"fb_model_real.sequence_model.{blk}"
        assert torch.equal(bugged_tcn_block(None)(x, p, prefix, dil), fsnp_torch.tcn_block(x, p, prefix, dil))


def test_clean_float32_oracle_is_inside_the_caps(clean):
    """The reference's own fp32 rounding, times the smallest margin k = 8, fits under both caps: the yardstick alone meets the condition."""
    profile, _, _, s64, s32 = clean
    for tag in STAGE_TAGS:
        errs, where = plane_errs(s32[tag].numpy(), s64[tag].numpy())
        print(f"{profile} {tag}: float32 oracle vs float64 {errs} at {where}")
        assert max(errs) < STAGE_CAPS[tag[:tag.index("_")]] / 8, (profile, tag, errs, where)


@pytest.mark.parametrize("bug", BUGS)
def test_emulated_tcn_bug_exceeds_the_fullband_cap(clean, bug, monkeypatch):
    profile, sd, ins, s64, s32 = clean
    monkeypatch.setattr(fsnp_torch, "tcn_block", bugged_tcn_block(bug))
    bad = oracle_stages(sd, ins, DEFAULT_MODEL_ARGS)
    seen = {}
    for tag in STAGE_TAGS:
        errs, where = plane_errs(bad[tag].numpy(), s64[tag].numpy())
        if tag.startswith("att_"):
            assert max(errs) == 0.0                            # the bug sits behind the attention stage
            continue
        e32, _ = plane_errs(s32[tag].numpy(), s64[tag].numpy())
        seen[tag] = (errs, where, e32)
        print(f"{profile} {bug} {tag}: {errs} at {where}; float32 oracle {e32}")
    # every clip fails the check: its worst branch (fb_mag, whose input is the largest) is beyond the cap itself ...
    for b in range(B):
        assert max(seen[tag][0][b] for tag in seen) > STAGE_CAPS["fb"], (profile, bug, b, seen)
    # ... and every plane of every branch is beyond the largest bound the GPU test may ever use, 32 x the float32 oracle's own error
    for tag, (errs, where, e32) in seen.items():
        assert min(errs) > 32 * max(e32), (profile, bug, tag, errs, where, e32)

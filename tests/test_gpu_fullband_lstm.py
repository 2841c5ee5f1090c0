"""GPU tests of the full-band stage of the original FullSubNet (run_fullband_fullsubnet, csrc/fsnp_abi.hip: launch_frontend_mag -> one of
three recurrent kernels -> launch_linear_act) at the stage itself and per kernel path, not through the final mask: the sub-band model
attenuates a full-band error 40 to 400 times, and the faults tests/test_host_fullband_lstm_metric.py emulates pass the end-to-end 1e-3
while they sit 45 to 80000 times above the bound asserted here.

A case runs whole forwards in batch_mode "full", then check_errors() and read_stage("fb_mag") / read_stage("att_mag").

Reference: tests/_util.py oracle_fullband_fullsubnet in float64; for ragged batches (lengths= with garbage_tails inputs) the oracle of
each clip alone on its own lengths[b] frames.  Only a clip's own lengths[b] + look_ahead frames are compared, and they must be finite.
att_mag of this model is the padded magnitude itself: bit-equal to the input on a clip's frames, zero on its look-ahead frames.

Metric and bound: tests/_util.py plane_errs - max|got - want| / max|want| over ONE utterance's fb_mag plane.  The yardstick e32 of a
plane is the same metric of the float32 oracle against the float64 oracle: nothing of the code under test enters it.  Asserted of every
utterance of every batch: err <= min(K * max(e32, 2**-23), CAP) (tests/_util.py fullband_lstm_bound), K = 8 the margin the sibling stage
tests give kernels that sum in another association and use the hardware exp and reciprocal, CAP = 2e-5 what the suite asserts of every
recurrent kernel in dense mode, 2**-23 one fp32 spacing of the plane's maximum (below it e32 is luck, not a yardstick).  Every case's
figures go to fullband_lstm_report.json, next to the parity report of tests/test_gpu_parity.py.

Kernel paths: lstm_coop_pick_units (csrc/lstm_coop.hip), lstm_generic_rows_per_group (csrc/lstm_generic.hip), lstm_fbv_available
(csrc/lstm_fbv.hip) and fb_shape (csrc/fsnp_abi.hip) are restated below; every case names its path, asserts that fullband_launch reports
the restated kernel, tiles, rows per tile and units, and skips - it does not pass on another path - on a device whose CU count moves it
elsewhere.  Where lstm_fbv and the K-split kernel (debug_set_lstm_coop(2)) run the same input, their fb_mag bits must differ.

Row placement: the plane of a clip must not depend on the row it sits at (same kernel, same k order).  From B = 5 up the pool holds clip
0 again at rows 1, the last row of the first tile / group, the first row of the next and B - 1 (the rows between hold other clips), and
those planes must be bit-equal.  Up to B = 4 and in ragged batches that placement would leave no second clip in the batch (a kernel that
broadcast row 0 would pass), so every batch runs a second time rotated by one row and each clip's two planes must be bit-equal.

Measured on an MI355X (256 CUs), err / max(e32, 2**-23) over all cases: 0.93 ... 4.71, with e32 from 4.6e-8 to 6.6e-7 and err at most
1.6e-6.  The worst per kernel file: 3.27 lstm_fbv.hip (ragged, cumulative_laplace_norm, a one-frame clip); lstm_coop.hip 4.71 at 8 units
(B = 33, one step, look_ahead = 0), 3.53 at 16 units, 3.67 at 32 units, 3.32 as a GRU; lstm_generic.hip 4.17 (ragged,
cumulative_layer_norm, a one-frame clip), 3.22 as a GRU.  The 626-frame clip: 2.09 / 2.53 (lstm_fbv, default / harsh weights) and
1.99 / 2.47 (K-split) - no drift over the recurrence.  No path needs its own K; every placement was bit-equal; lstm_fbv and the K-split
kernel never gave the same bits.
"""
import os

import numpy as np
import pytest
import torch

from fullsubnet_plus_amd import FullSubNet
from oracle.make_golden import make_spec
from oracle.ref_loader import FULLSUBNET_MODEL_ARGS
from oracle.weights import make_state_dict_fullsubnet
from tests._util import (FB_LSTM_FLOOR, FB_LSTM_K, edge_lengths, fullband_lstm_bound, garbage_tails, oracle_fullband_fullsubnet,
                         oracle_rows, plane_errs)

pytestmark = pytest.mark.gpu
PATH_K = {}                  # a named path's own K, were one needed (at most twice its measured worst ratio; never beyond CAP): none is
PROFILES = ("default", "harsh")
REPORT = {}

torch.set_num_threads(min(16, os.cpu_count() or 1))


def _record(name, entry):
    """fullband_lstm_report.json, written the way (and where) tests/test_gpu_parity.py writes parity_report.json."""
    from tests.test_gpu_parity import _record as record
    record(name, _report=REPORT, _file="fullband_lstm_report.json", **entry)


# ------------------------------------------------------------------------------------------------ the launch, restated
def _cdiv(a, b):
    return -(-a // b)


def pick_units(H, row_tiles, cus, min_units=8):
    """lstm_coop_pick_units: the finest column split whose row_tiles * H / units workgroups are all resident at once, one per CU."""
    for u in (8, 16, 32, 64):
        if u >= min_units and H % u == 0 and row_tiles * (H // u) <= cus:
            return u
    return 0


def generic_rows_per_group(H, NIN, num_seq):
    """lstm_generic_rows_per_group: sequences per workgroup by the sequence count, halved while the LDS image exceeds 150 KiB."""
    def smem(rg):
        return rg * (_cdiv(NIN, 4) * 4 + 8 * _cdiv(H, 4) * 4) * 4
    rg = 8 if num_seq >= 2048 else 4 if num_seq >= 128 else 2 if num_seq >= 32 else 1
    while rg > 1 and smem(rg) > 150 * 1024:
        rg //= 2
    return rg if smem(rg) <= 150 * 1024 else 0


def expected_launch(args, B, cus, coop):
    """fb_shape: what fullband_launch(B) must report under debug_set_lstm_coop(coop)."""
    H, F, gru = args["fb_model_hidden_size"], args["num_freqs"], args["sequence_model"] == "GRU"
    if H != 512 or F > 264:
        rg = generic_rows_per_group(H, F, B)
        return {"kernel": "generic", "tiles": _cdiv(B, rg), "rows_per_tile": rg, "units": 0}
    if coop == 1 and not gru and F <= 288 and 1 <= B <= 4 and cus >= H // 8:
        return {"kernel": "fbv", "tiles": _cdiv(B, 32), "rows_per_tile": 32, "units": 0}
    u = pick_units(H, _cdiv(B, 32), cus)
    return {"kernel": "coop_seq", "tiles": _cdiv(B, 32), "rows_per_tile": 32, "units": 0 if u > 32 else u}


FBV, KS8, KS16, KS32 = ({"kernel": "fbv"}, {"kernel": "coop_seq", "units": 8}, {"kernel": "coop_seq", "units": 16},
                        {"kernel": "coop_seq", "units": 32})
BOTH = (("fbv", 1, FBV), ("ksplit", 2, KS8))             # B <= 4: lstm_fbv, then the K-split kernel it replaces, on the same input


def GEN(rows):
    return {"kernel": "generic", "rows_per_tile": rows}


# ------------------------------------------------------------------------------------------------ one case
_MODELS = {}


def _model(over, profile):
    """One model per (arguments, weight profile), shared by the cases."""
    key = (tuple(sorted(over.items())), profile)
    if key not in _MODELS:
        args = dict(FULLSUBNET_MODEL_ARGS, **over)
        sd = make_state_dict_fullsubnet(21, profile, num_freqs=args["num_freqs"], fb_hidden=args["fb_model_hidden_size"],
                                        sequence_model=args["sequence_model"])
        m = FullSubNet(**args)
        m.load_state_dict(sd, strict=True)
        m = m.to("cuda").eval()
        m.batch_mode = "full"
        _MODELS[key] = (m, sd, args)
    return _MODELS[key]


def _forward(m, mag, lens, T, la):
    """One forward -> the fb_mag planes [F, lens[b] + la] of its rows; att_mag checked against the input."""
    B = mag.shape[0]
    if any(n != T for n in lens):
        (x,) = garbage_tails([mag], lens, 9)
        m(x.cuda(), lengths=lens)
    else:
        m(mag.contiguous().cuda())
    m.check_errors()
    fb = m.read_stage("fb_mag", B, T).permute(0, 2, 1).numpy()
    att = m.read_stage("att_mag", B, T).permute(0, 2, 1)
    for b, n in enumerate(lens):
        assert torch.equal(att[b, :, :n], mag[b, 0, :, :n]), f"att_mag of row {b} is not the input"
        assert torch.count_nonzero(att[b, :, n:n + la]) == 0, f"att_mag of row {b}: look-ahead frames are not 0"
    return [fb[b, :, :n + la].copy() for b, n in enumerate(lens)]


def placement(B, rows_per_tile):
    """The rows clip 0 sits at in a batch of B >= 5."""
    return sorted({r for r in (0, 1, rows_per_tile - 1, rows_per_tile, B - 1) if 0 <= r < B})


def run_case(name, over, profile, B, T, paths, *, lengths=None, seed=0, ends=None):
    """paths: ((label, debug_set_lstm_coop mode, the launch the case names), ...).  Every row of every batch against the float64 oracle
    within fullband_lstm_bound(e32); the launch by formula and through fullband_launch; row placement and path differences by bits.
    ends: also record the ratios over the first and over the last `ends` frames."""
    m, sd, args = _model(over, profile)
    la, F = args["look_ahead"], args["num_freqs"]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    want_launch = {}
    for label, coop, named in paths:
        want_launch[label] = expected_launch(args, B, cus, coop)
        if any(want_launch[label][k] != v for k, v in named.items()):
            pytest.skip(f"{name}: on {cus} CUs B = {B} launches {want_launch[label]}, the case is about {named}")
    ragged = lengths is not None
    n = len(lengths) if ragged else B
    pool = make_spec(n, T, 4100 + seed, F)[0].clone()
    canon = list(range(n))                                   # canon[i]: the pool clip row i repeats
    if not ragged:
        lengths = [T] * B
        if B >= 5:
            for r in placement(B, want_launch[paths[0][0]]["rows_per_tile"])[1:]:
                pool[r] = pool[0]
                canon[r] = 0
    batches = [[(k + i) % n for i in range(B)] for k in range(0, n, B)]
    if ragged or 2 <= B <= 4:
        batches += [idx[1:] + idx[:1] for idx in batches]    # each batch again, rotated by one row
    want, want32 = ([r[0].numpy() for r in oracle_rows(lambda x, dt=dt: oracle_fullband_fullsubnet(sd, x, args, dt)["fb_mag"], [pool], lengths)]
                    for dt in (torch.float64, torch.float32))
    e32 = [plane_errs(w32[None], w[None])[0][0] for w, w32 in zip(want, want32)]
    entry = {"lengths": lengths if ragged else None, "B": B, "T": T, "e32_min_max": [min(e32), max(e32)]}
    failures, bits = [], {}
    try:
        for label, coop, _ in paths:
            m.debug_set_lstm_coop(coop)
            planes = {}                                      # canonical clip -> [(batch, row, plane)]
            worst = {"ratio": -1.0}
            k = PATH_K.get(label, FB_LSTM_K)
            for bi, idx in enumerate(batches):
                got = _forward(m, pool[idx], [lengths[i] for i in idx], T, la)
                launch = m.fullband_launch(B)
                assert launch == want_launch[label], (name, label, launch, want_launch[label])
                for row, (i, g) in enumerate(zip(idx, got)):
                    assert np.isfinite(g).all(), f"{name} {label}: batch {bi} row {row}: fb_mag is not finite on the clip's frames"
                    (err,), (where,) = plane_errs(g[None], want[i][None])
                    yard = max(e32[i], FB_LSTM_FLOOR)
                    if err / yard > worst["ratio"]:
                        worst = {"ratio": err / yard, "err_over_e32": err / e32[i], "err": err, "e32": e32[i], "clip": i, "row": row, "length": lengths[i], "bin_frame": list(where)}
                    if not err <= fullband_lstm_bound(e32[i], k):
                        failures.append((label, bi, row, i, lengths[i], where, err, fullband_lstm_bound(e32[i], k), err / yard))
                    planes.setdefault(canon[i], []).append((bi, row, g))
            moved = [(c, bi, row) for c, ps in planes.items() for bi, row, g in ps[1:] if not np.array_equal(g, ps[0][2])]
            worst["placements_checked"] = sum(len(ps) - 1 for ps in planes.values())
            worst["launch"] = want_launch[label]
            if ends:
                g, w, w32 = planes[0][0][2], want[0], want32[0]
                for tag, sl in (("first", slice(0, ends)), ("last", slice(-ends, None))):
                    (e,), _ = plane_errs(g[None, :, sl], w[None, :, sl])
                    (y,), _ = plane_errs(w32[None, :, sl], w[None, :, sl])
                    worst[f"ratio_{tag}_{ends}_frames"] = e / max(y, FB_LSTM_FLOOR)
            entry[label] = worst
            print(f"{name} {label}: worst {worst['ratio']:.2f} x e32 (err {worst['err']:.2e}, e32 {worst['e32']:.2e}) clip {worst['clip']} row "
                  f"{worst['row']} length {worst['length']} at (bin, frame) {worst['bin_frame']}; {want_launch[label]}")
            assert not moved, (name, label, "(clip, batch, row) whose plane differs in bits from the clip's first placement", moved[:8])
            assert worst["placements_checked"] > 0 or B == 1
            bits[label] = np.concatenate([g.ravel() for c in sorted(planes) for _, _, g in planes[c]])
    finally:
        m.debug_set_lstm_coop(1)
        _record(name, entry)
    assert not failures, (name, "(path, batch, row, clip, length, (bin, frame), err, bound, err / e32)", failures[:12])
    labels = list(bits)
    for a, b in zip(labels, labels[1:]):                     # another kernel (another k order) gives other bits
        assert not np.array_equal(bits[a], bits[b]), f"{name}: {a} and {b} gave the same fb_mag bits"
    return entry


# ------------------------------------------------------------------------------------------------ 1. lstm_fbv, B = 1 ... 4
@pytest.mark.parametrize("B", [1, 2, 3, 4])
@pytest.mark.parametrize("profile", PROFILES)
def test_lstm_fbv_and_the_ksplit_kernel_at_one_to_four_rows(profile, B):
    """NB = 1, 2, 4 with a padded row at B = 3; under debug_set_lstm_coop(2) the same batches are one to four live rows of a 32-row
    K-split tile.  257 = 64 * 4 + 1 input bins in a k range zero-padded to 288 (lstm_fbv) and to 264 (K-split)."""
    run_case(f"fbv_{profile}_B{B}", {}, profile, B, 10, BOTH, seed=B)


@pytest.mark.parametrize("profile", PROFILES)
def test_one_long_clip_on_both_kernels(profile):
    """626 steps (10 s at hop 256): drift over the recurrence; the ratios over the first and the last 100 frames are recorded apart."""
    run_case(f"fbv_{profile}_B1_T626", {}, profile, 1, 626, BOTH, seed=626, ends=100)


# ------------------------------------------------------------------------------------------------ 2. K-split sequence kernel, LSTM
@pytest.mark.parametrize("B,named", [(5, KS8), (31, KS8), (32, KS8), (33, KS8), (128, KS8), (129, KS16), (256, KS16), (257, KS32), (512, KS32)],
                         ids=lambda v: f"units{v['units']}" if isinstance(v, dict) else str(v))
@pytest.mark.parametrize("profile", PROFILES)
def test_ksplit_sequence_kernel_across_tiles_and_units(profile, B, named):
    """lstm2_coop_kernel<512, 264, 8 | 16 | 32, SEQ>: the units follow the tile count (on 256 CUs: 8 up to 4 tiles, 16 up to 8, 32 up to
    16); B = 33, 129, 257 put one live row in the last tile."""
    run_case(f"ksplit_{profile}_B{B}", {}, profile, B, 8 if B >= 129 else 10, (("ksplit", 1, named),), seed=B)


# ------------------------------------------------------------------------------------------------ 3. GRU full-band model
@pytest.mark.parametrize("B,named", [(1, KS8), (33, KS8), (129, KS16)], ids=lambda v: f"units{v['units']}" if isinstance(v, dict) else str(v))
@pytest.mark.parametrize("profile", PROFILES)
def test_gru_fullband_on_the_ksplit_kernel(profile, B, named):
    """sequence_model="GRU" has no lstm_fbv path: B = 1 is one live row of a K-split tile."""
    run_case(f"gru_{profile}_B{B}", {"sequence_model": "GRU"}, profile, B, 8 if B >= 129 else 10, (("ksplit_gru", 1, named),), seed=B)


@pytest.mark.parametrize("profile", PROFILES)
def test_gru_fullband_on_the_generic_kernel(profile):
    run_case(f"gru_fb300_{profile}_B33", {"sequence_model": "GRU", "fb_model_hidden_size": 300}, profile, 33, 10, (("generic_gru", 1, GEN(2)),), seed=300)


# ------------------------------------------------------------------------------------------------ 4. generic kernel
@pytest.mark.parametrize("B,rows", [(3, 1), (31, 1), (32, 2), (127, 2), (128, 4)])
@pytest.mark.parametrize("profile", PROFILES)
def test_generic_kernel_on_both_sides_of_each_rows_per_group_step(profile, B, rows):
    run_case(f"generic_fb300_{profile}_B{B}", {"fb_model_hidden_size": 300}, profile, B, 8 if B >= 127 else 10, (("generic", 1, GEN(rows)),), seed=B)


@pytest.mark.parametrize("B,rows", [(3, 1), (33, 2)])
@pytest.mark.parametrize("profile", PROFILES)
def test_generic_kernel_hidden_size_no_multiple_of_four(profile, B, rows):
    """fb_model_hidden_size = 302: the h1 row stride is align_up(302, 4) = 304, and the Linear reads the two pad columns."""
    run_case(f"generic_fb302_{profile}_B{B}", {"fb_model_hidden_size": 302}, profile, B, 10, (("generic", 1, GEN(rows)),), seed=302 + B)


@pytest.mark.parametrize("B,rows", [(2, 1), (33, 2)])
@pytest.mark.parametrize("profile", PROFILES)
def test_generic_kernel_at_the_first_bin_count_past_the_tuned_kernels(profile, B, rows):
    """num_freqs = 265 with hidden 512: one bin more than the K-split kernel's k range of 264."""
    run_case(f"generic_bins265_{profile}_B{B}", {"num_freqs": 265}, profile, B, 10, (("generic", 1, GEN(rows)),), seed=265 + B)


# ------------------------------------------------------------------------------------------------ 5. bin counts on the tuned kernels
@pytest.mark.parametrize("B", [2, 33])
@pytest.mark.parametrize("F", [264, 161])
@pytest.mark.parametrize("profile", PROFILES)
def test_other_bin_counts_on_the_tuned_kernels(profile, F, B):
    """F = 264: the K-split k range exactly full, no zero padding; F = 161 = 40 * 4 + 1: another k tail, another Linear N tail."""
    paths = BOTH if B == 2 else (("ksplit", 1, KS8),)
    run_case(f"bins{F}_{profile}_B{B}", {"num_freqs": F}, profile, B, 10, paths, seed=F + B)


# ------------------------------------------------------------------------------------------------ 6. norm types, ragged lengths
NORM_TYPES = ("offline_laplace_norm", "cumulative_laplace_norm", "offline_gaussian_norm", "cumulative_layer_norm")
RAGGED_T, RAGGED_EDGES = 260, (8, 32, 256)


@pytest.mark.parametrize("B,over,path", [(4, {}, ("fbv", 1, FBV)), (5, {}, ("ksplit", 1, KS8)), (3, {"fb_model_hidden_size": 300}, ("generic", 1, GEN(1)))],
                         ids=["fbv_B4", "ksplit_B5", "generic_B3"])
@pytest.mark.parametrize("norm_type", NORM_TYPES)
@pytest.mark.parametrize("profile", PROFILES)
def test_norm_types_on_ragged_batches(profile, norm_type, B, over, path):
    """lengths[b] + look_ahead one below, at and one above 8, 32 and 256 (fe_scan_kernel's chunk), the shortest clip (one frame) and the
    whole buffer: the per-frame md_seq table and a clip's own statistics, against each clip alone."""
    la = FULLSUBNET_MODEL_ARGS["look_ahead"]
    lengths = edge_lengths(RAGGED_T, la, 1, edges=RAGGED_EDGES)
    assert lengths[0] == 1 and lengths[-1] == RAGGED_T and {e + d - la for e in RAGGED_EDGES for d in (-1, 0, 1)} <= set(lengths)
    run_case(f"ragged_{norm_type}_{profile}_{path[0]}_B{B}", dict(over, norm_type=norm_type), profile, B, RAGGED_T, (path,), lengths=lengths, seed=260)


# ------------------------------------------------------------------------------------------------ 7. Linear epilogue
@pytest.mark.parametrize("B", [2, 33])
@pytest.mark.parametrize("act", ["ReLU", "ReLU6", "Tanh", False])
@pytest.mark.parametrize("profile", PROFILES)
def test_linear_epilogue_activations(profile, act, B):
    """launch_linear_act with every fb_output_activate_function; without one the plane is not half zeros and the N tail (column 256 =
    4 * 64) carries signal of either sign."""
    paths = (("fbv", 1, FBV),) if B == 2 else (("ksplit", 1, KS8),)
    run_case(f"act_{act or 'none'}_{profile}_B{B}", {"fb_output_activate_function": act}, profile, B, 10, paths, seed=70 + B)


# ------------------------------------------------------------------------------------------------ 8. step-count edges
@pytest.mark.parametrize("B,path", [(1, ("fbv", 1, FBV)), (5, ("ksplit", 1, KS8)), (33, ("ksplit", 1, KS8))], ids=["fbv_B1", "ksplit_B5", "ksplit_B33"])
@pytest.mark.parametrize("profile", PROFILES)
def test_step_count_edges(profile, B, path):
    """The K-split schedule's three-image rotation, fc_epilogue(t - 2) and its Tp >= 2 branches (and lstm_fbv's two parity images):
    Tp = 1, 2, 3, 4, 7 steps with look_ahead = 0, and Tp = 3 as one frame plus the default look-ahead."""
    for over, T in [({"look_ahead": 0}, t) for t in (1, 2, 3, 4, 7)] + [({}, 1)]:
        la = over.get("look_ahead", FULLSUBNET_MODEL_ARGS["look_ahead"])
        run_case(f"steps_{profile}_{path[0]}_B{B}_T{T}_la{la}", over, profile, B, T, (path,), seed=10 * B + T)

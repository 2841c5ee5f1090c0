"""GPU tests of the full-band stages (norm -> channel attention -> eight TCN blocks -> Linear; csrc/frontend.hip, csrc/tcn.hip) at the
stage itself and per kernel path, not through the final mask (the sub-band model attenuates a full-band error 25 to 100 times; the
bugs tests/test_host_stage_metric.py emulates pass the end-to-end 1e-3 and sit 15 to 1000 times above the bound asserted here).

Every case runs whole forwards in batch_mode "full" (the fast GEMM kernels only run inside one: launch_tcn turns them on for three
branches), one per debug_set_gemm_dma mode 1, 0, 2, 3, and reads att_* / fb_* with read_stage.

Reference: the same stages of the oracle in float64 (tests/_util.py oracle_stages); for ragged batches the oracle of each clip alone.
Only a clip's own lengths[b] + look_ahead frames are compared (they must be finite although the input past each length holds NaN and
1e6); nothing is asserted about stage frames past a clip.

Metric and bound: tests/_util.py plane_errs - max|got - want| / max|want| over ONE utterance's plane of ONE branch.  The yardstick e32
of a plane is the same metric of the oracle in float32 against the oracle in float64 on that plane: nothing of the code under test
enters it.  Asserted, plane by plane: plane_errs(hip, oracle64) <= min(K * e32, cap) with K = 8 and the caps the suite already
asserts at these stages (2e-5 att_*, 2e-4 fb_*).  A margin above 1 because the kernels sum
K = 512 in another association (four split-K partials, the MFMA k permutation, column N - 1 in fp32 FMAs) and fold GroupNorm
algebraically: they are as accurate as fp32, not more.  Every case's ratios err / e32 go to stage_report.json, next to
the parity report of tests/test_gpu_parity.py.

Kernel paths: launch_gemm_dma / launch_gemm_dma64 / pick_bn (csrc/tcn.hip) are restated below; every case asserts the path its
shape takes under each mode AND that the fb_* buffers differ bit for bit between modes exactly where the formulas say another
kernel ran, so a case cannot pass on a path it did not take.
"""
import os

import numpy as np
import pytest
import torch

from fullsubnet_plus_amd import FullSubNet_Plus
from oracle.make_golden import make_spec
from oracle.ref_loader import DEFAULT_MODEL_ARGS
from oracle.weights import make_state_dict
from tests._util import STAGE_CAPS, STAGE_TAGS, edge_lengths, garbage_tails, oracle_rows, oracle_stages, plane_errs

pytestmark = pytest.mark.gpu
K = 8                        # margin over the float32 oracle's own error (module docstring)
LA = DEFAULT_MODEL_ARGS["look_ahead"]
CH = 512                     # channels of the full-band TCN: conv1x1 is [M][F] x [F][CH], the sconv [M][CH] x [CH][F]
REPORT = {}

torch.set_num_threads(min(16, os.cpu_count() or 1))


def _record(name, entry):
    """stage_report.json, written the way (and where) tests/test_gpu_parity.py writes parity_report.json."""
    from tests.test_gpu_parity import _record as record
    record(name, _report=REPORT, _file="stage_report.json", **entry)


# ------------------------------------------------------------------------------------------------ csrc/tcn.hip, restated
def _cdiv(a, b):
    return -(-a // b)


def splitk_runs(n, Tp, B, cus):
    """launch_gemm_dma, mode 1: tcn_gemm_sk_kernel (32-row tiles, four waves split K) while its launch has <= 6 workgroups per CU."""
    return _cdiv(n, 64) * _cdiv(Tp, 32) * B * 3 <= 6 * cus


def rows64_runs(n, Tp, B, cus):
    """launch_gemm_dma64, modes 1 and 2, the sconv only: tcn_gemm_dma64_kernel (n // 64 column tiles + column n - 1 on the VALU) when
    it needs no more rounds of workgroups than the 128-row kernel, whose workgroups cost two."""
    if n % 64 != 1:
        return False
    cost64 = _cdiv((n // 64) * _cdiv(Tp, 64) * B * 3, cus)
    cost128 = 2 * _cdiv(_cdiv(n, 64) * _cdiv(Tp, 128) * B * 3, cus)
    return cost64 <= cost128


def pick_bn(n, row_tiles, cus, branches=3):
    """Column-tile width of the general tcn_gemm_kernel: the cheapest of 64 / 96 / 128 in rounds x width, ties to the narrower."""
    best, best_cost = 64, None
    for c in (64, 96, 128):
        cost = _cdiv(_cdiv(n, c) * row_tiles * branches, cus) * c
        if best_cost is None or cost < best_cost:
            best, best_cost = c, cost
    return best


def paths(F, Tp, B, cus):
    """Which kernel each GEMM of a forward takes under each debug mode."""
    sk_ch, sk_f, r64 = splitk_runs(CH, Tp, B, cus), splitk_runs(F, Tp, B, cus), rows64_runs(F, Tp, B, cus)
    rt = _cdiv(Tp, 128) * B
    return {"mode1": {"conv1x1": "splitk" if sk_ch else "rows128", "sconv": "splitk" if sk_f else ("rows64" if r64 else "rows128"),
                      "linear": "splitk" if sk_f else "rows128"},
            "mode2": {"conv1x1": "rows128", "sconv": "rows64" if r64 else "rows128", "linear": "rows128"},
            "mode3": {"conv1x1": "rows128", "sconv": "rows128", "linear": "rows128"},
            "mode0": {"conv1x1": f"general{pick_bn(CH, rt, cus)}", "sconv": f"general{pick_bn(F, rt, cus)}",
                      "linear": f"general{pick_bn(F, rt, cus)}"}}


# ------------------------------------------------------------------------------------------------ one case
_MODELS = {}


def _model(profile, F, fresh=False):
    """One model per (weight profile, bin count), shared by the cases that leave its planner alone."""
    key = (profile, F)
    if fresh or key not in _MODELS:
        args = dict(DEFAULT_MODEL_ARGS, num_freqs=F)
        sd = make_state_dict(21, profile, num_freqs=F)
        m = FullSubNet_Plus(**args)
        m.load_state_dict(sd, strict=True)
        m = m.to("cuda").eval()
        m.batch_mode = "full"
        if fresh:
            return m, sd, args
        _MODELS[key] = (m, sd, args)
    return _MODELS[key]


def _oracle(sd, args, pool, lengths, dtype):
    """-> rows[i] = {tag: [F, lengths[i] + LA]} of pool clip i alone (one oracle call per distinct length, tests/_util.py oracle_rows)."""
    def fn(*x):
        st = oracle_stages(sd, x, args, dtype)
        return torch.stack([st[tag] for tag in STAGE_TAGS], dim=1)
    return [{tag: r[0, k].numpy() for k, tag in enumerate(STAGE_TAGS)} for r in oracle_rows(fn, pool, lengths)]


def _forward_stages(m, pool, lengths, B, ragged, seed):
    """The pool batch by batch (the last batch filled up from the start of the pool) -> rows[i] = {tag: [F, lengths[i] + LA]}."""
    n, T = len(lengths), pool[0].shape[-1]
    rows = [None] * n
    for k in range(0, n, B):
        idx = [(k + i) % n for i in range(B)]
        lens = [lengths[i] for i in idx]
        if ragged:
            ins = garbage_tails([t[idx] for t in pool], lens, seed + k)
            m(*[t.cuda() for t in ins], lengths=lens)
        else:
            assert lens == [T] * B
            m(*[t[idx].cuda() for t in pool])
        m.check_errors()
        st = {tag: m.read_stage(tag, B, T).permute(0, 2, 1).numpy() for tag in STAGE_TAGS}        # [B, F, T + LA]
        for j, i in enumerate(idx):
            if rows[i] is None:
                rows[i] = {tag: st[tag][j, :, :lens[j] + LA].copy() for tag in STAGE_TAGS}
    return rows


def _fb_bits(rows):
    return np.concatenate([r[tag].ravel() for r in rows for tag in STAGE_TAGS if tag.startswith("fb_")])


def run_case(name, profile, B, T, *, F=257, lengths=None, cus=None, seed=0, reference=None):
    """Forwards under modes 1, 0, 2, 3; every plane of every stage against the float64 oracle within min(K * e32, cap); the kernel path
    of every mode by formula and by bit (in)equality of the fb_* buffers.  Returns the restated paths for the case's own assertions.
    reference: None, or (pool, float64 rows, float32 rows) of `lengths` computed by the caller."""
    ragged = lengths is not None
    if not ragged:
        lengths = [T] * B
    m, sd, args = _model(profile, F, fresh=cus is not None)
    real_cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus is not None:
        m.debug_set_num_cus(cus)
        m.debug_set_lstm_coop(0)             # the hook re-plans the sub-band LSTM too: keep it on the row-tile kernels (test_forward_with_valu_rows)
    if reference is None:
        pool = make_spec(len(lengths), T, 4000 + seed, F)
        want, want32 = (_oracle(sd, args, pool, lengths, dt) for dt in (torch.float64, torch.float32))
    else:
        pool, want, want32 = reference
    assert len(want) == len(lengths) and all(t.shape[0] == len(lengths) and t.shape[-1] == T for t in pool)
    # the yardstick, plane by plane: the float32 oracle's own error on clip i's plane of stage `tag`
    e32 = [{tag: plane_errs(w32[tag][None], w[tag][None])[0][0] for tag in STAGE_TAGS} for w, w32 in zip(want, want32)]
    got, failures = {}, []
    entry = {"lengths": lengths if ragged else None,
             "e32_min_max": {g: [f(e[tag] for e in e32 for tag in STAGE_TAGS if tag.startswith(g)) for f in (min, max)] for g in STAGE_CAPS}}
    try:
        for mode in (1, 0, 2, 3):
            m.debug_set_gemm_dma(mode)
            got[mode] = _forward_stages(m, pool, lengths, B, ragged, 9)
            worst = {g: {"ratio": 0.0} for g in STAGE_CAPS}
            for i, (g_i, w_i) in enumerate(zip(got[mode], want)):
                for tag in STAGE_TAGS:
                    grp = tag[:tag.index("_")]
                    (err,), (where,) = plane_errs(g_i[tag][None], w_i[tag][None])
                    ratio, bound = err / e32[i][tag], min(K * e32[i][tag], STAGE_CAPS[grp])
                    if ratio >= worst[grp]["ratio"]:
                        worst[grp] = {"ratio": ratio, "err": err, "e32": e32[i][tag], "tag": tag, "clip": i, "length": lengths[i],
                                      "bin_frame": list(where)}
                    if not err <= bound:
                        failures.append((mode, tag, i, lengths[i], where, err, bound, ratio))
            entry[f"mode{mode}"] = worst
            print(f"{name} mode {mode}: " + ", ".join(f"{g} worst {w['ratio']:.2f} x e32 ({w['err']:.2e} on {w['tag']} of clip {w['clip']}, "
                                                       f"length {w['length']}, at {w['bin_frame']})" for g, w in worst.items()))
    finally:
        m.debug_set_gemm_dma(1)
    Tp = T + LA
    p = paths(F, Tp, B, cus or real_cus)
    entry["paths"] = p
    bits = {mode: _fb_bits(rows) for mode, rows in got.items()}
    entry["bit_equal"] = {f"{a}=={b}": bool(np.array_equal(bits[a], bits[b])) for a, b in ((0, 1), (1, 2), (2, 3))}
    _record(name, entry)
    assert not failures, (name, "(mode, tag, clip, length, (bin, frame), err, bound, err / e32)", failures[:12])
    # the paths really ran: another kernel (another k order, the folded GroupNorm) gives other bits, the same kernel the same bits
    assert not np.array_equal(bits[0], bits[1]), "mode 0 (general kernel) == mode 1"
    assert np.array_equal(bits[1], bits[2]) == (p["mode1"] == p["mode2"]), (p["mode1"], p["mode2"])
    assert np.array_equal(bits[2], bits[3]) == (p["mode2"] == p["mode3"]), (p["mode2"], p["mode3"])
    return p


# ------------------------------------------------------------------------------------------------ 1. uniform batches
# Tp = T + look_ahead one below, at and one above each of the row-tile heights 32 (split-K) / 64 / 128 and 256, and the shortest legal
# clip (T = 8: the dilation-9 taps of blocks 3 and 7 reach exactly one real frame on each side; two DW_ROWS chunks).  Row tiles never
# straddle utterances, so the last tile of every plane is ragged; 3 B row-tile units are no multiple of the 8 xcd_grid pads to.
UNIFORM_TP = (10, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)


@pytest.mark.parametrize("Tp", UNIFORM_TP)
@pytest.mark.parametrize("B,profile", [(1, "default"), (3, "harsh")])
def test_uniform_batches(B, profile, Tp):
    p = run_case(f"uniform_{profile}_B{B}_Tp{Tp}", profile, B, Tp - LA, seed=Tp)
    # an MI355X at these sizes: split-K everywhere under mode 1 (at most 8 x 9 x 3 x 3 = 648 workgroups on 256 CUs), the 64-row sconv
    # kernel under mode 2, the 128-row kernel alone under mode 3 and the general kernel under mode 0: all four kernels on every shape
    assert set(p["mode1"].values()) == {"splitk"} and p["mode2"]["sconv"] == "rows64", p


# ------------------------------------------------------------------------------------------------ 2. ragged batches
RAGGED_EDGES = (8, 32, 64, 128, 256)
_RAGGED = {}


def _ragged_reference(profile):
    """One pool of 260-frame clips per weight profile, one clip per length of either buffer, and its oracle rows (float64, float32): a
    clip cut at its length is the same clip on the 130-frame and on the 260-frame buffer, so both cases share the reference."""
    if profile not in _RAGGED:
        min_len = max(DEFAULT_MODEL_ARGS["kersize"]) - LA
        lengths = sorted(set(edge_lengths(130, LA, min_len, edges=RAGGED_EDGES)) | set(edge_lengths(260, LA, min_len, edges=RAGGED_EDGES)))
        _, sd, args = _model(profile, 257)
        pool = make_spec(len(lengths), 260, 4260)
        _RAGGED[profile] = (lengths, pool) + tuple(_oracle(sd, args, pool, lengths, dt) for dt in (torch.float64, torch.float32))
    return _RAGGED[profile]


@pytest.mark.parametrize("T", [130, 260])
@pytest.mark.parametrize("profile", ["default", "harsh"])
def test_ragged_batches(profile, T):
    """B = 4 with lengths[b] + look_ahead one below, at and one above 8 / 32 / 64 / 128 / 256: tpb[utt] at the sub-tile, row-tile and
    DW_ROWS chunk boundaries while the buffer's Tp is elsewhere.  "harsh" stresses the cancellation in the folded GroupNorm,
    r * (sum a g W) + c1 - r * m * c2."""
    lengths = edge_lengths(T, LA, max(DEFAULT_MODEL_ARGS["kersize"]) - LA, edges=RAGGED_EDGES)
    assert lengths[0] == 8 and lengths[-1] == T and {e + d - LA for e in RAGGED_EDGES[1:] for d in (-1, 0, 1) if e + d - LA <= T} <= set(lengths)
    all_lengths, pool, want, want32 = _ragged_reference(profile)
    idx = [all_lengths.index(n) for n in lengths]
    reference = ([t[idx][..., :T] for t in pool], [want[i] for i in idx], [want32[i] for i in idx])
    run_case(f"ragged_{profile}_B4_T{T}", profile, 4, T, lengths=lengths, reference=reference)


# ------------------------------------------------------------------------------------------------ 3. other bin counts
@pytest.mark.parametrize("Tp", [33, 129])
@pytest.mark.parametrize("F", [161, 521])
def test_other_bin_counts(F, Tp):
    """3 and 9 column tiles, another k tail of conv1x1 and the Linear (161 = 10 * 16 + 1, 521 = 32 * 16 + 9).  N % 64 != 1: the 64-row
    kernel must not run, so modes 2 and 3 are the same launches (run_case asserts their bits equal through the restated paths)."""
    p = run_case(f"bins{F}_B2_Tp{Tp}", "harsh", 2, Tp - LA, F=F, seed=F + Tp)
    assert not rows64_runs(F, Tp, 2, 1) and p["mode2"] == p["mode3"] and p["mode2"]["sconv"] == "rows128", p


# ------------------------------------------------------------------------------------------------ 4. small-chip dispatch
def test_mixed_launch_on_a_pretend_8_cu_chip():
    """Mode 1 on 8 pretend CUs, B = 1, Tp = 65: the split-K kernel is refused for conv1x1 (8 x 3 x 3 = 72 workgroups > 48) and taken
    for the sconv and the Linear (45 <= 48) - the mix a 256-CU chip only reaches at large batches."""
    assert 8 * _cdiv(65, 32) * 3 == 72 and 5 * _cdiv(65, 32) * 3 == 45 and 6 * 8 == 48
    p = run_case("cus8_B1_Tp65_mixed", "harsh", 1, 65 - LA, cus=8, seed=65)
    assert p["mode1"] == {"conv1x1": "rows128", "sconv": "splitk", "linear": "splitk"}, p
    assert p["mode2"]["sconv"] == "rows64", p


def test_general_kernel_96_wide_tiles_on_a_pretend_9_cu_chip():
    """Mode 0 on 9 pretend CUs, B = 1, one ragged 128-row tile: pick_bn gives 96 for N = 257 (3 column tiles x 3 branches = one round
    of 9, against two rounds of 64-wide tiles), whose last column tile holds 257 - 192 = 65 columns; conv1x1 (N = 512) stays at 64.
    (128 is out of reach for N = 257 and N = 512 at any CU count: 96 has the same tile count for 257, and
    ceil(2 x) <= 2 ceil(x) rules it out for 512.)"""
    assert pick_bn(257, 1, 9) == 96 and pick_bn(512, 1, 9) == 64 and pick_bn(257, 1, 256) == 64
    for cus in range(1, 513):
        for rt in (1, 2, 3, 9):
            assert pick_bn(257, rt, cus) != 128 and pick_bn(512, rt, cus) != 128
    p = run_case("cus9_B1_Tp100_bn96", "harsh", 1, 100 - LA, cus=9, seed=100)
    assert p["mode0"] == {"conv1x1": "general64", "sconv": "general96", "linear": "general96"}, p

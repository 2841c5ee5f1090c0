"""GPU parity tests (run on an MI355X through gpurun): the HIP forward, called through the C ABI,
against (a) the golden vectors the REAL reference produced (tests/golden, oracle/make_golden.py) and
(b) the torch-CPU oracle restatement (oracle/fsnp_torch.py) at BASELINE.json sizes.

Tolerance: BASELINE.json's north_star states "within 1e-3 rel on fp32"; rel = max|hip - ref| / max|ref|.
Every test asserts rel < 1e-3 (TOL) and records the measured value in gpurun_out/parity_report.json;
tighter bounds are asserted where the kernels are expected to do much better.
"""
import json
import os
import time

import numpy as np
import pytest
import torch

from fullsubnet_plus_amd import FullSubNet_Plus
from oracle import fsnp_torch
from oracle.make_golden import make_spec
from oracle.ref_loader import DEFAULT_MODEL_ARGS
from oracle.weights import make_inputs, make_state_dict
from tests._util import Golden, golden_names, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}


def _record(name, _report=REPORT, _file="parity_report.json", **kw):
    """_report / _file: another test module's report dict and its file name in the same directory (tests/test_gpu_stages.py)."""
    _report[name] = {k: (float(v) if isinstance(v, (float, np.floating)) else v) for k, v in kw.items()}
    out = os.path.join(ROOT, "gpurun_out")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, _file), "w") as f:
        json.dump(_report, f, indent=1, sort_keys=True)


torch.set_num_threads(min(16, os.cpu_count() or 1))   # the CPU oracle collapses when oversubscribed


def _model(args, sd, mode="parity"):
    m = FullSubNet_Plus(**args)
    m.load_state_dict(sd, strict=True)
    m = m.to("cuda").eval()
    m.batch_mode = mode
    return m


def _cuda(ts):
    """Move to the GPU keeping the (non-contiguous, stft-like) strides."""
    out = []
    for t in ts:
        g = torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device="cuda")
        g.copy_(t)
        out.append(g)
    return out


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile,n,steps", [("default", 70, 12), ("harsh", 33, 40), ("default", 256, 6), ("harsh", 96, 260)])
def test_lstm2_fc_dense_vs_oracle(profile, n, steps):
    """Fused LSTM kernel alone on dense inputs (ragged tile counts) vs torch.lstm + linear.  ("harsh", 96, 260): cell states
    reach |c| ~ 40-60 - the packed cell update (lstm_common.h) forms sigmoid * tanh with ONE reciprocal of the product of
    both denominators, which must not overflow next to a saturated tanh (a clamp at 2^126 instead of 2^64 returned h = 0
    there: caught at B = 32 x 2 s in round 2, now pinned here)."""
    sd = make_state_dict(3, profile)
    m = _model(DEFAULT_MODEL_ARGS, sd)
    m.debug_set_lstm_coop(0)
    rng = np.random.Generator(np.random.PCG64(1234 + n))
    x = torch.from_numpy(rng.standard_normal((n, 34, steps)).astype(np.float32))
    want = fsnp_torch.lstm2_fc(x, sd).numpy()
    got = m.lstm2_fc(x.cuda()).cpu().numpy()
    err = rel_err(got, want)
    per_step = np.abs(got - want).max(axis=(0, 1)) / np.abs(want).max()
    per_row = np.abs(got - want).max(axis=(1, 2)) / np.abs(want).max()
    _record(f"lstm_dense_{profile}_{n}x{steps}", rel=err, first_steps=per_step[:4].tolist(),
            worst_rows=np.argsort(-per_row)[:8].tolist(), worst_row_err=float(per_row.max()))
    assert err < 2e-5, (err, per_step[:6], np.argsort(-per_row)[:8])


@pytest.mark.parametrize("n,cus,steps", [(66, 2, 9), (67, 2, 9), (70, 2, 9), (200, 2, 5), (257, 8, 7)])
def test_lstm2_fc_valu_rows_and_rounds(n, cus, steps):
    """Tiles with 1/2/4 extra VALU rows and several rounds (planner driven by a fake CU count)."""
    sd = make_state_dict(5, "harsh")
    m = _model(DEFAULT_MODEL_ARGS, sd)
    m.debug_set_num_cus(cus)
    m.debug_set_lstm_coop(0)
    rng = np.random.Generator(np.random.PCG64(99 + n))
    x = torch.from_numpy(rng.standard_normal((n, 34, steps)).astype(np.float32))
    want = fsnp_torch.lstm2_fc(x, sd).numpy()
    got = m.lstm2_fc(x.cuda()).cpu().numpy()
    per_row = np.abs(got - want).max(axis=(1, 2)) / np.abs(want).max()
    _record(f"lstm_valu_rows_{n}_cus{cus}", rel=float(per_row.max()), worst_rows=np.argsort(-per_row)[:6].tolist())
    assert per_row.max() < 2e-5, (per_row.max(), np.argsort(-per_row)[:8])


@pytest.mark.parametrize("n,steps", [(20, 5), (70, 33), (257, 128), (672, 9), (1000, 17), (1300, 12), (1376, 7),
                                     (1400, 9), (2700, 21), (2750, 8), (4096, 5), (4112, 14), (5440, 6)])
def test_lstm2_fc_cooperative_kernel(n, steps):
    """Column-split kernels: csrc/lstm_coop.hip (<= 42 row tiles: 6..48 workgroups share each 32-row tile, K split over
    the waves) and csrc/lstm_coopn.hip (43..170 row tiles: n = 1400..5440 here - 3 workgroups share 1 or 2 row tiles,
    incl. an odd tile count whose last group owns one tile; 1376 / 4096 / 4112: a full K-split launch plus a tiny one).  h is exchanged through global memory with one agent-scope
    barrier per step; results must match the oracle and the row-tile kernel."""
    sd = make_state_dict(9, "harsh")
    m = _model(DEFAULT_MODEL_ARGS, sd)
    rng = np.random.Generator(np.random.PCG64(77 + n))
    x = torch.from_numpy(rng.standard_normal((n, 34, steps)).astype(np.float32))
    want = fsnp_torch.lstm2_fc(x, sd).numpy()
    m.debug_set_lstm_coop(1)
    got = m.lstm2_fc(x.cuda()).cpu().numpy()
    m.check_errors()
    per_step = np.abs(got - want).max(axis=(0, 1)) / np.abs(want).max()
    _record(f"lstm_coop_{n}x{steps}", rel=float(per_step.max()), first_steps=per_step[:4].tolist())
    assert per_step.max() < 2e-5, (per_step.max(), per_step[:6])
    for _ in range(3):                                     # repeat: barriers / parity buffers must be re-entrant
        again = m.lstm2_fc(x.cuda()).cpu().numpy()
        assert np.array_equal(again, got)
    m.debug_set_lstm_coop(0)
    tile = m.lstm2_fc(x.cuda()).cpu().numpy()
    assert rel_err(tile, want) < 2e-5


@pytest.mark.parametrize("seq", ["LSTM", "GRU"])
@pytest.mark.parametrize("n,steps", [(7, 1), (32, 2), (40, 3), (257, 41), (514, 9), (1285, 6), (1344, 5)])
def test_layer_skewed_k_split_equals_serial_schedule(n, steps, seq):
    """csrc/lstm_coop.hip: lstm2_coop_skew_kernel runs layer 0 of step t+1 before layer 1 of step t (two arrival counters, three
    h0 images) so that every inter-workgroup wait is for an arrival one phase old.  Same arithmetic, same summation order:
    bit-identical to the serial schedule, for 1, 2, 3 and many steps, LSTM and GRU cells, every K-split width."""
    args = {**DEFAULT_MODEL_ARGS, "sequence_model": seq}
    sd = make_state_dict(9, "harsh", sequence_model=seq)
    m = _model(args, sd)
    rng = np.random.Generator(np.random.PCG64(321 + n))
    x = torch.from_numpy(rng.standard_normal((n, 34, steps)).astype(np.float32)).cuda()
    m.lstm2_fc(x[:1])
    m.debug_set_costs(None, 1)
    ksplit_only = m.planner_costs_raw()[:19]  # both runs on the same plan: the built-in table minus the half-tile ping-pong kernel and the
    m.debug_set_lstm_coop(2)                  # wave-owned split, which sum K in another order
    m.debug_set_costs(ksplit_only, 1)
    serial = m.lstm2_fc(x).cpu().numpy()
    m.check_errors()
    m.debug_set_lstm_coop(1)
    m.debug_set_costs(ksplit_only, 1)
    assert all(c["kernel"].startswith("lstm2_coop_kernel") for c in m.describe_plan(1))
    skew = m.lstm2_fc(x).cpu().numpy()       # (the skewed schedule is used from 16 units per workgroup up: n >= 257 here)
    m.check_errors()
    want = fsnp_torch.lstm2_fc(x.cpu(), sd).numpy()
    assert rel_err(skew, want) < 2e-5
    assert np.array_equal(skew, serial)
    for _ in range(3):
        assert np.array_equal(m.lstm2_fc(x).cpu().numpy(), skew)


# K split at 8 units cheap (a full launch and one tile), everything else priced out
_SERIAL_8_UNITS_COSTS = [5.0, 900.0] + [900.0] * 6 + [900.0] * 4 + [900.0, 0.11] + [5.0, 900.0, 900.0, 900.0] + [900.0]      # (19 values: the other launch shapes are priced out)


def _hp_only_costs():
    """A cost table (fsnp_get_costs layout) under which every column-split launch is the half-tile ping-pong kernel."""
    return [900.0] * 12 + [900.0, 0.11] + [900.0] * 4 + [900.0] + [5.0, 5.0]


def _coopw_only_costs(units):
    """A cost table under which every column-split launch is the wave-owned split at `units` (32 / 64 / 96) units per workgroup."""
    w = [5.0 if 32 * (i + 1) == units else 900.0 for i in range(2)]
    w96 = [5.0, 5.0] if units == 96 else [900.0, 900.0]
    return [900.0] * 12 + [900.0, 0.11] + [900.0] * 4 + [900.0] + [900.0, 900.0] + w + w + w96


@pytest.mark.parametrize("n,steps,hidden,fbn", [(1, 1, 384, 0), (16, 2, 384, 0), (17, 3, 384, 0), (32, 40, 384, 0), (33, 5, 384, 0), (257, 41, 384, 0),
                                                (300, 7, 384, 0), (320, 128, 384, 0), (500, 9, 384, 0), (48, 300, 384, 0), (257, 33, 256, 0), (40, 2, 256, 0),
                                                (257, 9, 384, 2), (40, 3, 256, 3)])
def test_half_tile_ping_pong_kernel_vs_oracle(n, steps, hidden, fbn):
    """csrc/lstm_hp.hip: 16 hidden units per workgroup (24 workgroups per row tile, one XCD), the four waves split the GATES over
    the whole K (v_mfma_f32_16x16x4_f32, weights resident, no partial tiles to reduce), every row tile worked on as two half
    tiles of 16 sequences in turn (the hand-off of one half is in flight while the other computes), operands by LDS DMA, fused
    two-layer phase.  The 16x16x4 MFMA sums K in another order than the 32x32x2 kernels: same oracle tolerance as every other
    recurrent kernel, bitwise repeatable; 1 ... 300 steps, ragged tiles (second half empty / one row), two launches (500), sub-band
    inputs of 46 / 52 features (fb_num_neighbors 2 / 3: the K = 64 instantiations)."""
    args = {**DEFAULT_MODEL_ARGS, "sb_model_hidden_size": hidden, "fb_num_neighbors": fbn}
    sd = make_state_dict(3, "harsh", sb_hidden=hidden, fb_num_neighbors=fbn)
    m = _model(args, sd)
    rng = np.random.Generator(np.random.PCG64(977 + n + steps))
    x = torch.from_numpy(rng.standard_normal((n, 31 + 3 * (2 * fbn + 1), steps)).astype(np.float32)).cuda()
    m.lstm2_fc(x[:1])
    m.debug_set_lstm_coop(4)
    m.debug_set_costs(_hp_only_costs(), 1)
    assert all(c["kernel"].startswith(("lstm2_coop_hp_kernel", "lstm2_coop_hpw_kernel")) for c in m.describe_plan(1)), m.describe_plan(1)
    got = m.lstm2_fc(x).cpu().numpy()
    m.check_errors()
    want = fsnp_torch.lstm2_fc(x.cpu(), sd).numpy()
    assert rel_err(got, want) < 2e-5, rel_err(got, want)
    for _ in range(3):
        assert np.array_equal(m.lstm2_fc(x).cpu().numpy(), got)
    m.check_errors()


@pytest.mark.parametrize("units,n,steps,fbn", [(32, 1, 1, 0), (32, 33, 2, 0), (32, 514, 41, 0), (32, 672, 3, 0), (32, 700, 9, 0),
                                               (64, 40, 1, 0), (64, 17, 2, 0), (64, 1285, 33, 0), (64, 1344, 7, 0), (64, 1400, 5, 0),
                                               (64, 2056, 128, 0), (32, 514, 9, 2), (64, 300, 5, 3), (64, 96, 300, 0),
                                               (96, 1, 1, 0), (96, 2048, 41, 0), (96, 2056, 128, 0), (96, 2100, 7, 0), (96, 1799, 9, 2), (96, 70, 300, 0)])
def test_wave_owned_column_split_kernel_vs_oracle(units, n, steps, fbn):
    """csrc/lstm_coopw.hip: a wave owns 8 / 16 hidden units (1 / 2 gate-interleaved accumulator tiles) over the whole K, 12 / 6
    workgroups share a row tile, layer-skewed schedule with the waves as participants, no workgroup barrier in the time loop, x in
    registers, h out as one 16-byte store per tile.  1 ... 300 steps, ragged tiles, one tile, a full launch (672 / 1344 sequences),
    a full launch + a second one (700 / 1400), B = 8's 2056 sequences at 128 steps (two launches), sub-band inputs of 46 / 52
    features (the K = 64 instantiations).  Same oracle tolerance as every other recurrent kernel, bitwise repeatable."""
    args = {**DEFAULT_MODEL_ARGS, "fb_num_neighbors": fbn}
    sd = make_state_dict(3, "harsh", fb_num_neighbors=fbn)
    m = _model(args, sd)
    rng = np.random.Generator(np.random.PCG64(4177 + n + steps))
    x = torch.from_numpy(rng.standard_normal((n, 31 + 3 * (2 * fbn + 1), steps)).astype(np.float32)).cuda()
    m.lstm2_fc(x[:1])
    m.debug_set_costs(_coopw_only_costs(units), 1)
    assert all(c["kernel"].startswith("lstm2_coopw_kernel") for c in m.describe_plan(1)), m.describe_plan(1)
    got = m.lstm2_fc(x).cpu().numpy()
    m.check_errors()
    want = fsnp_torch.lstm2_fc(x.cpu(), sd).numpy()
    per_step = np.abs(got - want).max(axis=(0, 1)) / np.abs(want).max()
    _record(f"lstm_coopw_{units}_{n}x{steps}_fbn{fbn}", rel=float(per_step.max()), first_steps=per_step[:4].tolist())
    assert per_step.max() < 2e-5, (per_step.max(), per_step[:6])
    for _ in range(3):
        assert np.array_equal(m.lstm2_fc(x).cpu().numpy(), got)
    m.check_errors()


@pytest.mark.parametrize("seq,hidden,fbn", [("LSTM", 320, 0), ("GRU", 190, 0), ("LSTM", 384, 6), ("LSTM", 1030, 0)])
def test_generic_recurrent_kernel_dense_vs_oracle(seq, hidden, fbn):
    """csrc/lstm_generic.hip: sizes without a tuned (MFMA) instantiation - any sb_model_hidden_size, more than 64 sub-band
    features - run on the runtime-sized fp32-FMA kernel instead of being rejected (the reference builds nn.LSTM / nn.GRU for
    any sizes, sequence_model.py:31-46).  Fused recurrent model + Linear alone on dense inputs, 1 / 2 / 4 / 8 sequences per
    workgroup (by sequence count), against torch.lstm / torch.gru + linear."""
    args = {**DEFAULT_MODEL_ARGS, "sequence_model": seq, "sb_model_hidden_size": hidden, "fb_num_neighbors": fbn}
    sd = make_state_dict(77, "harsh", sequence_model=seq, sb_hidden=hidden, fb_num_neighbors=fbn)
    m = _model(args, sd)
    nin = 31 + 3 * (2 * fbn + 1)
    for n, steps in ((3, 7), (300, 9), (700, 6), (1500, 5), (2500, 4)):
        if hidden > 1000 and n > 300:
            continue
        rng = np.random.Generator(np.random.PCG64(5 * n + hidden))
        x = torch.from_numpy(rng.standard_normal((n, nin, steps)).astype(np.float32))
        want = fsnp_torch.lstm2_fc(x, sd).numpy()
        got = m.lstm2_fc(x.cuda()).cpu().numpy()
        m.check_errors()
        assert all(c["kernel"].startswith("lstm2_generic_kernel") for c in m.describe_plan(1))
        err = rel_err(got, want)
        _record(f"generic_{seq}_h{hidden}_fbn{fbn}_{n}x{steps}", rel=err)
        assert err < 2e-5, (n, steps, err)
        assert np.array_equal(m.lstm2_fc(x.cuda()).cpu().numpy(), got)


@pytest.mark.parametrize("seq", ["LSTM", "GRU"])
@pytest.mark.parametrize("hidden", [256, 512])
def test_other_hidden_sizes_on_every_kernel(hidden, seq):
    """sb_model_hidden_size = 256 / 512 (fullsubnet_plus.py:25, sequence_model.py:31-46): the column-split kernels are
    instantiated for both, the one-tile-per-CU LSTM kernel for 256; 70 sequences run K-split, 2100 the three-way split,
    9000 a chip-filling round of the one-tile-per-CU kernel + remainder (LSTM, 256) or consecutive column-split launches."""
    args = {**DEFAULT_MODEL_ARGS, "sequence_model": seq, "sb_model_hidden_size": hidden}
    sd = make_state_dict(41, "harsh", sequence_model=seq, sb_hidden=hidden)
    m = _model(args, sd)
    for n, steps in ((70, 9), (2100, 5), (9000, 3)):
        rng = np.random.Generator(np.random.PCG64(17 * n + hidden))
        x = torch.from_numpy(rng.standard_normal((n, 34, steps)).astype(np.float32))
        want = fsnp_torch.lstm2_fc(x, sd).numpy()
        got = m.lstm2_fc(x.cuda()).cpu().numpy()
        m.check_errors()
        err = rel_err(got, want)
        _record(f"hidden{hidden}_{seq}_{n}x{steps}", rel=err)
        assert err < 2e-5, (n, err)
        assert np.array_equal(m.lstm2_fc(x.cuda()).cpu().numpy(), got)
    plan = [c["kernel"] for c in m.describe_plan(35)]       # 8995 sequences
    assert any("one 32-row tile per CU" in k for k in plan) == (hidden == 256 and seq == "LSTM")
    with pytest.raises(RuntimeError, match="384 only|LSTM sub-band model only"):
        m.set_precision("bf16_ih")


@pytest.mark.parametrize("n,steps", [(16, 3), (3855, 6), (4096, 9), (4112, 5), (4500, 4)])
def test_half_tile_kernel(n, steps):
    """csrc/lstm16.hip: the one-tile-per-CU decomposition on 16-row tiles (v_mfma_f32_16x16x4_f32), planned where one round of
    256 half tiles beats the column-split launches (3700...4096 sequences, e.g. the reference's literal drop-band call at
    B = 32: 4096 sequences) and as a full round + column-split remainder just above; ragged last tile, 16 sequences alone
    (forced through the cost table)."""
    sd = make_state_dict(12, "harsh")
    m = _model(DEFAULT_MODEL_ARGS, sd)
    rng = np.random.Generator(np.random.PCG64(1000 + n))
    x = torch.from_numpy(rng.standard_normal((n, 34, steps)).astype(np.float32))
    want = fsnp_torch.lstm2_fc(x, sd).numpy()
    m.lstm2_fc(x[:1].cuda())
    if n < 3000:                                   # make the half-tile kernel the cheapest shape for any size
        m.debug_set_costs([900] * 8 + [900] * 4 + [900, 0.11] + [900] * 4 + [10], 1)
    plan = m.describe_plan(1)                      # (the plan of lstm2_fc depends on n, not on this)
    got = m.lstm2_fc(x.cuda()).cpu().numpy()
    err = rel_err(got, want)
    _record(f"lstm16_{n}x{steps}", rel=err)
    assert err < 2e-5, err
    assert np.array_equal(m.lstm2_fc(x.cuda()).cpu().numpy(), got)
    m.debug_set_lstm_coop(0)
    assert rel_err(m.lstm2_fc(x.cuda()).cpu().numpy(), got) < 1e-5      # the 32-row kernel: same rows, other summation order
    del plan


def test_parity_b32_runs_on_half_tiles(b32):
    sd, (mag, real, imag), m, full = b32
    m.batch_mode = "parity"
    plan = m.describe_plan(32, parity=True)
    m.batch_mode = "full"
    assert plan[0]["kernel"].startswith("lstm2_fc16_kernel") and plan[0]["sequences"] == 4096 and len(plan) == 1, plan


CHEAP_TWO_PER_CU = [9, 12, 19, 25, 29, 38, 55, 70, 76, 95, 151, 190, 208, 0.11, 9, 19, 29, 55, 1000]   # a table in which two workgroups per CU pay


@pytest.mark.parametrize("n,steps", [(257, 40), (514, 20), (1285, 12), (2700, 9), (4112, 7), (5440, 6), (8000, 5), (10870, 4)])
def test_column_split_two_workgroups_per_cu(n, steps):
    """The planner may put TWO column-split workgroups on a CU (their hand-off stalls overlap: two independent row tiles share
    the CU's matrix pipes) when the kernels fit twice - 257 sequences then run at 8 units per workgroup (432 workgroups),
    129 tiles as one launch of 129 groups, 340 tiles as 170 groups of two.  Pinned here with a cost table that makes it pay;
    the result must equal the oracle (as the one-per-CU plan of round 1 does) and itself, bitwise, on repetition."""
    sd = make_state_dict(9, "harsh")
    m = _model(DEFAULT_MODEL_ARGS, sd)
    rng = np.random.Generator(np.random.PCG64(99 + n))
    x = torch.from_numpy(rng.standard_normal((n, 34, steps)).astype(np.float32)).cuda()
    m.lstm2_fc(x[:4])                                     # creates the handle, commits the weights
    m.debug_set_costs(None, 1)
    one = m.lstm2_fc(x).cpu().numpy()
    m.check_errors()
    m.debug_set_costs(CHEAP_TWO_PER_CU, 2)
    two = m.lstm2_fc(x).cpu().numpy()
    m.check_errors()
    want = fsnp_torch.lstm2_fc(x.cpu(), sd).numpy()
    _record(f"lstm_two_per_cu_{n}x{steps}", rel=rel_err(two, want), vs_one_per_cu=rel_err(two, one))
    assert rel_err(two, want) < 2e-5 and rel_err(one, want) < 2e-5
    for _ in range(3):
        assert np.array_equal(m.lstm2_fc(x).cpu().numpy(), two)


def test_planner_cost_table_has_not_drifted_from_the_kernels():
    """(Table = csrc/planner.cpp default_costs: round-3 measurements, after the arrival counters were padded.)  The planner minimises a built-in per-step cost table (fsnp.h: fsnp_get_costs).  fsnp_measure_costs times every launch
    shape on the device (two step counts, slope); the table must stay within 30 % of what the kernels really cost (box-to-box
    and clock-state spread is ~10 %), so a kernel change cannot silently mis-plan.  The measurement is kept in
    gpurun_out/planner_costs.json.  The B = 32 headline runs 8192 sequences on the one-tile-per-CU kernel first."""
    sd = make_state_dict(0, "default")
    m = _model(DEFAULT_MODEL_ARGS, sd, "full")
    m(*_cuda(make_spec(1, 12, 5)))
    table, got = m.planner_costs(), m.measure_costs()
    assert not table["calibrated"]
    with open(os.path.join(ROOT, "gpurun_out", "planner_costs.json"), "w") as f:
        json.dump({"built_in": table, "measured": got}, f, indent=1)
    pairs = [(table["ksplit_us"][u][k], got["ksplit_us"][u][k], f"ksplit {u} {k}") for u in (8, 16, 32, 64) for k in ("one_per_cu", "one_tile")]
    pairs += [(table["coopn_us"][r]["one_per_cu"], got["coopn_us"][r]["one_per_cu"], f"coopn {r}") for r in (1, 2)]
    pairs += [(table["rowtile_us"], got["rowtile_us"], "rowtile"), (table["rowtile16_us"], got["rowtile16_us"], "rowtile16")]
    pairs += [(table["halftile_pingpong_us"][k], got["halftile_pingpong_us"][k], f"half-tile ping-pong {k}") for k in ("one_tile", "full_launch")]
    for want, have, name in pairs:
        assert 0.7 * want < have < 1.3 * want, (name, want, have)
    plan = m.describe_plan(32)
    assert plan[0]["kernel"].startswith("lstm2_fc") and plan[0]["sequences"] == 8192
    gru = _model({**DEFAULT_MODEL_ARGS, "sequence_model": "GRU"}, make_state_dict(0, "default", sequence_model="GRU"), "full")
    gru(*_cuda(make_spec(1, 12, 5)))
    t2, g2 = gru.planner_costs(), gru.measure_costs()
    assert 0.7 * t2["rowtile_us"] < g2["rowtile_us"] < 1.3 * t2["rowtile_us"] and g2["rowtile_us"] < 0.85 * got["rowtile_us"]


def test_measured_cost_table_can_be_adopted(tmp_path):
    """FSNP_CALIBRATE=1 (fsnp.h): a handle adopts the cost table measured on the device at its first planning call.  Run in a
    subprocess (the switch is read at fsnp_create): the table is flagged calibrated, the headline plan is unchanged and the
    forward agrees with the default-table one."""
    import subprocess
    import sys
    code = (
        "import json, sys, torch\n"
        "sys.path.insert(0, %r)\n"
        "from fullsubnet_plus_amd import FullSubNet_Plus\n"
        "from fullsubnet_plus_amd.synthetic import DEFAULT_MODEL_ARGS, make_inputs, make_state_dict\n"
        "m = FullSubNet_Plus(**DEFAULT_MODEL_ARGS); m.load_state_dict(make_state_dict(0, 'default'), strict=True)\n"
        "m = m.to('cuda').eval(); m.batch_mode = 'full'\n"
        "out = m(*[t.cuda() for t in make_inputs(2, 0.5, 5)])\n"
        "c = m.planner_costs()\n"
        "print(json.dumps({'calibrated': c['calibrated'], 'rowtile': c['rowtile_us'], 'plan': [k['kernel'] for k in m.describe_plan(32)],\n"
        "                  'sum': float(out.double().sum())}))\n" % ROOT)
    res = {}
    for cal in ("0", "1"):
        env = dict(os.environ, FSNP_CALIBRATE=cal)
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res[cal] = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert not res["0"]["calibrated"] and res["1"]["calibrated"]
    assert 120.0 < res["1"]["rowtile"] < 320.0 and res["0"]["rowtile"] == 206.0       # (built-in: csrc/planner.cpp default_costs)
    assert res["1"]["plan"][0].startswith("lstm2_fc") and res["0"]["plan"] == res["1"]["plan"]
    assert abs(res["0"]["sum"] - res["1"]["sum"]) <= 1e-4 * abs(res["0"]["sum"])


@pytest.mark.parametrize("plan", ["default", "round4"])
def test_forward_b8_coopn_equals_row_tile_kernel_and_oracle(plan):
    """B = 8 (65 row tiles) through the whole forward, cumulative norm (per-row (m, d) tables) included: the default plan (round 6:
    64 row tiles on the wave-owned split at 96 units per workgroup + 1 on the K split) and the round-4 plan (lstm_coopn.hip, one row
    tile per group - what GRU models and the other hidden sizes still run)."""
    for norm in ("offline_laplace_norm", "cumulative_layer_norm"):
        args = {**DEFAULT_MODEL_ARGS, "norm_type": norm}
        sd = make_state_dict(21, "harsh")
        m = _model(args, sd, "full")
        cpu_in = make_spec(8, 22, 77)
        ins = _cuda(cpu_in)
        m.debug_set_lstm_coop(1)
        if plan == "round4":
            m.debug_set_costs(m.planner_costs_raw()[:19], 1)       # (neither the wave-owned split nor - round 6: cheap enough to lead - the half-tile ping-pong launches)
            assert [c["kernel"][:18] for c in m.describe_plan(8)] == ["lstm2_coopn_kernel"]
        else:
            assert [c["kernel"][:18] for c in m.describe_plan(8)] == ["lstm2_coopw_kernel", "lstm2_coop_kernel "]     # 64 tiles at 96 units + 1 K split
        a = m(*ins).cpu().numpy()
        m.check_errors()
        m.debug_set_lstm_coop(0)
        b = m(*ins).cpu().numpy()
        want = fsnp_torch.forward_full(sd, *[t[2:4] for t in cpu_in], norm_type=norm).numpy()
        _record(f"forward_b8_{plan}_{norm}", coop_vs_tile=rel_err(a, b), coop_vs_oracle=rel_err(a[2:4], want))
        assert rel_err(a, b) < 1e-5 and rel_err(a[2:4], want) < TOL


def test_forward_b1_cooperative_equals_row_tile_kernel():
    g = Golden("b1_2s_default")
    m = _model(g.args, g.state_dict())
    ins = _cuda(g.inputs())
    m.debug_set_lstm_coop(1)
    a = m(*ins).cpu().numpy()
    m.check_errors()
    m.debug_set_lstm_coop(0)
    b = m(*ins).cpu().numpy()
    _record("forward_b1_coop_vs_tile", rel=rel_err(a, b), coop_vs_ref=rel_err(a, g.arrays["out"]))
    assert rel_err(a, g.arrays["out"]) < TOL and rel_err(a, b) < 1e-5


@pytest.mark.parametrize("waves", [4, 12])
@pytest.mark.parametrize("n,cus,steps", [(70, 256, 11), (66, 2, 8), (67, 2, 8), (257, 7, 6)])
def test_lstm2_fc_wave_variants(waves, n, cus, steps):
    """Both workgroup shapes of the fused LSTM kernel (4 waves = 1/SIMD, 12 waves = 3/SIMD), with and without
    VALU rows, must agree with the oracle."""
    sd = make_state_dict(6, "default")
    m = _model(DEFAULT_MODEL_ARGS, sd)
    m.debug_set_num_cus(cus)
    m.debug_set_lstm_coop(0)
    m.debug_set_lstm_waves(waves)
    rng = np.random.Generator(np.random.PCG64(7 + n))
    x = torch.from_numpy(rng.standard_normal((n, 34, steps)).astype(np.float32))
    want = fsnp_torch.lstm2_fc(x, sd).numpy()
    got = m.lstm2_fc(x.cuda()).cpu().numpy()
    err = rel_err(got, want)
    _record(f"lstm_waves{waves}_{n}_cus{cus}", rel=err)
    assert err < 2e-5, err


@pytest.mark.parametrize("name", ["b1_t24_harsh_stages", "b1_t30_cum_layer", "b5_t16_default"])
def test_forward_with_valu_rows(name):
    """Whole forward with 33-row tiles (257 rows on a pretend 8-CU chip == B=32 on 256 CUs in miniature)."""
    g = Golden(name)
    m = _model(g.args, g.state_dict(), "parity")
    m.debug_set_num_cus(8 if g.meta["inp"]["B"] == 1 else 16)
    m.debug_set_lstm_coop(0)
    out = m(*_cuda(g.inputs())).cpu().numpy()
    err = rel_err(out, g.arrays["out"])
    _record(f"forward_valu_rows_{name}", rel_vs_ref32=err)
    assert err < TOL, err


def _with_stages():
    """Fixtures that carry the per-stage forward-hook captures (whatever their name)."""
    import numpy as _np
    out = []
    for n in golden_names():
        with _np.load(os.path.join(ROOT, "tests", "golden", n + ".npz")) as z:
            if "stage_att_mag" in z.files:
                out.append(n)
    return out


@pytest.mark.parametrize("name", _with_stages())
def test_stages_vs_reference(name):
    """Intermediate buffers (TSSE output, full-band outputs) vs forward-hook captures of the reference.  At B = 1, T = 24 every
    full-band GEMM is one ragged 32-row tile of the split-K kernel (tcn_gemm_sk_kernel) and nothing else: the other GEMM kernels, the
    tile edges, ragged batches and other bin counts are compared at these stages in tests/test_gpu_stages.py."""
    g = Golden(name)
    m = _model(g.args, g.state_dict())
    mag, real, imag = g.inputs()
    B, T = mag.shape[0], mag.shape[-1]
    m(*_cuda((mag, real, imag)))
    errs = {}
    for tag in ("att_mag", "att_real", "att_imag", "fb_mag", "fb_real", "fb_imag"):
        want = g.arrays["stage_" + tag]                       # [B,F,T']
        got = m.read_stage(tag, B, T).permute(0, 2, 1).numpy()
        errs[tag] = rel_err(got, want)
    _record(f"stages_{name}", **errs)
    for tag, e in errs.items():
        assert e < 2e-4, (tag, errs)


@pytest.mark.parametrize("name", golden_names())
def test_forward_vs_reference_golden(name):
    """The reference's literal batched call (drop_band active for B > 1) == batch_mode 'parity'."""
    g = Golden(name)
    m = _model(g.args, g.state_dict(), "parity")
    mag, real, imag = g.inputs()
    out = m(*_cuda((mag, real, imag))).cpu().numpy()[:, :, ::g.sub, :]
    want = g.arrays["out"]
    assert out.shape == want.shape
    err, err64 = rel_err(out, want), rel_err(out, g.arrays["out64"])
    ref_self = rel_err(want, g.arrays["out64"])
    _record(f"forward_{name}", rel_vs_ref32=err, rel_vs_ref64=err64, ref32_vs_ref64=ref_self)
    assert err < TOL, (err, err64, ref_self)
    if "full" in g.arrays:
        m.batch_mode = "full"
        full = m(*_cuda((mag, real, imag))).cpu().numpy()[:, :, ::g.sub, :]
        errf = rel_err(full, g.arrays["full"])
        _record(f"forward_full_{name}", rel_vs_ref32=errf)
        assert errf < TOL, errf


def test_enhance_epilogue_vs_oracle():
    """forward + decompress_cIRM + complex multiply (inferencer.py:143-157) in HIP."""
    sd = make_state_dict(21, "harsh")                       # harsh weights -> masks beyond +-9.9 exercise the clamp
    m = _model(DEFAULT_MODEL_ARGS, sd, "full")
    mag, real, imag = make_spec(2, 40, 5)
    X = torch.complex(real[:, 0], imag[:, 0])               # [B,F,T] with torch.stft strides
    Xg = torch.empty_strided(X.shape, X.stride(), dtype=X.dtype, device="cuda")
    Xg.copy_(X)
    got = m.enhance(Xg).cpu()
    mask = fsnp_torch.forward_full(sd, mag, real, imag)
    want = fsnp_torch.apply_cirm(mask, X)
    err = float((got - want).abs().max() / want.abs().max())
    _record("enhance_epilogue", rel=err, mask_absmax=float(mask.abs().max()))
    assert got.shape == want.shape and err < TOL, err


@pytest.mark.parametrize("n,cus", [(700, 256), (257, 8), (8192 + 32, 256)])
def test_bf16_ih_variant(n, cus):
    """BASELINE.json configs[4]: layer-1 ih-GEMM of the sub-band LSTM on bf16 MFMA (fp32 accumulate), everything else
    fp32.  Tolerance re-stated against the fp32 oracle: 2.5e-3 rel on the recurrent model alone (measured 1.1e-3 - 1.2e-3;
    bf16 has 8 mantissa bits: h0 and W_ih_l1 are each rounded to ~4e-3 relative, the fp32 accumulation averages it down);
    the fp32 path on the same inputs must stay at 2e-5."""
    sd = make_state_dict(10, "default")
    m = _model(DEFAULT_MODEL_ARGS, sd)
    m.debug_set_num_cus(cus)
    m.debug_set_lstm_coop(0)
    steps = 24
    rng = np.random.Generator(np.random.PCG64(55 + n))
    x = torch.from_numpy(rng.standard_normal((n, 34, steps)).astype(np.float32))
    want = fsnp_torch.lstm2_fc(x, sd).numpy()
    m.set_precision("bf16_ih")
    got = m.lstm2_fc(x.cuda()).cpu().numpy()
    err = rel_err(got, want)
    m.set_precision("fp32")
    got32 = m.lstm2_fc(x.cuda()).cpu().numpy()
    _record(f"bf16_ih_{n}_cus{cus}", rel_bf16=err, rel_fp32=rel_err(got32, want))
    assert rel_err(got32, want) < 2e-5
    assert 1e-6 < err < 2.5e-3, err          # must differ from fp32 (the mode is really on) and stay inside the stated bound


BF16_FORWARD_TOL = 4e-3     # whole forward under bf16_ih vs fp32 (profiles/r06_bf16_error.md: worst of six seed / clip-length rows 2.75e-3)


@pytest.mark.parametrize("wseed,iseed,seconds", [(1, 101, 2.0), (2, 102, 2.0), (3, 103, 2.0), (0, 100, 10.0), (1, 101, 10.0)])
def test_bf16_ih_forward_seeds_and_long_clips(wseed, iseed, seconds):
    """configs[4], owning the tolerance: the bound is asserted on FOUR weight seeds (with test_bf16_ih_forward_b32's seed 0)
    and on 10 s clips - the error must not grow with the clip length (the forget gates damp earlier steps' quantisation noise).  Round 5's
    arithmetic (h0_t as ONE bf16 image) measured 2.4e-3 ... 6.07e-3 over these rows, i.e. above its own 6e-3 bound on one seed; with h0_t as
    bf16 hi + lo (round 6) the worst row is 2.75e-3.  Every utterance against the fp32 HIP forward, utterances 0 / 15 / 31 against the fp32
    oracle."""
    sd = make_state_dict(wseed, "default")
    mag, real, imag = make_inputs(32, seconds, iseed)
    m = _model(DEFAULT_MODEL_ARGS, sd, "full")
    ins = _cuda((mag, real, imag))
    ref = m(*ins).cpu().numpy()
    m.set_precision("bf16_ih")
    got = m(*ins).cpu().numpy()
    per_utt = [rel_err(got[b:b + 1], ref[b:b + 1]) for b in range(32)]
    T = ref.shape[-1]
    halves = [rel_err(got[..., :T // 2], ref[..., :T // 2]), rel_err(got[..., T // 2:], ref[..., T // 2:])]
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    spots = {b: rel_err(got[b:b + 1], fsnp_torch.forward_full(sd, mag[b:b + 1], real[b:b + 1], imag[b:b + 1]).numpy()) for b in (0, 15, 31)}
    _record(f"bf16_ih_forward_w{wseed}_{seconds:g}s", rel_vs_fp32_hip_max=max(per_utt), worst_utt=int(np.argmax(per_utt)), first_half=halves[0],
            second_half=halves[1], rel_vs_oracle=spots)
    assert 1e-6 < max(per_utt) < BF16_FORWARD_TOL, per_utt
    assert max(spots.values()) < BF16_FORWARD_TOL, spots
    assert halves[1] < 1.5 * halves[0] + 1e-4, halves                 # no accumulation along the clip


def test_bf16_ih_forward_b32():
    """BASELINE configs[4] at its per-GPU shape (batch 32 x 2 s), tolerance re-stated against the fp32 ORACLE (and its fp64
    run) on every utterance: bound 4e-3 rel (round 6: h0_t as bf16 hi + lo - measured 2.75e-3; round 5: 5.8e-3 of 6e-3)."""
    sd = make_state_dict(0, "default")
    mag, real, imag = make_inputs(32, 2.0, 100)
    m = _model(DEFAULT_MODEL_ARGS, sd, "full")
    ins = _cuda((mag, real, imag))
    ref = m(*ins).cpu().numpy()
    m.set_precision("bf16_ih")
    got = m(*ins).cpu().numpy()
    err = rel_err(got, ref)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sd64 = {k: v.double() for k, v in sd.items()}
    e32, e64 = {}, {}
    for b in range(32):
        want = fsnp_torch.forward_full(sd, mag[b:b + 1], real[b:b + 1], imag[b:b + 1]).numpy()
        e32[b] = rel_err(got[b:b + 1], want)
        if b in (0, 7, 15, 23, 31):
            want64 = fsnp_torch.forward_full(sd64, mag[b:b + 1].double(), real[b:b + 1].double(), imag[b:b + 1].double()).numpy()
            e64[b] = rel_err(got[b:b + 1], want64)
    _record("bf16_ih_forward_b32", rel_vs_fp32_hip=err, rel_vs_oracle_max=max(e32.values()), rel_vs_oracle_worst_utt=max(e32, key=e32.get),
            rel_vs_fp64_max=max(e64.values()), plan=[c["kernel"] + f" x{c['sequences']}" for c in m.describe_plan(32)])
    assert 1e-6 < err < BF16_FORWARD_TOL, err            # must differ from fp32 (the mode is really on)
    assert max(e32.values()) < BF16_FORWARD_TOL and max(e64.values()) < BF16_FORWARD_TOL, (e32, e64)
    # the plan keeps the chip-filling chunk on the one-tile-per-CU kernel (whose bf16 round is 0.75 of its fp32 round): a planner that
    # prices it at the fp32 cost trades it for half-tile + column-split launches (27.6 instead of 20.9 ms: profiles/r05_bench_configs.md)
    plan = m.describe_plan(32)
    assert plan[0]["sequences"] == 8192 and "one 32-" in plan[0]["kernel"] and "bf16" in plan[0]["precision"], plan


@pytest.mark.parametrize("n", [4096, 4000, 4112])
def test_bf16_ih_on_the_half_tile_kernel(n):
    """configs[4] below the chip-filling batch (round 4): the half-tile kernel (csrc/lstm16.hip, 16-row tiles - B = 16 in full mode,
    the reference's literal drop-band call at B = 32) runs its layer-1 ih-GEMM on v_mfma_f32_16x16x32_bf16 under `bf16_ih`, so the mode
    means the same arithmetic there as on the one-tile-per-CU kernel.  Same re-stated tolerance (2.5e-3 on the recurrent model alone);
    4112 = 4096 on half tiles + 16 on a column-split kernel (those stay fp32: reported per launch)."""
    sd = make_state_dict(10, "default")
    m = _model(DEFAULT_MODEL_ARGS, sd)
    steps = 24
    rng = np.random.Generator(np.random.PCG64(555 + n))
    x = torch.from_numpy(rng.standard_normal((n, 34, steps)).astype(np.float32))
    want = fsnp_torch.lstm2_fc(x, sd).numpy()
    got32 = m.lstm2_fc(x.cuda()).cpu().numpy()
    assert rel_err(got32, want) < 2e-5
    m.set_precision("bf16_ih")
    got = m.lstm2_fc(x.cuda()).cpu().numpy()
    assert np.array_equal(m.lstm2_fc(x.cuda()).cpu().numpy(), got)
    err = rel_err(got, want)
    per_row = np.abs(got - want).max(axis=(1, 2)) / np.abs(want).max()
    _record(f"bf16_ih_half_tile_{n}", rel_bf16=err, rows_that_differ_from_fp32=int((np.abs(got - got32).max(axis=(1, 2)) > 0).sum()))
    assert 1e-6 < err < 2.5e-3, err
    # every row of the half-tile chunk really ran in bf16 (it differs from the fp32 run), inside the bound row by row
    assert (np.abs(got - got32).max(axis=(1, 2))[:min(n, 4096)] > 0).all() and per_row.max() < 2.5e-3
    m.set_precision("fp32")
    assert np.array_equal(m.lstm2_fc(x.cuda()).cpu().numpy(), got32)


def test_bf16_ih_forward_parity_mode_b32_and_b16():
    """... and through the whole forward: the reference's literal batched call at B = 32 (drop_band: 4096 sequences = 256 half tiles) and
    B = 16 in full mode (4112 = 4096 + 16) against the fp32 ORACLE on every utterance, bound 4e-3 as at the chip-filling batch;
    describe_plan reports the half-tile chunk as bf16 and the 16-sequence column-split chunk as fp32."""
    sd = make_state_dict(0, "default")
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for B, mode in ((32, "parity"), (16, "full")):
        mag, real, imag = make_inputs(B, 2.0, 100 + B)
        m = _model(DEFAULT_MODEL_ARGS, sd, mode)
        ins = _cuda((mag, real, imag))
        ref = m(*ins).cpu().numpy()
        m.set_precision("bf16_ih")
        plan = m.describe_plan(B, parity=(mode == "parity"))
        assert plan[0]["kernel"].startswith("lstm2_fc16_kernel") and plan[0]["precision"] == "f32 + bf16 layer-1 ih-GEMM", plan
        assert all(c["precision"] == "f32" for c in plan[1:]), plan
        got = m(*ins).cpu().numpy()
        want = (fsnp_torch.forward(sd, mag, real, imag) if mode == "parity" else fsnp_torch.forward_full(sd, mag, real, imag)).numpy()
        e_ref, e_bf = rel_err(ref, want), rel_err(got, want)
        _record(f"bf16_ih_forward_{mode}_b{B}", rel_fp32=e_ref, rel_bf16=e_bf, plan=[c["kernel"] + f" x{c['sequences']} [{c['precision']}]" for c in plan])
        assert e_ref < TOL and 1e-6 < rel_err(got, ref) and e_bf < BF16_FORWARD_TOL, (e_ref, e_bf)


def test_batch2_raises_like_reference():
    g = Golden("b4_t16_default")
    m = _model(g.args, g.state_dict(), "parity")
    mag, real, imag = _cuda(g.inputs())
    with pytest.raises(AssertionError):
        m(mag[:2], real[:2], imag[:2])


def test_contiguous_and_strided_inputs_agree():
    g = Golden("b1_t24_default_stages")
    m = _model(g.args, g.state_dict())
    mag, real, imag = _cuda(g.inputs())
    a = m(mag, real, imag)
    b = m(mag.contiguous(), real.contiguous(), imag.contiguous())
    assert not real.is_contiguous()
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------
# BASELINE.json configs[1]: batch = 32 x 2 s clips, full + parity, against the oracle on the same inputs
@pytest.fixture(scope="module")
def b32():
    sd = make_state_dict(0, "default")
    mag, real, imag = make_inputs(32, 2.0, 100)
    m = _model(DEFAULT_MODEL_ARGS, sd, "full")
    full = m(*_cuda((mag, real, imag))).cpu()
    return sd, (mag, real, imag), m, full


def test_b32_full_vs_oracle(b32):
    """BASELINE configs[1] at its benchmarked shape.  EVERY utterance against the oracle (round 2: a cell-update overflow that
    only fired where |c| > 42 hit 8 of the 32 utterances and none of the three that used to be sampled): in "full" mode rows
    are (utterance, bin) in order, so utterance 31's bins 225..256 are exactly the 32 sequences the planner hands to the
    remainder (K-split) kernel after the 8192 that fill the chip - all three kernels' rows are compared directly."""
    sd, (mag, real, imag), m, full = b32
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    plan = m.describe_plan(32)
    assert sum(c["sequences"] for c in plan) == 32 * 257
    errs = {}
    for b in range(32):
        want = fsnp_torch.forward_full(sd, mag[b:b + 1], real[b:b + 1], imag[b:b + 1]).numpy()
        errs[b] = rel_err(full[b:b + 1].numpy(), want)
        if b == 31 and len(plan) > 1:           # the remainder chunk's rows on their own
            n_rem = plan[-1]["sequences"]
            errs["remainder_rows"] = rel_err(full[31, :, 257 - n_rem:].numpy(), want[0, :, 257 - n_rem:])
    _record("b32_2s_full_vs_oracle_all_utterances", plan=[c["kernel"] + f" x{c['sequences']}" for c in plan],
            rel_max=max(errs.values()), rel_utt_0=errs[0], rel_utt_15=errs[15], rel_utt_31=errs[31], rel_remainder_rows=errs.get("remainder_rows"))
    assert full.shape == (32, 2, 257, 126)
    assert max(errs.values()) < TOL, errs


@pytest.mark.parametrize("profile,B,T", [("default", 3, 10.0), ("harsh", 2, 37.0), ("default", 2, 4.8), ("harsh", 1, 1.0), ("default", 4, 2.0), ("harsh", 3, 0.6),
                                         ("default", 16, 2.0)])
def test_dma_gemm_equals_general_gemm(profile, B, T):
    """csrc/tcn.hip: the DMA GEMM kernels (operands by LDS DMA, XOR-swizzled image, GroupNorm folded into the sconv weights; at these
    batch sizes tcn_gemm_sk_kernel, then tcn_gemm_dma_kernel through debug mode 2) against the general tcn_gemm_kernel on the same
    handle, and all three against the oracle.  T = clip length in SECONDS: 10 s / 37 s clips (many row tiles per plane, ragged last
    tile: the 128-row kernel only), 1 s / 0.6 s / 2 s clips at B = 1 ... 16 (the split-K kernel: one ... four 32-row tiles per plane,
    ragged).  (Round 3 ran 126 s / 300 s clips here by accident - frames passed as seconds; those are now
    tests/test_gpu_soak.py::test_long_recurrence_forward.)"""
    sd = make_state_dict(21, profile)
    m = _model(DEFAULT_MODEL_ARGS, sd, mode="full")
    mag, real, imag = make_inputs(B, T, 77)
    g = _cuda((mag, real, imag))
    fast = m(*g).cpu().numpy()
    m.debug_set_gemm_dma(0)
    general = m(*g).cpu().numpy()
    m.debug_set_gemm_dma(1)
    again = m(*g).cpu().numpy()
    want = fsnp_torch.forward_full(sd, mag, real, imag).numpy()
    e_fast, e_gen, e_pair = rel_err(fast, want), rel_err(general, want), rel_err(fast, general)
    _record(f"dma_gemm_{profile}_B{B}_T{T}", rel_dma=e_fast, rel_general=e_gen, rel_dma_vs_general=e_pair)
    assert np.array_equal(fast, again)
    assert e_fast < TOL and e_gen < TOL and e_pair < 1e-4, (e_fast, e_gen, e_pair)
    assert not np.array_equal(fast, general)      # the two kernels really are different code paths
    # small batches run the GEMMs on tcn_gemm_sk_kernel (32 x 64 tiles, four waves split K); mode 2 = the 128-row DMA kernel instead
    m.debug_set_gemm_dma(2)
    big_tiles = m(*g).cpu().numpy()
    m.debug_set_gemm_dma(1)
    e_big = rel_err(big_tiles, want)
    _record(f"dma_gemm_{profile}_B{B}_T{T}_128_row_tiles", rel=e_big, rel_vs_splitk=rel_err(big_tiles, fast))
    assert e_big < TOL and rel_err(big_tiles, fast) < 1e-4
    splitk = 8 * (-(-(mag.shape[-1] + 2) // 32)) * B * 3 <= 6 * 256       # csrc/tcn.hip launch_gemm_dma: at most 6 workgroups per CU
    assert np.array_equal(big_tiles, fast) != splitk, splitk              # another k order where the split-K kernel ran, the same kernel elsewhere
    # mode 3 = the 128-row kernel for every GEMM; modes 1 / 2 run the sconv GEMMs on 64-row tiles (tcn_gemm_dma64_kernel: four column
    # tiles + column 256 on the VALU) wherever that needs no more rounds of workgroups (csrc/tcn.hip launch_gemm_dma64)
    m.debug_set_gemm_dma(3)
    only128 = m(*g).cpu().numpy()
    m.debug_set_gemm_dma(1)
    _record(f"dma_gemm_{profile}_B{B}_T{T}_128_row_only", rel=rel_err(only128, want), rel_vs_mode2=rel_err(only128, big_tiles))
    assert rel_err(only128, want) < TOL and rel_err(only128, big_tiles) < 1e-4
    Tp = mag.shape[-1] + 2
    cost64, cost128 = -(-(4 * (-(-Tp // 64)) * B * 3) // 256), 2 * (-(-(5 * (-(-Tp // 128)) * B * 3) // 256))
    assert np.array_equal(only128, big_tiles) != (cost64 <= cost128), (cost64, cost128)


def test_b32_10s_full_vs_oracle():
    """BASELINE configs[3] at its benchmarked shape (batch 32 x 10 s clips, T = 626, look-ahead 2): every utterance against the
    oracle (the last one holds the remainder kernel's rows; a row-indexing slip once hit 8 rows of 32), plus batch independence of a
    middle one against a B = 1 run of the HIP path (a different kernel plan)."""
    sd = make_state_dict(0, "default")
    mag, real, imag = make_inputs(32, 10.0, 300)
    m = _model(DEFAULT_MODEL_ARGS, sd, "full")
    full = m(*_cuda((mag, real, imag))).cpu()
    assert full.shape == (32, 2, 257, 626)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    errs = {}
    for b0 in range(0, 32, 8):          # the oracle is per utterance in "full" mode: eight rows per call
        want = fsnp_torch.forward_full(sd, mag[b0:b0 + 8], real[b0:b0 + 8], imag[b0:b0 + 8]).numpy()
        for i in range(8):
            errs[b0 + i] = rel_err(full[b0 + i:b0 + i + 1].numpy(), want[i:i + 1])
    one = m(*_cuda((mag[17:18], real[17:18], imag[17:18]))).cpu()
    indep = rel_err(one.numpy(), full[17:18].numpy())
    worst = max(errs, key=errs.get)
    _record("b32_10s_full_vs_oracle_all_rows", rel_max=errs[worst], worst_row=worst, b1_vs_batch_row17=indep)
    assert max(errs.values()) < TOL, errs
    assert indep < 1e-5, indep


@pytest.mark.parametrize("case", ["cumulative_layer_norm", "cumulative_laplace_norm_positive"])
def test_b32_10s_cumulative_norms_vs_oracle(case):
    """BASELINE configs[3] as it is worded - "batch=32 x 10 s clips, cumulative-LN stress" - at its benchmarked shape: the
    fp32 oracle on utterances 0, 15 and 31 (the last one holds the remainder kernel's rows; per-row norm tables of 8224
    sequences x 628 steps).  cumulative_laplace_norm runs on its well-conditioned variant (strictly positive planes): on real
    STFT data the reference's own fp32 result is 1.5e-2 from its fp64 result (profiles/r03_cum_laplace.md)."""
    norm = case.replace("_positive", "")
    sd = make_state_dict(0, "default")
    mag, real, imag = make_inputs(32, 10.0, 300)
    ins = (mag, 0.5 * mag + 0.1, mag.sqrt()) if case.endswith("_positive") else (mag, real, imag)
    m = _model({**DEFAULT_MODEL_ARGS, "norm_type": norm}, sd, "full")
    full = m(*_cuda(ins)).cpu()
    assert full.shape == (32, 2, 257, 626)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    errs = {}
    for b in (0, 15, 31):
        want = fsnp_torch.forward_full(sd, *[t[b:b + 1] for t in ins], norm_type=norm).numpy()
        errs[b] = rel_err(full[b:b + 1].numpy(), want)
    _record(f"b32_10s_{case}_vs_oracle_utt_0_15_31", rel_0=errs[0], rel_15=errs[15], rel_31=errs[31])
    assert max(errs.values()) < TOL, errs


def test_b32_parity_vs_oracle_and_subselection(b32):
    sd, (mag, real, imag), m, full = b32
    m.batch_mode = "parity"
    par = m(*_cuda((mag, real, imag))).cpu().numpy()
    m.batch_mode = "full"
    want = fsnp_torch.forward(sd, mag, real, imag).numpy()                    # literal reference semantics
    err = rel_err(par, want)
    _record("b32_2s_parity_vs_oracle", rel=err)
    assert par.shape == (32, 2, 128, 126)
    assert err < TOL, err
    # size-independent property: parity rows are a sub-selection of full rows
    fulln = full.numpy()
    for r in range(32):
        s, p = (2 * r, 0) if r < 16 else (2 * (r - 16) + 1, 1)
        assert np.abs(par[r] - fulln[s][:, p:256:2, :]).max() < 1e-5 * np.abs(fulln).max()


def test_b32_batch_independence(b32):
    """Size-independent property: utterances are independent, so row b of the batch == the B=1 run."""
    sd, (mag, real, imag), m, full = b32
    for b in (0, 13, 31):
        one = m(*_cuda((mag[b:b + 1], real[b:b + 1], imag[b:b + 1]))).cpu()
        assert rel_err(one.numpy(), full[b:b + 1].numpy()) < 1e-5


def _fp64(sd):
    return {k: v.double() for k, v in sd.items()}


def test_long_clip_cumulative_norms_vs_oracle():
    """BASELINE.json configs[3] flavour: 10 s clips (T=626), cumulative norms, oracle on the same inputs.

    cumulative_laplace_norm divides by a running MEAN; on real STFT data the real/imag means are
    cancellation residues, the normalised values reach 1e8 and the reference's own fp32 result differs from
    its fp64 result by tens of percent (measured: 0.58 rel).  So every case is judged against the fp64
    oracle with the bound max(1e-3, 2 x the fp32 oracle's own error vs fp64), and a well-conditioned
    cumulative_laplace case (strictly positive "real"/"imag" planes) pins the kernel math itself at 1e-3."""
    sd = make_state_dict(11, "default")
    mag, real, imag = make_inputs(2, 10.0, 200)
    cases = [("cumulative_layer_norm", (mag, real, imag)), ("cumulative_laplace_norm", (mag, real, imag)),
             ("cumulative_laplace_norm_positive", (mag, 0.5 * mag + 0.1, mag.sqrt()))]
    for name, ins in cases:
        norm = name.replace("_positive", "")
        m = _model({**DEFAULT_MODEL_ARGS, "norm_type": norm}, sd, "full")
        got = m(*_cuda(ins)).cpu().numpy()
        ref32 = fsnp_torch.forward_full(sd, *ins, norm_type=norm).numpy()
        ref64 = fsnp_torch.forward_full(_fp64(sd), *[t.double() for t in ins], norm_type=norm).numpy()
        err, ref_err = rel_err(got, ref64), rel_err(ref32, ref64)
        _record(f"b2_10s_{name}", rel_vs_fp64=err, ref32_vs_fp64=ref_err, rel_vs_ref32=rel_err(got, ref32))
        assert err < max(TOL, 2 * ref_err), (name, err, ref_err)
        if name != "cumulative_laplace_norm":
            assert err < TOL and ref_err < TOL, (name, err, ref_err)


def test_forward_complex_equals_three_plane_forward():
    """fsnp_forward_complex derives mag / real / imag from the complex64 STFT buffer in the repack
    kernel; result == forward(|X|, X.real, X.imag) up to the rounding of |X| (hypotf vs torch.abs)."""
    g = Golden("b1_2s_default")
    m = _model(g.args, g.state_dict(), "full")
    mag, real, imag = g.inputs()
    X = torch.complex(real[:, 0], imag[:, 0])                     # [B,F,T] with stft strides
    Xg = torch.empty_strided(X.shape, X.stride(), dtype=X.dtype, device="cuda")
    Xg.copy_(X)
    a = m.forward_complex(Xg).cpu().numpy()
    b = m(*_cuda((mag, real, imag))).cpu().numpy()
    _record("forward_complex_vs_planes", rel=rel_err(a, b), vs_ref=rel_err(a, g.arrays["out"]))
    assert rel_err(a, b) < 1e-5
    assert rel_err(a, g.arrays["out"]) < TOL
    with pytest.raises(AssertionError):
        m.forward_complex(Xg.unsqueeze(1))


# ---------------------------------------------------------------- sub-band GRU (sequence_model.py:39-46)
@pytest.mark.parametrize("n,steps", [(50, 9), (257, 40), (1300, 7), (2750, 6), (6000, 5), (9000, 4)])
def test_gru2_fc_dense_vs_oracle(n, steps):
    """nn.GRU cells: on the column-split kernels (K split, three-way split) as the planner cuts them, beyond a chip-filling
    round on the one-tile-per-CU GRU kernel + a column-split remainder (9000 rows = 256 + 26 tiles), and on the
    one-tile-per-CU kernel alone."""
    args = {**DEFAULT_MODEL_ARGS, "sequence_model": "GRU"}
    sd = make_state_dict(31, "harsh", sequence_model="GRU")
    m = _model(args, sd)
    rng = np.random.Generator(np.random.PCG64(99 + n))
    x = torch.from_numpy(rng.standard_normal((n, 34, steps)).astype(np.float32))
    want = fsnp_torch.lstm2_fc(x, sd).numpy()
    got = m.lstm2_fc(x.cuda()).cpu().numpy()
    m.check_errors()
    err = rel_err(got, want)
    _record(f"gru2_fc_{n}x{steps}", rel=err)
    assert err < 2e-5, err
    assert np.array_equal(m.lstm2_fc(x.cuda()).cpu().numpy(), got)
    with pytest.raises(RuntimeError, match="LSTM sub-band model only"):
        m.set_precision("bf16_ih")
    # the one-tile-per-CU GRU kernel (csrc/lstm_gru.hip: three live gate tiles per k-group) on every row, ragged last tile
    m.debug_set_lstm_coop(0)
    assert all(c["kernel"].startswith("gru2_fc_kernel") for c in m.describe_plan(1))
    tile = m.lstm2_fc(x.cuda()).cpu().numpy()
    m.debug_set_lstm_coop(1)
    _record(f"gru2_fc_rowtile_{n}x{steps}", rel=rel_err(tile, want))
    assert rel_err(tile, want) < 2e-5


@pytest.mark.parametrize("scale,steps", [(40.0, 30), (400.0, 12)])
def test_gru_rowtile_saturated_gates(scale, steps):
    """gru2_fc_kernel's packed cell update (lstm_common.h gru_cell_pair) forms h' = [e_z (1 - e_n) + h (1 + e_n)] / ((1 + e_z)(1 + e_n))
    with ONE reciprocal; inputs 40x / 400x the usual scale drive a_z, a_n to +-hundreds, where the clamped exponents (2^60)
    must neither overflow the products nor change the result."""
    args = {**DEFAULT_MODEL_ARGS, "sequence_model": "GRU"}
    sd = make_state_dict(31, "harsh", sequence_model="GRU")
    m = _model(args, sd)
    m.debug_set_lstm_coop(0)
    rng = np.random.Generator(np.random.PCG64(4242))
    x = torch.from_numpy((rng.standard_normal((200, 34, steps)) * scale).astype(np.float32))
    want = fsnp_torch.lstm2_fc(x, sd).numpy()
    got = m.lstm2_fc(x.cuda()).cpu().numpy()
    m.check_errors()
    assert np.isfinite(got).all()
    err = rel_err(got, want)
    _record(f"gru2_fc_saturated_x{int(scale)}", rel=err)
    assert err < 2e-5, err


def test_gru_forward_b32_full_vs_oracle():
    args = {**DEFAULT_MODEL_ARGS, "sequence_model": "GRU"}
    sd = make_state_dict(32, "default", sequence_model="GRU")
    mag, real, imag = make_inputs(32, 1.0, 300)
    m = _model(args, sd, "full")
    out = m(*_cuda((mag, real, imag))).cpu().numpy()
    m.check_errors()
    pick = [0, 17, 31]
    want = fsnp_torch.forward_full(sd, mag[pick], real[pick], imag[pick]).numpy()
    err = rel_err(out[pick], want)
    _record("gru_forward_b32_full", rel=err)
    assert err < TOL, err


# ---------------------------------------------------------------- drop-in behaviour of the nn.Module shell
def test_weight_update_repacks_device_weights():
    """The packed device blob is rebuilt lazily when a parameter changes (load_state_dict / in-place update), as a
    torch module would behave (base_inferencer.py:100-107 loads AFTER construction)."""
    g = Golden("b1_t24_default_stages")
    m = _model(g.args, g.state_dict())
    ins = _cuda(g.inputs())
    a = m(*ins).cpu().numpy()
    sd2 = make_state_dict(123, "harsh")
    m.load_state_dict(sd2, strict=True)
    b = m(*ins).cpu().numpy()
    want = fsnp_torch.forward(sd2, *g.inputs(), **g.fwd_kwargs()).numpy()
    assert rel_err(b, want) < TOL and rel_err(a, b) > 1e-2
    with torch.no_grad():
        m.sb_model.fc_output_layer.bias += 0.5           # in-place edit bumps the parameter version
    c = m(*ins).cpu().numpy()
    assert abs(float((c - b).mean()) - 0.5) < 1e-4
    # an edit through .data bumps NOTHING (no pointer, no version): the handle's weight watch (fsnp_watch_weights: one fingerprint
    # kernel over the parameters' storage in front of every forward) notices it; under error_check="sync" the forward re-packs
    # and re-runs, so the caller never sees a result for the old weights
    key = m._weights_key()
    m.sb_model.fc_output_layer.bias.data.add_(0.25)
    assert m._weights_key() == key
    d = m(*ins).cpu().numpy()
    assert abs(float((d - c).mean()) - 0.25) < 1e-4
    assert np.array_equal(m(*ins).cpu().numpy(), d)                       # (the new pack is watched again: no re-pack, same result)
    m.fb_model.sequence_model[0].conv1x1.weight.data.copy_(torch.from_numpy(make_state_dict(5, "harsh")["fb_model.sequence_model.0.conv1x1.weight"].numpy()))
    e = m(*ins).cpu().numpy()
    sd3 = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    assert rel_err(e, fsnp_torch.forward(sd3, *g.inputs(), **g.fwd_kwargs()).numpy()) < TOL and rel_err(e, d) > 1e-4
    # the reference's own entry point (base_model.py:332-397, `model.apply(model.weight_init)`) edits through .data too
    torch.manual_seed(3)
    m.apply(m.weight_init)
    f = m(*ins).cpu().numpy()
    sd4 = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    assert rel_err(f, fsnp_torch.forward(sd4, *g.inputs(), **g.fwd_kwargs()).numpy()) < TOL
    # deferred mode does not wait for the watch: the stale forward is reported by poll_errors / check_errors ...
    m.error_check = "deferred"
    m(*ins)
    m.check_errors()
    m.sb_model.fc_output_layer.bias.data.add_(0.5)
    stale = m(*ins)
    with pytest.raises(RuntimeError, match="modified in place"):
        m.check_errors()
    assert np.array_equal(stale.cpu().numpy(), f)                         # (that result WAS computed with the old weights)
    # ... or, if nobody asked, by the next forward, which re-packs with a warning and runs on the new weights
    m.sb_model.fc_output_layer.bias.data.add_(0.5)
    m(*ins)
    torch.cuda.synchronize()
    with pytest.warns(RuntimeWarning, match="through .data"):
        h = m(*ins)
    m.check_errors()
    assert abs(float((h.cpu().numpy() - f).mean()) - 1.0) < 1e-4
    m.refresh_weights()                                                    # the explicit form
    m.check_errors()


def test_weight_watch_registered_on_a_side_stream_raises_no_false_alarm():
    """The watch's baseline fingerprint is taken on the CALLER's stream.  Round 5's first version zeroed its accumulators with a
    null-stream hipMemset, which does not order with torch's non-blocking side streams: now and then the tickets / the baseline were
    zeroed under the running baseline kernel and every later forward reported "weights modified" (seen once in the evidence run of
    874326c, test_forward_on_side_stream_and_second_handle).  Here: 24 registrations on a side stream that is kept busy, each followed
    by forwards that must neither flag nor re-pack, with a real .data edit in between to show the watch is alive."""
    g = Golden("b3_t20_harsh")
    m = _model(g.args, g.state_dict(), "full")
    ins = _cuda(g.inputs())
    ref = m(*ins).cpu().numpy()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    busy = torch.empty(64 << 20, device="cuda")
    m.error_check = "deferred"                              # ("sync" would hide a false alarm behind its re-pack + re-run)
    with torch.cuda.stream(side):
        for i in range(24):
            busy.add_(1.0)                                  # work in front of the registration on the side stream
            m.refresh_weights()
            for _ in range(2):
                out = m(*ins)
                m.check_errors()                            # raises on "weights modified"
                assert np.array_equal(out.cpu().numpy(), ref), i
        m.error_check = "sync"
        m.sb_model.fc_output_layer.bias.data.add_(0.25)
        out = m(*ins).cpu().numpy()
    assert abs(float((out - ref).mean()) - 0.25) < 1e-4
    m.check_errors()


@pytest.mark.parametrize("norm_type", ["offline_laplace_norm", "cumulative_laplace_norm", "offline_gaussian_norm", "cumulative_layer_norm"])
def test_norm_and_unfold_stage_entry_points_vs_oracle(norm_type):
    """fsnp_norm / fsnp_unfold (csrc/stages.hip) = `model.norm` / `model.unfold` of the reference's module protocol (base_model.py:15-47,
    210-330) on arbitrary [B, C, F, T] tensors: contiguous and torch.stft-style strided inputs, one and several channels (the sub-band
    input is normalised with C = 1 and F = 34 features), against the oracle's restatement of the reference functions.  The laplace norms
    divide by a mean: positive inputs (magnitudes), as in the model."""
    m = FullSubNet_Plus(**{**DEFAULT_MODEL_ARGS, "norm_type": norm_type}).cuda().eval()
    rng = np.random.Generator(np.random.PCG64(31))
    for shape in [(3, 1, 257, 20), (2, 3, 34, 61), (1, 2, 5, 300)]:
        x = torch.from_numpy(np.abs(rng.standard_normal(shape)).astype(np.float32) + 0.1)
        want = fsnp_torch.NORMS[norm_type](x).numpy()
        got = m.norm(x.cuda()).cpu().numpy()
        assert got.shape == want.shape and rel_err(got, want) < 2e-5, (shape, rel_err(got, want))
        xs = x.permute(0, 3, 2, 1).contiguous().permute(0, 3, 2, 1)          # same values, memory order [B][T][F][C]
        assert not xs.is_contiguous()
        assert np.array_equal(m.norm(xs.cuda()).cpu().numpy(), got)
        assert np.array_equal(m.norm_wrapper(norm_type)(x.cuda()).cpu().numpy(), got)
    for shape, nb in [((2, 1, 257, 12), 15), ((2, 3, 40, 7), 1), ((1, 2, 9, 5), 0), ((2, 1, 33, 4), 8)]:
        x = torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
        want = fsnp_torch.unfold(x, nb).numpy()
        got = m.unfold(x.cuda(), nb).cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), (shape, nb)
        xs = x.permute(0, 3, 2, 1).contiguous().permute(0, 3, 2, 1)
        assert np.array_equal(FullSubNet_Plus.unfold(xs.cuda(), nb).cpu().numpy(), want)


@pytest.mark.parametrize("kind", ["LSTM", "GRU"])
def test_sub_band_model_is_callable_as_a_submodule(kind):
    """`model.sb_model(x)` - the reference's `self.sb_model(sb_input)` (fullsubnet_plus.py:203; SequenceModel.forward, sequence_model.py:97-123)
    as a call on the parameter holder: runs the owning model's fused kernels (fsnp_lstm2_fc), equals `model.lstm2_fc` bit for bit and the
    oracle within the recurrent kernels' tolerance; a deep copy with other weights answers with ITS weights."""
    import copy as _copy
    args = {**DEFAULT_MODEL_ARGS, "sequence_model": kind}
    sd = make_state_dict(5, "harsh", sequence_model=kind)
    m = _model(args, sd)
    rng = np.random.Generator(np.random.PCG64(77))
    x = torch.from_numpy(rng.standard_normal((300, 34, 19)).astype(np.float32)).cuda()
    got = m.sb_model(x)
    assert got.shape == (300, 2, 19) and torch.equal(got, m.lstm2_fc(x))
    want = fsnp_torch.lstm2_fc(x.cpu(), sd).numpy()                               # (the oracle tells LSTM from GRU by the weight shapes)
    assert rel_err(got.cpu().numpy(), want) < 2e-5
    twin = _copy.deepcopy(m)
    with torch.no_grad():
        twin.sb_model.fc_output_layer.weight.mul_(2.0)
        twin.sb_model.fc_output_layer.bias.mul_(2.0)
    assert rel_err(twin.sb_model(x).cpu().numpy(), 2.0 * want) < 2e-5          # the copy's kernels, the copy's weights (no output activation)
    assert torch.equal(m.sb_model(x), got)                                       # ... and the original is untouched


@pytest.mark.parametrize("att", ["TSSE", "SE", "ECA", "CBAM"])
def test_attention_layers_and_fullband_stacks_are_callable_as_submodules(att):
    """`model.channel_attention(x)` / `model.fb_model(x)` and their `_real` / `_imag` siblings - what the reference's forward calls
    (fullsubnet_plus.py:160-165, 171-173) - as calls on the parameter holders: fsnp_channel_attention / fsnp_fullband_model run ONE
    branch's stage kernels on the caller's [B, F, T] tensor (contiguous, or strided like a view of the STFT), against the oracle's
    restatement of the layers.  The full-band stacks are checked once (they do not depend on the attention kind)."""
    args = {**DEFAULT_MODEL_ARGS, "channel_attention_model": att}
    sd = make_state_dict(9, "harsh", attention=att)
    m = _model(args, sd, "full")
    rng = np.random.Generator(np.random.PCG64(123))
    for branch, tag in enumerate(("", "_real", "_imag")):
        for B, T in ((3, 37), (1, 130)):
            x = torch.from_numpy(rng.standard_normal((B, 257, T)).astype(np.float32))
            want = fsnp_torch.attention(x, sd, "channel_attention" + tag, att).numpy()
            got = getattr(m, "channel_attention" + tag)(x.cuda())
            assert got.shape == x.shape and rel_err(got.cpu().numpy(), want) < 2e-5, (att, tag, B, T, rel_err(got.cpu().numpy(), want))
            xs = x.permute(0, 2, 1).contiguous().permute(0, 2, 1)            # same values, memory order [B][T][F]
            assert not xs.is_contiguous() and torch.equal(getattr(m, "channel_attention" + tag)(xs.cuda()), got)
            if att == "TSSE":
                want_fb = fsnp_torch.fb_sequence_model(x, sd, "fb_model" + tag, "ReLU").numpy()
                got_fb = getattr(m, "fb_model" + tag)(x.cuda())
                e = rel_err(got_fb.cpu().numpy(), want_fb)
                assert got_fb.shape == x.shape and e < 2e-4, (tag, B, T, e)
                assert torch.equal(getattr(m, "fb_model" + tag)(xs.cuda()), got_fb)
    # a forward before and after: the stage calls leave the handle's own workspace alone
    ins = _cuda(make_inputs(2, 0.6, 5))
    a = m(*ins).cpu().numpy()
    m.fb_model(torch.zeros(1, 257, 9, device="cuda"))
    assert np.array_equal(m(*ins).cpu().numpy(), a)


def test_weight_watch_registered_on_one_stream_forward_on_another():
    """fsnp_watch_weights queued its baseline fingerprint on the caller's stream without recording the handle's
    cross-stream event, so a forward on ANOTHER non-blocking stream could start its watch blocks (same ticket word, same baseline
    slot) under the running baseline kernel - a spurious code 6.  The registration now ends with mark_forward_done: 24 registrations
    on the default stream behind queued work, each followed at once by a forward on a side stream that never waited for the default
    stream by itself."""
    g = Golden("b3_t20_harsh")
    m = _model(g.args, g.state_dict(), "full")
    ins = _cuda(g.inputs())
    ref = m(*ins).cpu().numpy()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    busy = torch.empty(64 << 20, device="cuda")
    m.error_check = "deferred"
    for i in range(24):
        for _ in range(4):
            busy.add_(1.0)                                  # the default stream is busy when the baseline kernel is queued on it
        m.refresh_weights()
        m.set_verify(0)                                     # _ensure_handle on the DEFAULT stream: re-pack + watch registration
        with torch.cuda.stream(side):
            out = m(*ins)
            m.check_errors()                                # raises on a false "weights modified"
            assert np.array_equal(out.cpu().numpy(), ref), i
    torch.cuda.synchronize()


def test_box_probe_and_launch_clock():
    """bench.py's `box` object: the pure-MFMA probe reports a plausible fp32 MFMA rate for an MI355X (the data sheet's 157.3 TFLOP/s is
    2.4 GHz x 65,536 FLOP per cycle; a box under a power cap holds less) and a shader clock consistent with it; the dominant kernel's
    workgroup 0 stamps the launch it ran in."""
    from fullsubnet_plus_amd import box
    p = box.probe(20.0)
    assert p["compute_units"] >= 64 and 0.5 < p["frac_of_spec_peak"] <= 1.02, p
    assert 1200 < p["clock_mhz_slowest_cu"] <= p["clock_mhz"] <= p["clock_mhz_fastest_cu"] < 2600, p
    # the rate over the whole launch (hipEvents) can only be below the in-kernel rate; both describe the same clock
    assert p["mfma_tflops"] <= p["mfma_tflops_in_kernel"] * 1.005 and p["mfma_tflops"] > 0.9 * p["mfma_tflops_in_kernel"], p
    assert abs(p["mfma_tflops_in_kernel"] - p["clock_mhz"] * 1e6 * 65536 * p["compute_units"] / 256 / 1e12) < 1e-6 * p["mfma_tflops"]
    g = Golden("b4_t16_default")
    m = _model(g.args, g.state_dict(), "full")
    ins = _cuda(g.inputs())
    m(*ins)
    assert m.launch_clock() is None or m.launch_clock()["wall_ms"] > 0    # B = 4: column-split plan, no one-tile-per-CU launch yet
    m.debug_set_lstm_coop(0)
    m(*ins)
    torch.cuda.synchronize()
    c = m.launch_clock()
    assert c is not None and 0.01 < c["wall_ms"] < 100 and c["s_memtime_ticks"] > 0 and c["s_memtime_mhz"] > 50, c


def test_error_word_reports_every_condition_that_was_set():
    """the error word is taken with ONE atomic exchange and every bit that was set is named (a verify or stale-weights bit
    that coincides with a time-out used to be dropped)."""
    g = Golden("b3_t20_harsh")
    m = _model(g.args, g.state_dict(), "full")
    ins = _cuda(g.inputs())
    m.error_check = "deferred"
    ref = m(*ins).cpu().numpy()
    m.sb_model.fc_output_layer.bias.data.add_(0.5)           # -> the weight watch flags the next forward (code 6) ...
    m(*ins)
    torch.cuda.synchronize()
    m.debug_inject_error()                                   # ... and a (pretended) time-out lands in the same word (code 5)
    with pytest.raises(RuntimeError, match=r"(?s)timed out.*ALSO:.*watched source tensors") as ei:
        m.poll_errors()
    assert ei.value.code == 5
    m.poll_errors()                                          # taken: clean now
    m.sb_model.fc_output_layer.bias.data.sub_(0.5)
    m.refresh_weights()
    assert np.array_equal(m(*ins).cpu().numpy(), ref)
    m.check_errors()


def _sleep_cycles_for(seconds):
    """torch.cuda._sleep counts device clock ticks: calibrate them against the wall clock once."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    torch.cuda._sleep(20_000_000)
    torch.cuda.synchronize()
    per_tick = (time.perf_counter() - t0) / 20_000_000
    return int(seconds / per_tick)


@pytest.mark.parametrize("reserve", [False, True])
def test_variable_clip_lengths_never_synchronise_the_device(reserve):
    """SURVEY.md 8(b) "no internal synchronisation": a serving loop whose clips alternate T = 126 / 626 / 126 grows the
    handle's workspace in STREAM ORDER (hipMallocAsync / hipFreeAsync on the caller's stream; fsnp_reserve jumps to the
    high-water mark at once).  An in-flight marker kernel spins on a second stream while the longer clip is enqueued: the call
    must return while the marker is still running (a hipDeviceSynchronize / hipFree inside would wait for it), and the results
    must equal those of a fresh handle."""
    sd = make_state_dict(0, "default")
    m = _model(DEFAULT_MODEL_ARGS, sd, "full")
    m.error_check = "deferred"
    short = _cuda(make_inputs(3, 2.0, 5))
    long_ = _cuda(make_inputs(3, 10.0, 6))
    a0 = m(*short)                                       # creates the handle, packs the weights, first workspace
    if reserve:
        m.reserve(3, 626)
    torch.cuda.synchronize()
    ticks = _sleep_cycles_for(1.5)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        torch.cuda._sleep(ticks)                         # the in-flight marker: ~1.5 s on its own stream
    t0 = time.perf_counter()
    b = m(*long_)                                        # needs a (much) larger workspace unless reserved
    c = m(*short)
    host_s = time.perf_counter() - t0
    still_running = not side.query()
    torch.cuda.synchronize()
    m.check_errors()
    _record(f"variable_clip_lengths_reserve_{int(reserve)}", host_ms_for_two_forwards=host_s * 1e3, marker_still_running=bool(still_running))
    assert still_running and host_s < 0.5, (still_running, host_s)
    fresh = _model(DEFAULT_MODEL_ARGS, sd, "full")
    assert torch.equal(b, fresh(*long_)) and torch.equal(c, a0) and torch.equal(c, fresh(*short))


def test_host_time_per_forward_b1():
    """Host cost of one B = 1 forward in the deferred error mode (the binding's parameter-version check + the C ABI's launches),
    measured as the enqueue rate of a burst that fits the queue: must stay a small fraction of the 2.2 ms device time per step.
    Recorded in gpurun_out/parity_report.json (profiles/)."""
    sd = make_state_dict(0, "default")
    m = _model(DEFAULT_MODEL_ARGS, sd, "full")
    m.error_check = "deferred"
    ins = _cuda(make_inputs(1, 2.0, 9))
    for _ in range(3):
        m(*ins)
    torch.cuda.synchronize()
    for _ in range(2):
        m(*ins)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(8):                                   # 8 forwards stay far below the HIP queue depth: pure host time
        m(*ins)
    host = (time.perf_counter() - t0) / 8
    torch.cuda.synchronize()
    dev = (time.perf_counter() - t0) / 8
    m.check_errors()
    _record("host_time_per_forward_b1", host_us_plain=host * 1e6, device_us_plain=dev * 1e6)
    assert host < 0.5 * dev, (host, dev)                 # the host runs well ahead of the device


def test_pipelined_enhance_paths_equal_the_plain_ones():
    """fsnp_enhance_wave / FullSubNet_Plus.enhance with the pipelined serving mode on: the mask's deferred rows (at B = 1 the whole
    sub-band plan runs on the side stream) must be complete before the cIRM epilogue reads them - same waveforms / spectra as
    with the pipeline off, call after call."""
    from fullsubnet_plus_amd.synthetic import make_wave
    sd = make_state_dict(0, "default")
    m = _model(DEFAULT_MODEL_ARGS, sd, "full")
    m.error_check = "deferred"
    for B in (1, 3):
        wav = torch.from_numpy(make_wave(B, 1.0, 50 + B)).cuda()
        spec = m.stft(wav).clone()
        want_w = m.enhance_wave(wav).clone()
        want_s = m.enhance(spec).clone()
        torch.cuda.synchronize()
        m.set_pipeline(True)
        try:
            for _ in range(3):
                got_w = m.enhance_wave(wav)
                got_s = m.enhance(spec)
                torch.cuda.synchronize()
                assert torch.equal(got_w, want_w) and torch.equal(got_s, want_s)
        finally:
            m.flush()
            torch.cuda.synchronize()
            m.set_pipeline(False)
    m.check_errors()


def test_forward_on_side_stream_and_second_handle():
    """fsnp_forward enqueues on the caller's current HIP stream (no device sync inside); two modules own two
    independent handles."""
    g = Golden("b3_t20_harsh")
    m1 = _model(g.args, g.state_dict(), "full")
    m2 = _model(g.args, g.state_dict(), "full")
    ins = _cuda(g.inputs())
    ref = m1(*ins).cpu().numpy()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        o1 = m1(*ins)
        o2 = m2(*ins)
    side.synchronize()
    assert np.array_equal(o1.cpu().numpy(), ref) and np.array_equal(o2.cpu().numpy(), ref)
    assert rel_err(ref, g.arrays["full"]) < TOL
    import copy
    m3 = copy.deepcopy(m1)                                # a copied module gets its own handle lazily
    assert np.array_equal(m3(*ins).cpu().numpy(), ref)


def test_subband_tcn_b32_full_vs_oracle():
    """sequence_model="TCN": 8 TCNBlocks(34 -> 512 -> 34) + Linear(34, 2) over all 8224 sub-band sequences."""
    args = {**DEFAULT_MODEL_ARGS, "sequence_model": "TCN"}
    sd = make_state_dict(33, "default", sequence_model="TCN")
    mag, real, imag = make_inputs(32, 1.0, 301)
    m = _model(args, sd, "full")
    out = m(*_cuda((mag, real, imag))).cpu().numpy()
    pick = [0, 16, 31]
    want = fsnp_torch.forward_full(sd, mag[pick], real[pick], imag[pick]).numpy()
    err = rel_err(out[pick], want)
    _record("subband_tcn_b32_full", rel=err)
    assert err < TOL, err
    with pytest.raises(RuntimeError, match="no recurrent kernel"):
        m.lstm2_fc(torch.zeros(4, 34, 5, device="cuda"))


def test_device_side_failure_is_reported_by_the_next_call():
    """A timed-out inter-workgroup wait sets a host-mapped error word: the next forward (or check_errors) raises once,
    then the handle works again."""
    g = Golden("b1_t8_min")
    m = _model(g.args, g.state_dict())
    ins = _cuda(g.inputs())
    ok = m(*ins).cpu().numpy()
    m.debug_inject_error()
    with pytest.raises(RuntimeError, match="timed out"):
        m(*ins)
    assert np.array_equal(m(*ins).cpu().numpy(), ok)
    m.debug_inject_error()
    with pytest.raises(RuntimeError, match="timed out"):
        m.check_errors()
    m.check_errors()


def test_sync_error_policy_reruns_on_the_row_tile_kernel():
    """error_check="sync" (the default): forward() waits for its own launches and polls the error word; a launch that
    flagged the handle is re-run once on the one-tile-per-CU kernel, with a warning - never a silently invalid result."""
    g = Golden("b1_t8_min")
    m = _model(g.args, g.state_dict())
    assert m.error_check == "sync"
    ins = _cuda(g.inputs())
    ok = m(*ins).cpu().numpy()
    orig, calls = m._forward_impl, []

    def flagged_once(*a, **k):
        out = orig(*a, **k)
        if not calls:
            m.debug_inject_error()          # what a timed-out inter-workgroup wait of THIS launch does
        calls.append(1)
        return out
    m._forward_impl = flagged_once
    with pytest.warns(RuntimeWarning, match="one-tile-per-CU"):
        got = m(*ins).cpu().numpy()
    m._forward_impl = orig
    assert len(calls) == 2
    assert rel_err(got, ok) < 1e-5                      # other kernel, same rows
    assert [c["kernel"] for c in m.describe_plan(1)][0].startswith("lstm2_coop")   # the tuning switch was put back
    m.error_check = "deferred"
    m._forward_impl = flagged_once
    calls.clear()
    m(*ins)
    m._forward_impl = orig
    with pytest.raises(RuntimeError, match="timed out"):
        m.poll_errors()
    m.poll_errors()


@pytest.mark.parametrize("batch,tiles", [(1, 9), (2, 17)])
def test_sampled_exchange_verification_catches_a_corruption_in_an_unsampled_tile_within_a_cycle(batch, tiles):
    """fsnp_set_verify_sample (round 6; the default of error_check="sync" at every 16th forward): ONE row tile per sampled forward - the
    tiles of a launch come up in turn - is recomputed on the exchange-free half-tile kernel from a snapshot, on a stream of its own.
    (1) Without a fault nothing fires and outputs stay bit-identical; every eligible forward is sampled when the previous sample has
    finished.  (2) The corruption hook damages row tile 0 of every forward; the sampler is first moved to tile 3, so tile 0 is NOT the
    sampled one: the detector must fire within one cycle over the tiles, name utterance 0 / bin 0, and stay quiet afterwards."""
    sd = make_state_dict(0, "default")
    m = _model(DEFAULT_MODEL_ARGS, sd, "full")
    ins = _cuda(make_inputs(batch, 0.6, 40 + batch))
    m.error_check = "deferred"
    m.verify_sample_every = 0
    plain = m(*ins).cpu().numpy()
    assert len(m.describe_plan(batch)) == 1 and m.describe_plan(batch)[0]["tiles"] == tiles
    m.verify_sample_every = 1
    for i in range(3):                                                   # samples 0, 1, 2 = tiles 0, 1, 2: clean
        assert np.array_equal(m(*ins).cpu().numpy(), plain)
        m.check_errors()                                                 # (device synchronisation: the sample has been compared)
    st = m.verify_sample_stats()
    assert st["samples"] == 3 and st["skipped"] == 0, st
    fired_after = None
    for i in range(tiles + 1):
        m.debug_corrupt_exchange(5)
        bad = m(*ins).cpu().numpy()
        assert rel_err(bad, plain) > 1e-4
        try:
            m.check_errors()
        except RuntimeError as e:
            assert "exchange verification failed" in str(e) and "utterance 0, bin 0, frame" in str(e), str(e)
            assert getattr(e, "code", None) == 7
            fired_after = i + 1
            break
    assert fired_after == tiles - 3 + 1, fired_after                     # tiles 3 ... tiles - 1 are clean, tile 0 comes up next
    assert np.array_equal(m(*ins).cpu().numpy(), plain)
    m.check_errors()
    # back to back without waiting: a sample is skipped while the previous one is still in flight - never queued up behind it
    before = m.verify_sample_stats()
    for _ in range(6):
        m(*ins)
    m.check_errors()
    after = m.verify_sample_stats()
    assert after["samples"] + after["skipped"] - before["samples"] - before["skipped"] == 6 and after["samples"] > before["samples"], (before, after)
    # the module's default policy: 16 under "sync", off under "deferred"
    m.verify_sample_every = None
    m.error_check = "sync"
    s0 = m.verify_sample_stats()["samples"]
    for _ in range(17):
        assert np.array_equal(m(*ins).cpu().numpy(), plain)
    m.check_errors()
    assert 1 <= m.verify_sample_stats()["samples"] - s0 <= 2


@pytest.mark.parametrize("batch,kernel,round4", [(1, "lstm2_coop_hpw_kernel", False), (2, "lstm2_coopw_kernel", False), (8, "lstm2_coopw_kernel", False),
                                                 (3, "lstm2_coop_kernel", True), (8, "lstm2_coopn_kernel", True)])
def test_exchange_verification_detects_a_corrupted_exchange(batch, kernel, round4):
    """the column-split kernels' hand-off can only detect a TIME-OUT; a stale or corrupted exchange image would give a
    silently wrong mask.  fsnp_set_verify (model.verify_every = N): every Nth forward whose plan holds a column-split launch runs
    those sequences again on the one-tile-per-CU kernel (no exchange) and compares on the device.  fsnp_debug_corrupt_exchange makes
    ONE published h0 value wrong (row 0, unit 0 of a launch's first row tile at one step; the publisher's own state stays right) -
    exactly what a stale exchange looks like to the consumers: the detector must fire, name the place, and the sync policy must
    hand back the right mask.  Without the corruption nothing fires and the verified forward equals the plain one bit for bit."""
    sd = make_state_dict(0, "default")
    m = _model(DEFAULT_MODEL_ARGS, sd, "full")
    ins = _cuda(make_inputs(batch, 0.6, 40 + batch))
    if round4:                                                           # the K split / the three-way split lead the plan again
        m(*ins)                                                          # (19 values: neither the wave-owned split nor the half-tile
        m.debug_set_costs(m.planner_costs_raw()[:19], 1)                 #  ping-pong launches, which round 6 made cheap enough to lead B = 3)
    plain = m(*ins).cpu().numpy()
    assert m.describe_plan(batch)[0]["kernel"].startswith(kernel), m.describe_plan(batch)
    m.verify_every = 1
    assert np.array_equal(m(*ins).cpu().numpy(), plain) and m.verify_count() == 1
    m.verify_every = 3                                                   # every third forward
    for _ in range(3):
        assert np.array_equal(m(*ins).cpu().numpy(), plain)
    assert m.verify_count() == 2
    m.verify_every = 1
    m.error_check = "deferred"
    m.debug_corrupt_exchange(5)
    bad = m(*ins)
    with pytest.raises(RuntimeError, match="exchange verification failed.*utterance 0, bin 0, frame") as ei:
        m.check_errors()
    assert rel_err(bad.cpu().numpy(), plain) > 1e-4                      # (the corruption really moved the mask)
    frame = int(str(ei.value).split("frame ")[1].split(";")[0])
    assert frame <= 4                                                    # h0 of step 4 is wrong: visible from frame 4 - look_ahead on
    assert np.array_equal(m(*ins).cpu().numpy(), plain)                  # one forward only
    m.check_errors()
    m.error_check = "sync"
    m.debug_corrupt_exchange(9)
    with pytest.warns(RuntimeWarning, match="exchange verification failed"):
        fixed = m(*ins).cpu().numpy()
    assert rel_err(fixed, plain) < 1e-5                                  # re-run on the one-tile-per-CU kernel
    m.verify_every = 0
    assert np.array_equal(m(*ins).cpu().numpy(), plain)
    if not round4:
        # bf16-ih mode (configs[4]) leaves the column-split kernels in fp32: their check must stay fp32 as well (no false alarm), and
        # the re-run of <= 4096 sequences is one round of HALF tiles (half the price of a row-tile round)
        m.set_precision("bf16_ih")
        m.verify_every = 1
        m.error_check = "deferred"
        before = m.verify_count()
        got = m(*ins)
        m.check_errors()
        assert m.verify_count() == before + 1 and np.array_equal(got.cpu().numpy(), plain)
        m.set_precision("fp32")


def test_two_handles_overlapped_on_two_streams():
    """Two modules on two streams, both on column-split kernels (all workgroups of a launch must be co-resident): the
    launches are chained per device inside the library, so the overlapped forwards complete and agree with the serial
    ones - without FSNP_LSTM_COOP=0."""
    g = Golden("b3_t20_harsh")
    m1, m2 = _model(g.args, g.state_dict(), "full"), _model(g.args, g.state_dict(), "full")
    ins = _cuda(g.inputs())
    ref = m1(*ins).cpu().numpy()
    m2(*ins)
    for m in (m1, m2):
        m.error_check = "deferred"
        assert all(not c["kernel"].startswith("lstm2_fc") for c in m.describe_plan(3))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = []
    for _ in range(6):
        with torch.cuda.stream(s1):
            outs.append(m1(*ins))
        with torch.cuda.stream(s2):
            outs.append(m2(*ins))
    torch.cuda.synchronize()
    m1.poll_errors()
    m2.poll_errors()
    for o in outs:
        assert np.array_equal(o.cpu().numpy(), ref)


@pytest.mark.parametrize("batch", [32, 40])
def test_pipelined_mode_is_bit_identical(batch):
    """fsnp_set_pipeline: the remainder chunks of the sub-band plan run on the handle's side stream, overlapped with the
    next forward's full-band stages, on a double-buffered workspace.  Same bits as the plain call, for every forward of a
    back-to-back loop over DIFFERENT inputs (a stale or shared workspace half would show up here)."""
    sd = make_state_dict(0, "default")
    m = _model(DEFAULT_MODEL_ARGS, sd, "full")
    m.error_check = "deferred"
    batches = [_cuda(make_inputs(batch, 0.5, 900 + i)) for i in range(3)]
    plain = [m(*b).clone() for b in batches]
    plan = m.describe_plan(batch)
    assert len(plan) > 1 and plan[0]["kernel"].startswith("lstm2_fc") and not plan[-1]["kernel"].startswith("lstm2_fc")
    torch.cuda.synchronize()
    m.set_pipeline(True)
    piped = [m(*b) for b in batches] + [m(*batches[0])]
    m.flush()
    torch.cuda.synchronize()
    m.poll_errors()
    for a, b in zip(piped, plain + [plain[0]]):
        assert torch.equal(a, b)
    m.set_pipeline(False)
    assert torch.equal(m(*batches[1]), plain[1])


def test_pipelined_loop_at_every_plan_shape():
    """fsnp_set_pipeline at one batch per plan signature of B = 1 ... 128 (sub-band kernels, their tile counts, which launches are deferred
    to the side stream): a back-to-back loop over three different inputs and a repeat under error_check="deferred" is the plain call, bit
    for bit, after flush / poll_errors, and so is a final error_check="sync" call."""
    sd = make_state_dict(2, "default")
    m = _model(DEFAULT_MODEL_ARGS, sd, "full")
    m(*_cuda(make_inputs(1, 0.3, 1199)))                   # (the handle is made by the first forward)
    sig = {}
    for b in range(1, 129):
        key = tuple((c["kernel"], c["tiles"], c["deferred_when_pipelined"]) for c in m.describe_plan(b))
        sig.setdefault(key, []).append(b)
    chosen = sorted(v[0] for v in sig.values())
    if len(chosen) > 24:
        chosen = [chosen[round(i * (len(chosen) - 1) / 23)] for i in range(24)]
    _record("pipelined_plan_shapes", batches=chosen, signatures=len(sig))
    print("pipelined FullSubNet+ batches:", chosen)
    for b in chosen:
        m.error_check = "deferred"
        xs = [_cuda(make_inputs(b, 0.3, 1200 + 7 * b + i)) for i in range(3)]
        plain = [m(*x).clone() for x in xs]
        torch.cuda.synchronize()
        m.set_pipeline(True)
        try:
            seq = [0, 1, 2, 0]
            piped = [m(*xs[i]) for i in seq]
            m.flush()
            torch.cuda.synchronize()
            m.poll_errors()
            for k, (i, y) in enumerate(zip(seq, piped)):
                assert torch.equal(y, plain[i]), (b, k)
            m.error_check = "sync"
            assert torch.equal(m(*xs[1]), plain[1]), b
            m.check_errors()
        finally:
            m.set_pipeline(False)
            m.error_check = "sync"


@pytest.mark.parametrize("batch,mode,two_per_cu", [(1, "full", False), (3, "full", False), (8, "full", False), (16, "full", False),
                                                   (12, "parity", False), (40, "full", True), (5, "full", False)])
def test_pipelined_small_batches_run_whole_on_the_side_stream(batch, mode, two_per_cu):
    """Plans that START with a column-split launch (B = 1: one K-split launch on 216 CUs; B = 8: three-way split) are sent to the
    side stream whole in pipelined mode, so that the next forward's full-band stages run beside them (their workgroups claim
    the CU's LDS: no GEMM workgroup shares a CU with them).  Bit-identical to the plain call over a loop of different inputs;
    B = 16 (half-tile round + K-split remainder) takes the older deferred-remainder path."""
    sd = make_state_dict(3, "default")
    m = _model(DEFAULT_MODEL_ARGS, sd, mode)
    m.error_check = "deferred"
    batches = [_cuda(make_inputs(batch, 0.4, 1300 + i)) for i in range(4)]
    if two_per_cu:        # a plan with TWO column-split workgroups per CU must not claim the CU's whole LDS (they would not be co-resident)
        m(*batches[0])
        table = list(CHEAP_TWO_PER_CU)
        table[12] = 100.0                           # (a cheap row-tile round: B = 40 = 8192 sequences that fill the chip + a 66-tile
        m.debug_set_costs(table, 2)                 #  remainder in column-split launches, those that fit twice two per CU: 21 tiles
        plan = m.describe_plan(batch)               #  K split at 16 units = 504 workgroups - all deferred)
        assert plan[0]["kernel"].startswith("lstm2_fc_kernel") and len(plan) >= 2 and sum(c["tiles"] for c in plan[1:]) == 66, plan
        assert all("K split" in c["kernel"] or "three-way" in c["kernel"] for c in plan[1:]), plan
    plain = [m(*b).clone() for b in batches]
    torch.cuda.synchronize()
    m.set_pipeline(True)
    piped = [m(*b) for b in batches] + [m(*batches[0]), m(*batches[2])]
    m.flush()
    torch.cuda.synchronize()
    m.poll_errors()
    for a, b in zip(piped, plain + [plain[0], plain[2]]):
        assert torch.equal(a, b)
    m.error_check = "sync"                     # the sync policy flushes + polls after every call
    assert torch.equal(m(*batches[3]), plain[3])
    m.set_pipeline(False)
    assert torch.equal(m(*batches[1]), plain[1])


# ---------------------------------------------------------------- STFT / iSTFT / waveform -> waveform
@pytest.mark.parametrize("B,L", [(1, 32000), (3, 16000), (2, 12345), (1, 300)])
def test_stft_istft_vs_torch(B, L):
    """fsnp_stft / fsnp_istft (DFT as an fp32 MFMA GEMM) vs torch.stft / torch.istft on the CPU, the calls of
    audio_zen/acoustics/feature.py:10-56; plus the size-independent round trip istft(stft(x)) == x."""
    from oracle.weights import make_wave
    m = _model(DEFAULT_MODEL_ARGS, make_state_dict(0))
    wav = torch.from_numpy(make_wave(B, L / 16000.0, 400 + L))
    assert wav.shape == (B, L)
    want = fsnp_torch.stft(wav)
    got = m.stft(wav.cuda())
    assert got.shape == want.shape and got.stride() == want.stride()
    e_stft = float((got.cpu() - want).abs().max() / want.abs().max())
    back = m.istft(got, L).cpu()
    e_rt = float((back - wav).abs().max() / wav.abs().max())
    rng = torch.Generator().manual_seed(L)
    spec = torch.complex(torch.randn(B, 257, want.shape[-1], generator=rng), torch.randn(B, 257, want.shape[-1], generator=rng))
    w_i = fsnp_torch.istft(spec, L)
    g_i = m.istft(spec.cuda(), L).cpu()
    e_istft = float((g_i - w_i).abs().max() / w_i.abs().max())
    _record(f"stft_B{B}_L{L}", stft=e_stft, round_trip=e_rt, istft=e_istft)
    assert e_stft < 1e-5 and e_rt < 1e-5 and e_istft < 1e-5
    with pytest.raises(RuntimeError, match="reflect padding"):
        m.stft(torch.zeros(1, 200, device="cuda"))


def test_enhance_wave_vs_oracle():
    """fsnp_enhance_wave == inferencer.py:142-158 (stft -> model -> cIRM -> istft) run with torch on the CPU."""
    from oracle.weights import make_wave
    sd = make_state_dict(41, "harsh")
    m = _model(DEFAULT_MODEL_ARGS, sd, "parity")
    wav = torch.from_numpy(make_wave(3, 1.0, 500))
    got = m.enhance_wave(wav.cuda()).cpu()
    want = fsnp_torch.enhance_wave(sd, wav)
    err = float((got - want).abs().max() / want.abs().max())
    _record("enhance_wave", rel=err)
    assert got.shape == wav.shape and err < TOL, err
    # the two-step form (HIP stft -> enhance() -> HIP istft) is the same computation
    two = m.istft(m.enhance(m.stft(wav.cuda())), wav.shape[-1]).cpu()
    assert float((two - got).abs().max() / want.abs().max()) < 1e-5


@pytest.mark.parametrize("splits", [(16, 16), (5, 20, 7)])
def test_sharded_parity_mode_on_one_gpu(b32, splits):
    """Multi-GPU plumbing on the real kernels: a shard passes (batch_offset, global_batch) and writes only its rows of
    the GLOBAL drop_band output (frequency parity and row order follow the global sample index, feature.py:254-285);
    the shards' outputs sum to the unsharded call (what dist.forward_sharded's gather of row blocks assembles)."""
    sd, (mag, real, imag), m, _ = b32
    m.batch_mode = "parity"
    ins = _cuda((mag, real, imag))
    whole = m(*ins).cpu().numpy()
    acc = np.zeros_like(whole)
    lo = 0
    for n in splits:
        part = m(*[t[lo:lo + n] for t in ins], batch_offset=lo, global_batch=32).cpu().numpy()
        assert part.shape == whole.shape
        acc += part
        lo += n
    assert lo == 32
    m.batch_mode = "full"
    # shards of other sizes run other sub-band kernels (K-split / three-way split): same rows, different summation order
    assert rel_err(acc, whole) < 1e-5


@pytest.mark.parametrize("n,steps", [(8192 + 40, 5), (8192 + 1500, 4), (8192 + 4000, 4), (8192 + 6000, 3), (16384 + 70, 3)])
def test_lstm2_fc_composite_plans(n, steps):
    """More sequences than one round of the row-tile kernel: full rounds (256 x 32 rows) + the remainder on a column-split
    kernel when that is estimated cheaper than VALU rows / another round (fsnp_abi.hip plan_sb): 2 / 47 / 125 remainder
    tiles, a remainder too large for one column-split launch, and two full rounds + 3 tiles."""
    sd = make_state_dict(9, "harsh")
    m = _model(DEFAULT_MODEL_ARGS, sd)
    rng = np.random.Generator(np.random.PCG64(177 + n))
    x = torch.from_numpy(rng.standard_normal((n, 34, steps)).astype(np.float32))
    want = fsnp_torch.lstm2_fc(x, sd).numpy()
    got = m.lstm2_fc(x.cuda()).cpu().numpy()
    m.check_errors()
    err = rel_err(got, want)
    _record(f"lstm_composite_{n}x{steps}", rel=err)
    assert err < 2e-5, err
    m.debug_set_lstm_coop(0)                               # single row-tile plan
    assert rel_err(m.lstm2_fc(x.cuda()).cpu().numpy(), want) < 2e-5


def test_forward_b40_composite_vs_oracle():
    """B = 40 in full mode: 10280 sequences = one full row-tile round + 66 tiles on lstm_coopn.hip."""
    sd = make_state_dict(51, "default")
    mag, real, imag = make_inputs(40, 0.5, 302)
    for norm in ("offline_laplace_norm", "cumulative_layer_norm"):
        m = _model({**DEFAULT_MODEL_ARGS, "norm_type": norm}, sd, "full")
        out = m(*_cuda((mag, real, imag))).cpu().numpy()
        m.check_errors()
        pick = [0, 31, 32, 39]                             # utterances on both sides of the chunk boundary (row 8192 = utt 31)
        want = fsnp_torch.forward_full(sd, mag[pick], real[pick], imag[pick], norm_type=norm).numpy()
        err = rel_err(out[pick], want)
        _record(f"forward_b40_composite_{norm}", rel=err)
        assert err < TOL, err


@pytest.mark.parametrize("n,steps", [(257, 60), (1300, 20), (2750, 12)])
def test_column_split_exchange_under_load(n, steps):
    """The write-through inter-workgroup hand-off (sc1 stores / sc1 loads, no fences; csrc/lstm_common.h) under UNEVEN
    load: a bandwidth-heavy torch kernel hammers HBM / L2 on a second stream while the column-split kernels run;
    25 repetitions must be bit-identical to the quiet run and match the oracle (a stale read shows up as garbage)."""
    sd = make_state_dict(61, "harsh")
    m = _model(DEFAULT_MODEL_ARGS, sd)
    rng = np.random.Generator(np.random.PCG64(277 + n))
    x = torch.from_numpy(rng.standard_normal((n, 34, steps)).astype(np.float32)).cuda()
    quiet = m.lstm2_fc(x)
    want = fsnp_torch.lstm2_fc(x.cpu(), sd).numpy()
    assert rel_err(quiet.cpu().numpy(), want) < 2e-5
    side = torch.cuda.Stream()
    junk = torch.empty(64 * 1024 * 1024, device="cuda")           # 256 MB: beyond every cache level
    outs = []
    for i in range(25):
        with torch.cuda.stream(side):
            for _ in range(3):
                junk.mul_(1.0001).add_(0.5)
        outs.append(m.lstm2_fc(x))
    torch.cuda.synchronize()
    m.check_errors()
    for o in outs:
        assert torch.equal(o, quiet)


def test_c_abi_argument_errors_are_loud():
    """Error behaviour behind the Python asserts: too few frames for the TSSE kernels (the reference would fail inside
    Conv1d, attention_model.py:86), empty batches, wrong frequency count - a RuntimeError with the C message, never a
    wrong result; the handle keeps working afterwards."""
    g = Golden("b1_t8_min")
    m = _model(g.args, g.state_dict())
    ins = _cuda(g.inputs())
    ok = m(*ins).cpu().numpy()
    with pytest.raises(RuntimeError, match="too few frames"):
        m(*[t[..., :7] for t in ins])                       # T + look_ahead = 9 < kernel size 10
    with pytest.raises(RuntimeError, match="empty input"):
        m(*[t[:0] for t in ins])
    with pytest.raises(AssertionError):
        m(*[t[:, :, :200] for t in ins])
    assert np.array_equal(m(*ins).cpu().numpy(), ok)


def test_subband_tcn_with_cumulative_norm_vs_oracle():
    """sequence_model="TCN" + cumulative_layer_norm: the materialised sub-band input uses the per-sequence (m_t, d_t)
    tables (sb_cumulative_kernel -> sb_gather_kernel)."""
    args = {**DEFAULT_MODEL_ARGS, "sequence_model": "TCN", "norm_type": "cumulative_layer_norm"}
    sd = make_state_dict(34, "harsh", sequence_model="TCN")
    cpu_in = make_spec(3, 18, 303)
    m = _model(args, sd, "parity")
    out = m(*_cuda(cpu_in)).cpu().numpy()
    want = fsnp_torch.forward(sd, *cpu_in, norm_type="cumulative_layer_norm").numpy()
    err = rel_err(out, want)
    _record("subband_tcn_cumulative_layer", rel=err)
    assert out.shape == want.shape and err < TOL, err


def test_forward_from_plain_c(tmp_path):
    """The C ABI is self-sufficient: a plain C program (tests/c_abi/abi_forward.c: fsnp.h + the HIP runtime C API, no
    Python, no torch) loads the named weights, runs fsnp_forward on its own hipMalloc'ed buffers and reproduces the
    golden vector of the reference."""
    import ctypes
    import shutil
    import struct
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    from fullsubnet_plus_amd import _build, _lib
    g = Golden("b3_t20_harsh")
    m = FullSubNet_Plus(**g.args)
    sd = g.state_dict()
    cfg = m._config()
    (tmp_path / "config.bin").write_bytes(bytes(ctypes.string_at(ctypes.byref(cfg), ctypes.sizeof(cfg))))
    with open(tmp_path / "weights.bin", "wb") as f:
        for name, t in sd.items():
            arr = t.numpy().astype(np.float32).ravel()
            f.write(struct.pack("<i", len(name)) + name.encode() + struct.pack("<q", arr.size) + arr.tobytes())
    mag, real, imag = g.inputs()
    B, _, F, T = mag.shape
    for nm, t in (("mag", mag), ("real", real), ("imag", imag)):
        (tmp_path / f"{nm}.bin").write_bytes(t.contiguous().numpy().tobytes())
    (tmp_path / "dims.bin").write_bytes(struct.pack("<4i", B, F, T, _lib.MODE_PARITY))
    libdir = os.path.dirname(_build.LIB_PATH)
    exe = tmp_path / "abi_forward"
    cmd = ["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
           os.path.join(ROOT, "tests", "c_abi", "abi_forward.c"), "-o", str(exe), "-L", libdir, "-lfsnp_hip",
           "-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    run = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    out = np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.float32).reshape(g.arrays["out"].shape)
    err = rel_err(out, g.arrays["out"])
    _record("forward_from_plain_c", rel=err)
    assert err < TOL, err

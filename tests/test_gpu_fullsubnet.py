"""GPU parity tests of SURVEY.md 8(f-2): the original FullSubNet ``Model``
(speech_enhance/fullsubnet/model/fullsubnet.py:12-118) on the HIP kernels, through the C ABI, against the golden
vectors the REAL reference produced (tests/golden/fsn_*.npz, oracle/make_golden.py) and the torch-CPU oracle
(oracle/fsnp_torch.forward_fullsubnet) at the benchmark size.  Tolerance: 1e-3 rel (BASELINE.json north_star)."""
import json
import os

import numpy as np
import pytest
import torch

from fullsubnet_plus_amd import FullSubNet
from oracle import fsnp_torch
from oracle.ref_loader import FULLSUBNET_MODEL_ARGS
from oracle.weights import make_inputs, make_state_dict_fullsubnet
from tests._util import FB_LSTM_CAP, Golden, golden_names, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}

torch.set_num_threads(min(16, os.cpu_count() or 1))


def _record(name, **kw):
    REPORT[name] = {k: (float(v) if isinstance(v, (float, np.floating)) else v) for k, v in kw.items()}
    out = os.path.join(ROOT, "gpurun_out")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "parity_report_fullsubnet.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


def _model(args, sd, mode="parity"):
    m = FullSubNet(**args)
    m.load_state_dict(sd, strict=True)
    m = m.to("cuda").eval()
    m.batch_mode = mode
    return m


def _cuda(t):
    g = torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device="cuda")
    g.copy_(t)
    return g


@pytest.mark.parametrize("name", golden_names("fullsubnet"))
def test_fullsubnet_forward_vs_reference_golden(name):
    g = Golden(name)
    m = _model(g.args, g.state_dict(), "parity")
    mag = g.inputs()[0]
    B, T = mag.shape[0], mag.shape[-1]
    out = m(_cuda(mag)).cpu().numpy()
    m.check_errors()
    want = g.arrays["out"]
    assert out.shape == want.shape
    err, err64 = rel_err(out, want), rel_err(out, g.arrays["out64"])
    rec = dict(rel_vs_ref32=err, rel_vs_ref64=err64, ref32_vs_ref64=rel_err(want, g.arrays["out64"]))
    if "stage_fb_mag" in g.arrays:            # full-band LSTM + Linear + ReLU output, [B,F,T'] (forward hook on fb_model)
        fb = m.read_stage("fb_mag", B, T).permute(0, 2, 1).numpy()
        rec["fb_stage"] = rel_err(fb, g.arrays["stage_fb_mag"])
    _record(f"forward_{name}", **rec)
    assert err < TOL, rec
    if "fb_stage" in rec:
        assert rec["fb_stage"] < FB_LSTM_CAP, rec      # (<= 8.5e-7 measured; tests/test_gpu_fullband_lstm.py checks the stage per kernel path)
    if "full" in g.arrays:
        m.batch_mode = "full"
        full = m(_cuda(mag)).cpu().numpy()
        errf = rel_err(full, g.arrays["full"])
        _record(f"forward_full_{name}", rel_vs_ref32=errf)
        assert errf < TOL, errf


@pytest.mark.parametrize("batch", [32, 40])
def test_fullsubnet_batch_vs_oracle(batch):
    """Benchmark-sized call (one / two full-band row tiles, all bins) vs the oracle, + bitwise repeatability."""
    sd = make_state_dict_fullsubnet(11, "harsh")
    mag = make_inputs(batch, 1.0 if batch > 32 else 2.0, 31)[0]
    m = _model(dict(FULLSUBNET_MODEL_ARGS), sd, "full")
    x = _cuda(mag)
    out = m(x)
    out2 = m(x)
    m.check_errors()
    assert torch.equal(out, out2)
    kw = {k: FULLSUBNET_MODEL_ARGS[k] for k in ("look_ahead", "sb_num_neighbors", "fb_num_neighbors", "norm_type",
                                                "num_groups_in_drop_band", "fb_output_activate_function",
                                                "sb_output_activate_function")}
    pick = [0, batch // 2, batch - 1]          # the oracle is slow: check three utterances of the batch
    want = fsnp_torch.forward_fullsubnet_full(sd, mag[pick], **kw).numpy()
    err = rel_err(out[pick].cpu().numpy(), want)
    _record(f"fullsubnet_b{batch}_full_vs_oracle", rel=err)
    assert err < TOL, err
    # parity mode rows are a sub-selection of the full rows (drop_band, feature.py:254-285)
    m.batch_mode = "parity"
    par = m(x).cpu().numpy()
    full = out.cpu().numpy()
    n0 = (batch + 1) // 2
    for r in (0, 1, n0 - 1, n0, batch - 1):
        s, p = (2 * r, 0) if r < n0 else (2 * (r - n0) + 1, 1)
        assert np.abs(par[r] - full[s][:, p:256:2, :]).max() <= 1e-6 * np.abs(full).max()


@pytest.mark.parametrize("batch,seconds", [(1, 2.0), (2, 0.7), (3, 1.0), (4, 0.5), (1, 30.0)])
def test_fullsubnet_small_batches_run_the_full_band_lstm_on_the_valu(batch, seconds):
    """csrc/lstm_fbv.hip (round 5): with 1 ... 4 utterances the full-band LSTM(257 -> 512 x 2) of fullsubnet.py:39-47 is a matrix-VECTOR
    product per step - 64 workgroups x 8 units, weights resident, plain FMAs, one hand-off per step - instead of 32-row MFMA tiles with
    one live row.  Against the oracle, against the K-split kernel it replaces (debug mode 2 keeps that one), bitwise repeatable, under
    drift injection; 1 ... 4 rows (NB = 1, 2, 4 instantiations, a padded row at B = 3) and a 30 s clip (1,877 steps)."""
    sd = make_state_dict_fullsubnet(14, "harsh")
    mag = make_inputs(batch, seconds, 60 + batch)[0]
    m = _model(dict(FULLSUBNET_MODEL_ARGS), sd, "full")
    x = _cuda(mag)
    out = m(x)
    m.check_errors()
    assert torch.equal(m(x), out)
    T = mag.shape[-1]
    fb_valu = m.read_stage("fb_mag", batch, T).numpy()
    for seed in (3, 99):
        m.debug_set_chaos(seed)
        assert torch.equal(m(x), out), seed
    m.debug_set_chaos(0)
    m.debug_set_lstm_coop(2)                       # the round-4 kernels: K-split full-band LSTM, serial schedules
    ref = m(x)
    m.check_errors()
    fb_mfma = m.read_stage("fb_mag", batch, T).numpy()
    m.debug_set_lstm_coop(1)
    assert rel_err(fb_valu, fb_mfma) < 1e-5 and not np.array_equal(fb_valu, fb_mfma)      # (another kernel really ran)
    assert rel_err(out.cpu().numpy(), ref.cpu().numpy()) < 1e-5
    if seconds <= 2.0:
        kw = {k: FULLSUBNET_MODEL_ARGS[k] for k in ("look_ahead", "sb_num_neighbors", "fb_num_neighbors", "norm_type",
                                                    "num_groups_in_drop_band", "fb_output_activate_function",
                                                    "sb_output_activate_function")}
        want = fsnp_torch.forward_fullsubnet_full(sd, mag, **kw).numpy()
        err = rel_err(out.cpu().numpy(), want)
        _record(f"fullsubnet_valu_b{batch}", rel=err, fb_valu_vs_mfma=rel_err(fb_valu, fb_mfma))
        assert err < TOL, err


@pytest.mark.parametrize("batch", [32, 16])
def test_fullsubnet_pipelined_loop_is_bit_identical(batch):
    """fsnp_set_pipeline on the original FullSubNet: the deferred remainder chunk of forward i (side stream) and the full-band LSTM of
    forward i + 1 (caller's stream) are both column-split launches.  Round 6 lets them run side by side (csrc/fsnp_abi.hip
    launch_coop_chained: launches of ONE handle whose workgroups fit the chip together are not chained - B = 32: 29.7 -> 28.5 ms per
    forward); the masks of a back-to-back loop over different inputs must be the plain call's, bit for bit, and no hand-off may time out."""
    sd = make_state_dict_fullsubnet(0, "default")
    m = _model(FULLSUBNET_MODEL_ARGS, sd, "full")
    m.error_check = "deferred"
    batches = [make_inputs(batch, 0.5, 700 + i)[0].cuda() for i in range(3)]
    plain = [m(b).clone() for b in batches]
    torch.cuda.synchronize()
    assert any(c["deferred_when_pipelined"] for c in m.describe_plan(batch)), m.describe_plan(batch)
    m.set_pipeline(True)
    piped = [m(b) for b in batches * 4]
    m.flush()
    torch.cuda.synchronize()
    m.poll_errors()
    for a, b in zip(piped, plain * 4):
        assert torch.equal(a, b)
    m.set_pipeline(False)
    assert torch.equal(m(batches[1]), plain[1])
    m.check_errors()


FSN_KW = ("look_ahead", "sb_num_neighbors", "fb_num_neighbors", "norm_type", "num_groups_in_drop_band", "fb_output_activate_function",
          "sb_output_activate_function")
# 1 ... 16 full-band row tiles (8 / 16 / 32 units per workgroup), exactly full and one-row tiles, sub-band plans with 0 ... 16 full rounds
RANGE_BATCHES = [5, 8, 17, 31, 33, 48, 63, 64, 65, 96, 97, 128, 160, 255, 256, 257, 320, 511, 512]


def _picked_utterances(m, batch, limit=6):
    """The first and the last utterance, those holding a sub-band chunk boundary (describe_plan: sequences // 257) and both sides of
    32-row full-band tile boundaries (the last, then the first, then the middle one), at most `limit`."""
    cand = [0, batch - 1]
    row = 0
    for c in m.describe_plan(batch)[:-1]:
        row += c["sequences"]
        cand += [(row - 1) // 257, row // 257]
    bounds = list(range(32, batch, 32))
    for b in (bounds[-1:] + bounds[:1] + bounds[len(bounds) // 2:len(bounds) // 2 + 1]) if bounds else []:
        cand += [b - 1, b]
    out = []
    for u in cand:
        if u not in out and len(out) < limit:
            out.append(u)
    return sorted(out)


@pytest.mark.parametrize("batch", RANGE_BATCHES)
def test_fullsubnet_batch_range_vs_oracle(batch):
    """The full-band LSTM (257 -> 512 x 2) on lstm_coop_seq in 32-row tiles across the batch range the model accepts (B = 5 ... 512:
    1 ... 16 tiles, 256 workgroups at the top) and the sub-band plans those batches get, on 0.3 s clips against the fp32 oracle: the
    first / last utterance, both sides of full-band tile boundaries and the utterances holding the sub-band chunk boundaries; a second
    call is bitwise equal; parity-mode rows are a sub-selection of the full rows."""
    sd = make_state_dict_fullsubnet(11, "harsh")
    mag = make_inputs(batch, 0.3, 400 + batch)[0]
    m = _model(dict(FULLSUBNET_MODEL_ARGS), sd, "full")
    x = _cuda(mag)
    out = m(x)
    out2 = m(x)
    fb = m.fullband_launch(batch)
    tiles = -(-batch // 32)
    assert fb == {"kernel": "coop_seq", "tiles": tiles, "rows_per_tile": 32, "units": 8 if tiles <= 4 else 16 if tiles <= 8 else 32}, fb
    m.check_errors()
    assert torch.equal(out, out2)
    pick = _picked_utterances(m, batch)
    want = fsnp_torch.forward_fullsubnet_full(sd, mag[pick], **{k: FULLSUBNET_MODEL_ARGS[k] for k in FSN_KW}).numpy()
    err = rel_err(out[pick].cpu().numpy(), want)
    _record(f"fullsubnet_range_b{batch}_full_vs_oracle", rel=err, utterances=pick, fb_units=fb["units"],
            plan=[(c["kernel"].split()[0], c["tiles"]) for c in m.describe_plan(batch)])
    assert err < TOL, (err, pick)
    m.batch_mode = "parity"
    par = m(x).cpu().numpy()
    m.check_errors()
    full = out.cpu().numpy()
    n0 = (batch + 1) // 2
    for r in sorted({0, 1, n0 - 1, n0, batch - 1}):
        s, p = (2 * r, 0) if r < n0 else (2 * (r - n0) + 1, 1)
        assert np.abs(par[r] - full[s][:, p:256:2, :]).max() <= 1e-6 * np.abs(full).max(), r


@pytest.mark.parametrize("batch,rows_per_group", [(3, 1), (31, 1), (32, 2), (127, 2), (128, 4), (200, 4)])
def test_fullsubnet_runtime_sized_fullband_across_batches(batch, rows_per_group):
    """fb_model_hidden_size = 300 (no K-split instantiation): the full-band LSTM runs on the runtime-sized kernel (lstm_generic.hip), whose
    sequences per workgroup grow with the batch (lstm_generic_rows_per_group: 1 / 2 / 4 from 32 / 128 sequences) - both sides of each step,
    against the oracle, with the rows per group the handle used read back."""
    args = dict(FULLSUBNET_MODEL_ARGS, fb_model_hidden_size=300)
    sd = make_state_dict_fullsubnet(15, "default", fb_hidden=300)
    mag = make_inputs(batch, 0.3, 600 + batch)[0]
    m = _model(args, sd, "full")
    x = _cuda(mag)
    out = m(x)
    m.check_errors()
    fb = m.fullband_launch(batch)
    assert fb["kernel"] == "generic" and fb["rows_per_tile"] == rows_per_group and fb["tiles"] == -(-batch // rows_per_group), fb
    assert torch.equal(m(x), out)
    pick = sorted({0, batch // 2, batch - 1} | ({rows_per_group * (batch // rows_per_group) - 1} if batch >= rows_per_group else set()))
    want = fsnp_torch.forward_fullsubnet_full(sd, mag[pick], **{k: args[k] for k in FSN_KW}).numpy()
    err = rel_err(out[pick].cpu().numpy(), want)
    _record(f"fullsubnet_generic_fb300_b{batch}_full_vs_oracle", rel=err, utterances=pick, rows_per_group=rows_per_group)
    assert err < TOL, (err, pick)


def _pipelined_loop_matches_plain(m, batch, seed):
    """A back-to-back pipelined loop over three different inputs and a repeat (error_check="deferred") = the plain calls, bit for bit;
    then one error_check="sync" call.  -> coop_chain_stats() of the pipelined calls (the plain calls leave only launches on the caller's
    stream behind them)."""
    m.error_check = "deferred"
    xs = [_cuda(make_inputs(batch, 0.3, seed + i)[0]) for i in range(3)]
    plain = [m(x).clone() for x in xs]
    torch.cuda.synchronize()
    m.coop_chain_stats(reset=True)
    m.set_pipeline(True)
    try:
        seq = [0, 1, 2, 0]
        piped = [m(xs[i]) for i in seq]
        m.flush()
        torch.cuda.synchronize()
        m.poll_errors()
        for k, (i, y) in enumerate(zip(seq, piped)):
            assert torch.equal(y, plain[i]), (batch, k)
        m.error_check = "sync"
        assert torch.equal(m(xs[1]), plain[1]), batch
        m.check_errors()
        return m.coop_chain_stats()
    finally:
        m.set_pipeline(False)
        m.error_check = "sync"


def _pick_by_signature(batches, signature, limit=24):
    groups = {}
    for b in batches:
        groups.setdefault(signature(b), []).append(b)
    chosen = sorted(v[0] for v in groups.values())
    if len(chosen) > limit:
        chosen = [chosen[round(i * (len(chosen) - 1) / (limit - 1))] for i in range(limit)]
    return chosen, len(groups)


def test_fullsubnet_pipelined_loop_at_every_plan_shape():
    """fsnp_set_pipeline on the original FullSubNet at one batch per plan signature of the range above (sub-band kernels and tiles, what is
    deferred, the full-band launch, and whether that launch runs beside the deferred chunk - csrc/planner.h coop_side_by_side, per XCD):
    the handle's decision equals the host predicate fed this device's CU count and the full-band kernel's measured occupancy
    (fsnp_debug_fullsubnet_pairing), the launches really ran beside / were chained as decided, and every output is the plain call's."""
    import ctypes
    from fullsubnet_plus_amd import _lib
    sd = make_state_dict_fullsubnet(0, "default")
    m = _model(FULLSUBNET_MODEL_ARGS, sd, "full")
    m(_cuda(make_inputs(1, 0.3, 799)[0]))                 # (the handle is made by the first forward)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lib = _lib.load()

    def signature(b):
        fb = m.fullband_launch(b)
        return (tuple((c["kernel"], c["tiles"], c["deferred_when_pipelined"]) for c in m.describe_plan(b)),
                (fb["kernel"], fb["tiles"], fb["units"]), tuple(r["side_by_side"] for r in m.pipeline_pairing(b)))

    batches = [1, 2, 4, 16, 32] + RANGE_BATCHES
    for b in batches:                                  # the handle's decision = the host predicate's, for every batch of the range
        dev = m.pipeline_pairing(b)
        per_cu = {r["fb_per_cu"] for r in dev if r["fb_workgroups"]} or {1}
        assert len(per_cu) == 1, dev
        buf = (ctypes.c_int32 * (9 * 16))()
        n = lib.fsnp_debug_fullsubnet_pairing(b, cus, per_cu.pop(), None, buf, 16)
        assert n == len(dev) and [list(r.values()) for r in dev] == [list(buf[9 * i:9 * i + 9]) for i in range(n)], (b, dev)
    chosen, nsig = _pick_by_signature(batches, signature)
    _record("fullsubnet_pipelined_plan_shapes", batches=chosen, signatures=nsig,
            pairing={b: m.pipeline_pairing(b) for b in chosen})
    print("pipelined FullSubNet batches:", chosen)
    for b in chosen:
        beside, chained = _pipelined_loop_matches_plain(m, b, 800 + b)
        pairs = [r for r in m.pipeline_pairing(b) if r["fb_workgroups"]]
        if any(r["side_by_side"] for r in pairs):
            assert beside > 0 and chained == 0, (b, beside, chained, pairs)
        else:
            assert beside == 0, (b, beside, chained, pairs)
            if pairs:
                assert chained > 0, (b, beside, chained, pairs)


def test_fullsubnet_enhance_epilogue():
    sd = make_state_dict_fullsubnet(12, "default")
    mag, real, imag = make_inputs(2, 1.0, 32)
    X = torch.complex(real[:, 0], imag[:, 0])
    m = _model(dict(FULLSUBNET_MODEL_ARGS), sd, "parity")
    Xg = torch.empty_strided(X.shape, X.stride(), dtype=X.dtype, device="cuda")
    Xg.copy_(X)
    got = m.enhance(Xg).cpu()
    kw = {k: FULLSUBNET_MODEL_ARGS[k] for k in ("look_ahead", "sb_num_neighbors", "fb_num_neighbors", "norm_type",
                                                "num_groups_in_drop_band", "fb_output_activate_function",
                                                "sb_output_activate_function")}
    mask = fsnp_torch.forward_fullsubnet_full(sd, X.abs().unsqueeze(1), **kw)
    want = fsnp_torch.apply_cirm(mask, X)
    err = float((got - want).abs().max() / want.abs().max())
    _record("fullsubnet_enhance", rel=err)
    assert err < TOL


def test_fullsubnet_rejects_oversized_batch():
    m = _model(dict(FULLSUBNET_MODEL_ARGS), make_state_dict_fullsubnet(0), "full")
    x = torch.rand(513, 1, 257, 9, device="cuda")
    with pytest.raises(RuntimeError, match="split the batch"):
        m(x)


def test_fullsubnet_enhance_wave_vs_oracle():
    from oracle.weights import make_wave
    sd = make_state_dict_fullsubnet(13, "harsh")
    m = _model(dict(FULLSUBNET_MODEL_ARGS), sd)
    wav = torch.from_numpy(make_wave(2, 1.0, 501))
    got = m.enhance_wave(wav.cuda()).cpu()
    want = fsnp_torch.enhance_wave(sd, wav, fullsubnet=True)
    err = float((got - want).abs().max() / want.abs().max())
    _record("fullsubnet_enhance_wave", rel=err)
    assert err < TOL, err

"""The cases of tests/test_gpu_frontend.py, kept apart from it so that tests/test_host_frontend_metric.py can check, where no GPU is,
each case's yardstick on its actual inputs and that the cases together cross every edge of the front end's launch arithmetic.

The front end (csrc/frontend.hip) has no debug switch: the path a call takes is a pure function of its shape.  That arithmetic is
restated ONCE, below, as plain functions of (F, B, T', norm, attention, kersize, subband_num, input layout); a case names the values it
is there for (`why`), and the GPU test recomputes them from the model it built and the tensors it passed.
"""
from oracle.ref_loader import DEFAULT_MODEL_ARGS, FULLSUBNET_MODEL_ARGS
from tests._util import edge_lengths

LA = DEFAULT_MODEL_ARGS["look_ahead"]
OFFLINE = ("offline_laplace_norm", "offline_gaussian_norm")
CUMULATIVE = ("cumulative_laplace_norm", "cumulative_layer_norm")
NORMS = OFFLINE + CUMULATIVE
LAPLACE = ("offline_laplace_norm", "cumulative_laplace_norm")
ATTENTIONS = ("TSSE", "SE", "ECA", "CBAM")
PROFILES = ("default", "harsh")
GATE_THREADS, MAXK = 1024, 16


# ------------------------------------------------------------------------------------------------ csrc/frontend.hip, restated
def cdiv(a, b):
    return -(-a // b)


def padded_bins(F):
    """FP, the row pitch of every front-end buffer (csrc/fsnp_abi.hip: align_up(num_freqs, 4))."""
    return cdiv(F, 4) * 4


def gate_lds_bytes(F):
    """fe_gate_kernel's dynamic LDS: sq[FP] + hid[FP] + edge[2][16][FP] + feat3[3][FP] floats (launch_frontend)."""
    return (2 + 2 * MAXK + 3) * padded_bins(F) * 4


def gate_needs_lds_optin(F):
    """Beyond 64 KiB a launch needs hipFuncAttributeMaxDynamicSharedMemorySize (launch_frontend's gate_once)."""
    return gate_lds_bytes(F) > 64 * 1024


def ns1(F):
    """fe_gate_kernel: K slices of fc1 per output, `ns1 = Fr >= NTHR ? 1 : min(NTHR / Fr, (31 * FP) / (2 * Fr))`."""
    Fr, FP = F // 2, padded_bins(F)
    return 1 if Fr >= GATE_THREADS else min(GATE_THREADS // Fr, (31 * FP) // (2 * Fr))


def ns1_capped_by_lds(F):
    """Whether the LDS clause (FP + 2 ns1 Fr floats must fit edge's 32 FP) is the smaller term of ns1."""
    Fr, FP = F // 2, padded_bins(F)
    return Fr < GATE_THREADS and (31 * FP) // (2 * Fr) < GATE_THREADS // Fr


def ns2(F):
    """fe_gate_kernel: K slices of fc2 per output, `ns2 = F >= NTHR ? 1 : max(1, min(min(NTHR / F, (30 * FP) / F), Fr / 16))`."""
    Fr, FP = F // 2, padded_bins(F)
    return 1 if F >= GATE_THREADS else max(1, min(GATE_THREADS // F, (30 * FP) // F, Fr // 16))


def ns2_decided_by(F):
    """Which clause gives ns2: "F>=1024", "Fr/16", "threads" (NTHR / F) or "lds"."""
    if F >= GATE_THREADS:
        return "F>=1024"
    Fr, FP = F // 2, padded_bins(F)
    terms = {"threads": GATE_THREADS // F, "lds": (30 * FP) // F, "Fr/16": Fr // 16}
    return min(terms, key=lambda k: (terms[k], k != "Fr/16"))


def fsum_threads(F):
    """launch_frontend: `fthreads = F <= 256 ? 256 : F >= 512 ? 512 : (F + 63) / 64 * 64`."""
    return 256 if F <= 256 else 512 if F >= 512 else cdiv(F, 64) * 64


def fsum_rows(B):
    """fsum_rows_per_wg: frames per workgroup of fe_fsum_kernel."""
    return 32 if B >= 8 else 16 if B >= 4 else 8 if B >= 2 else 4


def scan_chunk(Tp):
    """fe_scan_kernel: frames per thread, `chunk = cdiv(Tp, 256)`."""
    return cdiv(Tp, 256)


def f_fast(stride_f, stride_t):
    """fe_repack_kernel / fe_repack_complex_kernel: `f_fast = sF <= sT`; the transposing branch runs where frames are fastest in memory."""
    return stride_f <= stride_t


def subband_pad(F, sn):
    """fe_gate_kernel, subband_num > 1: `pad = sn - F % sn` - a whole extra group when F % sn == 0."""
    return sn - F % sn


def reflected_row(F, row):
    """fe_gate_kernel, subband_num > 1: row >= F of the padded magnitude is row 2 (F - 1) - row."""
    return row if row < F else 2 * (F - 1) - row


def formulas(*, F, B, frames, norm, att, kersize=(3, 5, 10), sn=1, f_is_fast=True, stage=False):
    """Every value the front end's launches distinguish for one call: `frames` = the stage frames T' of each utterance of the batch
    (a clip's length + look_ahead; the buffer's T' is max(frames) for a uniform batch and given apart as frames["buffer"] otherwise).
    stage: the attention stage alone (launch_attention_stage: no norm, fsum always, no tot)."""
    Tp, tv = frames["buffer"], tuple(frames["clips"])
    cumulative = stage or norm in CUMULATIVE
    v = {"FP": padded_bins(F), "lds_bytes": gate_lds_bytes(F), "lds_optin": gate_needs_lds_optin(F), "f_fast": bool(f_is_fast),
         "repack_tiles": (cdiv(padded_bins(F), 32), cdiv(Tp, 32)), "gate_passes": cdiv(F, GATE_THREADS)}
    if cumulative:
        v.update(fsum_rows=fsum_rows(B), fsum_threads=fsum_threads(F), fsum_passes=cdiv(F, fsum_threads(F)))
    if cumulative and not stage:
        v.update(scan_chunk=scan_chunk(Tp))
    if att in ("TSSE", "SE", "CBAM"):
        v.update(ns1=ns1(F), ns1_capped_by_lds=ns1_capped_by_lds(F), ns2=ns2(F), ns2_decided_by=ns2_decided_by(F))
    if att == "TSSE":
        kmax = max(kersize)
        v.update(kmax=kmax, conv_with_k1=1 in kersize, edge_overlap=tuple(sorted({t < 2 * (kmax - 1) for t in tv})),
                 clip_of_kmax_frames=kmax in tv)
    if sn > 1:
        v.update(subband_pad=subband_pad(F, sn), subband_whole_group=F % sn == 0, subband_channels=(F + subband_pad(F, sn)) // sn)
    return v


# ------------------------------------------------------------------------------------------------ the cases
CASES = {}


def make_case(name, why, **kw):
    """section: "A" .. "E"; kind "forward" (a whole forward in batch_mode "full", att_* and gate_* read back), "stage" (one attention
    layer through model.channel_attention{,_real,_imag}) or "identity" (the original FullSubNet: att_mag is the padded magnitude);
    T: frames of the input buffer; lengths: None, or the ragged pool's clip lengths, run B clips at a time; route: "f" (make_spec's
    F-fastest views), "t" (contiguous tensors: frames fastest) or "complex" (forward_complex); inputs: "make_spec" / "spec_dc" /
    "randn"; why: the formula values the case is there for, a subset of formulas(...) of the case."""
    c = dict(name=name, why=why, section=name[0], kind="forward", profile="default", F=257, B=2, T=None, norm="offline_laplace_norm",
             att="TSSE", kersize=(3, 5, 10), sn=1, route="f", lengths=None, inputs=None, seed=0)
    assert set(kw) <= set(c), set(kw) - set(c)
    c.update(kw)
    if c["kind"] == "stage":
        c["route"] = "t"                     # a contiguous [B, F, T] tensor: frames fastest
    if c["inputs"] is None:
        c["inputs"] = "randn" if c["kind"] == "stage" else "spec_dc" if c["norm"] in LAPLACE and c["kind"] == "forward" else "make_spec"
    assert c["T"] is not None
    have = case_formulas(c)
    assert all(have.get(k) == v for k, v in why.items()), (name, why, have)
    return c


def case(name, why, **kw):
    assert name not in CASES
    CASES[name] = make_case(name, why, **kw)


def model_args(c):
    if c["kind"] == "identity":
        return dict(FULLSUBNET_MODEL_ARGS, num_freqs=c["F"], norm_type=c["norm"])
    return dict(DEFAULT_MODEL_ARGS, num_freqs=c["F"], norm_type=c["norm"], channel_attention_model=c["att"], kersize=list(c["kersize"]),
                subband_num=c["sn"])


def model_key(c):
    """Cases with the same key share one model (and one state dict, seed 21)."""
    return (c["kind"] == "identity", c["profile"], c["F"], c["norm"] if c["kind"] != "stage" else None, c["att"], tuple(c["kersize"]), c["sn"])


def stage_frames(c):
    """{"buffer": T' of the buffer, "clips": T' of every clip}: the stage alone pads nothing."""
    la = 0 if c["kind"] == "stage" else LA
    clips = [c["T"]] * c["B"] if c["lengths"] is None else list(c["lengths"])
    return {"buffer": c["T"] + la, "clips": tuple(n + la for n in clips)}


def case_formulas(c):
    return formulas(F=c["F"], B=c["B"], frames=stage_frames(c), norm=c["norm"], att=c["att"] if c["kind"] != "identity" else None,
                    kersize=c["kersize"], sn=c["sn"], f_is_fast=c["route"] != "t", stage=c["kind"] == "stage")


def _short(norm):
    return {"offline_laplace_norm": "offlap", "offline_gaussian_norm": "offgau", "cumulative_laplace_norm": "cumlap",
            "cumulative_layer_norm": "cumlay"}[norm]


# A. whole forwards at F = 257: 4 norms x 4 attention kinds x 2 weight profiles
#    - B = 3 uniform at T' = 31 / 32 / 33: one repack tile of frames, exactly one, one and a frame; 3 B = 9 (branch, utterance) planes
#    - B = 1 at T' = 255 / 256 / 257 / 513: fe_scan_kernel's chunk 1 -> 2 -> 3 (both cumulative norms, one offline norm)
#    - one pool of clips on a 140-frame buffer, ragged at B = 1 / 2 / 4 / 8: the four fe_fsum_kernel row counts, clips ending inside a
#      workgroup's frames, CBAM's max over time and the offline counts against NaN / 1e6 tails
RAGGED_T = 140
RAGGED_LENGTHS = edge_lengths(RAGGED_T, LA, max(DEFAULT_MODEL_ARGS["kersize"]) - LA, edges=(8, 32, 64, 128))
assert RAGGED_LENGTHS == [8, 29, 30, 31, 61, 62, 63, 125, 126, 127, 140]
SCAN_NORMS = CUMULATIVE + ("offline_gaussian_norm",)
for _p in PROFILES:
    for _a in ATTENTIONS:
        for _n in NORMS:
            _cum = _n in CUMULATIVE
            for _tp in (31, 32, 33):
                case(f"A_uniform_{_a}_{_short(_n)}_{_p}_B3_Tp{_tp}", dict(repack_tiles=(9, cdiv(_tp, 32)), **({"fsum_rows": 8} if _cum else {})),
                     profile=_p, att=_a, norm=_n, B=3, T=_tp - LA, seed=_tp)
            if _n in SCAN_NORMS:
                for _tp in (255, 256, 257, 513):
                    case(f"A_scan_{_a}_{_short(_n)}_{_p}_B1_Tp{_tp}", {"scan_chunk": cdiv(_tp, 256), "fsum_rows": 4} if _cum else {},
                         profile=_p, att=_a, norm=_n, B=1, T=_tp - LA, seed=_tp)
            for _b, _rows in ((1, 4), (2, 8), (4, 16), (8, 32)):
                case(f"A_ragged_{_a}_{_short(_n)}_{_p}_B{_b}", {"fsum_rows": _rows} if _cum else {},
                     profile=_p, att=_a, norm=_n, B=_b, T=RAGGED_T, lengths=RAGGED_LENGTHS, seed=140)

# B. TSSE kernel sizes (1, 2, 16) - a conv that stages nothing, kmax = MAXK - and (16, 16, 16) once: clips of exactly kmax stage frames
#    (one valid conv output), one more, 29 and 30 (2 (kmax - 1) = 30: the staged first and last frames overlap / just stop overlapping)
#    and 64; uniform at B = 2 and as the ragged lengths of one batch of 5
B_TP = (16, 17, 29, 30, 64)
B_NORMS = ("offline_laplace_norm", "cumulative_layer_norm")
for _p in PROFILES:
    for _n in B_NORMS:
        for _tp in B_TP:
            case(f"B_k1_2_16_{_short(_n)}_{_p}_B2_Tp{_tp}", dict(kmax=16, conv_with_k1=True, edge_overlap=(_tp < 30,), clip_of_kmax_frames=_tp == 16),
                 profile=_p, norm=_n, kersize=(1, 2, 16), T=_tp - LA, seed=_tp)
        case(f"B_k1_2_16_{_short(_n)}_{_p}_ragged_B5", dict(kmax=16, edge_overlap=(False, True), clip_of_kmax_frames=True),
             profile=_p, norm=_n, kersize=(1, 2, 16), B=5, T=max(B_TP) - LA, lengths=[t - LA for t in B_TP], seed=5)
case("B_k16_16_16_cumlay_harsh_B2_Tp16", dict(kmax=16, conv_with_k1=False, edge_overlap=(True,), clip_of_kmax_frames=True),
     profile="harsh", norm="cumulative_layer_norm", kersize=(16, 16, 16), T=16 - LA, seed=16)

# C. subband_num > 1 (ECA, uniform batches: the library refuses lengths= there): pad = 1, 3, 2 (a whole group: F % sn == 0) and 1
C_NORMS = ("offline_gaussian_norm", "cumulative_laplace_norm")
for _p in PROFILES:
    for _n in C_NORMS:
        for _f, _sn, _pad in ((257, 2, 1), (257, 4, 3), (256, 2, 2), (161, 3, 1)):
            case(f"C_subband_F{_f}_sn{_sn}_{_short(_n)}_{_p}", dict(subband_pad=_pad, subband_whole_group=_f % _sn == 0),
                 profile=_p, att="ECA", norm=_n, F=_f, sn=_sn, T=40 - LA, seed=_f + _sn)

# D. input routes: the same values as make_spec's F-fastest views, as contiguous [B, 1, F, T] tensors (frames fastest: the transposing
#    branch of the repack kernels) and through forward_complex; the original FullSubNet's att_mag on both layouts
D_NORMS = ("offline_laplace_norm", "cumulative_layer_norm")
for _p in PROFILES:
    for _n in D_NORMS:
        for _tp in (33, 129):
            for _r in ("f", "t", "complex"):
                case(f"D_route_{_r}_{_short(_n)}_{_p}_Tp{_tp}", dict(f_fast=_r != "t"), profile=_p, norm=_n, T=_tp - LA, route=_r, seed=_tp)
for _tp in (33, 129):
    for _r in ("f", "t"):
        case(f"D_fullsubnet_route_{_r}_Tp{_tp}", dict(f_fast=_r != "t"), kind="identity", T=_tp - LA, route=_r, seed=_tp)

# E. bin counts.  Whole forwards at F = 161 / 441 / 515: fe_fsum_kernel at 256 / 448 / 512 threads (two passes), the LDS opt-in, the
#    first F with Fr = 257 (part2 = part + ns1 Fr where a fixed + 256 aliased).  The attention stage alone at F = 33 (the LDS clause
#    caps ns1, Fr / 16 = 1 gives ns2 = 1), 440 | 441 (65120 | 65712 bytes of LDS), 513, 515 and 1025 (ns2 = 1 through F >= 1024, every
#    per-bin loop of the 1024-thread gate kernel takes a second pass)
E_NORMS = ("offline_gaussian_norm", "cumulative_laplace_norm")
for _p in PROFILES:
    for _a in ("TSSE", "CBAM"):
        for _n in E_NORMS:
            for _f, _thr in ((161, 256), (441, 448), (515, 512)):
                _w = dict(lds_optin=_f > 440, ns1=GATE_THREADS // (_f // 2))
                if _n in CUMULATIVE:
                    _w.update(fsum_threads=_thr, fsum_passes=cdiv(_f, _thr))
                case(f"E_forward_F{_f}_{_a}_{_short(_n)}_{_p}", _w, profile=_p, att=_a, norm=_n, F=_f, T=33 - LA, seed=_f)
    for _a in ATTENTIONS:
        for _f in (33, 440, 441, 513, 515, 1025):
            _w = dict(lds_optin=_f > 440, gate_passes=2 if _f == 1025 else 1, fsum_threads=256 if _f == 33 else 448 if _f < 512 else 512)
            if _a != "ECA":
                _w.update(ns1_capped_by_lds=_f == 33, ns2_decided_by={33: "Fr/16", 1025: "F>=1024"}.get(_f, "threads"))
            for _b, _t in ((1, 16), (1, 37), (3, 16), (3, 37)):
                case(f"E_stage_F{_f}_{_a}_{_p}_B{_b}_T{_t}", _w, kind="stage", profile=_p, att=_a, F=_f, B=_b, T=_t, seed=_f + _t + _b)


def cases_of(section, **match):
    return [c for c in CASES.values() if c["section"] == section and all(c[k] == v for k, v in match.items())]


# ------------------------------------------------------------------------------------------------ inputs, oracle and yardstick of a case
BRANCHES = ("mag", "real", "imag")
TAGS = tuple(f"{g}_{b}" for g in ("att", "gate") for b in BRANCHES)


def case_state_dict(c):
    from oracle.weights import make_state_dict, make_state_dict_fullsubnet
    if c["kind"] == "identity":
        return make_state_dict_fullsubnet(21, c["profile"], num_freqs=c["F"])
    return make_state_dict(21, c["profile"], attention=c["att"], num_freqs=c["F"], kersize=tuple(c["kersize"]))


def case_inputs(c):
    """forward / identity: (mag, real, imag) [N, 1, F, T] as make_spec lays them out (N = B, or the ragged pool's size); stage: three
    [B, F, T] tensors, one per branch.  Cases that differ in the route only get the same values."""
    import torch
    from oracle.make_golden import make_spec
    from tests._util import spec_dc
    n = c["B"] if c["lengths"] is None else len(c["lengths"])
    if c["inputs"] == "randn":
        g = torch.Generator().manual_seed(7000 + c["seed"])
        return tuple(torch.randn(n, c["F"], c["T"], generator=g) for _ in BRANCHES)
    return (spec_dc if c["inputs"] == "spec_dc" else make_spec)(n, c["T"], 6000 + c["seed"], c["F"])


def case_oracle(c, sd, ins, dtype):
    """-> rows[i] = {tag: [F, T'_i] (att_*) or [F, 1] (gate_*)} of clip i alone, from tests/_util.py oracle_frontend (stage:
    fsnp_torch.attention_gate and the multiply) in `dtype`.  Route "complex": the oracle's magnitude is |X| taken in `dtype`."""
    import torch
    from oracle import fsnp_torch
    from tests._util import oracle_frontend, oracle_rows
    args = model_args(c)
    if c["kind"] == "stage":
        p = {k: v.to(dtype) for k, v in sd.items() if k.startswith("channel_attention")}
        out = {}
        for b, x in zip(BRANCHES, ins):
            x = x.to(dtype)
            g = fsnp_torch.attention_gate(x, p, "channel_attention" + ("" if b == "mag" else "_" + b), c["att"])
            out["att_" + b], out["gate_" + b] = x * g.unsqueeze(2), g.unsqueeze(2)
        return [{t: out[t][i].numpy() for t in TAGS} for i in range(c["B"])]

    def fn(mag, real, imag):
        if c["route"] == "complex":
            cd = torch.complex128 if dtype == torch.float64 else torch.complex64
            mag = torch.complex(real, imag).to(cd).abs()
        st = oracle_frontend(sd, (mag, real, imag), args, dtype)
        return [{t: (st[t][i] if t.startswith("att_") else st[t][i].unsqueeze(1)).numpy() for t in TAGS} for i in range(mag.shape[0])]
    if c["lengths"] is None:
        return fn(*ins)
    rows = [None] * len(c["lengths"])
    for n in sorted(set(c["lengths"])):
        idx = [i for i, m in enumerate(c["lengths"]) if m == n]
        for i, r in zip(idx, fn(*[t[idx][..., :n] for t in ins])):
            rows[i] = r
    return rows


def yardstick(want64, want32):
    """e32[i][tag]: tests/_util.py plane_errs of the float32 oracle against the float64 oracle on clip i's plane (gate: one frame)."""
    from tests._util import plane_errs
    return [{t: plane_errs(w32[t][None], w[t][None])[0][0] for t in TAGS} for w, w32 in zip(want64, want32)]

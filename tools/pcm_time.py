#!/usr/bin/env python
"""What 16-bit PCM at the boundary costs and saves (include/fsnp_pcm.h): writes profiles/pcm16.md from ONE process.

    python tools/pcm_time.py [--steps 400 --warmup 50 --repeats 7 --out profiles/pcm16.md]

1. A live wave session at 1 slot, one hop (256 samples) per push, fed int16 as a socket delivers it, int16 back:
     "torch around fp32"  x.to(float32) / 32768 -> push -> mul / round / clamp / to(int16), the launches a caller writes today
     "PCM push"           push(int16) -> int16, the conversion inside the push's own two sample kernels
   for a planar buffer and for one channel of a two-channel interleaved buffer (the torch version selects the channel first).
2. enhance_wave at B = 32 x 2 s, int16 in pinned host memory -> int16 in pinned host memory, copies included, both ways.

Timing: a host clock around `steps` calls that end in one device synchronisation, after a warm-up of every shape; the two versions of a
row alternate repeat by repeat in the same process, and the table gives the median and the spread (min - max) over the repeats.
No number from the table is asserted anywhere."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fullsubnet_plus_amd import FullSubNet, FullSubNet_Plus  # noqa: E402
from fullsubnet_plus_amd.synthetic import (DEFAULT_MODEL_ARGS, FULLSUBNET_MODEL_ARGS, make_state_dict,  # noqa: E402
                                           make_state_dict_fullsubnet, make_wave)

HOP = 256


def _model(cls, args, sd):
    m = cls(**args)
    m.load_state_dict(sd, strict=True)
    m = m.to("cuda").eval()
    m.batch_mode, m.error_check = "full", "deferred"
    return m


def _to_s16(y):
    return y.mul(32768.0).round_().clamp_(-32768.0, 32767.0).to(torch.int16)


def _alternate(versions, steps, warmup, repeats):
    """versions: {name: fn}; -> {name: [us per call of every repeat]}, the versions alternating repeat by repeat"""
    for fn in versions.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    runs = {k: [] for k in versions}
    for _ in range(repeats):
        for name, fn in versions.items():
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            runs[name].append((time.perf_counter() - t0) / steps * 1e6)
    return runs


def _cell(v, unit_div=1.0):
    return f"{statistics.median(v) / unit_div:.1f} ({min(v) / unit_div:.1f} - {max(v) / unit_div:.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcm16.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/pcm_time.py measures on the GPU; there is none here")
    rows = []
    with torch.no_grad():
        # ---- 1. the live push
        m = _model(FullSubNet, dict(FULLSUBNET_MODEL_ARGS, norm_type="cumulative_layer_norm"), make_state_dict_fullsubnet(0, "default"))
        pcm = (torch.from_numpy(make_wave(2, HOP / 16000.0, 7)) * 32768).round().to(torch.int16).cuda()      # [2, 256]
        planar = pcm[:1].contiguous()                                    # [1, 256]
        inter = pcm.t().contiguous()                                     # [256, 2]: a two-channel interleaved frame
        chan = inter.t()[:1]                                             # channel 0 in place: [1, 256], sample step 2
        with m.open_wave_stream(1, max_samples=HOP, live=True) as ws:
            for name, x in (("planar", planar), ("2-channel interleaved, channel 0", chan)):
                runs = _alternate({
                    "fp32": lambda x=x: ws.push(x.to(torch.float32).div_(32768.0)),
                    "torch": lambda x=x: _to_s16(ws.push(x.to(torch.float32).div_(32768.0))),
                    "pcm": lambda x=x: ws.push(x),
                }, a.steps, a.warmup, a.repeats)
                assert ws.push(x).dtype == torch.int16
                rows.append((f"live push, 1 slot x {HOP} samples, {name}", "us", runs, 1.0))
            ws.reset()
        m.poll_errors()
        # ---- 2. whole clips through pinned host memory
        B, seconds = 32, 2.0
        mp = _model(FullSubNet_Plus, DEFAULT_MODEL_ARGS, make_state_dict(0, "default"))
        wav = torch.from_numpy(make_wave(B, seconds, 1000))
        L = wav.shape[1]
        h_in = (wav * 32768).round().clamp(-32768, 32767).to(torch.int16).pin_memory()
        h_out = torch.empty((B, L), dtype=torch.int16).pin_memory()
        h_out32 = torch.empty((B, L), dtype=torch.float32).pin_memory()
        d_in = torch.empty((B, L), dtype=torch.int16, device="cuda")

        def torch_way():
            d_in.copy_(h_in, non_blocking=True)
            h_out.copy_(_to_s16(mp.enhance_wave(d_in.to(torch.float32).div_(32768.0))), non_blocking=True)

        def fp32_back():      # what a caller without a device-side conversion does: fp32 back, twice the bytes
            d_in.copy_(h_in, non_blocking=True)
            h_out32.copy_(mp.enhance_wave(d_in.to(torch.float32).div_(32768.0)), non_blocking=True)

        def pcm_way():
            d_in.copy_(h_in, non_blocking=True)
            h_out.copy_(mp.enhance_wave(d_in), non_blocking=True)

        def pcm_peak():
            d_in.copy_(h_in, non_blocking=True)
            h_out.copy_(mp.enhance_wave(d_in, out_format="s16_peak"), non_blocking=True)

        mp.reserve(B, 1 + L // HOP, max_samples=L)
        steps = max(a.steps // 20, 10)
        runs = _alternate({"fp32": fp32_back, "torch": torch_way, "pcm": pcm_way, "peak": pcm_peak}, steps, max(a.warmup // 10, 3), a.repeats)
        rows.append((f"enhance_wave, B = {B} x {seconds:g} s ({L} samples), int16 pinned host -> int16 pinned host", "ms", runs, 1e3))
        mp.poll_errors()

    props = torch.cuda.get_device_properties(0)
    lines = ["# 16-bit PCM at the boundary: the conversion inside the sample kernels against torch launches around them", "",
             f"Box: {props.name} ({getattr(props, 'gcnArchName', '?')}), {props.multi_processor_count} CUs, torch {torch.__version__}; "
             f"`python tools/pcm_time.py --steps {a.steps} --warmup {a.warmup} --repeats {a.repeats}`, one process.", "",
             "Host wall time per call over a window of calls that ends in one device synchronisation (error_check=\"deferred\"): median "
             "(min - max) over the repeats; the versions of a row alternate repeat by repeat.  \"fp32 in the middle, torch in front\" converts the "
             "input with torch and leaves the output fp32 (for the whole clips: copies fp32 back, twice the bytes); \"torch around "
             "fp32\" also converts the output with torch (mul, round, clamp, to int16); \"PCM\" hands int16 in and takes int16 out.", "",
             "| case | unit | fp32 in the middle, torch in front | torch around fp32 | PCM | PCM / torch around fp32 | s16_peak |",
             "|---|---|---|---|---|---|---|"]
    verdicts = []
    for name, unit, runs, div in rows:
        ratio = statistics.median(runs["pcm"]) / statistics.median(runs["torch"])
        peak = _cell(runs["peak"], div) if "peak" in runs else ""
        lines.append(f"| {name} | {unit} | {_cell(runs['fp32'], div)} | {_cell(runs['torch'], div)} | {_cell(runs['pcm'], div)} | {ratio:.2f} | {peak} |")
        overlap = min(runs["torch"]) <= max(runs["pcm"]) and min(runs["pcm"]) <= max(runs["torch"])
        verdict = "NOT measurably different: the two spreads overlap" if overlap else "FASTER" if ratio < 1 else "NOT faster"
        verdicts.append(f"- {name}: PCM is {verdict} ({ratio:.2f} of the torch version's median)")
    lines += ["", "Expectation to confirm or refute: the fused conversion is faster than the three to five torch launches around a push "
              "that DESIGN.md prices at 61 us per step at one slot.  If a row says NOT faster or NOT measurably different, the feature "
              "stands on its interface there.  These are wall times of a Python caller's loop: where a live push takes several times "
              "those 61 us, the window is bound by the host side of a push, and the row shows what the extra torch calls cost the "
              "caller's thread, not device time.", ""]
    lines += verdicts
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""What enhance_wave_windowed (include/ext/fsnp_windowed.h) costs next to its alternatives: writes profiles/windowed.md from ONE process.

    python tools/windowed_time.py [--warmup 2 --repeats 7 --commit <label> --out profiles/windowed.md]

FullSubNet+ on one 60 s clip and on a ragged batch of 32 clips of 5 - 15 s, fp32 device buffers, W = 32 000, V = 4000, max_batch = 32:
     A   enhance_wave of the whole clips (lengths= for the batch).  Reported only: it computes something else.
     B   enhance_wave_windowed.
     C   the same windows through what the library offered before: enhance_wave on batches of 32 windows gathered with as_strided,
         lengths= where a batch holds short last windows, and the cross-fade in torch.

Timing: device events around every call, after a warm-up of every version; the versions alternate repeat by repeat in the same
process, and the table gives the median and the spread (min - max) over the repeats.  No number from the table is asserted anywhere."""
import argparse
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fullsubnet_plus_amd import FullSubNet_Plus, window_count  # noqa: E402
from fullsubnet_plus_amd.synthetic import DEFAULT_MODEL_ARGS, make_state_dict, make_wave  # noqa: E402

W, V, MAX_BATCH = 32000, 4000, 32
S = W - V


def windows_in_torch(m, wav, lengths, g):
    """Version C: wav [B, L] fp32 on the device, lengths a list -> [B, L].  The windows of every clip as rows of one [sum K, W] tensor
    (as_strided over the clip for the full ones, the last one zero-padded), enhance_wave over 32 rows at a time, torch cross-fade."""
    rows, lens = [], []
    for b, L in enumerate(lengths):
        K = window_count(L, W, V)
        full = K if (K - 1) * S + W <= L else K - 1
        if full:
            rows.append(torch.as_strided(wav[b], (full, W), (S, 1)))
        if full < K:
            last = wav.new_zeros((1, W))
            last[0, :L - full * S] = wav[b, full * S:L]
            rows.append(last)
        lens += [min(W, L - k * S) for k in range(K)]
    rows = torch.cat(rows)
    y = torch.empty_like(rows)
    for r0 in range(0, rows.shape[0], MAX_BATCH):
        n = lens[r0:r0 + MAX_BATCH]
        x = rows[r0:r0 + MAX_BATCH, :max(n)]
        y[r0:r0 + MAX_BATCH, :max(n)] = m.enhance_wave(x) if min(n) == max(n) else m.enhance_wave(x, lengths=n)
    out = torch.zeros_like(wav)
    r = 0
    for b, L in enumerate(lengths):
        K = window_count(L, W, V)
        for k in range(K):
            n = lens[r + k]
            out[b, k * S:k * S + n] = y[r + k, :n]
            if k:
                prev = y[r + k - 1, S:S + V]
                out[b, k * S:k * S + V] = torch.addcmul(prev, g, y[r + k, :V] - prev)
        r += K
    return out


def _alternate(versions, warmup, repeats):
    """versions: {name: fn} -> {name: [device ms of every repeat]}, the versions alternating repeat by repeat"""
    for fn in versions.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    runs = {k: [] for k in versions}
    for _ in range(repeats):
        for name, fn in versions.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            runs[name].append(e0.elapsed_time(e1))
    return runs


def _cell(v):
    return f"{statistics.median(v):.2f} ({min(v):.2f} - {max(v):.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "windowed.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/windowed_time.py measures on the GPU; there is none here")
    rng = np.random.default_rng(3)
    cases = [("one clip of 60 s", [960000]), ("32 clips of 5 - 15 s", sorted(int(v) for v in rng.integers(80000, 240001, size=32)))]
    table, verdicts = [], []
    with torch.no_grad():
        m = FullSubNet_Plus(**DEFAULT_MODEL_ARGS)
        m.load_state_dict(make_state_dict(0, "default"), strict=True)
        m = m.to("cuda").eval()
        m.batch_mode, m.error_check = "full", "deferred"
        g = torch.from_numpy((0.5 - 0.5 * np.cos(np.pi * np.arange(V) / V)).astype(np.float32)).cuda()
        for name, lengths in cases:
            B, L = len(lengths), max(lengths)
            wav = torch.from_numpy(make_wave(B, L / 16000, 2000 + B))[:, :L].contiguous().cuda()
            lens = None if B == 1 else lengths
            versions = {"A": lambda: m.enhance_wave(wav, lengths=lens),
                        "B": lambda: m.enhance_wave_windowed(wav, W, V, lengths=lens, max_batch=MAX_BATCH),
                        "C": lambda: windows_in_torch(m, wav, lengths, g)}
            b, c = versions["B"](), versions["C"]()
            agree = float((b - c).abs().max() / c.abs().max())          # the same forwards: fp32 rounding of the fade apart
            runs = _alternate(versions, a.warmup, a.repeats)
            K = sum(window_count(n, W, V) for n in lengths)
            table.append(f"| {name} ({K} windows, {math.ceil(K / MAX_BATCH)} forwards) | " + " | ".join(_cell(runs[k]) for k in "ABC") + " |")
            mb, mc = statistics.median(runs["B"]), statistics.median(runs["C"])
            sc, sb = max(runs["C"]) - min(runs["C"]), max(runs["B"]) - min(runs["B"])
            verdicts.append(f"- {name}: median B - median C = {mb - mc:+.2f} ms ({100 * (mb - mc) / mc:+.2f} %); C's own spread (max - min) "
                            f"{sc:.2f} ms, B's {sb:.2f} ms; B's median is {'at or below' if mb <= max(runs['C']) else 'above'} C's slowest "
                            f"repeat ({max(runs['C']):.2f} ms).  max |B - C| / max |C| = {agree:.1e}")
            m.poll_errors()
    props = torch.cuda.get_device_properties(0)
    lines = ["# enhance_wave_windowed: one long recording in overlapping windows", "",
             f"Box: {props.name} ({getattr(props, 'gcnArchName', '?')}), {props.multi_processor_count} CUs, torch {torch.__version__}; commit {a.commit}; "
             f"`python tools/windowed_time.py --warmup {a.warmup} --repeats {a.repeats}`, one process.", "",
             f"FullSubNet+, fp32 device buffers, W = {W}, V = {V} (2 s windows, 0.25 s overlap), max_batch = {MAX_BATCH}, error_check=\"deferred\".  "
             "Device time per call in ms (events around the call): median (min - max) over the repeats; the versions of a row alternate "
             "repeat by repeat.", "",
             "- A: `enhance_wave` of the whole clips.  Reported only: every statistic is taken over the whole recording, another result.",
             "- B: `enhance_wave_windowed`.",
             "- C: the same windows through `enhance_wave` on `as_strided` batches of 32 (with `lengths=` for short last windows) and a "
             "cross-fade in torch.", "",
             "| case | A | B | C |", "|---|---|---|---|"]
    lines += table + ["", "Acceptance: B no slower than C beyond C's own run-to-run spread.", ""] + verdicts + [""]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

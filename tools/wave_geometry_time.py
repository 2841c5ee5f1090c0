#!/usr/bin/env python
"""What enhance_wave costs at an STFT geometry other than bench.py's (which measures the default 257 bins / hop 256 and stays as it is).

    python tools/wave_geometry_time.py --num-freqs 161 --hop 80 --batch 32 --seconds 2 [--steps 20 --warmup 5 --repeats 3]

One JSON line: ms per enhance_wave call of every repeat (bench.py --wave's loop: deferred error policy, one synchronisation around the
timed steps), the frame count and the geometry.  profiles/stft_geometry.md holds the rows measured with it."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fullsubnet_plus_amd import FullSubNet_Plus  # noqa: E402
from fullsubnet_plus_amd.synthetic import DEFAULT_MODEL_ARGS, make_state_dict, make_wave  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-freqs", type=int, default=257)
    ap.add_argument("--hop", type=int, default=None, help="default: num_freqs - 1")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    model = FullSubNet_Plus(**{**DEFAULT_MODEL_ARGS, "num_freqs": a.num_freqs})
    model.load_state_dict(make_state_dict(0, "default", num_freqs=a.num_freqs), strict=True)
    model = model.to("cuda").eval()
    model.batch_mode, model.error_check = "full", "deferred"
    if a.hop is not None:
        model.hop_length = a.hop
    wav = torch.from_numpy(make_wave(a.batch, a.seconds, 1000)).cuda()
    runs = []
    with torch.no_grad():
        for _ in range(max(a.warmup, 1)):
            model.enhance_wave(wav)
        torch.cuda.synchronize()
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            for _ in range(a.steps):
                model.enhance_wave(wav)
            torch.cuda.synchronize()
            runs.append((time.perf_counter() - t0) / a.steps * 1e3)
        model.poll_errors()
    print(json.dumps({"num_freqs": a.num_freqs, "n_fft": 2 * (a.num_freqs - 1), "hop_length": model.hop_length, "batch": a.batch,
                      "samples": wav.shape[1], "frames": 1 + wav.shape[1] // model.hop_length, "steps": a.steps,
                      "ms_per_call": [round(r, 3) for r in runs]}))


if __name__ == "__main__":
    main()

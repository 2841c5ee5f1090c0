"""What batching clips of different lengths buys: 64 seeded clips of 1 to 10 s, run two ways on one MI355X.

  b1     : one clip per forward at B = 1 (the reference CLI's pattern)
  ragged : the same clips sorted by length, in batches of 32 with per-utterance lengths (forward(..., lengths=...))

Prints one JSON line: frames/s of both (median of --runs timed passes), their ratio, and the mean-to-max length ratio of the
ragged batches (the part of a batch's frames that are padding is (1 - that)).  Not part of bench.py.

    python tools/ragged_throughput.py [--clips 64] [--batch 32] [--runs 3] [--seed 0]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fullsubnet_plus_amd import FullSubNet_Plus  # noqa: E402
from fullsubnet_plus_amd.synthetic import DEFAULT_MODEL_ARGS, make_inputs, make_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()

    model = FullSubNet_Plus(**DEFAULT_MODEL_ARGS)
    model.load_state_dict(make_state_dict(0, "default"), strict=True)
    model = model.to("cuda").eval()
    model.batch_mode = "full"
    model.error_check = "deferred"

    rng = np.random.default_rng(a.seed)
    seconds = rng.uniform(1.0, 10.0, size=a.clips)
    mag, real, imag = make_inputs(a.clips, 10.0, a.seed)          # [N, 1, F, 626]: clip i is its first 1 + 16000 s_i / 256 frames
    lengths = [int(1 + round(16000 * s) // 256) for s in seconds]
    x = [t.contiguous().cuda() for t in (mag, real, imag)]
    total = sum(lengths)

    order = sorted(range(a.clips), key=lambda i: lengths[i])
    batches = []
    for k in range(0, a.clips, a.batch):
        idx = order[k:k + a.batch]
        T = max(lengths[i] for i in idx)
        batches.append(([t[idx, :, :, :T].contiguous() for t in x], [lengths[i] for i in idx]))
    singles = [[t[i:i + 1, :, :, :lengths[i]].contiguous() for t in x] for i in range(a.clips)]

    def run_b1():
        for ins in singles:
            model(*ins)

    def run_ragged():
        for ins, lens in batches:
            model(*ins, lengths=lens)

    res = {}
    with torch.no_grad():
        for name, fn in (("b1", run_b1), ("ragged", run_ragged)):
            fn()                                                  # warm-up: handle, workspace, plans
            torch.cuda.synchronize()
            rates = []
            for _ in range(a.runs):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                rates.append(total / (time.perf_counter() - t0))
            res[name] = statistics.median(rates)
    fill = statistics.mean(sum(l) / (len(l) * max(l)) for _, l in batches)
    print(json.dumps({"clips": a.clips, "batch": a.batch, "frames": total, "b1_frames_per_s": round(res["b1"], 1),
                      "ragged_frames_per_s": round(res["ragged"], 1), "speedup": round(res["ragged"] / res["b1"], 3),
                      "mean_to_max_length": round(fill, 4)}))


if __name__ == "__main__":
    main()

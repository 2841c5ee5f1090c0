#!/usr/bin/env python
"""What another sample rate costs enhance_wave (include/fsnp_resample.h): writes profiles/resample.md from ONE process.

    python tools/resample_time.py [--steps 20 --warmup 3 --repeats 7 --commit <label> --out profiles/resample.md]

enhance_wave with int16 in and int16 out ("s16"), device buffers, at B = 32 x 2 s and at B = 1 x 2 s:
     "16 kHz"     the clips at the model's rate: the call as it has always been
     "48 kHz"     the same seconds of audio at 48 kHz (96000 samples per clip), sample_rate=48000
     "44.1 kHz"   at 44.1 kHz (88200 samples), sample_rate=44100
and, to say where the added time goes, the two conversions of a call on their own (model.resample): to the model's rate with fp32
out - the sums the pad kernel's loads do - and the fp32 model-rate clip back to int16 at the caller's rate.

Timing: a host clock around `steps` calls that end in one device synchronisation, after a warm-up of every shape; the versions of a
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

from fullsubnet_plus_amd import FullSubNet_Plus, resample_length  # noqa: E402
from fullsubnet_plus_amd.synthetic import DEFAULT_MODEL_ARGS, make_state_dict, make_wave  # noqa: E402

RATES = (48000, 44100)


def _alternate(versions, steps, warmup, repeats):
    """versions: {name: fn}; -> {name: [ms per call of every repeat]}, the versions alternating repeat by repeat"""
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
            runs[name].append((time.perf_counter() - t0) / steps * 1e3)
    return runs


def _cell(v):
    return f"{statistics.median(v):.3f} ({min(v):.3f} - {max(v):.3f})"


def _pcm(B, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8000, 8000, (B, n), generator=g, dtype=torch.int16).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/resample_time.py measures on the GPU; there is none here")
    seconds = 2.0
    table, phases, verdicts = [], [], []
    with torch.no_grad():
        m = FullSubNet_Plus(**DEFAULT_MODEL_ARGS)
        m.load_state_dict(make_state_dict(0, "default"), strict=True)
        m = m.to("cuda").eval()
        m.batch_mode, m.error_check = "full", "deferred"
        for B in (32, 1):
            n16 = int(seconds * 16000)
            x16 = (torch.from_numpy(make_wave(B, seconds, 1000)) * 32768).round().clamp(-32768, 32767).to(torch.int16).cuda()
            assert x16.shape == (B, n16)
            m.reserve(B, 1 + n16 // m.hop_length, max_samples=n16)
            versions = {"16 kHz": lambda x=x16: m.enhance_wave(x)}
            clips = {}
            for R in RATES:
                n = int(seconds * R)
                assert resample_length(n, R, 16000) == n16
                clips[R] = m.resample(x16, 16000, R)                          # the same audio at R: int16 [B, n]
                assert clips[R].shape == (B, n) and clips[R].dtype == torch.int16
                m.reserve(B, 1 + n16 // m.hop_length, max_samples=n, sample_rate=R)
                versions[f"{R / 1000:g} kHz"] = lambda x=clips[R], R=R: m.enhance_wave(x, sample_rate=R)
            steps = a.steps if B > 1 else a.steps * 10
            runs = _alternate(versions, steps, a.warmup, a.repeats)
            base = statistics.median(runs["16 kHz"])
            table.append(f"| enhance_wave, B = {B} x {seconds:g} s | " + " | ".join(_cell(runs[k]) for k in versions) + " |")
            for R in RATES:
                k = f"{R / 1000:g} kHz"
                added = statistics.median(runs[k]) - base
                overlap = min(runs[k]) <= max(runs["16 kHz"])
                verdicts.append(f"- B = {B}, {k}: {added:+.3f} ms on {base:.3f} ms = {100 * added / base:+.2f} % "
                                f"({'the spreads overlap' if overlap else 'the spreads do not overlap'}; reporting threshold 3 %)")
            # the two conversions on their own
            y16 = m.enhance_wave(x16, out_format="f32")
            ph = {}
            for R in RATES:
                ph[f"{R / 1000:g} kHz in -> fp32 at 16 kHz"] = lambda x=clips[R], R=R: m.resample(x, R, 16000, out_format="f32")
                ph[f"fp32 at 16 kHz -> int16 at {R / 1000:g} kHz"] = lambda y=y16, R=R: m.resample(y, 16000, R, out_format="s16")
            pruns = _alternate(ph, a.steps * 10, a.warmup, a.repeats)
            for k, v in pruns.items():
                phases.append(f"| B = {B}: {k} | {_cell(v)} |")
            m.poll_errors()

    props = torch.cuda.get_device_properties(0)
    lines = ["# enhance_wave at another sample rate: what the conversion on the device costs", "",
             f"Box: {props.name} ({getattr(props, 'gcnArchName', '?')}), {props.multi_processor_count} CUs, torch {torch.__version__}; commit {a.commit}; "
             f"`python tools/resample_time.py --steps {a.steps} --warmup {a.warmup} --repeats {a.repeats}`, one process.", "",
             "Host wall time per call in ms over a window of calls that ends in one device synchronisation (error_check=\"deferred\", areas "
             "reserved, int16 device buffers in and out): median (min - max) over the repeats; the versions of a row alternate repeat by "
             "repeat.  The yardstick is the 16 kHz call for the same seconds of audio, in the same process on the same box.", "",
             "| case | 16 kHz | " + " | ".join(f"{R / 1000:g} kHz" for R in RATES) + " |", "|---|---|" + "---|" * len(RATES)]
    lines += table
    lines += ["", "Added time against the 16 kHz call (medians):", ""] + verdicts
    lines += ["", "The two conversions of a call as free-standing launches (`model.resample`, torch's allocation of the result included) - "
              "the sums of the first are what the fused pad kernel does in its loads, the second is the launch the call itself runs on the "
              "way out:", "", "| conversion | ms |", "|---|---|"] + phases
    lines += ["", "Expectation that was to be confirmed or refuted: from arithmetic and bytes alone, well under 0.2 ms on the 28 ms call at "
              "B = 32.  Below 3 % - the spread between boxes the README reports - a difference is not resolvable.", ""]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What a (re-)pack of the weights costs, host path against device path (include/fsnp_device_weights.h, model.weight_upload).

    python tools/commit_time.py --commit <sha> --out profiles/device_weights.md          (on an MI355X, one process)

For the default FullSubNet+ and the default FullSubNet, under weight_upload = "host" (fsnp_set_weight + fsnp_commit_weights: every
tensor to the CPU, the blob built on the host, one upload - the yardstick.  It has the shape of the path before the device hand-over,
but it is THIS tree's host packer, which walks the images through csrc/weight_layouts.h and not through the earlier per-kernel loops:
the column is not a measurement of an earlier commit's code) and "device" (fsnp_set_weight_device + fsnp_commit_weights_on), wall
time on the host of
  first     the first _ensure_handle of a model on the GPU: fsnp_create, the hand-over of all tensors, the commit, the weight watch;
  re-pack   _ensure_handle after load_state_dict of other weights (same handle);
  watch     a forward (B = 1, 16 frames, error_check="sync") after an edit through .data: the weight watch flags it, the forward re-packs
            and runs again - next to a plain forward of the same input;
each between two device synchronisations, median and range of --repeats runs, with the copy counts of fsnp_debug_commit_stats for the
last commit.  A throw-away model is packed first, so that no column pays for loading the library and its code objects."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fullsubnet_plus_amd import FullSubNet, FullSubNet_Plus, _lib  # noqa: E402
from fullsubnet_plus_amd.synthetic import (DEFAULT_MODEL_ARGS, FULLSUBNET_MODEL_ARGS, make_inputs, make_state_dict,  # noqa: E402
                                           make_state_dict_fullsubnet)

MODELS = [("FullSubNet+ (default)", FullSubNet_Plus, DEFAULT_MODEL_ARGS, make_state_dict, 3),
          ("FullSubNet (default)", FullSubNet, FULLSUBNET_MODEL_ARGS, make_state_dict_fullsubnet, 1)]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats_of(model):
    out = (ctypes.c_int64 * 4)()
    _lib.check(_lib.load().fsnp_debug_commit_stats(model._handle, ctypes.byref(out)), "fsnp_debug_commit_stats")
    return list(out)


def fmt(ms):
    return f"{statistics.median(ms):.1f} ({min(ms):.1f} - {max(ms):.1f})"


def measure(cls, args, make_sd, nin, upload, repeats, dev):
    first, repack, watch, plain = [], [], [], []
    ins = [t.to(dev) for t in make_inputs(1, 0.25, 3)[:nin]]
    sds = [make_sd(s, "default") for s in range(2)]
    counts = {}
    for r in range(repeats):
        m = cls(**args)
        m.load_state_dict(sds[0], strict=True)
        m = m.to(dev).eval()
        m.weight_upload, m.error_check, m.batch_mode = upload, "sync", "full"
        first.append(timed(lambda: m._ensure_handle(dev))[0])
        counts["first"] = stats_of(m)
        m.load_state_dict(sds[1], strict=True)
        repack.append(timed(lambda: m._ensure_handle(dev))[0])
        counts["re-pack"] = stats_of(m)
        with torch.no_grad():
            m(*ins)
            plain.append(timed(lambda: m(*ins))[0])
            m.sb_model.fc_output_layer.bias.data.add_(0.125)
            watch.append(timed(lambda: m(*ins))[0])
        counts["watch"] = stats_of(m)
        del m
    return {"first": first, "re-pack": repack, "watch": watch, "plain": plain, "counts": counts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_weights.md"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    props = torch.cuda.get_device_properties(dev)
    warm = FullSubNet_Plus(**DEFAULT_MODEL_ARGS).to(dev).eval()
    warm._ensure_handle(dev)
    del warm
    lines = ["# Weight (re-)pack: host path against device path", "",
             f"Box: {props.name} ({getattr(props, 'gcnArchName', 'arch unknown')}), {props.multi_processor_count} CUs, "
             f"torch {torch.__version__}; commit {a.commit}; "
             f"`python tools/commit_time.py --repeats {a.repeats}`, one process.", "",
             "Host wall time in ms between two device synchronisations: median (min - max).  \"host\" is the yardstick: every tensor to "
             "the CPU, the blob packed on the host, one upload - the steps of the path before the device hand-over, run by this "
             "tree's host packer (which walks the layouts of csrc/weight_layouts.h; the earlier per-kernel loops were not "
             "measured).  \"device\" hands device pointers over and packs with kernels.  Copies: bytes host to device / bytes device to host / pack kernels of the LAST commit of that "
             "column (fsnp_debug_commit_stats; the `tensor.to(\"cpu\")` copies of the host column happen in Python and are not in them).", "",
             "| model | step | host: ms | host: up / down / kernels | device: ms | device: up / down / kernels | device / host |",
             "|---|---|---|---|---|---|---|"]
    verdict = []
    for title, cls, args, make_sd, nin in MODELS:
        res = {u: measure(cls, args, make_sd, nin, u, a.repeats, dev) for u in ("host", "device")}
        for step in ("first", "re-pack", "watch"):
            h, d = res["host"][step], res["device"][step]
            ch, cd = res["host"]["counts"][step], res["device"]["counts"][step]
            ratio = statistics.median(d) / statistics.median(h)
            verdict.append((title, step, ratio, cd))
            name = {"first": "first _ensure_handle", "re-pack": "re-pack after load_state_dict",
                    "watch": "forward sent back by the watch"}[step]
            lines.append(f"| {title} | {name} | {fmt(h)} | {ch[1]} / {ch[2]} / {ch[3]} | {fmt(d)} | {cd[1]} / {cd[2]} / {cd[3]} | {ratio:.2f} |")
        lines.append(f"| {title} | (a plain forward of that input) | {fmt(res['host']['plain'])} | | {fmt(res['device']['plain'])} | | |")
    slower = [f"{t}, {s} ({r:.2f} x)" for t, s, r, _ in verdict if r > 1.0]
    down = [f"{t}, {s}" for t, s, _, c in verdict if c[0] != 1 or c[2] != 0]
    lines += ["", "Expectation to confirm or refute: \"device\" is slower nowhere, and its re-packs copy nothing device to host.", "",
              "- slower than the host path: " + ("; ".join(slower) if slower else "nowhere"),
              "- device-path commits that copied to the host or took the host path: " + ("; ".join(down) if down else "none"), ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""What a window session (include/session/fsnp_window_stream.h) costs: writes profiles/window_stream.md from ONE process.

    python tools/window_stream_time.py [--repeats 15 --e2e-seconds 60 --commit <label> --out profiles/window_stream.md]

FullSubNet+, fp32 device buffers, W = 32 000, V = 4000 (2 s windows, 0.25 s overlap), 160-sample blocks (10 ms), max_batch = 32:
  1. a push that completes no window, 1 and 32 slots: pure glue (append + emit).  Device time of groups of GROUP consecutive such
     pushes (events around the group) over the group's pushes -> us per push, and GB/s against the bytes the two kernels move
     (per slot and push: the block read, written to the history, as many pending samples read and written out: 4 * 160 * 4 bytes).
  2. a window-completing push of 32 slots (append, pad, one forward of 32 windows, overlap-add, emit, compaction; events around
     the one push) against enhance_wave of a [32, 32000] batch, which is the same forward in the whole-clip call that existed before
     the sessions.  A window-completing push stands behind ~170 glue pushes that leave the GPU idle, so both calls are timed in both
     places - behind the idle stretch and behind the other one's forward - the order alternating window after window, and the
     surplus is taken like against like.  The session's surplus is the cost of the feature.
  3. end to end: 32 clips of --e2e-seconds fed in 160-sample blocks (all pushes + finish, host clock around work that ends in a
     synchronise: what a serving loop sees, Python included) against enhance_wave_windowed of the same clips (events around the
     call: the procedure of tools/windowed_time.py); the two alternate.

Every measured line carries the shader clock the box held in a 50 ms pure-MFMA probe right before it (fullsubnet_plus_amd.box.probe:
what bench.py --full reports).  Median (min - max) over the repeats.  No number from the table is asserted anywhere."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fullsubnet_plus_amd import FullSubNet_Plus, box, window_stream_plan  # noqa: E402
from fullsubnet_plus_amd.synthetic import DEFAULT_MODEL_ARGS, make_state_dict, make_wave  # noqa: E402

W, V, BLOCK, MAX_BATCH, GROUP = 32000, 4000, 160, 32, 25
S = W - V


def _cell(v, fmt="{:.2f}"):
    return f"{fmt.format(statistics.median(v))} ({fmt.format(min(v))} - {fmt.format(max(v))})"


def _events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def _clock():
    return box.probe(50.0)["clock_mhz"]


def _timed(fn):
    e0, e1 = _events()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stream_windows(m, slots, repeats, baseline):
    """Feed `slots` streams block by block.  -> (us per glue push of every glue group, then ms per call in four lists:) the
    window-completing push and baseline() each timed in both places a call can stand - "idle": right behind the ~170 glue pushes that
    precede a window, when the GPU has had microseconds of work per 10 ms block; "busy": right behind the other one's forward.  Windows
    alternate between push-then-baseline and baseline-then-push, `repeats` of each (baseline None: push only, 2 x repeats windows)."""
    wav = torch.from_numpy(make_wave(slots, (W + (2 * repeats + 1) * S) / 16000, 3000 + slots)).cuda()
    glue, t = [], {"push_idle": [], "base_busy": [], "base_idle": [], "push_busy": []}
    with m.open_window_stream(slots, W, V, max_samples=BLOCK, max_batch=MAX_BATCH) as ws:
        held, group, windows = 0, [], 0
        while held + BLOCK <= wav.shape[1]:
            block = wav[:, held:held + BLOCK]
            if window_stream_plan(held, BLOCK, W, V)[1] > 0:
                torch.cuda.synchronize()
                measured = held > W                                # (the first window is the warm-up of every shape)
                if baseline is not None and windows % 2 == 1:
                    tb, tp = _timed(baseline), _timed(lambda: ws.push(block))
                    if measured:
                        t["base_idle"].append(tb)
                        t["push_busy"].append(tp)
                else:
                    tp = _timed(lambda: ws.push(block))
                    tb = _timed(baseline) if baseline is not None else None
                    if measured:
                        t["push_idle"].append(tp)
                        if tb is not None:
                            t["base_busy"].append(tb)
                windows += 1
                group = []
            else:
                if not group:
                    e0, e1 = _events()
                    e0.record()
                ws.push(block)
                group.append(e0)
                if len(group) == GROUP:
                    e1.record()
                    e1.synchronize()
                    if held > 2 * W:                               # pending samples are read only once the clip is a window old
                        glue.append(1e3 * group[0].elapsed_time(e1) / GROUP)
                    group = []
            held += BLOCK
    return glue, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--e2e-seconds", type=float, default=60.0)
    ap.add_argument("--e2e-repeats", type=int, default=15)
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_stream.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/window_stream_time.py measures on the GPU; there is none here")
    lines = []
    with torch.no_grad():
        m = FullSubNet_Plus(**DEFAULT_MODEL_ARGS)
        m.load_state_dict(make_state_dict(0, "default"), strict=True)
        m = m.to("cuda").eval()
        m.batch_mode, m.error_check = "full", "deferred"
        batch = torch.from_numpy(make_wave(32, W / 16000, 2999)).cuda()
        for _ in range(2):
            m.enhance_wave(batch)
        torch.cuda.synchronize()
        # 1., 2.
        rows = []
        for slots in (1, 32):
            mhz = _clock()
            glue, t = stream_windows(m, slots, a.repeats, (lambda: m.enhance_wave(batch)) if slots == 32 else None)
            moved = 4 * BLOCK * 4 * slots
            gbs = [moved / (us * 1e-6) / 1e9 for us in glue]
            rows.append(f"| glue push, {slots} slot{'s' if slots > 1 else ''} | {len(glue)} groups of {GROUP} | {_cell(glue)} us per push | "
                        f"{_cell(gbs, '{:.3f}')} GB/s of {moved} B | {mhz:.0f} |")
            if slots == 32:
                names = {"push_idle": "window-completing push, 32 slots, behind idle glue pushes (where a serving loop has it)",
                         "base_idle": f"`enhance_wave` of [32, {W}] in that place", "push_busy": "the push right behind that `enhance_wave`",
                         "base_busy": f"`enhance_wave` of [32, {W}] right behind a push"}
                for k in ("push_idle", "base_idle", "push_busy", "base_busy"):
                    rows.append(f"| {names[k]} | {len(t[k])} | {_cell(t[k])} ms | - | {mhz:.0f} |")
                med = {k: statistics.median(v) for k, v in t.items()}
                spread = {k: max(t[k]) - min(t[k]) for k in ("base_idle", "base_busy")}

                def judge(push, base):
                    d = med[push] - med[base]
                    return (f"{d:+.2f} ms ({100 * d / med[base]:+.2f} % of that baseline's median), {'inside' if abs(d) <= spread[base] else 'outside'} "
                            f"the baseline's own spread (max - min) of {spread[base]:.2f} ms")
                verdict = ("- Surplus of the session's push over the same forward as a whole-clip call, like against like: behind idle "
                           f"glue {judge('push_idle', 'base_idle')}; behind a forward {judge('push_busy', 'base_busy')}.\n"
                           f"- The place alone (behind idle glue - behind a forward) moves the baseline by {med['base_idle'] - med['base_busy']:+.2f} ms "
                           f"and the push by {med['push_idle'] - med['push_busy']:+.2f} ms.")
            m.poll_errors()
        lines += ["| measurement | repeats | device time: median (min - max) | rate | held clock (MHz) |", "|---|---|---|---|---|"] + rows + ["", verdict, ""]
        # 3.
        L = int(a.e2e_seconds * 16000) // BLOCK * BLOCK
        wav = torch.from_numpy(make_wave(32, L / 16000, 2998))[:, :L].contiguous().cuda()

        def session():
            with m.open_window_stream(32, W, V, max_samples=BLOCK, max_batch=MAX_BATCH) as ws:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for at in range(0, L, BLOCK):
                    ws.push(wav[:, at:at + BLOCK])
                ws.finish()
                torch.cuda.synchronize()
                return 1e3 * (time.perf_counter() - t0)

        def whole():
            e0, e1 = _events()
            e0.record()
            m.enhance_wave_windowed(wav, W, V, max_batch=MAX_BATCH)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)
        session(), whole()
        mhz = _clock()
        runs = {"session": [], "whole": []}
        for _ in range(a.e2e_repeats):
            runs["session"].append(session())
            runs["whole"].append(whole())
        pushes = L // BLOCK
        ms, mw = statistics.median(runs["session"]), statistics.median(runs["whole"])
        lines += [f"End to end, 32 clips of {L / 16000:.1f} s ({pushes} pushes of {BLOCK} samples + finish), {a.e2e_repeats} repeats, the two alternating; "
                  f"held clock {mhz:.0f} MHz:", "",
                  "| version | ms: median (min - max) |", "|---|---|",
                  f"| window session: all pushes + finish, host clock to the final synchronise | {_cell(runs['session'])} |",
                  f"| `enhance_wave_windowed` of the same clips, device events | {_cell(runs['whole'])} |", "",
                  f"- The session takes {ms - mw:+.1f} ms ({100 * (ms - mw) / mw:+.1f} %) over the whole-clip call: {(ms - mw) / pushes * 1e3:.1f} us per "
                  f"push, host time of the Python loop included; audio arrives in {1e3 * L / 16000:.0f} ms, so the session runs at "
                  f"{1e3 * L / 16000 / ms:.1f} x real time for 32 streams.", ""]
        m.poll_errors()
    props = torch.cuda.get_device_properties(0)
    head = ["# Window sessions: live audio through FullSubNet+ in cross-faded windows", "",
            f"Box: {props.name} ({getattr(props, 'gcnArchName', '?')}), {props.multi_processor_count} CUs, torch {torch.__version__}; commit {a.commit}; "
            f"`python tools/window_stream_time.py --repeats {a.repeats} --e2e-seconds {a.e2e_seconds:g} --e2e-repeats {a.e2e_repeats}`, one process.", "",
            f"FullSubNet+, fp32 device buffers, W = {W}, V = {V}, blocks of {BLOCK} samples, max_batch = {MAX_BATCH}, error_check=\"deferred\".  "
            "What each line measures and how: the docstring of tools/window_stream_time.py.", ""]
    text = "\n".join(head + lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

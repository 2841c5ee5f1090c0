"""What streaming the original FullSubNet costs: time per push for S slots x n frames per push on one MI355X, next to the whole-clip
forward of the same S clips of 2 s measured in the same run on the unchanged offline path.

For every S in --slots and n in --chunks: median time per push (each timed run = --pushes pushes after a warm-up, median of --runs
runs), streams served in real time (= 16 ms * n / time per push * S; a frame is 16 ms of audio at hop 256 / 16 kHz) and the cost per
frame relative to forward(..., lengths=None) of the S clips.  Prints one JSON line per cell and one for each offline forward.  Not part
of bench.py.

    python tools/stream_throughput.py [--slots 1 8 32 64] [--chunks 1 4 16 64] [--runs 5] [--pushes 8]

--wave times wave sessions instead (FullSubNet.open_wave_stream: samples in, samples out): for every S in --slots, hop-sized pushes of
audio (one frame of the model per push) next to the mag push of n = 1 frame at the same S in the same run; one JSON line per S.

    python tools/stream_throughput.py --wave [--slots 1 32] [--runs 5] [--pushes 8]

--live adds a live session (open_stream(..., live=True): per-step kernels that fill the chip at one slot) beside the default one in every
cell it takes (n <= 16), timed in the same run right after it: "live_ms_per_push", the spread of both modes' runs (min and max of the
--runs timed runs, per push) and "live_speedup" = default / live.  With --wave the wave session is timed in both modes as well.

    python tools/stream_throughput.py --live [--slots 1 8 32 64] [--chunks 1 4 16]

--spec times spectrum sessions (FullSubNet.open_spec_stream: noisy STFT frames in, enhanced frames out).  Per cell and in one process:
the mag push alone, the loop a caller of a mag session writes around it to get enhanced frames (X.abs(), a per-slot list of the noisy
frames that wait look_ahead steps for their masks, a concatenate-and-slice per slot, the cIRM epilogue with lengths), and the spectrum
push that does the same on the device.  One JSON line per cell and session mode (--live adds the live sessions, n <= 16): medians with
min and max of the --runs timed runs, per push.

    python tools/stream_throughput.py --spec --live [--slots 1 8 64] [--chunks 1 4]

--rate times rate sessions (FullSubNet.open_wave_stream(..., live=True, sample_rate=R): 10 ms of audio at R per push, converted to and
from the model's rate inside the push) next to the model-rate live wave session fed the same 10 ms as 160-sample pushes.  All sessions
of one S are open at once and take turns run by run, so drift of the machine falls on all of them alike; one JSON line per S and
session: median with min and max of the --runs timed runs, per push.  --rates without a value times the model-rate session alone.

    python tools/stream_throughput.py --rate [--slots 1 8] [--rates 48000 44100 8000] [--runs 7] [--pushes 50]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fullsubnet_plus_amd import FullSubNet  # noqa: E402
from fullsubnet_plus_amd._args import _host_lengths  # noqa: E402
from fullsubnet_plus_amd.synthetic import FULLSUBNET_MODEL_ARGS, make_inputs, make_state_dict_fullsubnet, make_wave  # noqa: E402

FRAME_MS = 16.0


LIVE_MAX_CHUNK = 16


def timed_all(fn, runs):
    """every timed run's seconds (after one warm-up run)"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def timed(fn, runs):
    return statistics.median(timed_all(fn, runs))


def wave_mode(model, a):
    """hop-sized wave pushes next to the mag push of one frame, per S"""
    hop = model.num_freqs - 1
    for S in a.slots:
        mag = make_inputs(S, 2.0, 3)[0][..., :1].contiguous().cuda()
        wav = torch.from_numpy(make_wave(S, 2.0, 3)).cuda()
        blocks = [wav[:, k * hop:(k + 1) * hop].contiguous() for k in range(a.pushes)]
        with model.open_stream(S, max_chunk=1) as st:
            def run_mag():
                for _ in range(a.pushes):
                    st.push(mag)
            mag_push = timed(run_mag, a.runs) / a.pushes
        with model.open_wave_stream(S, max_samples=hop) as ws:
            def run_wave():
                for blk in blocks:
                    ws.push(blk)
            wave_push = timed(run_wave, a.runs) / a.pushes
        rec = {"slots": S, "samples_per_push": hop, "wave_ms_per_push": round(wave_push * 1e3, 4),
               "mag_ms_per_push": round(mag_push * 1e3, 4), "wave_minus_mag_ms": round((wave_push - mag_push) * 1e3, 4),
               "real_time_streams": round(FRAME_MS * 1e-3 / wave_push * S, 1)}
        if a.live:
            with model.open_wave_stream(S, max_samples=hop, live=True) as ws:
                def run_live():
                    for blk in blocks:
                        ws.push(blk)
                live_push = timed(run_live, a.runs) / a.pushes
            rec.update({"live_wave_ms_per_push": round(live_push * 1e3, 4), "live_speedup": round(wave_push / live_push, 2),
                        "live_real_time_streams": round(FRAME_MS * 1e-3 / live_push * S, 1)})
        print(json.dumps(rec))


def rate_mode(model, a):
    """10 ms pushes: the model-rate live wave session and a live rate session per rate in a.rates, alternating run by run"""
    for S in a.slots:
        wav = torch.from_numpy(make_wave(S, 2.0, 3)).cuda()
        sessions = {}
        try:
            for rate in [model.sample_rate] + list(a.rates):
                c = rate // 100
                assert a.pushes * c <= wav.shape[1], "--pushes: 2 s of audio per slot"
                kw = {} if rate == model.sample_rate else {"sample_rate": rate}
                ws = model.open_wave_stream(S, max_samples=c, live=True, **kw)
                sessions[rate] = (ws, [wav[:, k * c:(k + 1) * c].contiguous() for k in range(a.pushes)], [])
            for rnd in range(a.runs + 1):                              # round 0 warms every session up
                for rate, (ws, blocks, runs) in sessions.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for blk in blocks:
                        ws.push(blk)
                    torch.cuda.synchronize()
                    if rnd:
                        runs.append((time.perf_counter() - t0) / a.pushes)
            base = statistics.median(sessions[model.sample_rate][2])
            for rate, (ws, blocks, runs) in sessions.items():
                med = statistics.median(runs)
                print(json.dumps({"slots": S, "sample_rate": rate, "samples_per_push": rate // 100, "delay_ms": round(1e3 * ws.delay / rate, 2),
                                  "ms_per_push": round(med * 1e3, 4), "ms_per_push_min_max": [round(min(runs) * 1e3, 4), round(max(runs) * 1e3, 4)],
                                  "minus_model_rate_ms": round((med - base) * 1e3, 4), "real_time_streams": round(10e-3 / med * S, 1)}))
        finally:
            for ws, _, _ in sessions.values():
                ws.close()


def recipe_push(model, st, X, counts, lengths, delay):
    """One push of a mag session with the other half of a spectrum session written out in torch: -> enhanced [S, F, n] complex64.
    delay[b]: the noisy frames of slot b that have no mask yet, complex [F, <= look_ahead] (frames P - w .. P - 1)."""
    S, F, n = X.shape
    la = st.look_ahead
    mask = st.push(X.abs().unsqueeze(1), counts)              # column j of slot b = cIRM of frame P_b + j - look_ahead
    aligned = torch.zeros((S, n, F), dtype=torch.complex64, device=X.device).transpose(1, 2)
    for b in range(S):
        c = counts[b]
        if c == 0:
            continue
        w = delay[b].shape[1]
        buf = torch.cat([delay[b], X[b, :, :c]], dim=1)       # frames P - w .. P + c - 1
        lead = la - w                                         # columns of steps before look_ahead: the mask is exactly 0 there
        if c > lead:
            aligned[b, :, lead:c] = buf[:, :c - lead]
        delay[b] = buf[:, max(w + c - la, 0):]
    return model._apply_cirm(mask, aligned, lengths)          # fsnp_apply_cirm_lengths: exactly 0 past counts[b]


def spec_mode(model, a):
    """the mag push, the recipe around it and the spectrum push, per cell and session mode"""
    F = model.num_freqs

    def ms(runs):
        return {"median": round(statistics.median(runs) * 1e3, 4), "min": round(min(runs) * 1e3, 4), "max": round(max(runs) * 1e3, 4)}

    for S in a.slots:
        _, re, im = make_inputs(S, 2.0, 3)
        full = torch.complex(re[:, 0], im[:, 0]).cuda()
        for n in a.chunks:
            reps = (n + full.shape[-1] - 1) // full.shape[-1]
            X = full.repeat(1, 1, reps)[:, :, :n].transpose(1, 2).contiguous().transpose(1, 2)      # torch.stft's order: bins fastest
            mag = X.abs().unsqueeze(1)
            counts = [n] * S
            lengths = _host_lengths(counts, S, "stream_throughput")
            for live in ([False, True] if a.live and n <= LIVE_MAX_CHUNK else [False]):
                with model.open_stream(S, max_chunk=n, live=live) as st:
                    def run_mag():
                        for _ in range(a.pushes):
                            st.push(mag)
                    mag_runs = [t / a.pushes for t in timed_all(run_mag, a.runs)]
                    st.reset()
                    delay = {b: torch.empty((F, 0), dtype=torch.complex64, device="cuda") for b in range(S)}

                    def run_recipe():
                        for _ in range(a.pushes):
                            recipe_push(model, st, X, counts, lengths, delay)
                    recipe_runs = [t / a.pushes for t in timed_all(run_recipe, a.runs)]
                with model.open_spec_stream(S, max_chunk=n, live=live) as ss:
                    def run_spec():
                        for _ in range(a.pushes):
                            ss.push(X)
                    spec_runs = [t / a.pushes for t in timed_all(run_spec, a.runs)]
                m, r, p = (statistics.median(v) for v in (mag_runs, recipe_runs, spec_runs))
                print(json.dumps({"slots": S, "chunk": n, "live": live, "mag_ms_per_push": ms(mag_runs), "recipe_ms_per_push": ms(recipe_runs),
                                  "spec_ms_per_push": ms(spec_runs), "spec_minus_mag_ms": round((p - m) * 1e3, 4),
                                  "recipe_over_spec": round(r / p, 2), "spec_at_or_below_recipe_max": bool(p <= max(recipe_runs))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wave", action="store_true", help="time wave sessions (hop-sized pushes) next to the mag push of one frame")
    ap.add_argument("--spec", action="store_true", help="time spectrum sessions next to the mag push and the host-side loop they replace")
    ap.add_argument("--live", action="store_true", help="time a live session beside the default one in every cell of n <= 16 frames")
    ap.add_argument("--rate", action="store_true", help="time live rate sessions (10 ms per push) next to the model-rate live wave session")
    ap.add_argument("--rates", type=int, nargs="*", default=[48000, 44100, 8000], help="--rate: the sample rates (none: the model-rate session alone)")
    ap.add_argument("--slots", type=int, nargs="+", default=[1, 8, 32, 64])
    ap.add_argument("--chunks", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--pushes", type=int, default=8)
    a = ap.parse_args()

    model = FullSubNet(**dict(FULLSUBNET_MODEL_ARGS, norm_type="cumulative_laplace_norm"))
    model.load_state_dict(make_state_dict_fullsubnet(0, "default"), strict=True)
    model = model.to("cuda").eval()
    model.batch_mode = "full"
    model.error_check = "deferred"

    with torch.no_grad():
        if a.rate:
            rate_mode(model, a)
            model.check_errors()
            return
        if a.wave:
            wave_mode(model, a)
            model.check_errors()
            return
        if a.spec:
            spec_mode(model, a)
            model.check_errors()
            return
        for S in a.slots:
            mag = make_inputs(S, 2.0, 3)[0].contiguous().cuda()          # [S, 1, F, 126]
            T = mag.shape[-1]
            off = timed(lambda: model(mag), a.runs)
            off_frame = off / T
            print(json.dumps({"slots": S, "offline_frames": T, "offline_ms": round(off * 1e3, 3), "offline_us_per_frame": round(off_frame * 1e6, 2)}))
            for n in a.chunks:
                x = mag[..., :n].contiguous() if n <= T else mag.repeat(1, 1, 1, (n + T - 1) // T)[..., :n].contiguous()
                with model.open_stream(S, max_chunk=n) as st:
                    def run():
                        for _ in range(a.pushes):
                            st.push(x)
                    runs = [t / a.pushes for t in timed_all(run, a.runs)]
                per_push = statistics.median(runs)
                rec = {"slots": S, "chunk": n, "ms_per_push": round(per_push * 1e3, 4),
                       "us_per_frame": round(per_push / n * 1e6, 2),
                       "real_time_streams": round(FRAME_MS * 1e-3 * n / per_push * S, 1),
                       "per_frame_vs_offline": round(per_push / n / off_frame, 3)}
                if a.live and n <= LIVE_MAX_CHUNK:
                    with model.open_stream(S, max_chunk=n, live=True) as st:
                        live_runs = [t / a.pushes for t in timed_all(run, a.runs)]
                    live = statistics.median(live_runs)
                    rec.update({"ms_per_push_min_max": [round(min(runs) * 1e3, 4), round(max(runs) * 1e3, 4)],
                                "live_ms_per_push": round(live * 1e3, 4),
                                "live_ms_per_push_min_max": [round(min(live_runs) * 1e3, 4), round(max(live_runs) * 1e3, 4)],
                                "live_speedup": round(per_push / live, 2),
                                "live_real_time_streams": round(FRAME_MS * 1e-3 * n / live * S, 1)})
                print(json.dumps(rec))
    model.check_errors()


if __name__ == "__main__":
    main()

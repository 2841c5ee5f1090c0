"""The test / bench / tuning hooks of a model: the Python counterpart of include/fsnp_debug.h, apart from the product surface in model.py
as that header is apart from include/fsnp.h.  _HipModel inherits the mixin, which uses its _handle, _hip, _ensure_handle and _setting."""
import ctypes

import torch

from . import _call, _lib


class _DebugHooks:
    def verify_sample_stats(self):
        """-> {"samples", "skipped", "eligible_forwards"} of the sampled exchange verification (fsnp_set_verify_sample)."""
        out = (ctypes.c_int64 * 3)()
        _call.check(_lib.load().fsnp_debug_verify_sample_stats, self._handle, ctypes.byref(out))
        return {"samples": int(out[0]), "skipped": int(out[1]), "eligible_forwards": int(out[2])}

    def debug_corrupt_exchange(self, step):
        """Test hook (fsnp_debug_corrupt_exchange): the next forward's column-split launches publish one wrong h0 value at `step` - 1."""
        _call.check(_lib.load().fsnp_debug_corrupt_exchange, self._handle, int(step))

    def read_stage(self, name, batch, frames):
        """Stage buffer of the last forward, time-major: [B, T', F] (gates: [B, F])."""
        rows = batch if name.startswith("gate_") else batch * (frames + self.look_ahead)
        host = torch.empty((rows, self.num_freqs), dtype=torch.float32)
        _call.check(_lib.load().fsnp_read_stage, self._handle, name.encode(), host.data_ptr(), host.numel())
        return host if name.startswith("gate_") else host.view(batch, frames + self.look_ahead, self.num_freqs)

    def debug_set_num_cus(self, num_cus, device="cuda"):
        """Test hook: plan LSTM tiles as if the chip had `num_cus` CUs (exercises multi-round / VALU-row tiles)."""
        self._setting("fsnp_debug_set_num_cus", int(num_cus), device=device)

    def debug_set_lstm_waves(self, waves, device="cuda"):
        """Tuning hook: waves per workgroup of the fused LSTM kernel (12 = three per SIMD, or 4)."""
        self._setting("fsnp_debug_set_lstm_waves", int(waves), device=device)

    def debug_set_lstm_coop(self, mode, device="cuda"):
        """Tuning hook: 1 = use the column-split LSTM kernels for small batches (default), 0 = never, 2 = as 1 with the
        K-split kernel's serial (round-1) step schedule instead of the layer-skewed one and without the half-tile ping-pong
        kernel, 4 = as 1 + the half-tile ping-pong kernel even where FSNP_COOP_HP=0."""
        self._setting("fsnp_debug_set_lstm_coop", int(mode), device=device)
        self.__dict__["_lstm_coop_mode"] = int(mode)

    def debug_set_gemm_dma(self, mode, device="cuda"):
        """Tuning hook: 1 = full-band TCN GEMMs on the LDS-DMA kernels with GroupNorm folded into the weights (default; small
        batches: the split-K kernel tcn_gemm_sk_kernel; sconv of larger problems: the 64-row kernel tcn_gemm_dma64_kernel), 2 = as 1 but
        never the small-batch kernel, 3 = the 128-row DMA kernel only, 0 = the general GEMM kernel."""
        self._setting("fsnp_debug_set_gemm_dma", int(mode), device=device)

    def debug_set_chaos(self, seed, device="cuda"):
        """Test hook: drift injection for the column-split recurrent kernels (fsnp_debug_set_chaos); 0 = off."""
        self._setting("fsnp_debug_set_chaos", int(seed), device=device)

    def debug_window_roundtrip(self, wav, window, overlap, lengths=None, out_format=None, clipped=None, max_batch=32):
        """Test hook (fsnp_debug_window_roundtrip, include/ext/fsnp_windowed.h): enhance_wave_windowed with the model replaced by a copy
        of every window, so that only the plan and its two kernels run: the result equals wav bit for bit, 0 past the lengths."""
        enqueue, out = self._windowed_call("fsnp_debug_window_roundtrip", "debug_window_roundtrip", wav, window, overlap, lengths, out_format,
                                           clipped, max_batch)
        _lib.check(enqueue(), "fsnp_debug_window_roundtrip")
        return out

    def debug_open_window_stream_copy(self, slots, window, overlap, max_samples=4096, max_batch=32, device="cuda"):
        """Test hook (fsnp_debug_window_stream_create_copy, include/session/fsnp_window_stream.h): open_window_stream with every
        forward replaced by a copy of its windows, so that only the schedule and the session's kernels run: the session returns its
        input `window` samples late, bit for bit.  Skips the model's minimum clip."""
        from ._args import window_stream_args
        from .stream import WindowStream

        class _CopyWindowStream(WindowStream):
            _copy = True
        args = window_stream_args(slots, window, overlap, max_samples, max_batch, self.num_freqs, "debug_open_window_stream_copy")
        return _CopyWindowStream(self, *args, _call.resolve_device(device))

    def debug_inject_error(self):
        """Test hook: pretend an inter-workgroup wait timed out (see fsnp_debug_inject_error)."""
        _call.check(_lib.load().fsnp_debug_inject_error, self._handle)

    def set_timing(self, enable=True):
        _call.check(_lib.load().fsnp_set_timing, self._handle, int(bool(enable)))

    def get_timing(self, reset=True):
        """-> {"lstm_ms", "fullband_ms", "forward_ms", "count"}: hipEvent sums on the forward's stream."""
        ms = (ctypes.c_double * 4)()
        cnt = (ctypes.c_int64 * 4)()
        _call.check(_lib.load().fsnp_get_timing, self._handle, ctypes.byref(ms), ctypes.byref(cnt), int(reset))
        return {"lstm_ms": ms[0], "fullband_ms": ms[1], "forward_ms": ms[2], "lstm_first_chunk_ms": ms[3], "count": int(cnt[0])}

    def launch_clock(self):
        """-> {"wall_ms", "s_memtime_ticks", "s_memtime_mhz"} of the LAST launch of the one-tile-per-CU LSTM kernel on this handle, as its
        workgroup 0 stamped them (fsnp_debug_launch_clock; synchronise first), or None if there was no such launch."""
        out = (ctypes.c_double * 7)()
        if _call.enqueue(_lib.load().fsnp_debug_launch_clock, self._hip.device, self._handle, ctypes.byref(out), stream=False) != 0:
            return None
        return {"wall_ms": out[2], "s_memtime_ticks": out[0], "s_memtime_mhz": out[3], "slowest_workgroup_ms": out[4],
                "fastest_workgroup_ms": out[5], "most_cycles_of_a_workgroup": out[6]}

    def describe_plan(self, batch, parity=False):
        """-> [{"kernel", "sequences", "tiles", "valu_rows", "precision", "workgroups", "deferred_when_pipelined"}, ...]: how the
        sub-band sequences of a `batch`-utterance forward are cut into kernel launches, the arithmetic each launch runs in under the
        current set_precision mode, and whether the pipelined serving loop sends it to the side stream (fsnp_describe_plan_ex)."""
        buf = (ctypes.c_int32 * 112)()
        n = _lib.load().fsnp_describe_plan_ex(self._handle, int(batch), int(parity), buf, 16)
        if n < 0:
            raise RuntimeError(_lib.last_error())
        names = {0: ("gru2_fc_kernel" if self.sequence_model == "GRU" else "lstm2_fc_kernel") + " (one 32-row tile per CU)",
                 1: "lstm2_coop_kernel (K split)",
                 2: "lstm2_coopn_kernel (three-way column split)", 3: "sub-band TCN",
                 4: "lstm2_fc16_kernel (one 16-row tile per CU)",
                 11: "lstm2_generic_kernel (runtime-sized fp32 FMA kernel: no tuned instantiation for these sizes)",
                 12: "lstm2_coop_hp_kernel (16 units per workgroup, gate-split waves, two half tiles per row tile in turn)",
                 13: "lstm2_coopw_kernel (a wave owns 8 / 16 units over the whole K, layer-skewed, no workgroup barrier)",
                 14: "lstm2_coop_hpw_kernel (16 units per workgroup, a wave owns 4 of them over the whole K, two half tiles per row tile in turn, no workgroup barrier)"}
        prec = {0: "f32", 1: "f32 + bf16 layer-1 ih-GEMM"}
        return [{"kernel": names[buf[7 * i]], "sequences": buf[7 * i + 1], "tiles": buf[7 * i + 2], "valu_rows": buf[7 * i + 3],
                 "precision": prec[buf[7 * i + 4]], "workgroups": buf[7 * i + 5], "deferred_when_pipelined": bool(buf[7 * i + 6])} for i in range(n)]

    def pipeline_pairing(self, batch):
        """-> [{"chunk", "kind", "tiles", "workgroups", "max_per_xcd", "fb_workgroups", "fb_max_per_xcd", "fb_per_cu", "side_by_side"}, ...]:
        for each sub-band launch the pipelined loop defers at `batch` utterances (full mode), whether the next forward's full-band LSTM
        runs beside it or is chained behind it, as this handle decides it (fsnp_debug_pipeline_pairing; FullSubNet+: [])."""
        buf = (ctypes.c_int32 * (9 * 16))()
        n = _lib.load().fsnp_debug_pipeline_pairing(self._handle, int(batch), buf, 16)
        if n < 0:
            raise RuntimeError(_lib.last_error())
        keys = ("chunk", "kind", "tiles", "workgroups", "max_per_xcd", "fb_workgroups", "fb_max_per_xcd", "fb_per_cu", "side_by_side")
        return [dict(zip(keys, buf[9 * i:9 * i + 9])) for i in range(n)]

    def fullband_launch(self, batch):
        """-> {"kernel", "tiles", "rows_per_tile", "units"}: the full-band LSTM launch of a `batch`-utterance forward of the original
        FullSubNet (fsnp_debug_fullband_launch; kernel: "coop_seq" / "fbv" / "generic")."""
        out = (ctypes.c_int32 * 4)()
        _call.check(_lib.load().fsnp_debug_fullband_launch, self._handle, int(batch), ctypes.byref(out))
        return {"kernel": ("coop_seq", "fbv", "generic")[out[0]], "tiles": out[1], "rows_per_tile": out[2], "units": out[3]}

    def coop_chain_stats(self, reset=False):
        """-> (beside, chained): this handle's column-split launches that ran beside / were chained behind one of its own launches on
        another stream since the last reset (fsnp_debug_coop_chain_stats)."""
        out = (ctypes.c_int64 * 2)()
        _call.check(_lib.load().fsnp_debug_coop_chain_stats, self._handle, ctypes.byref(out), int(bool(reset)))
        return int(out[0]), int(out[1])

    def debug_set_costs(self, costs=None, workgroups_per_cu=1, device="cuda"):
        """Test hook: pin the planner's cost table (_lib.NUM_COSTS values, fsnp_get_costs order; None = built-in) and whether it
        may put two column-split workgroups on a CU (fsnp_debug_set_costs).  A shorter table prices the launch shapes it does
        not name out of every plan (19 values = no half-tile ping-pong kernel and no wave-owned column split, 21 = no wave-owned
        column split)."""
        n = _lib.NUM_COSTS
        if costs is not None and len(costs) < n:
            costs = list(costs) + [1e9] * (n - len(costs))
        arr = (ctypes.c_double * n)(*costs) if costs is not None else None
        self._setting("fsnp_debug_set_costs", arr, int(workgroups_per_cu), device=device)

    @staticmethod
    def _cost_dict(v):
        return {"ksplit_us": {u: {"one_per_cu": v[2 * i], "two_per_cu": v[2 * i + 1], "one_tile": v[14 + i]} for i, u in enumerate((8, 16, 32, 64))},
                "coopn_us": {r: {"one_per_cu": v[8 + 2 * i], "two_per_cu": v[9 + 2 * i]} for i, r in enumerate((1, 2))},
                "rowtile_us": v[12], "valu_row_surcharge": v[13], "rowtile16_us": v[18],
                "halftile_pingpong_us": {"one_tile": v[19], "full_launch": v[20]},
                "coopw_us": {**{u: {"one_tile": v[23 + i], "full_launch": v[21 + i]} for i, u in enumerate((32, 64))},
                             96: {"one_tile": v[26], "full_launch": v[25]}}}

    def measure_costs(self):
        """-> the same table MEASURED on the device (fsnp_measure_costs; ~0.3 s, synchronises; the plan is not touched)."""
        buf = (ctypes.c_double * _lib.NUM_COSTS)()
        _call.call(_lib.load().fsnp_measure_costs, self._hip.device, self._handle, ctypes.byref(buf), stream=False)
        return self._cost_dict(list(buf))

    def dump_config(self):
        """-> text: the handle's configuration and every effective FSNP_* setting (fsnp_dump_config), for bug reports."""
        lib = _lib.load()
        n = lib.fsnp_dump_config(self._handle, None, 0)
        buf = ctypes.create_string_buffer(int(n))
        lib.fsnp_dump_config(self._handle, buf, n)
        return buf.value.decode()

    def planner_costs_raw(self):
        """-> the _lib.NUM_COSTS values of fsnp_get_costs (the layout debug_set_costs takes)."""
        buf = (ctypes.c_double * _lib.NUM_COSTS)()
        _call.check(_lib.load().fsnp_get_costs, self._handle, ctypes.byref(buf), None, None)
        return list(buf)

    def planner_costs(self):
        """-> the per-step cost table (us) the sub-band planner minimises (fsnp_get_costs)."""
        buf, cal, occ = (ctypes.c_double * _lib.NUM_COSTS)(), ctypes.c_int32(), ctypes.c_int32()
        _call.check(_lib.load().fsnp_get_costs, self._handle, ctypes.byref(buf), ctypes.byref(cal), ctypes.byref(occ))
        return {**self._cost_dict(list(buf)), "calibrated": bool(cal.value), "workgroups_per_cu": occ.value}

    def forward_flops(self, batch, frames, parity=False):
        return float(_lib.load().fsnp_forward_flops(self._handle, batch, frames, int(parity)))

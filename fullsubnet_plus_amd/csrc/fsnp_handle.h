// fsnp_handle.h - the handle behind the C ABI (include/fsnp.h) and the helpers its translation units share:
// fsnp_abi.hip (create / forward orchestration / workspace / calibration), forward_kernels.hip (the forward's small kernels),
// fsnp_verify.hip (exchange verification), fsnp_debug_abi.hip (include/fsnp_debug.h: test and tuning hooks), fsnp_weights.hip
// (strict weight loading + packing), fsnp_stft_abi.hip (STFT / iSTFT / waveform entry points), fsnp_windowed_abi.hip, fsnp_stream_abi.hip,
// fsnp_wave_stream_abi.hip, fsnp_spec_stream_abi.hip and fsnp_wave_rate_stream_abi.hip (stream, wave, spectrum and rate sessions, and the
// slot helpers they share), fsnp_window_stream_abi.hip (window sessions).  Host only.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "fsnp_common.h"
#include "planner.h"
#include "resample.h"
#include "windowed.h"

namespace fsnp {

struct WeightSpec {
    std::string name;
    int64_t numel;
};

struct Workspace {
    // offsets in bytes from the workspace base
    size_t att, fb, raw, x, y1, y2, gate, md, md_utt, md_row, rows, fb_rows, frame, sbt_x0, sbt_x, sbt_fb, sbt_y1, sbt_y2, zero_begin,
        fsum, fe_tot, gn, sb_acc, coop_hx, coop_bar, coop_abort, fb_hx, fb_bar, sbt_gn, zero_end, dbg_tcn0,
        lens,   // fsnp_forward_lengths only (0 bytes otherwise): int32 [2][B] = lengths[b], lengths[b] + look_ahead
        total;
};

struct TimingRec {
    hipEvent_t e[4];  // start, after full-band stages, after the sub-band model (= end), after its FIRST chunk
};

// Every entry point that touches the device runs on the handle's device and puts the caller's current device back.
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess; else prev = -1;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
#define FSNP_ON_DEVICE(h)                                                              \
    fsnp::DeviceGuard _dev_guard((h)->device);                                         \
    if (!_dev_guard.ok) { fsnp::set_error("hipSetDevice(%d) failed", (h)->device); return 1; }

}  // namespace fsnp

using namespace fsnp;      // (internal header of the host translation units)

struct fsnp_handle {
    fsnp_config cfg{};
    int device = 0;
    int F = 0, FP = 0, CH = 0, H = 0, NSB = 0, NIN = 0, KX = 0, NB = 0, Fr = 0;
    std::vector<WeightSpec> specs;
    // the parameters as the caller gave them, back to back in specs order: a host copy (fsnp_set_weight) and a device copy
    // (fsnp_set_weight_device; one allocation, made on first use).  spec_src[i]: 0 = never given, 1 = the host copy is the newest,
    // 2 = the device copy is, 3 = both hold it (a device-given tensor that a host-path commit downloaded)
    std::vector<float> host_arena;
    std::vector<long long> spec_off;         // float offset of spec i in either arena
    std::vector<unsigned char> spec_src;
    std::map<std::string, int> spec_index;
    long long arena_floats = 0;
    float* d_arena = nullptr;
    hipEvent_t ev_arena = nullptr;           // recorded behind every arena copy on its own stream: a copy or a pack on another stream waits for it
    hipStream_t arena_stream = nullptr;
    bool arena_valid = false;
    bool committed = false;

    float* d_weights = nullptr;
    size_t blob_floats = 0;                  // size of d_weights (depends on the configuration only)
    std::vector<float> refl_host;            // device commit: the unfold multiplicities, uploaded from here (kept alive for the copy)
    int64_t commit_stats[4] = {0, 0, 0, 0};  // fsnp_debug_commit_stats: path, bytes host -> device, bytes device -> host, pack kernels
    hipEvent_t ev_packed = nullptr;          // end of the last device pack: stream-session pushes on another stream wait for it
    hipStream_t packed_stream = nullptr;
    bool packed_valid = false;
    FrontendWeights fw{};
    TcnWeights tw{};
    LstmWeights lw{};
    // original FullSubNet only: full-band 2-layer LSTM(F -> CH) (cooperative kernel) + Linear(CH, F) (GEMM)
    int model = FSNP_MODEL_FULLSUBNET_PLUS;
    int NFB = 3;                 // full-band features per sub-band frame: 3 (FullSubNet+) or 1 (FullSubNet)
    int gru = 0;                 // 1 = nn.GRU cells (sub-band model; FullSubNet: also the full-band model)
    PlannerOptions planner{};    // what the sub-band planner knows of the handle besides its sizes (planner.h; occupancies measured at commit)
    int occ_fb[3] = {0, 0, 0};   // FullSubNet: workgroups of the full-band lstm_coop_seq at 8 / 16 / 32 units one CU holds (measured at commit; 0 = unknown)
    int calibrate = 0;           // FSNP_CALIBRATE=1: replace the built-in table by one measured on this device at the first planning call
    int sb_tcn = 0;              // 1 = the sub-band model is a TCN stack (FullSubNet+ with sequence_model="TCN")
    TcnWeights sbt{};            //     its weights (one branch, NIN input channels)
    int XS = 0;                  //     row stride of its [slot][t][NIN] activations
    int NG = 4;                  // gate blocks per weight matrix: 4 (LSTM) or 3 (GRU)
    LstmWeights fbw{};
    const float* fsn_wf = nullptr;   // [F pad 384][CH pad 16]
    const float* fsn_bf = nullptr;   // [F pad 384]
    int fsn_kp = 0;
    const float* d_refl_w = nullptr;
    const float* d_refl_wfb = nullptr;

    unsigned char* ws = nullptr;
    size_t ws_bytes = 0;
    Workspace last_ws{};
    Dims last_dims{};
    bool have_last = false;
    bool debug = false;
    int num_cus = 256;
    int num_cus_real = 256;   // never overridden: residency of the cooperative kernel depends on the real chip
    int ih_bf16 = 0;             // 1 = BASELINE.json configs[4]: layer-1 ih-GEMM of the sub-band LSTM in bf16
    int coop_chaos = 0;          // fsnp_debug_set_chaos: drift injection seed for the column-split kernels (0 = off)
    int coop_skew = 1;           // K-split kernel: 1 = layer-skewed schedule (lstm2_coop_skew_kernel), 0 = the serial one (FSNP_COOP_SKEW=0)
    bool generic_sb = false;     // the sub-band recurrent model runs on the runtime-sized kernel (lstm_generic.hip): a hidden size or an
                                 // input width no tuned kernel is instantiated for
    bool generic_fb = false;     // FullSubNet: the same for the full-band recurrent model (fb_model_hidden_size != 512 or > 264 bins)
    int hp_wave = 1;             // HalfTilePingPong launches run on the wave-owned variant (lstm_hpw.hip); FSNP_HP_WAVE=0: lstm_hp.hip
    int coop_hp_cfg = 0;         // planner.coop_hp as FSNP_COOP_HP set it (fsnp_debug_set_lstm_coop(h, 1) restores it)
    int fb_valu = 1;             // FullSubNet: the full-band LSTM of <= 4 utterances runs on the VALU kernel (lstm_fbv.hip); fsnp_debug_set_gemm_dma-like
                                 // test switch: fsnp_debug_set_lstm_coop(h, 2) turns it off together with the other round-3+ schedules
    unsigned* d_err = nullptr;   // [0] = error bits of finished launches (kErr*): an inter-workgroup wait timed out in a column-split LSTM
                                 // kernel / the watched source tensors no longer match the packed weights / a verification pass
                                 // disagreed.  Host-mapped, so the NEXT call on
                                 // the handle can fail loudly without a device synchronisation
    // fsnp_watch_weights: the caller's SOURCE tensors of the packed weights, fingerprinted on the device in front of every forward
    void* watch_segs = nullptr;              // device: WatchSeg[watch_nseg]
    unsigned long long* watch_acc = nullptr; // device: {-, finished blocks, baseline, ..., [8 + b] partial sum of block b}
    int watch_nseg = 0, watch_every = 1;
    long long watch_calls = 0;
    // fsnp_set_verify: every Nth forward whose plan holds a column-split launch is re-run on the one-tile-per-CU kernel and compared
    int verify_every = 0;
    long long verify_calls = 0, verify_runs = 0;
    float* verify_out = nullptr;             // scratch mask of the verification pass (stream-ordered allocation)
    unsigned long long* d_clk = nullptr;     // device: clock stamps of the last one-tile-per-CU LSTM launch (LstmArgs::clk, fsnp_debug_launch_clock)
    unsigned long long* verify_key_sampled = nullptr;   // the same key of the sampled check (inside vs_buf)
    unsigned long long* verify_key = nullptr; // device: smallest (utterance << 44 | bin << 24 | frame) at which a verification pass disagreed
    size_t verify_bytes = 0;
    // fsnp_set_verify_sample (round 6): every Nth forward whose plan is column-split launches only, ONE row tile of one of them (they come
    // up in turn) is recomputed on the exchange-free half-tile kernel from a snapshot, on a stream of its own, beside the forwards that follow
    int vs_every = 0;
    long long vs_calls = 0, vs_runs = 0, vs_skipped = 0;
    hipStream_t vs_stream = nullptr;
    hipEvent_t ev_vs_snap = nullptr, ev_vs_done = nullptr;
    bool vs_busy = false;                    // ev_vs_done has been recorded and not yet seen complete
    unsigned char* vs_buf = nullptr;         // snapshot + reference buffers (private: nothing a later forward or the caller touches)
    size_t vs_bytes = 0;
    int corrupt_exchange = 0;                // fsnp_debug_corrupt_exchange: flip one word of the next column-split launch's exchange (test hook)
    int lstm_waves = 0;   // 0 = auto: 12 waves when the tile plan uses VALU rows, else 4

    // STFT / iSTFT around the model (stft.hip): DFT GEMM operands, built on first use, and an I/O workspace
    float* d_stft = nullptr;     // [fwd (2F pad 384) x (n_fft pad 16)][inv (n_fft pad 384) x (2F pad 16)][window n_fft][zero bias]
    int hop_length = 0;          // fsnp_set_hop_length (include/fsnp_stft_geometry.h); 0 = never set: n_fft / 2
    unsigned char* io = nullptr;
    size_t io_bytes = 0;
    // include/fsnp_resample.h: the tap tables of the (up, down) pairs this handle has run, at most kResampleMaxPairs, never evicted
    std::vector<fsnp::ResampleCached> resample;
    // include/ext/fsnp_windowed.h: the windows' enhanced fp32 rows [windows][window] (behind them the first pass of FSNP_SAMPLE_S16_PEAK),
    // grown stream-ordered like io, and the cross-fade tables of the overlaps this handle has run, at most kWindowMaxFades, never
    // evicted (like `resample`)
    unsigned char* win_stage = nullptr;
    size_t win_stage_bytes = 0;
    std::vector<fsnp::WindowFade> win_fades;

    bool timing = false;
    std::vector<TimingRec> timing_recs;   // recorded, not yet read back (drained by fsnp_get_timing, or when 256 pile up)
    std::vector<hipEvent_t> event_pool;   // events are re-used: a forward with timing on allocates nothing in steady state
    double acc_ms[4] = {0, 0, 0, 0};
    int64_t acc_cnt[4] = {0, 0, 0, 0};

    // pipelined serving mode (fsnp_set_pipeline): the column-split remainder chunks that follow a row-tile chunk run on
    // `side_stream`, so that they overlap the full-band stages of the NEXT forward (which leave most CUs idle); the
    // workspace is double buffered because forward i+1 rebuilds att / fb while the remainder of forward i still reads them
    int pipeline = 0;
    int defer_small = 1;         // pipelined mode: plans that start with a column-split launch run on the side stream whole (FSNP_DEFER_SMALL=0: off)
    int ws_slots = 1, ws_slot = 0;
    hipStream_t side_stream = nullptr;
    hipEvent_t ev_main = nullptr, ev_side[2] = {nullptr, nullptr};
    bool side_used[2] = {false, false};
    // this handle's column-split launches that ran beside [0] / were chained behind [1] one of its own on another stream (launch_coop_chained)
    mutable int64_t coop_chain_stats[2] = {0, 0};
    unsigned char* last_base = nullptr;   // workspace half of the last forward (fsnp_read_stage)
    hipEvent_t ev_done = nullptr;         // end of the last forward on its stream: a forward on another stream waits for it
    hipStream_t done_stream = nullptr;
    bool done_valid = false;
};


namespace fsnp {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// bits of the host-mapped error word (fsnp_handle::d_err[0])
constexpr unsigned kErrTimeout = 1u, kErrStaleWeights = 2u, kErrVerify = 4u;
// fsnp_weights.hip: fingerprint of the watched source tensors on stream s (no-op without a watch); the device function is shared with
// the forward's prologue kernel (forward_kernels.hip), which runs the same blocks beside its zeroing / row-descriptor blocks
int launch_weight_watch(fsnp_handle* h, hipStream_t s, bool baseline);
struct WatchSeg { const unsigned* p; unsigned n; unsigned long long first; };      // (device function: weight_watch.h)
constexpr int kWatchSeg = 8192;              // elements per segment of the watched tensors (8 uint4 loads per thread of a 256-thread block)
constexpr int kWatchBlocks = 512;            // blocks of one fingerprint pass (each walks its share of the segments)
void drop_weight_watch(fsnp_handle* h);
// decodes and clears the error word: 0 = clean, else the return code of the call that notices (5 time-out, 6 stale weights, 7 verify) + message
int take_device_errors(fsnp_handle* h, const char* where);
// fsnp_weights.hip
void build_specs(fsnp_handle* h);
// cross-stream ordering of a handle's shared buffers (fsnp_abi.hip)
int order_after_last_forward(fsnp_handle* h, hipStream_t s);
int mark_forward_done(fsnp_handle* h, hipStream_t s);
// fsnp_weights.hip: orders `s` behind a device pack of the weights (fsnp_commit_weights_on) that ran on ANOTHER stream - for the
// entry points that read the blob without going through order_after_last_forward (stream-session pushes, the stage calls
// fsnp_channel_attention / fsnp_fullband_model)
int order_after_weight_pack(fsnp_handle* h, hipStream_t s);
// clips of different lengths: 0 when lengths[0 .. batch) (host, frames per utterance) is acceptable for a forward of `frames` frames on
// this handle, else 2 with the error set (naming the utterance).  Nothing is launched.
int check_lengths(const fsnp_handle* h, const int32_t* lengths, int batch, int frames, const char* where);
// fsnp_abi.hip: workspace (grown stream-ordered on s), timing records, the planner's view of a handle and its calibration
int ensure_workspace(fsnp_handle* h, size_t bytes, hipStream_t s);
int drain_timing(fsnp_handle* h);
PlannerCtx pctx(const fsnp_handle* h);
int rows_per_utt(const fsnp_handle* h, int mode);
SbPlan plan_sb(const fsnp_handle* h, int num_rows, double gather_bytes = 0.0);     // gather_bytes: the furthest byte a launch reads
int chunk_workgroups(const fsnp_handle* h, const SbChunk& c);
int plan_first_deferred(const fsnp_handle* h, const SbPlan& plan);     // pipelined loop: first chunk on the side stream
int calibrate_costs(fsnp_handle* h, bool adopt = true, CostTable* measured = nullptr);
// the sub-band launches of chunks [first_chunk, last_chunk) on s (-1: to the end; after_first: recorded behind the range's first chunk),
// and the count of this handle's column-split launches that ran beside [0] / were chained behind [1] one of its own on another stream
void launch_sb_lstm(const fsnp_handle* h, const SbPlan& plan, const LstmArgs& a, float* hx, unsigned* bar, unsigned* abort_word,
                    hipStream_t s, hipEvent_t after_first = nullptr, int first_chunk = 0, int last_chunk = -1);
void take_coop_chain_stats(fsnp_handle* h, int64_t out[2], bool reset);
constexpr int kOwnCuLds = 160 * 1024 - 256;     // LDS a column-split launch claims to keep its CUs to itself (LstmArgs::coop_own_cu)
// the full-band LSTM launch of a FullSubNet forward (fsnp_debug_fullband_launch reports the kernel's number), and the side-by-side
// decision of the pipelined FullSubNet loop (fsnp_debug_pipeline_pairing)
enum class FbKernel { KSplitSeq = 0, Valu = 1, Generic = 2 };     // lstm_coop_seq, lstm_fbv, lstm_generic
struct FbShape { FbKernel kernel; int tiles, rows_per_tile, units; };
FbShape fb_shape(const fsnp_handle* h, int batch);
int pipeline_pairing(const PlannerCtx& c, bool defer_small, int F, int CH, int batch, const int fb_per_cu[3], bool fb_valu,
                     int32_t* out, int max_records);
// forward_kernels.hip: row descriptors of rows [row0, row0 + num_rows) on num_tiles tiles of rows_per_tile slots, for the forward's
// mask (F bins, mode, drop_band groups) or a dense [n][OC][T] output; the forward's prologue (one launch for up to kPrologueChunks
// chunks, else zero_region + build_rows + launch_weight_watch); per-utterance lengths and the zeroed mask tails past them
struct RowTiles { int num_rows, num_tiles, rows_per_tile, row0; };
struct RowLayout { int F, T, mode, batch_offset, global_batch, dense_out, groups, OC; };
inline RowLayout dense_rows(int T, int OC) { return {1, T, 0, 0, 1, 1, 2, OC}; }
void launch_build_rows(RowDesc* rows, const RowTiles& t, const RowLayout& l, hipStream_t s);
void launch_build_rows(const SbPlan& plan, RowDesc* rows, const RowLayout& l, hipStream_t s);     // every chunk of the plan
void launch_zero_region(void* p, size_t bytes, hipStream_t s);
constexpr int kPrologueChunks = 8;
void launch_prologue_kernel(const fsnp_handle* h, const SbPlan& plan, RowDesc* rows, const RowLayout& l, void* zero, size_t zero_bytes,
                            bool watch, hipStream_t s);
void launch_set_lengths(const int32_t* lengths, int B, int LA, int* lens, int* tpb, hipStream_t s);
void launch_zero_tails(float* out, const int* lens, int B, int rows_per_utt, int T, hipStream_t s);
// fsnp_verify.hip: fsnp_set_verify (verify_pass, on the forward's stream behind its launches) and fsnp_set_verify_sample
bool plan_has_exchange(const SbPlan& plan);
int verify_pass(fsnp_handle* h, const SbPlan& plan, const Dims& d, int mode, int batch_offset, int global_batch, const LstmArgs& a,
                const SubbandBuffers& sbuf, size_t out_elems, hipStream_t s);
bool plan_can_be_sampled(const fsnp_handle* h, const SbPlan& plan);
int verify_sample(fsnp_handle* h, const SbPlan& plan, const Dims& d, const LstmArgs& a, const SubbandBuffers& sbuf, hipStream_t st);
// fsnp_stft_abi.hip
// The geometry rules (include/fsnp_stft_geometry.h): n_fft = 2 (F - 1), periodic Hann of n_fft, n_fft / 8 <= hop <= n_fft / 2, hop % 4 == 0
// (frame row t of the forward DFT GEMM starts at float t * hop of the padded signal and is read as float4).  `half` = n_fft / 2 is the
// reflect padding and the distance from a frame's start to its centre; it is the hop only in the default geometry.
struct StftPlan {
    int n_fft, hop, half, F, N2, sp;    // sp = padded float stride of one internal spectrum row (multiple of 4)
    size_t o_fwd, o_inv, o_win, o_zero, total;   // float offsets inside d_stft
    int fwd_ld, inv_ld;                 // row strides of the two DFT matrices: n_fft and 2F padded to the GEMM's k-tile (16)
    int xl;                             // row stride of a wave session's gathered frames: n_fft padded to a float4
};
StftPlan stft_plan(const fsnp_handle* h);
// 0, or 2 with the error set: the rule `hop` breaks for a handle of F bins.  Host arithmetic only.
int check_hop_length(int F, int hop, const char* where);
int ensure_stft(fsnp_handle* h);
int ensure_io(fsnp_handle* h, size_t bytes, hipStream_t s);
// The io area of fsnp_enhance_wave for `batch` clips of up to max_samples samples: what the call lays out and what fsnp_reserve sizes.
// Byte offsets of the padded signal [batch][xs], the noisy and the enhanced spectra [batch][T][sp] (+ 256 bytes each), the mask
// [batch][2][F][T] and the inverse DFT's frames [batch][T][n_fft]; T = 1 + max_samples / hop.  stage_samples > 0 (fsnp_enhance_wave_rate:
// max_samples counts at the model's rate, stage_samples at the caller's): behind them fp32 rows [batch][stage_samples], the staging of
// FSNP_SAMPLE_S16_PEAK at the caller's rate
struct WaveIo {
    int T;
    long xs;
    size_t xp, noisy, enh, mask, fr, stage, total;
};
WaveIo wave_io(const StftPlan& p, int batch, int max_samples, int stage_samples = 0);
// The model between the two sample kernels of a waveform call, on the io area laid out by `io` (grown by the caller): the padded rows
// at io.xp, already written on the stream -> forward DFT, forward (frames: NULL, or each row's HOST frame count as check_lengths
// accepted it), flush in pipelined mode, cIRM, inverse DFT -> the frames [batch][io.T][n_fft] at io.fr, ready for launch_istft_ola
int enhance_padded(fsnp_handle* h, const StftPlan& p, const WaveIo& io, int batch, const int32_t* frames, void* hip_stream);
// fsnp_resample_abi.hip (include/fsnp_resample.h): 0, or 2 with the error set when the `count` pairs would take the handle past
// kResampleMaxPairs tables (nothing is enqueued); the device table of a pair on s, built and uploaded on first use (taps = nullptr for
// equal rates) - between order_after_last_forward and mark_forward_done, which order other streams behind the upload
int resample_room(const fsnp_handle* h, const char* where, const ResamplePlan* plans, int count);
int resample_table(fsnp_handle* h, const ResamplePlan& p, hipStream_t s, ResampleTable& t);
// 0, or 2 with the error set: the format and step rules of include/fsnp_pcm.h for one sample buffer (`what`: "input" / "output";
// peak_ok: FSNP_SAMPLE_S16_PEAK is a format this buffer may have)
int check_sample_format(const char* where, const char* what, int32_t format, int64_t step, bool peak_ok);
// fsnp_windowed_abi.hip: the handle's cross-fade table of overlap V, or NULL; and its device copy on s, built and uploaded on first use
// (between order_after_last_forward and mark_forward_done, by a caller that has checked that the handle has room for it)
const WindowFade* find_window_fade(const fsnp_handle* h, int V);
int window_fade_device(fsnp_handle* h, int V, hipStream_t s, const float*& g);
// fsnp_abi.hip: the fewest frames of a clip the model accepts (TSSE: its largest kernel - look_ahead; else 1) - what check_lengths and
// the equal-length forward call "too few frames"
int min_clip_frames(const fsnp_handle* h);
// ---- stream, wave and spectrum sessions (fsnp_stream_abi.hip, fsnp_wave_stream_abi.hip, fsnp_spec_stream_abi.hip) ----
// argument checks of their entry points: `where` names the entry point in every message; 0, or 2 with the error set
inline int check_slot(const char* where, int slot, int S) {
    if (slot < 0 || slot >= S) { set_error("%s: slot %d outside [0, %d)", where, slot, S); return 2; }
    return 0;
}
inline int check_slots(const char* where, const int32_t* slots, int32_t num, int S) {      // slots = NULL: every slot
    if (!slots) return 0;
    if (num < 0) { set_error("%s: num = %d", where, num); return 2; }
    for (int i = 0; i < num; ++i)
        if (const int rc = check_slot(where, slots[i], S)) return rc;
    return 0;
}
inline int read_counts(const char* where, const int32_t* counts, int S, int n, SlotCounts& c) {      // counts = NULL: n for every slot
    for (int b = 0; b < S; ++b) {
        const int v = counts ? counts[b] : n;
        if (v < 0 || v > n) { set_error("%s: slot %d: count %d outside [0, n = %d]", where, b, v, n); return 2; }
        c.v[b] = v;
    }
    return 0;
}
// what every call that enqueues a push asks last: committed weights, and no error left behind by an earlier call on the handle
inline int push_preamble(fsnp_handle* h, const char* where) {
    if (!h->committed) { set_error("%s: weights not committed (call fsnp_commit_weights)", where); return 2; }
    return take_device_errors(h, "an earlier call on this handle failed");
}
// One device array of per-slot records [S][bytes]: the mag record, the wave record, the look-ahead ring.  Zero bytes (a ring at
// look_ahead = 0) is an array without memory on which every call does nothing.  The caller is on the handle's device.
struct SlotRecords {
    unsigned char* base = nullptr;
    size_t bytes = 0;      // one slot
    int S = 0;
    unsigned char* slot(int b) const { return base + (size_t)b * bytes; }
    hipError_t create(size_t slot_bytes, int slots) {      // zeroed
        bytes = slot_bytes; S = slots;
        if (!bytes) return hipSuccess;
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&base), bytes * S);
        return e != hipSuccess ? e : hipMemset(base, 0, bytes * S);
    }
    void free() { if (base) (void)hipFree(base); base = nullptr; }      // (hipFree waits for the device: pushes still in flight finish first)
    int reset(const int32_t* slots, int32_t num, hipStream_t s) {      // stream-ordered zeroing of checked slots (NULL: all)
        if (!bytes) return 0;
        if (!slots) { FSNP_HIP_CHECK(hipMemsetAsync(base, 0, bytes * S, s)); return 0; }
        for (int i = 0; i < num; ++i) FSNP_HIP_CHECK(hipMemsetAsync(slot(slots[i]), 0, bytes, s));
        return 0;
    }
    int get(int b, void* blob, size_t at, hipStream_t s) const {      // slot b -> blob + at (device memory)
        if (bytes) FSNP_HIP_CHECK(hipMemcpyAsync(static_cast<unsigned char*>(blob) + at, slot(b), bytes, hipMemcpyDeviceToDevice, s));
        return 0;
    }
    int set(int b, const void* blob, size_t at, hipStream_t s) {      // blob + at -> slot b
        if (bytes) FSNP_HIP_CHECK(hipMemcpyAsync(slot(b), static_cast<const unsigned char*>(blob) + at, bytes, hipMemcpyDeviceToDevice, s));
        return 0;
    }
};
// fsnp_stream_abi.hip: one mag push behind its checks, and session creation behind fsnp_stream_create (live = 0) and
// fsnp_stream_create_live (live = 1: pushes run on lstm_step.hip, max_chunk <= kLiveMaxChunk)
int stream_push_body(fsnp_stream* st, const float* mag, const int64_t strides[3], const SlotCounts& c, float* out, int n, hipStream_t s);
constexpr int kLiveMaxChunk = 16;
int stream_create(fsnp_handle* h, int32_t slots, int32_t max_chunk, int live, const char* where, fsnp_stream** out);
// one ring push behind its checks - what a spectrum session's push is, and what a wave session runs between
// its two transforms.  |spec| -> mag push of `mag` -> cIRM of every step times its waiting spectrum -> the ring advanced.
//   ring        the look-ahead ring of slot 0 ([look_ahead][F] complex64), ring_stride bytes between slots
//   mag, mask   scratch [S][n][FP] and [S][2][F][n]
//   spec, out   complex64 with strides (slot, f, frame) in complex elements; out column j = the enhanced frame of step j, exactly 0
//               where the step has no frame or the slot no such step
//   write_idle  a call in which no slot steps still writes out (all zeros: a spectrum push owes them to its caller; a wave call, which
//               then transforms nothing back, does not and launches nothing for them)
//   spectra     per slot, the new spectra in spec; steps = the mag push's counts: the same, but 1 and 1 + look_ahead for a wave slot
//               that is finished (its ring then takes the clip's last spectrum, and the reset that ends finish clears it)
struct SpecRing { unsigned char* ring; size_t ring_stride; int look_ahead; };
int spec_push_body(fsnp_stream* mag_session, const SpecRing& ring, float* mag, float* mask, const float* spec, const int64_t strides[3],
                   const SlotCounts& spectra, const SlotCounts& steps, float* out, const int64_t out_strides[3], bool write_idle, int n,
                   hipStream_t s);
// fsnp_wave_stream_abi.hip: what the public push, finish and set_state of a wave session run behind their NULL and format checks
// (`where` names the entry point in every message) - and what a rate session (fsnp_wave_rate_stream_abi.hip) drives its inner session
// through, on workspace rows.  wave_set_state: known = NULL reads the loaded sample count back (one wait); a caller that knows it passes it.
int wave_push(fsnp_wave_stream* w, const char* where, const PcmIn& wav, const int32_t* counts, const PcmOut& out, int32_t n, void* hip_stream);
int wave_finish(fsnp_wave_stream* w, const char* where, const int32_t* slots, int32_t num, const PcmOut& out, void* hip_stream);
int wave_set_state(fsnp_wave_stream* w, int32_t slot, const void* dev_src, const long long* known, void* hip_stream);

}  // namespace fsnp

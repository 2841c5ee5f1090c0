// fsnp_weights.hip - strict weight loading of the C ABI: the parameter tree a handle expects (reference names / shapes,
// base_inferencer.py:100-107 loads with strict=True) and its packing into the device layouts of the kernels (MFMA fragment order,
// transposed / zero-padded GEMM operands, GroupNorm folded into the sconv weights, summed biases) - on the host, or on the device
// from tensors the caller handed over there (include/fsnp_device_weights.h; the layouts: weight_layouts.h, the kernels: weight_pack.hip).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fsnp_handle.h"
#include "weight_layouts.h"
#include "weight_watch.h"

namespace fsnp {

static const int kDilations[8] = {1, 2, 5, 9, 1, 2, 5, 9};  // sequence_model.py:48-57
static const char* kAtt[3] = {"channel_attention", "channel_attention_real", "channel_attention_imag"};
static const char* kFb[3] = {"fb_model", "fb_model_real", "fb_model_imag"};
static const char* kConvNames[3] = {"smallConv1d", "middleConv1d", "largeConv1d"};

static void list_specs(fsnp_handle* h) {
    auto add = [&](const std::string& n, int64_t numel) { h->specs.push_back({n, numel}); };
    const int F = h->F, CH = h->CH, H = h->H, Fr = h->Fr;
    const int att = h->cfg.attention;
    const bool fsn = h->model == FSNP_MODEL_FULLSUBNET;
    if (fsn) {   // fullsubnet.py:39-47: SequenceModel(257 -> 512 x 2 -> 257), same key layout as nn.LSTM
        const std::string f = "fb_model.sequence_model.";
        const int64_t G = h->NG;
        add(f + "weight_ih_l0", G * CH * F);
        add(f + "weight_hh_l0", G * CH * CH);
        add(f + "bias_ih_l0", G * CH);
        add(f + "bias_hh_l0", G * CH);
        add(f + "weight_ih_l1", G * CH * CH);
        add(f + "weight_hh_l1", G * CH * CH);
        add(f + "bias_ih_l1", G * CH);
        add(f + "bias_hh_l1", G * CH);
        add("fb_model.fc_output_layer.weight", (int64_t)F * CH);
        add("fb_model.fc_output_layer.bias", F);
    }
    for (int a = 0; a < 3 && !fsn; ++a) {
        const std::string p = kAtt[a];
        if (att == FSNP_ATT_TSSE) {
            for (int c = 0; c < 3; ++c) {
                add(p + "." + kConvNames[c] + ".0.weight", (int64_t)F * h->cfg.kersize[c]);
                add(p + "." + kConvNames[c] + ".0.bias", F);
            }
            add(p + ".feature_concate_fc.weight", 3);
            add(p + ".feature_concate_fc.bias", 1);
        }
        if (att == FSNP_ATT_ECA) {
            add(p + ".conv.weight", 3);
        } else {
            add(p + ".fc1.weight", (int64_t)Fr * F);
            add(p + ".fc1.bias", Fr);
            add(p + ".fc2.weight", (int64_t)F * Fr);
            add(p + ".fc2.bias", F);
        }
    }
    for (int b = 0; b < 3 && !fsn; ++b) {
        for (int i = 0; i < h->NB; ++i) {
            const std::string p = std::string(kFb[b]) + ".sequence_model." + std::to_string(i);
            add(p + ".conv1x1.weight", (int64_t)CH * F);
            add(p + ".conv1x1.bias", CH);
            add(p + ".prelu1.weight", 1);
            add(p + ".norm1.weight", CH);
            add(p + ".norm1.bias", CH);
            add(p + ".depthwise_conv.weight", (int64_t)CH * 3);
            add(p + ".depthwise_conv.bias", CH);
            add(p + ".prelu2.weight", 1);
            add(p + ".norm2.weight", CH);
            add(p + ".norm2.bias", CH);
            add(p + ".sconv.weight", (int64_t)F * CH);
            add(p + ".sconv.bias", F);
        }
        add(std::string(kFb[b]) + ".fc_output_layer.weight", (int64_t)F * F);
        add(std::string(kFb[b]) + ".fc_output_layer.bias", F);
    }
    if (h->sb_tcn) {
        for (int i = 0; i < 8; ++i) {
            const std::string p = "sb_model.sequence_model." + std::to_string(i);
            add(p + ".conv1x1.weight", (int64_t)CH * h->NIN);
            add(p + ".conv1x1.bias", CH);
            add(p + ".prelu1.weight", 1);
            add(p + ".norm1.weight", CH);
            add(p + ".norm1.bias", CH);
            add(p + ".depthwise_conv.weight", (int64_t)CH * 3);
            add(p + ".depthwise_conv.bias", CH);
            add(p + ".prelu2.weight", 1);
            add(p + ".norm2.weight", CH);
            add(p + ".norm2.bias", CH);
            add(p + ".sconv.weight", (int64_t)h->NIN * CH);
            add(p + ".sconv.bias", h->NIN);
        }
        add("sb_model.fc_output_layer.weight", (int64_t)h->cfg.output_size * h->NIN);
        add("sb_model.fc_output_layer.bias", h->cfg.output_size);
        return;
    }
    const std::string s = "sb_model.sequence_model.";
    const int64_t G = h->NG;
    add(s + "weight_ih_l0", G * H * h->NIN);
    add(s + "weight_hh_l0", G * H * H);
    add(s + "bias_ih_l0", G * H);
    add(s + "bias_hh_l0", G * H);
    add(s + "weight_ih_l1", G * H * H);
    add(s + "weight_hh_l1", G * H * H);
    add(s + "bias_ih_l1", G * H);
    add(s + "bias_hh_l1", G * H);
    add("sb_model.fc_output_layer.weight", (int64_t)h->cfg.output_size * H);
    add("sb_model.fc_output_layer.bias", h->cfg.output_size);
}

void build_specs(fsnp_handle* h) {
    list_specs(h);
    long long at = 0;
    for (size_t i = 0; i < h->specs.size(); ++i) {
        h->spec_off.push_back(at);
        h->spec_index[h->specs[i].name] = (int)i;
        at += h->specs[i].numel;
    }
    h->arena_floats = at;
    h->spec_src.assign(h->specs.size(), 0);
    h->host_arena.assign((size_t)at, 0.0f);
}

// ---- fsnp_watch_weights: a 64-bit fingerprint of the caller's source tensors, taken on the device in front of every forward.
// sum over all elements of bits(x_i) * (2 i + 1) mod 2^64 (i = position in the concatenation): any single changed element changes
// it, the sum is order-independent (integer adds), so blocks accumulate with one atomic each and the LAST block to finish compares.
__global__ __launch_bounds__(256) void weight_watch_kernel(const WatchSeg* __restrict__ segs, int nseg, unsigned long long* acc,
                                                           int baseline, unsigned* err_host) {
    weight_watch_block(segs, nseg, acc, baseline, err_host, (int)blockIdx.x, (int)gridDim.x);
}
int launch_weight_watch(fsnp_handle* h, hipStream_t s, bool baseline) {
    if (h->watch_nseg <= 0) return 0;
    const int grid = h->watch_nseg < kWatchBlocks ? h->watch_nseg : kWatchBlocks;
    hipLaunchKernelGGL(weight_watch_kernel, dim3(grid), dim3(256), 0, s, static_cast<const WatchSeg*>(h->watch_segs), h->watch_nseg,
                       h->watch_acc, baseline ? 1 : 0, h->d_err);
    FSNP_HIP_CHECK(hipGetLastError());
    return 0;
}
void drop_weight_watch(fsnp_handle* h) {
    if (h->watch_segs) (void)hipFree(h->watch_segs);
    if (h->watch_acc) (void)hipFree(h->watch_acc);
    h->watch_segs = nullptr; h->watch_acc = nullptr; h->watch_nseg = 0;
}

}  // namespace fsnp

extern "C" {

int fsnp_watch_weights(fsnp_handle* h, const void* const* dev_ptrs, const int64_t* numels, int32_t n, int32_t every, void* hip_stream) {
    if (!h || n < 0 || (n > 0 && (!dev_ptrs || !numels)) || every < 1) { set_error("fsnp_watch_weights: bad argument"); return 1; }
    if (!h->committed) { set_error("fsnp_watch_weights: commit the weights first (the baseline fingerprint belongs to the packed set)"); return 2; }
    FSNP_ON_DEVICE(h);
    FSNP_HIP_CHECK(hipDeviceSynchronize());           // (an earlier watch kernel may still read the old table)
    drop_weight_watch(h);
    h->watch_every = every; h->watch_calls = 0;
    if (n == 0) return 0;
    std::vector<WatchSeg> segs;
    unsigned long long first = 0;
    constexpr int64_t kSeg = kWatchSeg;               // elements per segment (32 KB): ~1400 segments for the default model
    for (int i = 0; i < n; ++i) {
        if (!dev_ptrs[i] || numels[i] < 0) { set_error("fsnp_watch_weights: tensor %d is null / negative", i); return 1; }
        for (int64_t o = 0; o < numels[i]; o += kSeg) {
            const int64_t c = numels[i] - o < kSeg ? numels[i] - o : kSeg;
            segs.push_back(WatchSeg{static_cast<const unsigned*>(dev_ptrs[i]) + o, (unsigned)c, first + (unsigned long long)o});
        }
        first += (unsigned long long)numels[i];
    }
    if (segs.empty()) return 0;
    FSNP_HIP_CHECK(hipMalloc(&h->watch_segs, segs.size() * sizeof(WatchSeg)));
    FSNP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&h->watch_acc), (8 + kWatchBlocks) * 8));     // {-, tickets, baseline, -, ...; a partial sum per block}
    FSNP_HIP_CHECK(hipMemcpy(h->watch_segs, segs.data(), segs.size() * sizeof(WatchSeg), hipMemcpyHostToDevice));
    // (on the CALLER's stream, like the baseline kernel behind it: a null-stream hipMemset of device memory returns before it has run
    // and does not order with a non-blocking stream - on torch side streams it zeroed the tickets / the baseline under the running
    // baseline kernel now and then: a false "stale weights" flag, profiles/r05_pytest_gpu_runA.log)
    FSNP_HIP_CHECK(hipMemsetAsync(h->watch_acc, 0, (8 + kWatchBlocks) * 8, static_cast<hipStream_t>(hip_stream)));
    h->watch_nseg = (int)segs.size();
    if (const int rc = launch_weight_watch(h, static_cast<hipStream_t>(hip_stream), true)) return rc;
    // the baseline belongs to the handle's shared state like a forward's workspace: a later forward on ANOTHER (non-blocking) stream
    // must not start its watch blocks (same ticket word, same baseline slot) before this kernel has finished (a spurious
    // code 6 when the watch was registered on the default stream and the forward ran on a torch side stream)
    return mark_forward_done(h, static_cast<hipStream_t>(hip_stream));
}

int fsnp_num_weights(const fsnp_handle* h) { return h ? (int)h->specs.size() : 0; }

int fsnp_weight_info(const fsnp_handle* h, int index, const char** name, int64_t* numel) {
    if (!h || index < 0 || index >= (int)h->specs.size()) { set_error("fsnp_weight_info: bad index"); return 1; }
    if (name) *name = h->specs[index].name.c_str();
    if (numel) *numel = h->specs[index].numel;
    return 0;
}

}  // extern "C"

namespace fsnp {

int order_after_weight_pack(fsnp_handle* h, hipStream_t s) {
    if (h->packed_valid && h->packed_stream != s) FSNP_HIP_CHECK(hipStreamWaitEvent(s, h->ev_packed, 0));
    return 0;
}

// name / size checks shared by the two setters: the spec's index, or -1 with the error set (code 2)
static int find_spec(fsnp_handle* h, const char* name, int64_t numel) {
    const auto it = h->spec_index.find(name);
    if (it == h->spec_index.end()) { set_error("unexpected key in state_dict: %s", name); return -1; }
    const WeightSpec& s = h->specs[it->second];
    if (s.numel != numel) {
        set_error("size mismatch for %s: expected %lld elements, got %lld", name, (long long)s.numel, (long long)numel);
        return -1;
    }
    return it->second;
}

// the device-given tensors the host arena does not hold yet -> host arena (a host-path commit of device-given weights)
static int download_device_given(fsnp_handle* h, int64_t* bytes) {
    *bytes = 0;
    bool any = false;
    for (unsigned char v : h->spec_src) any = any || v == 2;
    if (!any) return 0;
    FSNP_ON_DEVICE(h);
    FSNP_HIP_CHECK(hipDeviceSynchronize());           // (the arena copies run on the caller's streams)
    for (size_t i = 0; i < h->specs.size(); ++i) {
        if (h->spec_src[i] != 2) continue;
        const size_t nb = (size_t)h->specs[i].numel * sizeof(float);
        FSNP_HIP_CHECK(hipMemcpy(h->host_arena.data() + h->spec_off[i], h->d_arena + h->spec_off[i], nb, hipMemcpyDeviceToHost));
        h->spec_src[i] = 3;
        *bytes += (int64_t)nb;
    }
    return 0;
}

// Lays the blob out (the same walk for both paths: offsets and images depend on the configuration only), packs it - on the host from
// the host arena and uploads it, or on the device from the device arena on stream s - and binds the kernels' pointers into it.
static int commit_impl(fsnp_handle* h, bool on_device, hipStream_t s) {
    const int F = h->F, CH = h->CH, H = h->H, NB = h->NB, Fr = h->Fr;
    std::vector<PackJob> jobs;
    size_t total = 0;
    auto alloc = [&](size_t n) { const size_t o = total; total = align_up(o + n, 64); return o; };
    auto off = [&](const std::string& n) { return h->spec_off[h->spec_index.at(n)]; };
    auto numel = [&](const std::string& n) { return h->specs[h->spec_index.at(n)].numel; };
    auto emit = [&](PackJob J, size_t o, size_t n) { J.out = (long long)o; J.n = (long long)n; if (n) jobs.push_back(J); };
    auto put = [&](const std::string& n) {           // a plain copy
        const int c = (int)numel(n);
        const size_t o = alloc(c);
        PackJob J = make_job(PK_PADMAT, 1, c, 1, c);
        J.s[0] = off(n);
        emit(J, o, c);
        return o;
    };
    auto transposed = [&](const std::string& n, int R, int C) {      // [R][C] -> [C][R]
        const size_t o = alloc((size_t)R * C);
        PackJob J = make_job(PK_TRANSPOSE, R, C);
        J.s[0] = off(n);
        emit(J, o, (size_t)R * C);
        return o;
    };

    // ---- frontend (TSSE) : reference layouts are already what the kernels want
    size_t o_conv_w[3][3] = {}, o_conv_b[3][3] = {}, o_cat_w[3] = {}, o_cat_b[3] = {}, o_fc1w[3] = {}, o_fc1b[3] = {},
           o_fc2w[3] = {}, o_fc2b[3] = {};
    const int att = h->cfg.attention;
    const bool fsn = h->model == FSNP_MODEL_FULLSUBNET;
    const int nbr_w = fsn ? 0 : 3;          // the original FullSubNet has neither attention nor TCN branches
    for (int a = 0; a < nbr_w; ++a) {
        const std::string p = kAtt[a];
        if (att == FSNP_ATT_TSSE) {
            for (int c = 0; c < 3; ++c) {
                o_conv_w[a][c] = put(p + "." + kConvNames[c] + ".0.weight");
                o_conv_b[a][c] = put(p + "." + kConvNames[c] + ".0.bias");
            }
            o_cat_w[a] = put(p + ".feature_concate_fc.weight");
            o_cat_b[a] = put(p + ".feature_concate_fc.bias");
        }
        if (att == FSNP_ATT_ECA) {
            o_cat_w[a] = put(p + ".conv.weight");            // the 3 taps of Conv1d(1,1,3) over the channel axis
            continue;
        }
        o_fc1w[a] = transposed(p + ".fc1.weight", Fr, F);    // transposed copies: fc1 [Fr][F] -> [F][Fr], fc2 [F][Fr] -> [Fr][F]
        o_fc2w[a] = transposed(p + ".fc2.weight", F, Fr);
        o_fc1b[a] = put(p + ".fc1.bias");
        o_fc2b[a] = put(p + ".fc2.bias");
    }
    // ---- TCN stacks (SequenceModel(sequence_model="TCN"), sequence_model.py:47-58,80-81): zero-padded row-major
    // [N pad 384][K pad 16] GEMM operands, [model][block] major.  `cin` channels in / out of every TCNBlock, `fc_out` rows of
    // the final Linear(cin, fc_out).  Used for the three full-band models and for a sub-band TCN.
    struct TcnOff { size_t w1, b1, a1, g1w, g1b, dw, db, a2, g2w, g2b, w2, b2, w2g, c1, c2, wf, bf; int NB, N1P, K1P, N2P, K2P; };
    bool regular = true;
    auto pack_tcn = [&](const std::vector<std::string>& models, int nb, int cin, int fc_out) {
        TcnOff t{};
        const size_t nm = models.size() ? models.size() : 1;
        t.NB = nb; t.N1P = (int)align_up(CH, 384); t.K1P = (int)align_up(cin, 16); t.N2P = (int)align_up(cin, 384); t.K2P = (int)align_up(CH, 16);
        const int nimg = models.empty() ? 0 : (int)(nm * nb), nfc = models.empty() ? 0 : (int)nm;
        // one image over all blocks of all models: block (b, i) of tensor `leaf` lies b * stride_out + i * stride_in floats behind
        // block (0, 0) in the arena, because every block (and every model) holds the same tensors in the same order
        auto blk = [&](size_t b, int i, const char* leaf) { return off(models[b] + ".sequence_model." + std::to_string(i) + leaf); };
        auto fc = [&](size_t b, const char* leaf) { return off(models[b] + ".fc_output_layer" + leaf); };
        auto image = [&](PackJob J, size_t size, std::initializer_list<const char*> leaves, bool per_block) {
            const size_t o = alloc(size);
            J.nsub = per_block ? nimg : nfc;
            J.nb = per_block ? nb : 1;
            if (J.nsub > 0) {
                int k = 0;
                for (const char* leaf : leaves) {
                    J.s[k] = per_block ? blk(0, 0, leaf) : fc(0, leaf);
                    if (per_block) {
                        J.stride_in = nb > 1 ? blk(0, 1, leaf) - J.s[k] : 0;
                        J.stride_out = nm > 1 ? blk(1, 0, leaf) - J.s[k] : 0;
                        for (size_t b = 0; b < nm; ++b)
                            for (int i = 0; i < nb; ++i) regular = regular && blk(b, i, leaf) == J.s[k] + (long long)b * J.stride_out + i * J.stride_in;
                    } else {
                        J.stride_out = nm > 1 ? fc(1, leaf) - J.s[k] : 0;
                        for (size_t b = 0; b < nm; ++b) regular = regular && fc(b, leaf) == J.s[k] + (long long)b * J.stride_out;
                    }
                    ++k;
                }
            }
            emit(J, o, size);
            return o;
        };
        auto vec = [&](int len, int padded) { return make_job(PK_PADMAT, 1, len, 1, padded); };
        t.w1 = image(make_job(PK_PADMAT, CH, cin, t.N1P, t.K1P), nm * nb * t.N1P * t.K1P, {".conv1x1.weight"}, true);       // [CH][cin][1]
        t.b1 = image(vec(CH, t.N1P), nm * nb * t.N1P, {".conv1x1.bias"}, true);
        t.a1 = image(vec(1, 1), nm * nb + 1, {".prelu1.weight"}, true);
        t.g1w = image(vec(CH, CH), nm * nb * CH, {".norm1.weight"}, true);
        t.g1b = image(vec(CH, CH), nm * nb * CH, {".norm1.bias"}, true);
        t.dw = image(make_job(PK_TRANSPOSE, CH, 3), nm * nb * 3 * CH, {".depthwise_conv.weight"}, true);                     // [CH][1][3] -> tap major
        t.db = image(vec(CH, CH), nm * nb * CH, {".depthwise_conv.bias"}, true);
        t.a2 = image(vec(1, 1), nm * nb + 1, {".prelu2.weight"}, true);
        t.g2w = image(vec(CH, CH), nm * nb * CH, {".norm2.weight"}, true);
        t.g2b = image(vec(CH, CH), nm * nb * CH, {".norm2.bias"}, true);
        t.w2 = image(make_job(PK_PADMAT, cin, CH, t.N2P, t.K2P), nm * nb * t.N2P * t.K2P, {".sconv.weight"}, true);         // [cin][CH][1]
        t.b2 = image(vec(cin, t.N2P), nm * nb * t.N2P, {".sconv.bias"}, true);
        // GroupNorm 2 folded into the sconv GEMM (tcn.hip tcn_gemm_dma_kernel): weights times gamma, and the two per-output
        // constants (weight_layouts.h: PK_FOLDW, fold_row)
        t.w2g = image(make_job(PK_FOLDW, cin, CH, t.N2P, t.K2P), nm * nb * t.N2P * t.K2P, {".sconv.weight", ".norm2.weight"}, true);
        t.c1 = image(make_job(PK_FOLDC, cin, CH, t.N2P, 0), nm * nb * t.N2P, {".sconv.weight", ".norm2.weight", ".norm2.bias", ".sconv.bias"}, true);
        t.c2 = image(make_job(PK_FOLDC, cin, CH, t.N2P, 1), nm * nb * t.N2P, {".sconv.weight", ".norm2.weight", ".norm2.bias", ".sconv.bias"}, true);
        t.wf = image(make_job(PK_PADMAT, fc_out, cin, t.N2P, t.K1P), nm * t.N2P * t.K1P, {".weight"}, false);   // [fc_out][cin]: top rows of a zero-padded [N2P][K1P]
        t.bf = image(vec(fc_out, t.N2P), nm * t.N2P, {".bias"}, false);
        return t;
    };
    auto bind_tcn = [&](TcnWeights& t, const TcnOff& o, const float* d) {
        t.w1 = d + o.w1; t.b1 = d + o.b1; t.a1 = d + o.a1; t.g1w = d + o.g1w; t.g1b = d + o.g1b;
        t.dw = d + o.dw; t.db = d + o.db; t.a2 = d + o.a2; t.g2w = d + o.g2w; t.g2b = d + o.g2b;
        t.w2 = d + o.w2; t.b2 = d + o.b2; t.wf = d + o.wf; t.bf = d + o.bf;
        t.w2g = d + o.w2g; t.c1 = d + o.c1; t.c2 = d + o.c2;
        t.num_cus = h->num_cus; t.NB = o.NB; t.N1P = o.N1P; t.K1P = o.K1P; t.N2P = o.N2P; t.K2P = o.K2P;
        for (int i = 0; i < o.NB; ++i) t.dilation[i] = kDilations[i];
        const char* de = getenv("FSNP_GEMM_DMA");          // 0 = the general GEMM kernel everywhere (tuning / A-B)
        t.gemm_dma = de && de[0] == '0' ? 0 : 1;
    };
    std::vector<std::string> fb_models;
    for (int b = 0; b < nbr_w; ++b) fb_models.push_back(kFb[b]);
    const TcnOff fb_off = pack_tcn(fb_models, NB, F, F);
    const TcnOff sb_off = h->sb_tcn ? pack_tcn({"sb_model"}, 8, h->NIN, h->cfg.output_size) : TcnOff{};
    if (!regular) { set_error("fsnp_commit_weights: the TCN blocks are not evenly spaced in the parameter list"); return 3; }
    // ---- recurrent models: MFMA B-fragment order + summed biases, cut from the FOUR-slot view of the reference's matrices
    // (weight_layouts.h: rnn_w, rnn_bias)
    auto rnn = [&](int kind, const std::string& pre, int Hh, int nin, int kx, int P) {
        PackJob J = make_job(kind, Hh, nin, kx, P, h->gru);
        static const char* leaves[8] = {"weight_ih_l0", "weight_hh_l0", "weight_ih_l1", "weight_hh_l1", "bias_ih_l0", "bias_hh_l0", "bias_ih_l1", "bias_hh_l1"};
        for (int i = 0; i < 8; ++i) J.s[i] = off(pre + leaves[i]);
        const size_t o = alloc((size_t)J.n);
        emit(J, o, (size_t)J.n);
        return o;
    };
    const std::string sbp = "sb_model.sequence_model.";
    auto sb = [&](int kind, int P = 0) { return rnn(kind, sbp, H, h->NIN, h->KX, P); };
    const bool tuned = !h->sb_tcn && !h->generic_sb;            // MFMA kernels exist for this cell / hidden size / input width
    size_t o_wgen = 0;
    if (h->generic_sb) o_wgen = sb(PK_GENERIC);                 // runtime-sized kernel: transposed [layer][k][4H]
    size_t o_wpack = 0, o_wpack12 = 0, o_wpack_bf[2] = {0, 0};
    if (!h->gru && tuned && (H == 384 || H == 256)) {      // the row-tile kernel (and its bf16 variant) exists for LSTM only
        o_wpack = sb(PK_ROWTILE, 4);
        if (H == 384) o_wpack12 = sb(PK_ROWTILE, 12);
        // the bf16-ih variant is built for the default input width only (and needs a spare input column: its layer-0 bias rides there)
        for (int i = 0; i < 2 && h->KX == 40 && H == 384 && h->NIN < h->KX; ++i) o_wpack_bf[i] = sb(PK_ROWTILE_BF, i == 0 ? 4 : 12);
    }
    size_t o_wpack16 = 0, o_wpack16_bf = 0;
    bool have16_bf = false;
    if (h->planner.lstm16_ok) {
        o_wpack16 = sb(PK_HALF);
        if (h->KX == 40 && H == 384) {                 // bf16-ih stream of the half-tile kernel (configs[4], round 4)
            o_wpack16_bf = sb(PK_HALF_BF);
            have16_bf = true;
        }
    }
    size_t o_wpack_gru = 0;
    if (h->gru && tuned && H == 384) o_wpack_gru = sb(PK_GRU, 4);
    size_t o_wpack_coop[4] = {0, 0, 0, 0};
    for (int ui = 0; ui < 4 && tuned; ++ui) o_wpack_coop[ui] = sb(PK_KSPLIT, 8 << ui);
    size_t o_wpack_hp = 0, o_wpack_hpw = 0;
    if (h->planner.hp_ok) {
        o_wpack_hp = sb(PK_HP);
        o_wpack_hpw = sb(PK_HPW);
    }
    size_t o_wpack_coopw = 0;
    if (h->planner.coopw_ok) o_wpack_coopw = sb(PK_COOPW);
    const size_t o_wpack_coopn = tuned ? sb(PK_COOPN) : alloc(0);
    // ---- original FullSubNet: full-band recurrent model (cooperative kernel, KX = 264) + Linear(CH, F) as a GEMM operand
    constexpr int KXF = 264;
    size_t o_fbpack[3] = {0, 0, 0}, o_fbbias = 0, o_fsn_wf = 0, o_fsn_bf = 0, o_fbgen = 0, o_fbv = 0;
    bool have_fbv = false;
    const int fsn_kp = (int)align_up(CH, 16), fsn_np = (int)align_up(F, 384);
    if (fsn) {
        const std::string fbp = "fb_model.sequence_model.";
        // (LSTM: also what a stream session's full-band pushes run on - launch_lstm_generic_stream)
        if (h->generic_fb || !h->gru) o_fbgen = rnn(PK_GENERIC, fbp, CH, F, 0, 0);
        for (int ui = 0; ui < 3 && !h->generic_fb; ++ui) o_fbpack[ui] = rnn(PK_KSPLIT, fbp, CH, F, KXF, 8 << ui);
        if (!h->generic_fb && !h->gru && CH == 512 && F <= 288) {          // small batches: matrix-vector products on the VALU (lstm_fbv.hip)
            o_fbv = rnn(PK_FBV, fbp, CH, F, 0, 0);
            have_fbv = true;
        }
        o_fbbias = rnn(PK_BIAS, fbp, CH, F, 0, 0);
        o_fsn_wf = alloc((size_t)fsn_np * fsn_kp);
        PackJob J = make_job(PK_PADMAT, F, CH, fsn_np, fsn_kp);         // [F][CH]
        J.s[0] = off("fb_model.fc_output_layer.weight");
        emit(J, o_fsn_wf, (size_t)fsn_np * fsn_kp);
        o_fsn_bf = alloc(fsn_np);
        PackJob Jb = make_job(PK_PADMAT, 1, F, 1, fsn_np);
        Jb.s[0] = off("fb_model.fc_output_layer.bias");
        emit(Jb, o_fsn_bf, fsn_np);
    }
    const size_t o_lbias = h->sb_tcn ? alloc(0) : sb(PK_BIAS);
    const size_t o_wfc = h->sb_tcn ? 0 : put("sb_model.fc_output_layer.weight");
    const size_t o_bfc = h->sb_tcn ? 0 : put("sb_model.fc_output_layer.bias");
    // ---- unfold multiplicities w_r, by brute force over (f, j): they depend on the configuration only, so
    // both paths compute them on the host (once) and upload them
    const size_t o_refl = alloc(F), o_reflfb = alloc(F);
    const size_t refl_floats = total - o_refl;
    if (h->refl_host.size() != refl_floats) {
        h->refl_host.assign(refl_floats, 0.0f);
        for (int f = 0; f < F; ++f) {
            for (int j = 0; j < h->NSB; ++j) h->refl_host[reflect_index(f - h->cfg.sb_num_neighbors + j, F)] += 1.0f;
            for (int j = 0; j < 2 * h->cfg.fb_num_neighbors + 1; ++j) h->refl_host[o_reflfb - o_refl + reflect_index(f - h->cfg.fb_num_neighbors + j, F)] += 1.0f;
        }
    }

    FSNP_ON_DEVICE(h);
    int64_t stats[4] = {on_device ? 1 : 0, 0, 0, 0};
    if (!on_device) {
        std::vector<float> blob(total, 0.0f);
        for (const PackJob& J : jobs) pack_image_host(J, h->host_arena.data(), blob.data() + J.out, (long long)align_up((size_t)J.n, 64));
        std::copy(h->refl_host.begin(), h->refl_host.end(), blob.begin() + o_refl);
        if (h->d_weights) { FSNP_HIP_CHECK(hipDeviceSynchronize()); FSNP_HIP_CHECK(hipFree(h->d_weights)); h->d_weights = nullptr; }
        FSNP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&h->d_weights), blob.size() * sizeof(float)));
        FSNP_HIP_CHECK(hipMemcpy(h->d_weights, blob.data(), blob.size() * sizeof(float), hipMemcpyHostToDevice));
        h->blob_floats = total;
        h->packed_valid = false;
        stats[1] = (int64_t)(blob.size() * sizeof(float));
    } else {
        // Behind everything already enqueued for the handle: forwards on other streams (their event), a pipelined deferred chunk
        // (the flush).  What these two do not see - a stream-session push or a sampled verification pass on a stream of its own -
        // is covered by a device-wide wait in front of the overwrite, as on the host path; the first pack writes a fresh
        // allocation and waits for nothing.
        if (order_after_last_forward(h, s)) return 4;
        if (h->pipeline && fsnp_flush(h, s)) return 4;
        // the arena copies ran on another stream: wait for the event recorded behind the last of them
        if (h->arena_valid && h->arena_stream != s) FSNP_HIP_CHECK(hipStreamWaitEvent(s, h->ev_arena, 0));
        if (h->d_weights && h->blob_floats != total) { FSNP_HIP_CHECK(hipDeviceSynchronize()); FSNP_HIP_CHECK(hipFree(h->d_weights)); h->d_weights = nullptr; }
        if (h->d_weights) FSNP_HIP_CHECK(hipDeviceSynchronize());
        else FSNP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&h->d_weights), total * sizeof(float)));
        h->blob_floats = total;
        h->committed = false;                                 // (a launch that fails leaves a partly written blob behind)
        for (const PackJob& J : jobs) {
            if (const int rc = launch_pack_image(J, h->d_arena, h->arena_floats, h->d_weights, (long long)align_up((size_t)J.n, 64), s)) return rc;
            ++stats[3];
        }
        FSNP_HIP_CHECK(hipMemcpyAsync(h->d_weights + o_refl, h->refl_host.data(), refl_floats * sizeof(float), hipMemcpyHostToDevice, s));
        stats[1] = (int64_t)(refl_floats * sizeof(float));
        if (!h->ev_packed) FSNP_HIP_CHECK(hipEventCreateWithFlags(&h->ev_packed, hipEventDisableTiming));
        FSNP_HIP_CHECK(hipEventRecord(h->ev_packed, s));
        h->packed_stream = s; h->packed_valid = true;
        if (mark_forward_done(h, s)) return 4;                // forwards on other streams wait for the pack
    }
    for (int i = 0; i < 4; ++i) if (i != 2) h->commit_stats[i] = stats[i];
    const float* d = h->d_weights;
    for (int a = 0; a < 3; ++a) {
        for (int c = 0; c < 3; ++c) { h->fw.conv_w[a][c] = d + o_conv_w[a][c]; h->fw.conv_b[a][c] = d + o_conv_b[a][c]; }
        h->fw.cat_w[a] = d + o_cat_w[a]; h->fw.cat_b[a] = d + o_cat_b[a];
        h->fw.fc1_wT[a] = d + o_fc1w[a]; h->fw.fc1_b[a] = d + o_fc1b[a];
        h->fw.fc2_wT[a] = d + o_fc2w[a]; h->fw.fc2_b[a] = d + o_fc2b[a];
    }
    for (int c = 0; c < 3; ++c) h->fw.ksize[c] = h->cfg.kersize[c];
    h->fw.attention = h->cfg.attention;
    h->fw.subband_num = h->cfg.subband_num > 0 ? h->cfg.subband_num : 1;
    bind_tcn(h->tw, fb_off, d);
    h->lw.wpack = d + o_wpack; h->lw.wpack12 = d + o_wpack12; for (int ui = 0; ui < 4; ++ui) h->lw.wpack_coop[ui] = d + o_wpack_coop[ui];
    h->lw.wpack_coopn = d + o_wpack_coopn;
    h->lw.wpack_hp = d + o_wpack_hp;
    h->lw.wpack_hpw = h->planner.hp_ok ? d + o_wpack_hpw : nullptr;
    h->lw.hp_wave = h->hp_wave;
    h->lw.wpack_coopw = h->planner.coopw_ok ? d + o_wpack_coopw : nullptr;
    h->lw.wpack_gru = d + o_wpack_gru;
    h->lw.wpack16 = d + o_wpack16;
    h->lw.wpack16_bf = have16_bf ? d + o_wpack16_bf : nullptr;
    h->lw.wpack_bf[0] = d + o_wpack_bf[0]; h->lw.wpack_bf[1] = d + o_wpack_bf[1]; h->lw.ih_bf16 = h->ih_bf16; h->lw.waves = h->lstm_waves; h->lw.bias = d + o_lbias; h->lw.wfc = d + o_wfc; h->lw.bfc = d + o_bfc;
    h->lw.H = H; h->lw.NIN = h->NIN; h->lw.KX = h->KX; h->lw.OUT = h->cfg.output_size; h->lw.gru = h->gru;
    h->lw.wgen = d + o_wgen;
    if (h->sb_tcn) bind_tcn(h->sbt, sb_off, d);
    if (fsn) {
        h->fbw = LstmWeights{};
        for (int ui = 0; ui < 3; ++ui) h->fbw.wpack_coop[ui] = d + o_fbpack[ui];
        h->fbw.bias = d + o_fbbias;
        h->fbw.H = CH; h->fbw.NIN = F; h->fbw.KX = KXF; h->fbw.OUT = 0; h->fbw.gru = h->gru;
        h->fbw.wgen = d + o_fbgen;
        h->fbw.wpack_fbv = have_fbv ? d + o_fbv : nullptr;
        h->fsn_wf = d + o_fsn_wf; h->fsn_bf = d + o_fsn_bf; h->fsn_kp = fsn_kp;
    }
    h->d_refl_w = d + o_refl;
    h->d_refl_wfb = d + o_reflfb;
    if (tuned) {                                // which column-split instantiations fit twice on a CU (registers, LDS)
        for (int ui = 0; ui < 4; ++ui) h->planner.occ_ksplit[ui] = std::max(1, lstm_coop_occupancy(h->lw, 8 << ui));
        for (int rpg = 1; rpg <= 2; ++rpg) h->planner.occ_coopn[rpg - 1] = std::max(1, lstm_coopn_occupancy(h->lw, rpg));
    }
    for (int ui = 0; ui < 3 && fsn && !h->generic_fb; ++ui) h->occ_fb[ui] = lstm_coop_seq_occupancy(h->fbw, 8 << ui);   // (pipelined loop: launch_coop_chained)
    if (h->generic_sb && lstm_generic_check(h->H, h->NIN, false)) return 2;
    if (h->generic_fb && lstm_generic_check(h->CH, h->F, true)) return 2;
    h->committed = true;
    return 0;
}

static int missing_key(const fsnp_handle* h) {
    for (size_t i = 0; i < h->specs.size(); ++i)
        if (!h->spec_src[i]) { set_error("missing key in state_dict: %s", h->specs[i].name.c_str()); return 2; }
    return 0;
}

// fsnp_commit_weights / the mixed case of fsnp_commit_weights_on: whatever only the device arena holds comes down first
static int commit_host(fsnp_handle* h) {
    int64_t down = 0;
    if (const int rc = download_device_given(h, &down)) return rc;
    h->commit_stats[2] = down;
    return commit_impl(h, false, nullptr);
}

}  // namespace fsnp

extern "C" {

int fsnp_set_weight(fsnp_handle* h, const char* name, const float* host_data, int64_t numel) {
    if (!h || !name || !host_data) { set_error("fsnp_set_weight: null argument"); return 1; }
    const int i = find_spec(h, name, numel);
    if (i < 0) return 2;
    std::copy(host_data, host_data + numel, h->host_arena.begin() + h->spec_off[i]);
    h->spec_src[i] = 1;
    h->committed = false;
    h->watch_nseg = 0;            // the watched tensors belonged to the previous weight set (fsnp_watch_weights again after the commit)
    return 0;
}

int fsnp_set_weight_device(fsnp_handle* h, const char* name, const float* dev_data, int64_t numel, void* hip_stream) {
    if (!h || !name || !dev_data) { set_error("fsnp_set_weight_device: null argument"); return 1; }
    const int i = find_spec(h, name, numel);
    if (i < 0) return 2;
    FSNP_ON_DEVICE(h);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (!h->d_arena) FSNP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&h->d_arena), (size_t)std::max<long long>(h->arena_floats, 1) * sizeof(float)));
    if (!h->ev_arena) FSNP_HIP_CHECK(hipEventCreateWithFlags(&h->ev_arena, hipEventDisableTiming));
    // the arena is written in the order of the calls, whatever streams they name, and never under a pack that still reads it
    // (ev_arena is recorded behind every copy on the copy's own stream - never later on a stream the caller may have destroyed - and
    //  a call on another stream waits for it first, so the event of the LAST copy stands for all of them)
    if (h->arena_valid && h->arena_stream != s) FSNP_HIP_CHECK(hipStreamWaitEvent(s, h->ev_arena, 0));
    if (const int rc = order_after_weight_pack(h, s)) return rc;
    FSNP_HIP_CHECK(hipMemcpyAsync(h->d_arena + h->spec_off[i], dev_data, (size_t)numel * sizeof(float), hipMemcpyDeviceToDevice, s));
    FSNP_HIP_CHECK(hipEventRecord(h->ev_arena, s));
    h->arena_stream = s; h->arena_valid = true;
    h->spec_src[i] = 2;
    h->committed = false;
    h->watch_nseg = 0;
    return 0;
}

int fsnp_commit_weights(fsnp_handle* h) {
    if (!h) { set_error("null handle"); return 1; }
    if (const int rc = missing_key(h)) return rc;
    return commit_host(h);
}

int fsnp_commit_weights_on(fsnp_handle* h, void* hip_stream) {
    if (!h) { set_error("null handle"); return 1; }
    if (const int rc = missing_key(h)) return rc;
    bool all_device = true;
    for (unsigned char v : h->spec_src) all_device = all_device && v >= 2;
    if (!all_device) return commit_host(h);
    h->commit_stats[2] = 0;
    return commit_impl(h, true, static_cast<hipStream_t>(hip_stream));
}

}  // extern "C"

// HuBERT-large as a device program over MtGraph (mt_graph.h).
//
// transformers HubertModel, configuration of facebook/hubert-large-ls960-ft (feat_extract_norm="layer", conv_bias,
// do_stable_layer_norm, feat_proj_layer_norm), called as avatars/ultralight/audio2feature.py:35,45 calls it: no attention mask,
// last_hidden_state.  For a clip of n samples:
//   feature_extractor.conv_layers.0            Conv1d(1, 512, 10, 5) + LayerNorm(512) + GELU            hubert_layer0_kernel
//   feature_extractor.conv_layers.1-6          Conv1d(512, 512, k 3,3,3,3,2,2, stride 2)                 add_conv2 (k x 1 on a [T][1] map)
//                              .i.layer_norm   LayerNorm(512) + GELU                                     ln_gelu512_kernel
//   feature_projection.layer_norm / .projection                                                          LayerNorm, linear 512 -> 1024
//   encoder.pos_conv_embed                     h + GELU(grouped Conv1d k 128 (h)[..., :-1])              hubert_posconv_kernel
//   encoder.layers.l   h += attn(layer_norm(h)); h += feed_forward(final_layer_norm(h))                  as the Whisper layers, k with a bias
//   encoder.layer_norm
// The depth is the number of encoder.layers.N in the state dict.
//
// A program has fixed geometry, so there is one per clip length; the packed weights (0.63 GB of fp16 at 24 layers) exist once, in the
// graph mt_build_hubert_weights builds: every program is built over it (MtGraph::share) and owns its activations and op list only.
// Nothing is reused between the activations of a program: a 1000-row program (the 320 080-sample clip) holds 0.19 GB of
// feature-extractor maps and 25 MB per encoder layer, 0.79 GB at 24 layers.
#include <math.h>

#include <algorithm>

#include "mt_graph.h"
#include "hubert_kernels.h"
#include "nn_kernels.h"

namespace ltk {

namespace {

constexpr int kHbConvK[7] = {10, 3, 3, 3, 3, 2, 2};
constexpr int kHbConvS[7] = {5, 2, 2, 2, 2, 2, 2};
constexpr int kHbD = 1024, kHbHeads = 16, kHbFF = 4096, kHbC = 512;
constexpr int kHbProtoSamples = 16640;         // the length the weights' owner is laid out for: 51 rows, so every linear layer gets its row-GEMM plan

int hb_norm(MtGraph& g, SD& sd, MtOpType type, const std::string& name, const MtTensor& x, const MtTensor& y, int C) {
    const float *gm = nullptr, *bt = nullptr;
    if (!g.share) {
        gm = sd.get(name + ".weight", C);
        bt = sd.get(name + ".bias", C);
        if (!gm || !bt) { g.err = sd.err; return -1; }
    }
    MtOp op;
    op.type = type; op.name = name; op.x = x; op.y = y; op.eps = 1e-5f;
    op.gamma = g.add_named_vec(name + ".weight", gm, (size_t)C * sizeof(float));
    op.beta = g.add_named_vec(name + ".bias", bt, (size_t)C * sizeof(float));
    if (op.gamma < 0 || op.beta < 0) return -1;
    g.ops.push_back(op);
    g.named[name] = y;
    return 0;
}

// linear / k x 1 conv under the state dict's name `p`; qscale folds the attention's d^-0.5 into weight and bias
int hb_conv(MtGraph& g, SD& sd, const std::string& p, int Cin, int Cout, int k, int stride, const MtTensor& x, const MtTensor& y,
            const MtTensor* res, int act, float qscale = 1.f) {
    if (g.share) return g.add_conv2(p, nullptr, nullptr, Cin, Cout, k, 1, stride, 1, 0, 0, x, y, res, act, 0);
    const float* w = sd.get(p + ".weight", (size_t)Cout * Cin * k);
    const float* b = sd.get(p + ".bias", Cout);
    if (!w || !b) { g.err = sd.err; return -1; }
    if (qscale == 1.f) return g.add_conv2(p, w, b, Cin, Cout, k, 1, stride, 1, 0, 0, x, y, res, act, 0);
    std::vector<float> ws((size_t)Cout * Cin * k), bs(Cout);
    for (size_t i = 0; i < ws.size(); ++i) ws[i] = w[i] * qscale;
    for (int i = 0; i < Cout; ++i) bs[i] = b[i] * qscale;
    return g.add_conv2(p, ws.data(), bs.data(), Cin, Cout, k, 1, stride, 1, 0, 0, x, y, res, act, 0);
}

}  // namespace

int hubert_rows(int n_samples) {
    long long t = n_samples;
    for (int i = 0; i < 7; ++i) {
        if (t < kHbConvK[i]) return 0;
        t = (t - kHbConvK[i]) / kHbConvS[i] + 1;
    }
    return (int)t;
}

int mt_build_hubert(MtGraph& g, const ltk_named_tensor* t, int n, int n_samples) {
    SD sd{t, n, ""};
    const int D = kHbD, C = kHbC;
    if (g.share) g.hb_layers = g.share->hb_layers;
    else {
        while (sd.has("encoder.layers." + std::to_string(g.hb_layers) + ".layer_norm.weight")) ++g.hb_layers;
        if (g.hb_layers == 0) { g.err = "state_dict has no encoder.layers.0"; return -1; }
    }
    int len[7];
    {
        long long tt = n_samples;
        for (int i = 0; i < 7; ++i) { tt = (tt - kHbConvK[i]) / kHbConvS[i] + 1; len[i] = (int)tt; }
    }
    const int T = len[6];
    if (T < 1) { g.err = "clip too short"; return -1; }
    g.hb_samples = n_samples; g.hb_rows = T;
    g.hb_pcm_buf = (int)g.buf_halfs.size();
    g.buf_halfs.push_back((size_t)n_samples * 2);                  // fp32 samples

    // layer 0
    MtTensor h = g.alloc(C, len[0], 1);
    {
        const std::string p = "feature_extractor.conv_layers.0";
        const float *w = nullptr, *b = nullptr, *gm = nullptr, *bt = nullptr;
        if (!g.share) {
            w = sd.get(p + ".conv.weight", (size_t)C * 10); b = sd.get(p + ".conv.bias", C);
            gm = sd.get(p + ".layer_norm.weight", C); bt = sd.get(p + ".layer_norm.bias", C);
            if (!w || !b || !gm || !bt) { g.err = sd.err; return -1; }
        }
        MtOp op;
        op.type = OP_HB_L0; op.name = p + ".layer_norm"; op.y = h; op.eps = 1e-5f;
        op.wvec = g.add_named_vec(p + ".conv.weight", w, (size_t)C * 10 * sizeof(float));
        op.bvec = g.add_named_vec(p + ".conv.bias", b, (size_t)C * sizeof(float));
        op.gamma = g.add_named_vec(p + ".layer_norm.weight", gm, (size_t)C * sizeof(float));
        op.beta = g.add_named_vec(p + ".layer_norm.bias", bt, (size_t)C * sizeof(float));
        if (op.wvec < 0 || op.bvec < 0 || op.gamma < 0 || op.beta < 0) return -1;
        g.ops.push_back(op);
        g.named[op.name] = h;
    }
    for (int i = 1; i < 7; ++i) {
        const std::string p = "feature_extractor.conv_layers." + std::to_string(i);
        MtTensor c = g.alloc(C, len[i], 1), a = g.alloc(C, len[i], 1);
        if (hb_conv(g, sd, p + ".conv", C, C, kHbConvK[i], kHbConvS[i], h, c, nullptr, 0)) return -1;
        if (hb_norm(g, sd, OP_LNGELU, p + ".layer_norm", c, a, C)) return -1;
        h = a;
    }
    MtTensor fn = g.alloc(C, T, 1), h0 = g.alloc(D, T, 1);
    if (hb_norm(g, sd, OP_LN, "feature_projection.layer_norm", h, fn, C)) return -1;
    if (hb_conv(g, sd, "feature_projection.projection", C, D, 1, 1, fn, h0, nullptr, 0)) return -1;
    h = g.alloc(D, T, 1);
    {
        const std::string p = "encoder.pos_conv_embed";
        MtOp op;
        op.type = OP_POSCONV; op.name = p; op.x = h0; op.y = h;
        if (g.share) {
            op.wvec = g.add_named_vec(p + ".conv.weight", nullptr, 0);
            op.bvec = g.add_named_vec(p + ".conv.bias", nullptr, 0);
        } else {
            const float* w = sd.get(p + ".conv.weight", (size_t)D * 64 * 128);
            const float* b = sd.get(p + ".conv.bias", D);
            if (!w || !b) { g.err = sd.err; return -1; }
            std::vector<f16> packed(kPosConvPackHalfs);
            hubert_posconv_pack(w, packed.data());
            op.wvec = g.add_named_vec(p + ".conv.weight", packed.data(), packed.size() * sizeof(f16));
            op.bvec = g.add_named_vec(p + ".conv.bias", b, (size_t)D * sizeof(float));
        }
        if (op.wvec < 0 || op.bvec < 0) return -1;
        g.ops.push_back(op);
        g.named[p] = h;
    }
    const int d = D / kHbHeads;
    const float qscale = 1.0f / sqrtf((float)d);
    for (int l = 0; l < g.hb_layers; ++l) {
        const std::string p = "encoder.layers." + std::to_string(l), a = p + ".attention";
        MtTensor n1 = g.alloc(D, T, 1), q = g.alloc(D, T, 1), k = g.alloc(D, T, 1), v = g.alloc(D, T, 1), o = g.alloc(D, T, 1);
        MtTensor h1 = g.alloc(D, T, 1), n2 = g.alloc(D, T, 1), f1 = g.alloc(kHbFF, T, 1), h2 = g.alloc(D, T, 1);
        if (hb_norm(g, sd, OP_LN, p + ".layer_norm", h, n1, D)) return -1;
        if (hb_conv(g, sd, a + ".q_proj", D, D, 1, 1, n1, q, nullptr, 0, qscale)) return -1;
        if (hb_conv(g, sd, a + ".k_proj", D, D, 1, 1, n1, k, nullptr, 0)) return -1;
        if (hb_conv(g, sd, a + ".v_proj", D, D, 1, 1, n1, v, nullptr, 0)) return -1;
        g.add_attn(a, q, k, v, o, kHbHeads, d);
        if (hb_conv(g, sd, a + ".out_proj", D, D, 1, 1, o, h1, &h, 0)) return -1;
        if (hb_norm(g, sd, OP_LN, p + ".final_layer_norm", h1, n2, D)) return -1;
        if (hb_conv(g, sd, p + ".feed_forward.intermediate_dense", D, kHbFF, 1, 1, n2, f1, nullptr, 2)) return -1;       // GELU
        if (hb_conv(g, sd, p + ".feed_forward.output_dense", kHbFF, D, 1, 1, f1, h2, &h1, 0)) return -1;
        h = h2;
    }
    MtTensor fin = g.alloc(D, T, 1);
    if (hb_norm(g, sd, OP_LN, "encoder.layer_norm", h, fin, D)) return -1;
    g.hb_out = new MtTensor(fin);
    return 0;
}

// ------------------------------------------------------------------------------------------ public wrappers (musetalk.h)
int mt_build_hubert_weights(MtGraph* g, const ltk_named_tensor* sd, int n) {
    return mt_build_hubert(*g, sd, n, kHbProtoSamples);           // packs every layer; no activations: this graph is never run
}
int mt_build_hubert_program(MtGraph* g, const MtGraph* weights, int n_samples, int frames) {
    g->share = weights;
    if (mt_build_hubert(*g, nullptr, 0, n_samples)) return -1;
    return mt_graph_alloc(*g, frames);
}

// mt_build_hubert's buffer list: the waveform, layer 0's map, conv + LayerNorm map of layers 1-6, the projection's two, the positional
// conv's, nine maps per encoder layer (eight of 1024 channels, the FFN's 4096), the final LayerNorm, the attention's transposed values
size_t hubert_clip_activation_bytes(int n_samples, int layers) {
    size_t len[7];
    long long tt = n_samples;
    for (int i = 0; i < 7; ++i) {
        if (tt < kHbConvK[i]) return 0;
        tt = (tt - kHbConvK[i]) / kHbConvS[i] + 1;
        len[i] = (size_t)tt;
    }
    const size_t T = len[6];
    size_t halfs = (size_t)n_samples * 2 + (size_t)kHbC * len[0];
    for (int i = 1; i < 7; ++i) halfs += 2 * (size_t)kHbC * len[i];
    halfs += (size_t)kHbC * T + 2 * (size_t)kHbD * T;
    halfs += (size_t)layers * (8 * (size_t)kHbD + kHbFF) * T;
    halfs += (size_t)kHbD * T;
    halfs += (size_t)kHbHeads * attn_dv32(kHbD / kHbHeads) * attn_tkp((int)T);
    return halfs * sizeof(f16);
}

std::vector<HubertRun> hubert_batch_plan(const int* n_samples, int nreq, int layers) {
    std::vector<HubertRun> runs;
    std::vector<char> taken((size_t)std::max(nreq, 0), 0);
    for (int r = 0; r < nreq; ++r) {
        if (taken[r]) continue;
        std::vector<int> group;
        for (int q = r; q < nreq; ++q)
            if (!taken[q] && n_samples[q] == n_samples[r]) { group.push_back(q); taken[q] = 1; }
        const size_t clip = hubert_clip_activation_bytes(n_samples[r], layers);
        const bool fits = clip > 0 && clip * kHubertBatchClips < kHubertBatchBudget;
        for (size_t i0 = 0; i0 < group.size(); i0 += kHubertBatchClips) {
            const size_t m = std::min(group.size() - i0, (size_t)kHubertBatchClips);
            if (fits && m > 1) {
                HubertRun run;
                run.n_samples = n_samples[r]; run.batched = true;
                run.req.assign(group.begin() + i0, group.begin() + i0 + m);
                runs.push_back(run);
            } else {
                for (size_t i = i0; i < i0 + m; ++i) {
                    HubertRun run;
                    run.n_samples = n_samples[r];
                    run.req.push_back(group[i]);
                    runs.push_back(run);
                }
            }
        }
    }
    return runs;
}
int mt_hubert_layers(const MtGraph* g) { return g->hb_layers; }
int mt_hubert_rows(const MtGraph* g) { return g->hb_rows; }
float* mt_hubert_pcm_in(MtGraph* g) { return reinterpret_cast<float*>(g->bufs[g->hb_pcm_buf]); }
f16* mt_hubert_out(MtGraph* g, int* cbt, int* cb0) {
    *cbt = g->hb_out->ld / 16; *cb0 = g->hb_out->coff / 16;
    return g->bufs[g->hb_out->buf];
}

}  // namespace ltk

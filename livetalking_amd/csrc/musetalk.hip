// MuseTalk per-frame generator on the HIP engine: conditional U-Net + VAE decoder as a static launch program.
//
// Reference call sites: avatars/musetalk_avatar.py:130-152 (MuseReal.inference_batch),
// avatars/musetalk/models/unet.py:12-46 (PositionalEncoding, diffusers UNet2DConditionModel),
// avatars/musetalk/models/vae.py:96-108 (decode_latents).  The diffusers graph itself is restated in
// oracle/musetalk_oracle.py (the checker); this file is its device program: every conv / linear is one launch of
// the MFMA conv kernels (conv3_mfma.hip / conv_mfma.hip: a Linear over channels is a 1x1 conv on the token map),
// GroupNorm / LayerNorm / attention / GEGLU are nn_kernels.hip.  Load-time folding:
//   * the timestep is the constant 0 (musetalk_avatar.py:61,148-150): time_embedding and every resnet's
//     time_emb_proj collapse into the bias of that resnet's conv1;
//   * the attention scale d^-0.5 goes into to_q; heads of 40 channels are padded to 48 (three channel blocks)
//     by permuting to_q/to_k/to_v rows and to_out columns;
//   * 1/scaling_factor (vae.py:103) goes into post_quant_conv;
//   * torch.cat([h, skip]) of the up path is a channel-block range of one buffer.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "mt_graph.h"
#include "tune.h"
#include "nn_kernels.h"
#include "facedet.h"
#include "faceparse.h"
#include "parse_kernels.h"
#include "s3fd_kernels.h"

namespace ltk {

namespace {

// ------------------------------------------------------------------------------------------ weight transforms
// Linear [Cout][Cin] whose OUTPUT channels are per-head slices of d channels -> heads padded to d16 (zero rows)
std::vector<float> pad_heads_rows(const float* w, int C, int Cin, int heads, int d, int d16, float scale) {
    std::vector<float> o((size_t)heads * d16 * Cin, 0.f);
    for (int h = 0; h < heads; ++h)
        for (int j = 0; j < d; ++j) {
            const float* src = w + (size_t)(h * d + j) * Cin;
            float* dst = o.data() + (size_t)(h * d16 + j) * Cin;
            for (int i = 0; i < Cin; ++i) dst[i] = src[i] * scale;
        }
    (void)C;
    return o;
}
std::vector<float> pad_heads_vec(const float* b, int heads, int d, int d16, float scale) {
    std::vector<float> o((size_t)heads * d16, 0.f);
    if (b)
        for (int h = 0; h < heads; ++h)
            for (int j = 0; j < d; ++j) o[h * d16 + j] = b[h * d + j] * scale;
    return o;
}
// Linear [Cout][C] whose INPUT channels are per-head slices -> padded input columns
std::vector<float> pad_heads_cols(const float* w, int Cout, int heads, int d, int d16) {
    std::vector<float> o((size_t)Cout * heads * d16, 0.f);
    for (int co = 0; co < Cout; ++co)
        for (int h = 0; h < heads; ++h)
            for (int j = 0; j < d; ++j) o[(size_t)co * heads * d16 + h * d16 + j] = w[(size_t)co * heads * d + h * d + j];
    return o;
}

// LayerNorm folded into the linear layer behind it (MT_FUSE bit 2): y = W LN(x) + b = rstd * (W' x - mean * scale) + shift with
//   W'[co][ci] = W[co][ci] gamma[ci]   (what is packed as the layer's fp16 weights),
//   scale[co]  = sum_ci fp16(W'[co][ci])   (of the ROUNDED weights, so that the mean term cancels exactly what the MFMAs summed),
//   shift[co]  = sum_ci W[co][ci] beta[ci] + b[co];
// mean / rstd per token come from the partial sums the producer of x wrote (stats_buf).
struct LnFold { const float* gamma; const float* beta; int C; int stats_buf; float eps; };
void ln_fold(const float* w, const float* bias, int Cout, const LnFold& ln, std::vector<float>* wf, std::vector<float>* scale,
             std::vector<float>* shift) {
    const int C = ln.C;
    wf->resize((size_t)Cout * C); scale->assign(Cout, 0.f); shift->assign(Cout, 0.f);
    for (int co = 0; co < Cout; ++co) {
        double ssum = 0.0, bsum = bias ? (double)bias[co] : 0.0;
        for (int ci = 0; ci < C; ++ci) {
            const float v = w[(size_t)co * C + ci] * ln.gamma[ci];
            (*wf)[(size_t)co * C + ci] = v;
            ssum += (double)(float)(f16)v;
            bsum += (double)w[(size_t)co * C + ci] * ln.beta[ci];
        }
        (*scale)[co] = (float)ssum;
        (*shift)[co] = (float)bsum;
    }
}

float silu_h(float v) { return v / (1.f + expf(-v)); }

// UNet2DConditionModel time_proj(flip_sin_to_cos=True, freq_shift=0) + time_embedding at timestep t, then SiLU
// (what every ResnetBlock2D feeds its time_emb_proj): fp32 [1280]
int time_embedding_silu(SD& sd, float t, std::vector<float>* out) {
    const int dim = 320, td = 1280;
    const float* w1 = sd.get("time_embedding.linear_1.weight", (size_t)td * dim);
    const float* b1 = sd.get("time_embedding.linear_1.bias", td);
    const float* w2 = sd.get("time_embedding.linear_2.weight", (size_t)td * td);
    const float* b2 = sd.get("time_embedding.linear_2.bias", td);
    if (!w1 || !b1 || !w2 || !b2) return -1;
    std::vector<float> emb(dim);
    const int half = dim / 2;
    for (int i = 0; i < half; ++i) {
        const float f = expf(-logf(10000.f) * (float)i / (float)half);
        emb[i] = cosf(t * f);            // flip_sin_to_cos: cos first
        emb[half + i] = sinf(t * f);
    }
    std::vector<float> h1(td), h2(td);
    for (int o = 0; o < td; ++o) {
        double a = b1[o];
        for (int i = 0; i < dim; ++i) a += (double)w1[(size_t)o * dim + i] * emb[i];
        h1[o] = silu_h((float)a);
    }
    for (int o = 0; o < td; ++o) {
        double a = b2[o];
        for (int i = 0; i < td; ++i) a += (double)w2[(size_t)o * td + i] * h1[i];
        h2[o] = silu_h((float)a);
    }
    *out = h2;
    return 0;
}

// ------------------------------------------------------------------------------------------ blocks
// diffusers ResnetBlock2D; temb_silu (or null) is folded into conv1's bias
int build_resnet(MtGraph& g, SD& sd, const std::string& p, const MtTensor& x, const MtTensor& out, int Cin, int Cout,
                 const std::vector<float>* temb_silu, float eps) {
    const int H = x.H, W = x.W;
    MtTensor t1 = (g.fp8 && Cin % 32 == 0) ? g.alloc_q8(Cin, H, W) : g.alloc(Cin, H, W);
    if (g.add_gn(p + ".norm1", sd, p + ".norm1", x, t1, eps, 1)) return -1;
    const float* w1 = sd.get(p + ".conv1.weight", (size_t)Cout * Cin * 9);
    const float* b1 = sd.get(p + ".conv1.bias", Cout);
    if (!w1 || !b1) { g.err = sd.err; return -1; }
    std::vector<float> bias1(b1, b1 + Cout);
    if (temb_silu) {
        const int td = (int)temb_silu->size();
        const float* wt = sd.get(p + ".time_emb_proj.weight", (size_t)Cout * td);
        const float* bt = sd.get(p + ".time_emb_proj.bias", Cout);
        if (!wt || !bt) { g.err = sd.err; return -1; }
        for (int o = 0; o < Cout; ++o) {
            double a = bt[o];
            for (int i = 0; i < td; ++i) a += (double)wt[(size_t)o * td + i] * (*temb_silu)[i];
            bias1[o] += (float)a;
        }
    }
    MtTensor h = g.alloc(Cout, H, W);
    if (g.add_conv(p + ".conv1", w1, bias1.data(), Cin, Cout, 3, 1, 1, t1, h, nullptr, 0, 0)) return -1;
    MtTensor t2 = (g.fp8 && Cout % 32 == 0) ? g.alloc_q8(Cout, H, W) : g.alloc(Cout, H, W);
    if (g.add_gn(p + ".norm2", sd, p + ".norm2", h, t2, eps, 1)) return -1;
    MtTensor skip = x;
    if (sd.has(p + ".conv_shortcut.weight")) {
        const float* ws = sd.get(p + ".conv_shortcut.weight", (size_t)Cout * Cin);
        const float* bs = sd.get(p + ".conv_shortcut.bias", Cout);
        if (!ws || !bs) { g.err = sd.err; return -1; }
        skip = g.alloc(Cout, H, W);
        if (g.add_conv(p + ".conv_shortcut", ws, bs, Cin, Cout, 1, 1, 0, x, skip, nullptr, 0, 0)) return -1;
    } else if (Cin != Cout) {
        g.err = p + ": missing conv_shortcut"; return -1;
    }
    const float* w2 = sd.get(p + ".conv2.weight", (size_t)Cout * Cout * 9);
    const float* b2 = sd.get(p + ".conv2.bias", Cout);
    if (!w2 || !b2) { g.err = sd.err; return -1; }
    return g.add_conv(p + ".conv2", w2, b2, Cout, Cout, 3, 1, 1, t2, out, &skip, 0, 0);
}

// diffusers Attention (to_q / to_k / to_v / to_out.0), q from x (C channels), k/v from ctx (Cctx channels);
// out = to_out(attn) + res
// `kv_pre` (or null): {k view, v view} of a projection that already ran (the hoisted, stacked k | v projection of every
// cross-attention, mt_build_unet), `vt_pre` the buffer its transposed values are in
int build_attention(MtGraph& g, SD& sd, const std::string& p, const MtTensor& x, const MtTensor& ctx, int C, int Cctx, int heads,
                    bool qkv_bias, const MtTensor& res, const MtTensor& out, const MtTensor* kv_pre = nullptr, int vt_pre = -1,
                    const LnFold* ln = nullptr, int ln_out_buf = -1) {
    // `ln`: x is the RAW tensor of a LayerNorm in front of this attention; the projections that read it are built folded (ln_fold).
    // `ln_out_buf` >= 0: to_out.0 (+ residual) also writes the per-token partial statistics of its output there (the next LayerNorm's)
    const int d = C / heads, d16 = up16(d), Cp = heads * d16;
    const float scale = 1.0f / sqrtf((float)d);
    const float* wq = sd.get(p + ".to_q.weight", (size_t)C * C);
    const float* wk = sd.get(p + ".to_k.weight", (size_t)C * Cctx);
    const float* wv = sd.get(p + ".to_v.weight", (size_t)C * Cctx);
    const float* wo = sd.get(p + ".to_out.0.weight", (size_t)C * C);
    const float* bo = sd.get(p + ".to_out.0.bias", C);
    if (!wq || !wk || !wv || !wo || !bo) { g.err = sd.err; return -1; }
    const float *bq = nullptr, *bk = nullptr, *bv = nullptr;
    if (qkv_bias) {
        bq = sd.get(p + ".to_q.bias", C); bk = sd.get(p + ".to_k.bias", C); bv = sd.get(p + ".to_v.bias", C);
        if (!bq || !bk || !bv) { g.err = sd.err; return -1; }
    }
    const std::vector<float> wqp = pad_heads_rows(wq, C, C, heads, d, d16, scale), bqp = pad_heads_vec(bq, heads, d, d16, scale);
    const std::vector<float> wkp = pad_heads_rows(wk, C, Cctx, heads, d, d16, 1.f), bkp = pad_heads_vec(bk, heads, d, d16, 1.f);
    const std::vector<float> wvp = pad_heads_rows(wv, C, Cctx, heads, d, d16, 1.f), bvp = pad_heads_vec(bv, heads, d, d16, 1.f);
    const std::vector<float> wop = pad_heads_cols(wo, C, heads, d, d16);
    // Projections that read the same tensor are ONE launch (rows of the weight matrices stacked, outputs = channel-block
    // ranges of one buffer): q|k|v for self-attention, k|v for cross-attention.  These are 1-3 GFLOP GEMMs whose cost is
    // the launch, not the math.
    auto stack = [](std::initializer_list<const std::vector<float>*> parts) {
        std::vector<float> o;
        for (const std::vector<float>* v : parts) o.insert(o.end(), v->begin(), v->end());
        return o;
    };
    const bool self = x.buf == ctx.buf && x.coff == ctx.coff && x.C == ctx.C;
    MtTensor q, k, v, o = g.alloc(Cp, x.H, x.W);
    // a projection of x: plain, or with the LayerNorm in front of it folded in
    auto proj_x = [&](const std::string& name, const std::vector<float>& w, const std::vector<float>& b, int Cout, const MtTensor& y) -> int {
        if (!ln) return g.add_conv(name, w.data(), b.data(), C, Cout, 1, 1, 0, x, y, nullptr, 0, 0);
        std::vector<float> wf, sc, sf;
        ln_fold(w.data(), b.data(), Cout, *ln, &wf, &sc, &sf);
        if (g.add_conv(name, wf.data(), sf.data(), C, Cout, 1, 1, 0, x, y, nullptr, 0, 0, sc.data())) return -1;
        MtOp& op = g.ops.back();
        op.ln_in_buf = ln->stats_buf; op.ln_in_tiles = ln->C / 32; op.ln_eps = ln->eps;
        return 0;
    };
    if (ln && !(kv_pre || self)) { g.err = p + ": the LayerNorm fold needs the stacked q|k|v projection or a hoisted k|v"; return -1; }
    if (kv_pre) {
        q = g.alloc(Cp, x.H, x.W);
        if (proj_x(p + ".to_q", wqp, bqp, Cp, q)) return -1;
        k = kv_pre[0]; v = kv_pre[1];
    } else if (self) {
        MtTensor qkv = g.alloc(3 * Cp, x.H, x.W);
        const std::vector<float> w3 = stack({&wqp, &wkp, &wvp}), b3 = stack({&bqp, &bkp, &bvp});
        if (proj_x(p + ".to_qkv", w3, b3, 3 * Cp, qkv)) return -1;
        q = MtGraph::view(qkv, 0, Cp); k = MtGraph::view(qkv, Cp, Cp); v = MtGraph::view(qkv, 2 * Cp, Cp);
    } else {
        q = g.alloc(Cp, x.H, x.W);
        MtTensor kv = g.alloc(2 * Cp, ctx.H, ctx.W);
        const std::vector<float> w2 = stack({&wkp, &wvp}), b2 = stack({&bkp, &bvp});
        if (g.add_conv(p + ".to_q", wqp.data(), bqp.data(), C, Cp, 1, 1, 0, x, q, nullptr, 0, 0)) return -1;
        if (g.add_conv(p + ".to_kv", w2.data(), b2.data(), Cctx, 2 * Cp, 1, 1, 0, ctx, kv, nullptr, 0, 0)) return -1;
        k = MtGraph::view(kv, 0, Cp); v = MtGraph::view(kv, Cp, Cp);
    }
    g.named[p + ".to_q"] = q; g.named[p + ".to_k"] = k; g.named[p + ".to_v"] = v;
    g.add_attn(p, q, k, v, o, heads, d16, kv_pre ? vt_pre : -1);
    if (g.add_conv(p + ".to_out.0", wop.data(), bo, Cp, C, 1, 1, 0, o, out, &res, 0, 0)) return -1;
    g.ops.back().ln_out_buf = ln_out_buf;
    return 0;
}

// diffusers Transformer2DModel (conv proj_in/out) with one BasicTransformerBlock (GEGLU feed-forward)
int build_transformer(MtGraph& g, SD& sd, const std::string& p, const MtTensor& x, const MtTensor& ctx, const MtTensor& out, int C) {
    const int H = x.H, W = x.W;
    MtTensor t = g.alloc(C, H, W);
    if (g.add_gn(p + ".norm", sd, p + ".norm", x, t, 1e-6f, 0)) return -1;
    const float* wi = sd.get(p + ".proj_in.weight", (size_t)C * C);
    const float* bi = sd.get(p + ".proj_in.bias", C);
    if (!wi || !bi) { g.err = sd.err; return -1; }
    MtTensor h0 = g.alloc(C, H, W);
    if (g.add_conv(p + ".proj_in", wi, bi, C, C, 1, 1, 0, t, h0, nullptr, 0, 0)) return -1;
    const std::string b = p + ".transformer_blocks.0";
    // MT_FUSE bit 2: the three LayerNorms disappear into the linear layers around them - the producer of a normalised tensor
    // (proj_in, attn1.to_out.0, attn2.to_out.0) writes per-token partial sums beside its output, the consumer (to_qkv, attn2.to_q,
    // ff.net.0.proj) reads the raw tensor with gamma folded into its weights and normalises in its epilogue (ln_fold).  48 launches
    // and as many tensor round trips of a pass; needs the stacked q|k|v projection and the hoisted cross-attention k|v (bit 1).
    const bool fold = (knob(K_MT_FUSE) & 4) && (knob(K_MT_FUSE) & 2) && C % 32 == 0 &&
                      g.kv_pre.find(b + ".attn2") != g.kv_pre.end();
    LnFold l1{nullptr, nullptr, C, -1, 1e-5f}, l2 = l1, l3 = l1;
    if (fold) {
        const char* nm[3] = {".norm1", ".norm2", ".norm3"};
        LnFold* ls[3] = {&l1, &l2, &l3};
        for (int i = 0; i < 3; ++i) {
            ls[i]->gamma = sd.get(b + nm[i] + ".weight", C);
            ls[i]->beta = sd.get(b + nm[i] + ".bias", C);
            if (!ls[i]->gamma || !ls[i]->beta) { g.err = sd.err; return -1; }
            ls[i]->stats_buf = g.alloc_ln_stats(C, H, W);
        }
        g.ops.back().ln_out_buf = l1.stats_buf;           // proj_in
    }
    MtTensor n1, h1 = g.alloc(C, H, W);
    if (fold) {
        if (build_attention(g, sd, b + ".attn1", h0, h0, C, C, 8, false, h0, h1, nullptr, -1, &l1, l2.stats_buf)) return -1;
    } else {
        n1 = g.alloc(C, H, W);
        if (g.add_ln(b + ".norm1", sd, b + ".norm1", h0, n1, 1e-5f)) return -1;
        if (build_attention(g, sd, b + ".attn1", n1, n1, C, C, 8, false, h0, h1)) return -1;
    }
    MtTensor n2, h2 = g.alloc(C, H, W);
    if (fold) {
        auto kv = g.kv_pre.find(b + ".attn2");
        const MtTensor pre[2] = {kv->second.k, kv->second.v};
        if (build_attention(g, sd, b + ".attn2", h1, ctx, C, 384, 8, false, h1, h2, pre, kv->second.vt_buf, &l2, l3.stats_buf)) return -1;
    } else {
        n2 = g.alloc(C, H, W);
        if (g.add_ln(b + ".norm2", sd, b + ".norm2", h1, n2, 1e-5f)) return -1;
        auto kv = g.kv_pre.find(b + ".attn2");
        if (kv != g.kv_pre.end()) {
            const MtTensor pre[2] = {kv->second.k, kv->second.v};
            if (build_attention(g, sd, b + ".attn2", n2, ctx, C, 384, 8, false, h1, h2, pre, kv->second.vt_buf)) return -1;
        } else if (build_attention(g, sd, b + ".attn2", n2, ctx, C, 384, 8, false, h1, h2)) return -1;
    }
    MtTensor n3, f1, gg = g.alloc(4 * C, H, W), h3 = g.alloc(C, H, W);
    if (!(knob(K_MT_FUSE) & 1)) f1 = g.alloc(8 * C, H, W);
    if (!fold) {
        n3 = g.alloc(C, H, W);
        if (g.add_ln(b + ".norm3", sd, b + ".norm3", h2, n3, 1e-5f)) return -1;
    }
    const float* w1 = sd.get(b + ".ff.net.0.proj.weight", (size_t)8 * C * C);
    const float* b1 = sd.get(b + ".ff.net.0.proj.bias", 8 * C);
    const float* w2 = sd.get(b + ".ff.net.2.weight", (size_t)C * 4 * C);
    const float* b2 = sd.get(b + ".ff.net.2.bias", C);
    if (!w1 || !b1 || !w2 || !b2) { g.err = sd.err; return -1; }
    // the projection as the device runs it: LayerNorm folded in (fold), rows permuted for the GEGLU epilogue (bit 0)
    std::vector<float> wff, scf, sff;
    const float *wp1 = w1, *bp1 = b1, *sp1 = nullptr;
    if (fold) { ln_fold(w1, b1, 8 * C, l3, &wff, &scf, &sff); wp1 = wff.data(); bp1 = sff.data(); sp1 = scf.data(); }
    const MtTensor& ffin = fold ? h2 : n3;
    if (knob(K_MT_FUSE) & 1) {
        // GEGLU in the projection's epilogue: rows permuted so that every 32-row tile is [16 value rows | their 16 gate rows]
        // (value = rows [0, 4C), gate = rows [4C, 8C) of ff.net.0.proj: diffusers GEGLU chunks the projection in that order)
        const int F = 4 * C;
        std::vector<float> wp((size_t)8 * C * C), bp((size_t)8 * C), sp((size_t)8 * C, 1.f);
        for (int tl = 0; tl < F / 16; ++tl)
            for (int r = 0; r < 32; ++r) {
                const int src = (r < 16) ? tl * 16 + r : F + tl * 16 + (r - 16);
                memcpy(&wp[(size_t)(tl * 32 + r) * C], &wp1[(size_t)src * C], (size_t)C * sizeof(float));
                bp[tl * 32 + r] = bp1[src];
                if (sp1) sp[tl * 32 + r] = sp1[src];
            }
        if (g.add_conv(b + ".ff.net.0.proj", wp.data(), bp.data(), C, 8 * C, 1, 1, 0, ffin, gg, nullptr, 4, 0, sp1 ? sp.data() : nullptr)) return -1;
        g.named.erase(b + ".ff.net.0.proj");          // the projection itself is never materialised
        g.named[b + ".ff.geglu"] = gg;
    } else {
        if (g.add_conv(b + ".ff.net.0.proj", wp1, bp1, C, 8 * C, 1, 1, 0, ffin, f1, nullptr, 0, 0, sp1)) return -1;
    }
    if (fold) { MtOp& op = g.ops[g.ops.size() - 1]; op.ln_in_buf = l3.stats_buf; op.ln_in_tiles = C / 32; op.ln_eps = l3.eps; }
    if (!(knob(K_MT_FUSE) & 1)) g.add_geglu(b + ".ff.geglu", f1, gg);
    if (g.add_conv(b + ".ff.net.2", w2, b2, 4 * C, C, 1, 1, 0, gg, h3, &h2, 0, 0)) return -1;
    const float* wo = sd.get(p + ".proj_out.weight", (size_t)C * C);
    const float* bo = sd.get(p + ".proj_out.bias", C);
    if (!wo || !bo) { g.err = sd.err; return -1; }
    return g.add_conv(p + ".proj_out", wo, bo, C, C, 1, 1, 0, h3, out, &x, 0, 0);
}

}  // namespace

// ------------------------------------------------------------------------------------------ U-Net
int mt_build_unet(MtGraph& g, const ltk_named_tensor* t, int n, MtTensor* latent_in, MtTensor* ctx_in, MtTensor* out) {
    SD sd{t, n, ""};
    const int ch[4] = {320, 640, 1280, 1280};
    const bool down_attn[4] = {true, true, true, false};
    const bool up_attn[4] = {false, true, true, true};
    std::vector<float> temb;
    if (time_embedding_silu(sd, 0.f, &temb)) { g.err = sd.err; return -1; }

    *latent_in = g.alloc(8, 32, 32);         // 16-channel block, 8 real
    *ctx_in = g.alloc(384, 50, 1);
    g.named["latent_in"] = *latent_in;
    g.named["encoder_hidden_states"] = *ctx_in;      // the position-encoded audio context as the pass wrote it (debug read-back only)

    // Hoisted cross-attention k | v (MT_FUSE bit 1): the k and v projections of the 16 cross-attentions read the audio context
    // only, so they are ONE stacked 384 -> 25 600 projection at the head of the pass (rows [k_0 | v_0 | k_1 | v_1 ...], heads padded
    // as in build_attention) and ONE launch that transposes the 16 value tensors - instead of 16 + 16 launches on the critical
    // path of their blocks (320 us of a 16-frame pass).
    if (knob(K_MT_FUSE) & 2) {
        struct Blk { std::string p; int C; };
        std::vector<Blk> blks;
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 2; ++j) blks.push_back({"down_blocks." + std::to_string(i) + ".attentions." + std::to_string(j), ch[i]});
        blks.push_back({"mid_block.attentions.0", 1280});
        const int revc[4] = {1280, 1280, 640, 320};
        for (int i = 1; i < 4; ++i) for (int j = 0; j < 3; ++j) blks.push_back({"up_blocks." + std::to_string(i) + ".attentions." + std::to_string(j), revc[i]});
        int total = 0;
        for (const Blk& b : blks) total += 2 * 8 * up16(b.C / 8);
        std::vector<float> wall((size_t)total * 384);
        size_t row = 0;
        std::vector<int> offs;
        for (const Blk& b : blks) {
            const std::string a = b.p + ".transformer_blocks.0.attn2";
            const int d = b.C / 8, d16 = up16(d);
            const float* wk = sd.get(a + ".to_k.weight", (size_t)b.C * 384);
            const float* wv = sd.get(a + ".to_v.weight", (size_t)b.C * 384);
            if (!wk || !wv) { g.err = sd.err; return -1; }
            const std::vector<float> wkp = pad_heads_rows(wk, b.C, 384, 8, d, d16, 1.f), wvp = pad_heads_rows(wv, b.C, 384, 8, d, d16, 1.f);
            offs.push_back((int)row);
            memcpy(&wall[row * 384], wkp.data(), wkp.size() * sizeof(float)); row += (size_t)8 * d16;
            memcpy(&wall[row * 384], wvp.data(), wvp.size() * sizeof(float)); row += (size_t)8 * d16;
        }
        MtTensor kv_all = g.alloc(total, 50, 1);
        if (g.add_conv("attn2.to_kv_all", wall.data(), nullptr, 384, total, 1, 1, 0, *ctx_in, kv_all, nullptr, 0, 0)) return -1;
        MtOp vt;
        vt.type = OP_VT; vt.name = "attn2.v_transpose_all";
        for (size_t bi = 0; bi < blks.size(); ++bi) {
            const int d16 = up16(blks[bi].C / 8), Cp = 8 * d16;
            MtGraph::KvPre pre;
            pre.k = MtGraph::view(kv_all, offs[bi], Cp);
            pre.v = MtGraph::view(kv_all, offs[bi] + Cp, Cp);
            pre.vt_buf = (int)g.buf_halfs.size();
            g.buf_halfs.push_back((size_t)8 * attn_dv32(d16) * attn_tkp(50));
            g.kv_pre[blks[bi].p + ".transformer_blocks.0.attn2"] = pre;
            g.vt_items.push_back({pre.v, 8, d16, 50, pre.vt_buf});
        }
        g.ops.push_back(vt);
    }

    // skip tensors live inside the cat buffers of the up path: plan those first (pop order of down_block_res_samples)
    struct SkipSpec { int C, HW; };
    const SkipSpec skips[12] = {{320, 32}, {320, 32}, {320, 32}, {320, 16}, {640, 16}, {640, 16}, {640, 8}, {1280, 8}, {1280, 8}, {1280, 4}, {1280, 4}, {1280, 4}};
    // channels of h entering each up resnet (block i, resnet j)
    const int up_h[4][3] = {{1280, 1280, 1280}, {1280, 1280, 1280}, {1280, 640, 640}, {640, 320, 320}};
    MtTensor cat[4][3], skip_dst[12];
    {
        int si = 11;
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 3; ++j, --si) {
                cat[i][j] = g.alloc(up_h[i][j] + skips[si].C, skips[si].HW, skips[si].HW);
                skip_dst[si] = MtGraph::view(cat[i][j], up_h[i][j], skips[si].C);
            }
    }
    int si = 0;
    const float* wci = sd.get("conv_in.weight", (size_t)320 * 8 * 9);
    const float* bci = sd.get("conv_in.bias", 320);
    if (!wci || !bci) { g.err = sd.err; return -1; }
    if (g.add_conv("conv_in", wci, bci, 8, 320, 3, 1, 1, *latent_in, skip_dst[si], nullptr, 0, 0)) return -1;
    g.named["conv_in"] = skip_dst[si];
    MtTensor h = skip_dst[si++];
    int C = 320;
    for (int i = 0; i < 4; ++i) {
        for (int j = 0; j < 2; ++j) {
            const std::string rp = "down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j);
            MtTensor dst = skip_dst[si++];
            if (down_attn[i]) {
                MtTensor r = g.alloc(ch[i], h.H, h.W);
                if (build_resnet(g, sd, rp, h, r, C, ch[i], &temb, 1e-5f)) return -1;
                if (build_transformer(g, sd, "down_blocks." + std::to_string(i) + ".attentions." + std::to_string(j), r, *ctx_in, dst, ch[i])) return -1;
            } else {
                if (build_resnet(g, sd, rp, h, dst, C, ch[i], &temb, 1e-5f)) return -1;
            }
            C = ch[i];
            h = dst;
            g.named["down_blocks." + std::to_string(i) + "." + std::to_string(j)] = h;
        }
        if (i < 3) {
            const std::string dp = "down_blocks." + std::to_string(i) + ".downsamplers.0.conv";
            const float* w = sd.get(dp + ".weight", (size_t)C * C * 9);
            const float* b = sd.get(dp + ".bias", C);
            if (!w || !b) { g.err = sd.err; return -1; }
            MtTensor dst = skip_dst[si++];
            if (g.add_conv(dp, w, b, C, C, 3, 2, 1, h, dst, nullptr, 0, 0)) return -1;
            h = dst;
            g.named["down_blocks." + std::to_string(i) + ".down"] = h;
        }
    }
    {
        MtTensor r0 = g.alloc(C, h.H, h.W), a0 = g.alloc(C, h.H, h.W);
        if (build_resnet(g, sd, "mid_block.resnets.0", h, r0, C, C, &temb, 1e-5f)) return -1;
        if (build_transformer(g, sd, "mid_block.attentions.0", r0, *ctx_in, a0, C)) return -1;
        MtTensor dst = MtGraph::view(cat[0][0], 0, up_h[0][0]);
        if (build_resnet(g, sd, "mid_block.resnets.1", a0, dst, C, C, &temb, 1e-5f)) return -1;
        g.named["mid_block"] = dst;
    }
    const int rev[4] = {1280, 1280, 640, 320};
    MtTensor hup;
    for (int i = 0; i < 4; ++i) {
        for (int j = 0; j < 3; ++j) {
            const MtTensor& in = cat[i][j];                    // [h | skip]
            // where this resnet(+attention) writes: the h half of the next cat buffer, or a fresh tensor
            MtTensor dst;
            const bool last_in_block = (j == 2);
            if (!last_in_block) dst = MtGraph::view(cat[i][j + 1], 0, up_h[i][j + 1]);
            else dst = g.alloc(rev[i], in.H, in.W);
            const std::string rp = "up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j);
            if (up_attn[i]) {
                MtTensor r = g.alloc(rev[i], in.H, in.W);
                if (build_resnet(g, sd, rp, in, r, in.C, rev[i], &temb, 1e-5f)) return -1;
                if (build_transformer(g, sd, "up_blocks." + std::to_string(i) + ".attentions." + std::to_string(j), r, *ctx_in, dst, rev[i])) return -1;
            } else {
                if (build_resnet(g, sd, rp, in, dst, in.C, rev[i], &temb, 1e-5f)) return -1;
            }
            g.named["up_blocks." + std::to_string(i) + "." + std::to_string(j)] = dst;
            hup = dst;
        }
        if (i < 3) {
            const std::string up = "up_blocks." + std::to_string(i) + ".upsamplers.0.conv";
            const float* w = sd.get(up + ".weight", (size_t)rev[i] * rev[i] * 9);
            const float* b = sd.get(up + ".bias", rev[i]);
            if (!w || !b) { g.err = sd.err; return -1; }
            MtTensor dst = MtGraph::view(cat[i + 1][0], 0, up_h[i + 1][0]);
            MtTensor xin = hup;
            xin.H *= 2; xin.W *= 2;                               // logical (upsampled) size the conv runs on
            if (g.add_conv(up, w, b, rev[i], rev[i], 3, 1, 1, xin, dst, nullptr, 0, 1)) return -1;
            g.named["up_blocks." + std::to_string(i) + ".up"] = dst;
        }
    }
    MtTensor tn = g.alloc(320, 32, 32);
    if (g.add_gn("conv_norm_out", sd, "conv_norm_out", hup, tn, 1e-5f, 1)) return -1;
    const float* wo = sd.get("conv_out.weight", (size_t)4 * 320 * 9);
    const float* bo = sd.get("conv_out.bias", 4);
    if (!wo || !bo) { g.err = sd.err; return -1; }
    *out = g.alloc(4, 32, 32);
    if (g.add_conv("conv_out", wo, bo, 320, 4, 3, 1, 1, tn, *out, nullptr, 0, 0)) return -1;
    g.named["conv_out"] = *out;
    return 0;
}

// ------------------------------------------------------------------------------------------ VAE decoder
int mt_build_vae(MtGraph& g, const ltk_named_tensor* t, int n, const MtTensor& z, MtTensor* out) {
    SD sd{t, n, ""};
    const float kScaling = 0.18215f;       // AutoencoderKL config.scaling_factor of sd-vae-ft-mse (vae.py:35,103)
    const float* wq = sd.get("post_quant_conv.weight", 16);
    const float* bq = sd.get("post_quant_conv.bias", 4);
    if (!wq || !bq) { g.err = sd.err; return -1; }
    std::vector<float> wqs(16);
    for (int i = 0; i < 16; ++i) wqs[i] = wq[i] / kScaling;
    MtTensor pq = g.alloc(4, 32, 32);
    if (g.add_conv("post_quant_conv", wqs.data(), bq, 4, 4, 1, 1, 0, z, pq, nullptr, 0, 0)) return -1;
    const float* wi = sd.get("decoder.conv_in.weight", (size_t)512 * 4 * 9);
    const float* bi = sd.get("decoder.conv_in.bias", 512);
    if (!wi || !bi) { g.err = sd.err; return -1; }
    MtTensor h = g.alloc(512, 32, 32);
    if (g.add_conv("decoder.conv_in", wi, bi, 4, 512, 3, 1, 1, pq, h, nullptr, 0, 0)) return -1;
    g.named["decoder.conv_in"] = h;
    {
        MtTensor r0 = g.alloc(512, 32, 32);
        if (build_resnet(g, sd, "decoder.mid_block.resnets.0", h, r0, 512, 512, nullptr, 1e-6f)) return -1;
        const std::string a = "decoder.mid_block.attentions.0";
        MtTensor gn = g.alloc(512, 32, 32), ao = g.alloc(512, 32, 32);
        if (g.add_gn(a + ".group_norm", sd, a + ".group_norm", r0, gn, 1e-6f, 0)) return -1;
        if (build_attention(g, sd, a, gn, gn, 512, 512, 1, true, r0, ao)) return -1;
        MtTensor r1 = g.alloc(512, 32, 32);
        if (build_resnet(g, sd, "decoder.mid_block.resnets.1", ao, r1, 512, 512, nullptr, 1e-6f)) return -1;
        h = r1;
        g.named["decoder.mid_block"] = h;
    }
    const int chs[4] = {512, 512, 256, 128};
    int C = 512;
    for (int i = 0; i < 4; ++i) {
        for (int j = 0; j < 3; ++j) {
            MtTensor r = g.alloc(chs[i], h.H, h.W);
            if (build_resnet(g, sd, "decoder.up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), h, r, C, chs[i], nullptr, 1e-6f)) return -1;
            C = chs[i];
            h = r;
        }
        g.named["decoder.up_blocks." + std::to_string(i)] = h;
        if (i < 3) {
            const std::string up = "decoder.up_blocks." + std::to_string(i) + ".upsamplers.0.conv";
            const float* w = sd.get(up + ".weight", (size_t)C * C * 9);
            const float* b = sd.get(up + ".bias", C);
            if (!w || !b) { g.err = sd.err; return -1; }
            MtTensor xin = h;
            xin.H *= 2; xin.W *= 2;
            MtTensor dst = g.alloc(C, xin.H, xin.W);
            if (g.add_conv(up, w, b, C, C, 3, 1, 1, xin, dst, nullptr, 0, 1)) return -1;
            h = dst;
        }
    }
    MtTensor tn = g.alloc(128, 256, 256);
    if (g.add_gn("decoder.conv_norm_out", sd, "decoder.conv_norm_out", h, tn, 1e-6f, 1)) return -1;
    const float* wo = sd.get("decoder.conv_out.weight", (size_t)3 * 128 * 9);
    const float* bo = sd.get("decoder.conv_out.bias", 3);
    if (!wo || !bo) { g.err = sd.err; return -1; }
    *out = g.alloc(3, 256, 256);
    if (g.add_conv("decoder.conv_out", wo, bo, 128, 3, 3, 1, 1, tn, *out, nullptr, 0, 0)) return -1;
    g.named["decoder.conv_out"] = *out;
    return 0;
}

// ------------------------------------------------------------------------------------------ VAE encoder
// AutoencoderKL.encode of sd-vae (avatars/musetalk/models/vae.py:84-94 encode_latents; avatar preparation,
// avatars/musetalk/genavatar.py:116-128): conv_in, 4 down blocks x 2 resnets with asymmetric-pad stride-2 convs,
// mid (resnet, attention, resnet), GN-SiLU-conv_out (8 = mean | logvar), quant_conv.
int mt_build_vae_encoder(MtGraph& g, const ltk_named_tensor* t, int n, MtTensor* img_in, MtTensor* moments) {
    SD sd{t, n, ""};
    *img_in = g.alloc(3, 256, 256);
    const float* wi = sd.get("encoder.conv_in.weight", (size_t)128 * 3 * 9);
    const float* bi = sd.get("encoder.conv_in.bias", 128);
    if (!wi || !bi) { g.err = sd.err; return -1; }
    MtTensor h = g.alloc(128, 256, 256);
    if (g.add_conv("encoder.conv_in", wi, bi, 3, 128, 3, 1, 1, *img_in, h, nullptr, 0, 0)) return -1;
    const int chs[4] = {128, 256, 512, 512};
    int C = 128;
    for (int i = 0; i < 4; ++i) {
        for (int j = 0; j < 2; ++j) {
            MtTensor r = g.alloc(chs[i], h.H, h.W);
            if (build_resnet(g, sd, "encoder.down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), h, r, C, chs[i], nullptr, 1e-6f)) return -1;
            C = chs[i];
            h = r;
        }
        if (i < 3) {
            const std::string dp = "encoder.down_blocks." + std::to_string(i) + ".downsamplers.0.conv";
            const float* w = sd.get(dp + ".weight", (size_t)C * C * 9);
            const float* b = sd.get(dp + ".bias", C);
            if (!w || !b) { g.err = sd.err; return -1; }
            MtTensor d = g.alloc(C, h.H / 2, h.W / 2);
            if (g.add_conv_down_asym(dp, w, b, C, h, d)) return -1;
            h = d;
        }
        g.named["encoder.down_blocks." + std::to_string(i)] = h;
    }
    {
        MtTensor r0 = g.alloc(512, 32, 32);
        if (build_resnet(g, sd, "encoder.mid_block.resnets.0", h, r0, 512, 512, nullptr, 1e-6f)) return -1;
        const std::string a = "encoder.mid_block.attentions.0";
        MtTensor gn = g.alloc(512, 32, 32), ao = g.alloc(512, 32, 32), r1 = g.alloc(512, 32, 32);
        if (g.add_gn(a + ".group_norm", sd, a + ".group_norm", r0, gn, 1e-6f, 0)) return -1;
        if (build_attention(g, sd, a, gn, gn, 512, 512, 1, true, r0, ao)) return -1;
        if (build_resnet(g, sd, "encoder.mid_block.resnets.1", ao, r1, 512, 512, nullptr, 1e-6f)) return -1;
        h = r1;
        g.named["encoder.mid_block"] = h;
    }
    MtTensor tn = g.alloc(512, 32, 32), co = g.alloc(8, 32, 32);
    if (g.add_gn("encoder.conv_norm_out", sd, "encoder.conv_norm_out", h, tn, 1e-6f, 1)) return -1;
    const float* wo = sd.get("encoder.conv_out.weight", (size_t)8 * 512 * 9);
    const float* bo = sd.get("encoder.conv_out.bias", 8);
    const float* wq = sd.get("quant_conv.weight", 64);
    const float* bq = sd.get("quant_conv.bias", 8);
    if (!wo || !bo || !wq || !bq) { g.err = sd.err; return -1; }
    if (g.add_conv("encoder.conv_out", wo, bo, 512, 8, 3, 1, 1, tn, co, nullptr, 0, 0)) return -1;
    *moments = g.alloc(8, 32, 32);
    if (g.add_conv("quant_conv", wq, bq, 8, 8, 1, 1, 0, co, *moments, nullptr, 0, 0)) return -1;
    return 0;
}

// ------------------------------------------------------------------------------------------ public wrappers (musetalk.h)
int mt_build(MtGraph* g, const ltk_named_tensor* unet_sd, int n_unet, const ltk_named_tensor* vae_sd, int n_vae, int frames) {
    g->t_latent = new MtTensor(); g->t_ctx = new MtTensor(); g->t_unet_out = new MtTensor(); g->t_vae_out = new MtTensor();
    if (mt_build_unet(*g, unet_sd, n_unet, g->t_latent, g->t_ctx, g->t_unet_out)) return -1;
    if (mt_build_vae(*g, vae_sd, n_vae, *g->t_unet_out, g->t_vae_out)) return -1;
    return mt_graph_alloc(*g, frames);
}
static f16* tptr(MtGraph* g, const MtTensor* t, int* cbt) { if (cbt) *cbt = t->ld / 16; return g->bufs[t->buf]; }
f16* mt_latent_in(MtGraph* g, int* cbt) { return tptr(g, g->t_latent, cbt); }
f16* mt_ctx_in(MtGraph* g, int* cbt) { return tptr(g, g->t_ctx, cbt); }
f16* mt_unet_out(MtGraph* g, int* cbt) { return tptr(g, g->t_unet_out, cbt); }
f16* mt_vae_out(MtGraph* g, int* cbt) { return tptr(g, g->t_vae_out, cbt); }
int mt_build_vae_encoder_graph(MtGraph* g, const ltk_named_tensor* sd, int n, int frames) {
    g->t_latent = new MtTensor();          // image input
    g->t_unet_out = new MtTensor();        // moments output
    if (mt_build_vae_encoder(*g, sd, n, g->t_latent, g->t_unet_out)) return -1;
    return mt_graph_alloc(*g, frames);
}

// ------------------------------------------------------------------------------------------ face parser (avatar preparation: blend masks)
// BiSeNet's main output (avatars/musetalk/utils/face_parsing/model.py BiSeNet.forward()[0], resnet.py) + argmax as the 41 launches of
// fp_program, wired by fp_plan (faceparse.h) and by nothing else: the plan's buffers become the graph's under the same ids, its views
// the ops' tensors.  Convs are the library's with eval-mode BatchNorm folded into the fp32 scale / shift of the epilogue
// (state_dict.h fold_bn; ffm.conv1, ffm.conv2 and conv_out.conv_out have neither BatchNorm nor bias); the stem's weights are packed once.
namespace {
// the state-dict names behind a conv of the list: its weight is `w`.weight, its BatchNorm `bn`.* (empty: none)
void fp_keys(const std::string& name, std::string* w, std::string* bn) {
    auto swap_tail = [&](const char* tail, const char* with) {
        const size_t n = strlen(tail);
        if (name.size() < n || name.compare(name.size() - n, n, tail) != 0) return false;
        *bn = name.substr(0, name.size() - n) + with;
        return true;
    };
    *w = name; bn->clear();
    if (name.rfind("cp.resnet.", 0) == 0) {                      // resnet.py: conv1 / bn1, conv2 / bn2, downsample.0 / downsample.1
        if (!swap_tail("conv1", "bn1") && !swap_tail("conv2", "bn2")) (void)swap_tail("downsample.0", "downsample.1");
    } else if (swap_tail("conv_atten", "bn_atten")) {            // AttentionRefinementModule (model.py:66-67)
    } else if (name == "ffm.conv1" || name == "ffm.conv2" || name == "conv_out.conv_out") {
    } else {                                                      // ConvBNReLU (model.py:14-24): .conv / .bn
        *w = name + ".conv"; *bn = name + ".bn";
    }
}
MtTensor fp_tensor(const FpView& v) {
    MtTensor t;
    t.buf = v.buf; t.C = v.C; t.ld = v.ld; t.coff = v.coff; t.H = v.H; t.W = v.W;
    return t;
}
}  // namespace

int mt_build_face_parse_graph(MtGraph* gp, const ltk_named_tensor* t, int n, int size, int max_images) {
    MtGraph& g = *gp;
    FpPlan pl;
    if (fp_plan(size, max_images, &pl, &g.err)) return -1;
    SD sd{t, n, ""};
    g.fp_size = size; g.fp_img_buf = pl.image_buf; g.fp_label_buf = pl.label_buf;
    g.no_rowgemm = true;
    for (size_t i = 0; i < pl.buf_elems.size(); ++i) {
        const bool bytes = (int)i == pl.image_buf || (int)i == pl.label_buf;
        g.buf_halfs.push_back(bytes ? (pl.buf_elems[i] + 1) / 2 : pl.buf_elems[i]);
    }
    constexpr float kBnEps = 1e-5f;                                // nn.BatchNorm2d's default, which the reference keeps
    for (size_t i = 0; i < pl.ops.size(); ++i) {
        const FpOp& p = pl.ops[i];
        const FpBind& b = pl.bind[i];
        const MtTensor x = fp_tensor(b.x), y = fp_tensor(b.y);
        if (p.type == 0 || p.type == 10) {
            std::string wk, bk;
            fp_keys(p.name, &wk, &bk);
            const float* w = sd.get(wk + ".weight", (size_t)p.cout * p.cin * p.k * p.k);
            if (!w) { g.err = sd.err; return -1; }
            std::vector<float> scale((size_t)p.cout, 1.f), shift((size_t)p.cout, 0.f);
            if (!bk.empty()) {
                const float* ga = sd.get(bk + ".weight", p.cout);
                const float* be = ga ? sd.get(bk + ".bias", p.cout) : nullptr;
                const float* mu = be ? sd.get(bk + ".running_mean", p.cout) : nullptr;
                const float* va = mu ? sd.get(bk + ".running_var", p.cout) : nullptr;
                if (!va) { g.err = sd.err; return -1; }
                fold_bn(ga, be, mu, va, nullptr, kBnEps, p.cout, scale.data(), shift.data());
            }
            if (p.type == 10) {
                if (p.cout != kStemCout || p.cin != 3 || p.k != 7) { g.err = p.name + ": not the stem parse_stem_kernel serves"; return -1; }
                std::vector<f16> wq(kStemWHalfs);
                parse_stem_pack(w, wq.data());
                MtOp op;
                op.type = OP_FP_STEM; op.fp_type = p.type; op.name = p.name; op.y = y;
                op.wvec = g.add_named_vec(p.name + ".wq", wq.data(), wq.size() * sizeof(f16));
                op.gamma = g.add_vec(scale.data(), p.cout);
                op.beta = g.add_vec(shift.data(), p.cout);
                if (op.wvec < 0 || op.gamma < 0 || op.beta < 0) return -4;
                g.ops.push_back(op);
                g.named[p.name] = y;
                g.macs += (double)p.cin * p.cout * p.k * p.k * y.P();
                continue;
            }
            const MtTensor r = fp_tensor(b.r);
            MtTensor xin = x;
            if (p.ups) { xin.H *= 2; xin.W *= 2; }        // the logical (upsampled) size the conv runs on; the view is the stored map
            if (xin.H != p.H || xin.W != p.W || y.H != p.Ho || y.W != p.Wo) { g.err = p.name + ": the bound maps are not the op's"; return -1; }
            if (g.add_conv(p.name, w, shift.data(), p.cin, p.cout, p.k, p.stride, p.pad, xin, y, b.r.buf >= 0 ? &r : nullptr, p.relu ? 1 : 0, p.ups,
                           scale.data()))
                return -1;
            g.ops.back().fp_type = 0;
            // conv3 under its own rule, as the conv planner is held to for every conv of the list (tests/test_faceparse_host.py): not the
            // U-Net's measured forced tiles (and no row-GEMM form for ffm.conv2's 64 -> 256 channels on one pixel: no_rowgemm above)
            g.ops.back().unet3x3 = false;
            continue;
        }
        MtOp op;
        op.fp_type = p.type; op.name = p.name; op.x = x; op.y = y;
        if (p.type == 11) op.type = OP_FP_MAXPOOL;
        else if (p.type == 12) op.type = OP_FP_GAP;
        else if (p.type == 13) {
            op.type = OP_FP_GATE; op.plus1 = p.plus1;
            op.ga = fp_tensor(b.a); op.gb = fp_tensor(b.b); op.r = fp_tensor(b.r);
            // launch_chan_gate reads the attention and the added value as dense tensors
            if (op.ga.buf < 0 || op.ga.coff || op.ga.ld != x.C || (op.gb.buf >= 0 && (op.gb.coff || op.gb.ld != x.C))) {
                g.err = p.name + ": the gate's attention / broadcast operand is not a dense tensor of its channels";
                return -1;
            }
        } else if (p.type == 14) {
            op.type = OP_FP_LABELS;
            op.y = MtTensor();                    // bytes in fp_label_buf: no fp16 output tensor (nothing to scan, nothing to read back)
            if (x.ld != 32 || x.coff || x.C != 32) { g.err = p.name + ": the logits must be a dense 32-channel tensor"; return -1; }
        } else { g.err = p.name + ": unknown op type"; return -1; }
        g.ops.push_back(op);
        if (p.type != 14) g.named[p.name] = y;
    }
    return mt_graph_alloc(g, max_images);
}
uint8_t* mt_face_parse_image_in(MtGraph* g) { return reinterpret_cast<uint8_t*>(g->bufs[g->fp_img_buf]); }
const uint8_t* mt_face_parse_labels(MtGraph* g) { return reinterpret_cast<const uint8_t*>(g->bufs[g->fp_label_buf]); }

// ------------------------------------------------------------------------------------------ face detector (avatar preparation: face boxes)
// S3FD (avatars/wav2lip/face_detection/detection/sfd/net_s3fd.py) + batch_detect's per-level work (detect.py:71-89) as the 39 launches
// of fd_program, wired by fd_plan (facedet.h) and by nothing else.  Convs are the library's with the conv bias as the epilogue's fp32
// shift and the ReLU folded; a level's conf and loc convs are stacked into ONE conv of 16 outputs (conf rows at 0.., loc rows at 4..7,
// zero rows and zero biases elsewhere), 6 launches instead of 12.
int mt_build_face_detect_graph(MtGraph* gp, const MtGraph* share, const ltk_named_tensor* t, int n, int H, int W, int max_images, bool allocate) {
    MtGraph& g = *gp;
    FdPlan pl;
    if (fd_plan(H, W, max_images, &pl, &g.err)) return -1;
    SD sd{t, n, ""};
    g.share = share;
    g.fd_H = H; g.fd_W = W; g.fd_img_buf = pl.image_buf; g.fd_cap = kFdDevCap;
    g.no_rowgemm = true;
    for (size_t i = 0; i < pl.buf_elems.size(); ++i) g.buf_halfs.push_back((int)i == pl.image_buf ? (pl.buf_elems[i] + 1) / 2 : pl.buf_elems[i]);
    g.fd_rec_buf = pl.rec_buf;
    auto tensor = [](const FdView& v) {
        MtTensor x;
        x.buf = v.buf; x.C = v.C; x.ld = v.ld; x.coff = v.coff; x.H = v.H; x.W = v.W;
        return x;
    };
    for (size_t i = 0; i < pl.ops.size(); ++i) {
        const FdOp& p = pl.ops[i];
        const MtTensor x = tensor(pl.bind[i].x), y = tensor(pl.bind[i].y);
        if (p.type == 20) {
            if (p.cout != kFdStemCout || p.cin != 3 || p.k != 3) { g.err = p.name + ": not the stem s3fd_stem_kernel serves"; return -1; }
            std::vector<f16> wq(kFdStemWHalfs);
            const float* b = nullptr;
            if (!share) {
                const float* w = sd.get(p.name + ".weight", (size_t)p.cout * p.cin * 9);
                b = w ? sd.get(p.name + ".bias", p.cout) : nullptr;
                if (!b) { g.err = sd.err; return -1; }
                s3fd_stem_pack(w, wq.data());
            }
            MtOp op;
            op.type = OP_FD_STEM; op.fp_type = p.type; op.name = p.name; op.y = y;
            op.wvec = g.add_named_vec(p.name + ".wq", wq.data(), wq.size() * sizeof(f16));
            op.beta = g.add_named_vec(p.name + ".bias", b, (size_t)p.cout * sizeof(float));
            if (op.wvec < 0 || op.beta < 0) return share ? -1 : -4;
            g.ops.push_back(op);
            g.named[p.name] = y;
            g.macs += (double)p.cin * p.cout * 9 * y.P();
        } else if (p.type == 0) {
            std::vector<float> wm, bm;
            const float *w = nullptr, *b = nullptr;
            if (!share && p.level < 0) {
                w = sd.get(p.name + ".weight", (size_t)p.cout * p.cin * p.k * p.k);
                b = w ? sd.get(p.name + ".bias", p.cout) : nullptr;
                if (!b) { g.err = sd.err; return -1; }
            } else if (!share) {
                const int nconf = p.maxout ? 4 : 2;
                const size_t row = (size_t)p.cin * 9;
                const float* wc = sd.get(p.name + "_conf.weight", nconf * row);
                const float* bc = wc ? sd.get(p.name + "_conf.bias", nconf) : nullptr;
                const float* wl = bc ? sd.get(p.name + "_loc.weight", 4 * row) : nullptr;
                const float* bl = wl ? sd.get(p.name + "_loc.bias", 4) : nullptr;
                if (!bl) { g.err = sd.err; return -1; }
                wm.assign(16 * row, 0.f); bm.assign(16, 0.f);
                memcpy(wm.data(), wc, nconf * row * sizeof(float)); memcpy(bm.data(), bc, nconf * sizeof(float));
                memcpy(wm.data() + 4 * row, wl, 4 * row * sizeof(float)); memcpy(bm.data() + 4, bl, 4 * sizeof(float));
                w = wm.data(); b = bm.data();
            }
            if (x.H != p.H || x.W != p.W || y.H != p.Ho || y.W != p.Wo) { g.err = p.name + ": the bound maps are not the op's"; return -1; }
            if (g.add_conv(p.name, w, b, p.cin, p.cout, p.k, p.stride, p.pad, x, y, nullptr, p.relu ? 1 : 0, 0)) return -1;
            g.ops.back().fp_type = 0;
            g.ops.back().unet3x3 = false;           // conv3 under its own rule, as the conv planner is held to for every conv of the list
            g.ops.back().own_split = true;          // an image's records must not depend on the images beside it
        } else {
            MtOp op;
            op.fp_type = p.type; op.name = p.name; op.x = x; op.y = y;
            if (p.type == 21) op.type = OP_FD_POOL;
            else if (p.type == 22) {
                op.type = OP_FD_L2NORM;
                const float* w = share ? nullptr : sd.get(p.name + ".weight", p.cin);
                if (!share && !w) { g.err = sd.err; return -1; }
                op.gamma = g.add_named_vec(p.name + ".weight", w, (size_t)p.cin * sizeof(float));
                if (op.gamma < 0) return share ? -1 : -4;
            } else if (p.type == 23) {
                op.type = OP_FD_DETECT; op.fd_level = p.level; op.fd_maxout = p.maxout;
                op.y = MtTensor();                  // records in fd_rec_buf: no fp16 output tensor (nothing to scan, nothing to read back)
                if (x.ld != 16 || x.coff || x.C != 16) { g.err = p.name + ": the head map must be a dense 16-channel tensor"; return -1; }
            } else { g.err = p.name + ": unknown op type"; return -1; }
            g.ops.push_back(op);
            if (p.type != 23) g.named[p.name] = y;
        }
    }
    return allocate ? mt_graph_alloc(g, max_images) : 0;
}
uint8_t* mt_face_detect_image_in(MtGraph* g) { return reinterpret_cast<uint8_t*>(g->bufs[g->fd_img_buf]); }
uint8_t* mt_face_detect_records(MtGraph* g) { return reinterpret_cast<uint8_t*>(g->bufs[g->fd_rec_buf]); }
bool mt_face_detect_thresh_is(const MtGraph* g, float thresh) { return g->fd_thresh == thresh; }
void mt_face_detect_set_thresh(MtGraph* g, float thresh) { g->fd_thresh = thresh; }
int mt_named_writers(MtGraph* g, const char* name) {
    auto it = g->named.find(name);
    if (it == g->named.end()) return 0;
    int n = 0;
    for (const MtOp& op : g->ops) n += op.y.buf == it->second.buf;
    return n;
}

}  // namespace ltk

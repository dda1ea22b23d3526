// Whisper encoder as a device program over MtGraph (mt_graph.h):
// transformers WhisperEncoder (whisper-tiny: d 384, 4 layers, 6 heads, ffn 1536), the Audio2Feature model
// (avatars/musetalk/whisper/audio2feature.py:15-23,106-117).  In-tree statement of the same encoder:
// avatars/musetalk/whisper/whisper/model.py (AudioEncoder, ResidualAttentionBlock).  state_dict = model.encoder's.
// x: log-mel [80][3000] as a [3000][1] token map.  states[5] = hidden_states (embeddings, layers 0-2, final LN).
#include <math.h>

#include <algorithm>

#include "mt_graph.h"

namespace ltk {

namespace {

// A graph with `share` set (the batched program, mt_build_whisper_batch_graph) has no state dict: its convs take the owner's plans
// by name (add_conv_shared), and what the owner holds as unnamed vectors - the LayerNorms' affine pairs, the position table - is
// taken from the owner's op of the same name.  Handles are copied, nothing is freed twice (mt_graph_free).
const MtOp* wh_owner_op(MtGraph& g, const std::string& name, MtOpType type) {
    for (const MtOp& o : g.share->ops)
        if (o.type == type && o.name == name) return &o;
    g.err = "the shared weights have no " + name;
    return nullptr;
}
int wh_shared_vec(MtGraph& g, int owner_vec) {
    g.vecs.push_back(g.share->vecs[owner_vec]);
    return (int)g.vecs.size() - 1;
}
int wh_ln(MtGraph& g, SD& sd, const std::string& name, const MtTensor& x, const MtTensor& y) {
    if (!g.share) return g.add_ln(name, sd, name, x, y, 1e-5f);
    const MtOp* o = wh_owner_op(g, name, OP_LN);
    if (!o) return -1;
    MtOp op;
    op.type = OP_LN; op.name = name; op.x = x; op.y = y; op.eps = o->eps;
    op.gamma = wh_shared_vec(g, o->gamma); op.beta = wh_shared_vec(g, o->beta);
    g.ops.push_back(op);
    g.named[name] = y;
    return 0;
}

}  // namespace

int mt_build_whisper(MtGraph& g, const ltk_named_tensor* t, int n, MtTensor* mel_in, MtTensor states[5], int* pos_vec) {
    SD sd{t, n, ""};
    const int D = 384, L = 4, HEADS = 6, FF = 1536, T0 = 3000, T = 1500;
    *mel_in = g.alloc(80, T0, 1);
    g.named["input_features"] = *mel_in;
    const float *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr, *pos = nullptr;
    if (!g.share) {
        w1 = sd.get("conv1.weight", (size_t)D * 80 * 3);
        b1 = sd.get("conv1.bias", D);
        w2 = sd.get("conv2.weight", (size_t)D * D * 3);
        b2 = sd.get("conv2.bias", D);
        pos = sd.get("embed_positions.weight", (size_t)T * D);
        if (!w1 || !b1 || !w2 || !b2 || !pos) { g.err = sd.err; return -1; }
    }
    MtTensor c1 = g.alloc(D, T0, 1), h = g.alloc(D, T, 1);
    if (g.add_conv2("conv1", w1, b1, 80, D, 3, 1, 1, 1, 1, 0, *mel_in, c1, nullptr, 2, 0)) return -1;     // GELU
    if (g.add_conv2("conv2", w2, b2, D, D, 3, 1, 2, 1, 1, 0, c1, h, nullptr, 2, 0)) return -1;            // stride 2, GELU
    if (g.share) {
        const MtOp* o = wh_owner_op(g, "embed_positions", OP_ADDPOS);
        if (!o) return -1;
        *pos_vec = wh_shared_vec(g, o->gamma);
    } else {
        *pos_vec = g.add_vec(pos, T * D);
    }
    {
        MtOp op;
        op.type = OP_ADDPOS; op.name = "embed_positions"; op.x = h; op.y = h; op.gamma = *pos_vec;
        g.ops.push_back(op);
        g.named["embed_positions"] = h;
    }
    states[0] = h;
    for (int l = 0; l < L; ++l) {
        const std::string p = "layers." + std::to_string(l);
        MtTensor n1 = g.alloc(D, T, 1), h1 = g.alloc(D, T, 1);
        if (wh_ln(g, sd, p + ".self_attn_layer_norm", h, n1)) return -1;
        // WhisperAttention: q (bias, scaled by d^-0.5), k (no bias), v (bias), out (bias)
        const int d = D / HEADS;
        const float scale = 1.0f / sqrtf((float)d);
        const float *wk = nullptr, *wv = nullptr, *bv = nullptr, *wo = nullptr, *bo = nullptr;
        std::vector<float> wqs((size_t)D * D), bqs(D);
        if (!g.share) {
            const float* wq = sd.get(p + ".self_attn.q_proj.weight", (size_t)D * D);
            const float* bq = sd.get(p + ".self_attn.q_proj.bias", D);
            wk = sd.get(p + ".self_attn.k_proj.weight", (size_t)D * D);
            wv = sd.get(p + ".self_attn.v_proj.weight", (size_t)D * D);
            bv = sd.get(p + ".self_attn.v_proj.bias", D);
            wo = sd.get(p + ".self_attn.out_proj.weight", (size_t)D * D);
            bo = sd.get(p + ".self_attn.out_proj.bias", D);
            if (!wq || !bq || !wk || !wv || !bv || !wo || !bo) { g.err = sd.err; return -1; }
            for (size_t i = 0; i < wqs.size(); ++i) wqs[i] = wq[i] * scale;
            for (int i = 0; i < D; ++i) bqs[i] = bq[i] * scale;
        }
        MtTensor q = g.alloc(D, T, 1), k = g.alloc(D, T, 1), v = g.alloc(D, T, 1), o = g.alloc(D, T, 1);
        if (g.add_conv(p + ".self_attn.q_proj", wqs.data(), bqs.data(), D, D, 1, 1, 0, n1, q, nullptr, 0, 0)) return -1;
        if (g.add_conv(p + ".self_attn.k_proj", wk, nullptr, D, D, 1, 1, 0, n1, k, nullptr, 0, 0)) return -1;
        if (g.add_conv(p + ".self_attn.v_proj", wv, bv, D, D, 1, 1, 0, n1, v, nullptr, 0, 0)) return -1;
        g.add_attn(p + ".self_attn", q, k, v, o, HEADS, d);
        if (g.add_conv(p + ".self_attn.out_proj", wo, bo, D, D, 1, 1, 0, o, h1, &h, 0, 0)) return -1;
        MtTensor n2 = g.alloc(D, T, 1), f1 = g.alloc(FF, T, 1), h2 = g.alloc(D, T, 1);
        if (wh_ln(g, sd, p + ".final_layer_norm", h1, n2)) return -1;
        const float *wf1 = nullptr, *bf1 = nullptr, *wf2 = nullptr, *bf2 = nullptr;
        if (!g.share) {
            wf1 = sd.get(p + ".fc1.weight", (size_t)FF * D);
            bf1 = sd.get(p + ".fc1.bias", FF);
            wf2 = sd.get(p + ".fc2.weight", (size_t)D * FF);
            bf2 = sd.get(p + ".fc2.bias", D);
            if (!wf1 || !bf1 || !wf2 || !bf2) { g.err = sd.err; return -1; }
        }
        if (g.add_conv(p + ".fc1", wf1, bf1, D, FF, 1, 1, 0, n2, f1, nullptr, 2, 0)) return -1;               // GELU
        if (g.add_conv(p + ".fc2", wf2, bf2, FF, D, 1, 1, 0, f1, h2, &h1, 0, 0)) return -1;
        h = h2;
        if (l + 1 < L) states[l + 1] = h;
    }
    MtTensor fin = g.alloc(D, T, 1);
    if (wh_ln(g, sd, "layer_norm", h, fin)) return -1;
    states[4] = fin;
    for (int i = 0; i < 5; ++i) g.named["hidden_states." + std::to_string(i)] = states[i];
    return 0;
}

int mt_build_whisper_graph(MtGraph* g, const ltk_named_tensor* sd, int n) {
    g->t_latent = new MtTensor();                       // reused as the log-mel input tensor
    g->whisper_states = new MtTensor[5];
    int pos_vec = -1;
    if (mt_build_whisper(*g, sd, n, g->t_latent, g->whisper_states, &pos_vec)) return -1;
    return mt_graph_alloc(*g, 1);
}
int mt_build_whisper_batch_graph(MtGraph* g, const MtGraph* single, int frames) {
    g->share = single;
    g->t_latent = new MtTensor();
    g->whisper_states = new MtTensor[5];
    int pos_vec = -1;
    if (mt_build_whisper(*g, nullptr, 0, g->t_latent, g->whisper_states, &pos_vec)) return -1;
    return mt_graph_alloc(*g, frames);
}
std::vector<WhisperRun> whisper_batch_plan(int nreq, int cap) {
    std::vector<WhisperRun> runs;
    for (int r0 = 0; r0 < nreq; r0 += cap) {
        WhisperRun run;
        run.first = r0; run.count = std::min(cap, nreq - r0); run.batched = run.count > 1;
        runs.push_back(run);
    }
    return runs;
}
f16* mt_whisper_state(MtGraph* g, int i, int* cbt, int* cb0) {
    const MtTensor& t = g->whisper_states[i];
    *cbt = t.ld / 16; *cb0 = t.coff / 16;
    return g->bufs[t.buf];
}

}  // namespace ltk

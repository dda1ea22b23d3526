// Host-side statement of the Wav2Lip-256 generator graph
// (avatars/wav2lip/models/wav2lip_v2.py:12-91, forward :123-163) as a static
// layer program over a device activation arena: every layer is one launch of
// the MFMA implicit-GEMM kernels (conv3_mfma.hip / conv_mfma.hip); torch.cat skip
// connections are channel-block ranges of shared CB16 buffers; eval-mode BatchNorm
// is folded into the epilogue scale/shift at load time.
#include "engine_internal.h"

namespace {

// ---------------------------------------------------------------- network description
struct LayerDef {
    const char* prefix;
    bool transposed;
    int cin, cout, k, sh, sw, pad, out_pad;
    bool residual;
};

// wav2lip_v2.py:41-58
const LayerDef kAudio[] = {
    {"audio_encoder.0", false, 1, 32, 3, 1, 1, 1, 0, false},
    {"audio_encoder.1", false, 32, 32, 3, 1, 1, 1, 0, true},
    {"audio_encoder.2", false, 32, 32, 3, 1, 1, 1, 0, true},
    {"audio_encoder.3", false, 32, 64, 3, 3, 1, 1, 0, false},
    {"audio_encoder.4", false, 64, 64, 3, 1, 1, 1, 0, true},
    {"audio_encoder.5", false, 64, 64, 3, 1, 1, 1, 0, true},
    {"audio_encoder.6", false, 64, 128, 3, 3, 3, 1, 0, false},
    {"audio_encoder.7", false, 128, 128, 3, 1, 1, 1, 0, true},
    {"audio_encoder.8", false, 128, 128, 3, 1, 1, 1, 0, true},
    {"audio_encoder.9", false, 128, 256, 3, 3, 2, 1, 0, false},
    {"audio_encoder.10", false, 256, 256, 3, 1, 1, 1, 0, true},
    {"audio_encoder.11", false, 256, 512, 3, 1, 1, 0, 0, false},
    {"audio_encoder.12", false, 512, 512, 1, 1, 1, 0, 0, false},
};
// wav2lip_v2.py:12-39 (blocks separated by block index)
struct BlockLayer { int block; LayerDef d; };
const BlockLayer kFaceEnc[] = {
    {0, {"face_encoder_blocks.0.0", false, 6, 16, 7, 1, 1, 3, 0, false}},
    {1, {"face_encoder_blocks.1.0", false, 16, 32, 3, 2, 2, 1, 0, false}},
    {1, {"face_encoder_blocks.1.1", false, 32, 32, 3, 1, 1, 1, 0, true}},
    {1, {"face_encoder_blocks.1.2", false, 32, 32, 3, 1, 1, 1, 0, true}},
    {2, {"face_encoder_blocks.2.0", false, 32, 64, 3, 2, 2, 1, 0, false}},
    {2, {"face_encoder_blocks.2.1", false, 64, 64, 3, 1, 1, 1, 0, true}},
    {2, {"face_encoder_blocks.2.2", false, 64, 64, 3, 1, 1, 1, 0, true}},
    {2, {"face_encoder_blocks.2.3", false, 64, 64, 3, 1, 1, 1, 0, true}},
    {3, {"face_encoder_blocks.3.0", false, 64, 128, 3, 2, 2, 1, 0, false}},
    {3, {"face_encoder_blocks.3.1", false, 128, 128, 3, 1, 1, 1, 0, true}},
    {3, {"face_encoder_blocks.3.2", false, 128, 128, 3, 1, 1, 1, 0, true}},
    {4, {"face_encoder_blocks.4.0", false, 128, 256, 3, 2, 2, 1, 0, false}},
    {4, {"face_encoder_blocks.4.1", false, 256, 256, 3, 1, 1, 1, 0, true}},
    {4, {"face_encoder_blocks.4.2", false, 256, 256, 3, 1, 1, 1, 0, true}},
    {5, {"face_encoder_blocks.5.0", false, 256, 512, 3, 2, 2, 1, 0, false}},
    {5, {"face_encoder_blocks.5.1", false, 512, 512, 3, 1, 1, 1, 0, true}},
    {6, {"face_encoder_blocks.6.0", false, 512, 512, 3, 2, 2, 1, 0, false}},
    {6, {"face_encoder_blocks.6.1", false, 512, 512, 3, 1, 1, 1, 0, true}},
    {7, {"face_encoder_blocks.7.0", false, 512, 512, 4, 1, 1, 0, 0, false}},
    {7, {"face_encoder_blocks.7.1", false, 512, 512, 1, 1, 1, 0, 0, false}},
};
// wav2lip_v2.py:60-87
const BlockLayer kFaceDec[] = {
    {0, {"face_decoder_blocks.0.0", false, 512, 512, 1, 1, 1, 0, 0, false}},
    {1, {"face_decoder_blocks.1.0", true, 1024, 512, 4, 1, 1, 0, 0, false}},
    {1, {"face_decoder_blocks.1.1", false, 512, 512, 3, 1, 1, 1, 0, true}},
    {2, {"face_decoder_blocks.2.0", true, 1024, 512, 3, 2, 2, 1, 1, false}},
    {2, {"face_decoder_blocks.2.1", false, 512, 512, 3, 1, 1, 1, 0, true}},
    {3, {"face_decoder_blocks.3.0", true, 1024, 512, 3, 2, 2, 1, 1, false}},
    {3, {"face_decoder_blocks.3.1", false, 512, 512, 3, 1, 1, 1, 0, true}},
    {3, {"face_decoder_blocks.3.2", false, 512, 512, 3, 1, 1, 1, 0, true}},
    {4, {"face_decoder_blocks.4.0", true, 768, 384, 3, 2, 2, 1, 1, false}},
    {4, {"face_decoder_blocks.4.1", false, 384, 384, 3, 1, 1, 1, 0, true}},
    {4, {"face_decoder_blocks.4.2", false, 384, 384, 3, 1, 1, 1, 0, true}},
    {5, {"face_decoder_blocks.5.0", true, 512, 256, 3, 2, 2, 1, 1, false}},
    {5, {"face_decoder_blocks.5.1", false, 256, 256, 3, 1, 1, 1, 0, true}},
    {5, {"face_decoder_blocks.5.2", false, 256, 256, 3, 1, 1, 1, 0, true}},
    {6, {"face_decoder_blocks.6.0", true, 320, 128, 3, 2, 2, 1, 1, false}},
    {6, {"face_decoder_blocks.6.1", false, 128, 128, 3, 1, 1, 1, 0, true}},
    {6, {"face_decoder_blocks.6.2", false, 128, 128, 3, 1, 1, 1, 0, true}},
    {7, {"face_decoder_blocks.7.0", true, 160, 64, 3, 2, 2, 1, 1, false}},
    {7, {"face_decoder_blocks.7.1", false, 64, 64, 3, 1, 1, 1, 0, true}},
    {7, {"face_decoder_blocks.7.2", false, 64, 64, 3, 1, 1, 1, 0, true}},
};
const LayerDef kOutConv = {"output_block.0", false, 80, 32, 3, 1, 1, 1, 0, false};  // wav2lip_v2.py:89
const float kBnEps = 1e-5f;  // nn.BatchNorm2d default (conv.py:9,38)

int frame_bucket(int nf) { return nf <= 16 ? 0 : nf <= 32 ? 1 : nf <= 64 ? 2 : nf <= 128 ? 3 : 4; }

// Per-layer tile / split choices that beat conv3's rule inside a whole pass (scripts/tile_tune.py on MI355X,
// profiles/r02_tile_tune.txt: every layer timed between its neighbours, so with the cache state they leave).  Tiles never
// change an output element's summation order; the few split entries replace the split the rule would have chosen.
struct TileEntry { const char* layer; int bucket, pxw, nbt, ks; };
const TileEntry kTileTable[] = {
    // <= 16 frames per launch
    {"face_encoder_blocks.5.1", 0, 2, 1, 0},     // 512 ch @ 8^2: 27.7 -> 22.6 us (half the weight-slab re-reads of 128-px tiles)
    {"face_decoder_blocks.2.1", 0, 2, 1, 0},     // 512 ch @ 8^2: 28.1 -> 22.9 us
    {"face_encoder_blocks.6.0", 0, 0, 0, 8},     // 512 -> 512 stride 2 @ 8^2: 20.7 -> 18.1 us
    {"face_decoder_blocks.1.0", 0, 0, 0, 4},     // convT 4x4 on the 1x1 map: 20.9 -> 18.0 us
    {"audio_encoder.7", 0, 0, 0, 1},             // 128 ch @ 9x6: 14.1 -> 12.0 us unsplit
    {"audio_encoder.8", 0, 0, 0, 1},
    // <= 64 frames per launch
    {"face_decoder_blocks.4.1", 2, 2, 2, 0},     // 384 ch @ 32^2: 182 -> 150 us
    {"face_decoder_blocks.4.2", 2, 2, 2, 0},
    {"face_encoder_blocks.5.0", 2, 2, 1, 0},     // 256 -> 512 stride 2: 33.6 -> 26.5 us
    {"face_encoder_blocks.6.1", 2, 1, 2, 0},     // 512 ch @ 4^2: 29.0 -> 24.3 us
    {"face_decoder_blocks.1.1", 2, 1, 2, 0},     // 512 ch @ 4^2: 29.4 -> 23.2 us
    {"face_decoder_blocks.1.0", 2, 0, 0, 4},
};

// Device-free consistency check of kTileTable (include/ltk.h ltk_debug_tile_table_check): every entry names a layer of the network
// description above, a frame-count bucket, and a tile / split conv3 has an instantiation for on that layer.  The table is keyed by
// strings and was tuned on single boxes: an entry that no longer matches anything would cost speed silently.
int check_tile_table_impl(std::string& msg) {
    int bad = 0;
    auto find = [](const char* name) -> const LayerDef* {
        for (const LayerDef& d : kAudio) if (!strcmp(d.prefix, name)) return &d;
        for (const BlockLayer& b : kFaceEnc) if (!strcmp(b.d.prefix, name)) return &b.d;
        for (const BlockLayer& b : kFaceDec) if (!strcmp(b.d.prefix, name)) return &b.d;
        if (!strcmp(kOutConv.prefix, name)) return &kOutConv;
        return nullptr;
    };
    const size_t n = sizeof(kTileTable) / sizeof(kTileTable[0]);
    for (size_t i = 0; i < n; ++i) {
        const TileEntry& t = kTileTable[i];
        auto complain = [&](const char* what) { ++bad; msg += std::string(t.layer) + " (bucket " + std::to_string(t.bucket) + "): " + what + "; "; };
        const LayerDef* d = find(t.layer);
        if (!d) { complain("no such layer"); continue; }
        if (t.bucket < 0 || t.bucket >= 5) complain("bucket outside 0..4");
        if ((t.pxw == 0) != (t.nbt == 0)) complain("pxw and nbt must be given together");
        if (t.pxw != 0 && t.pxw != 1 && t.pxw != 2 && t.pxw != 4) complain("pxw must be 0, 1, 2 or 4");
        if (t.nbt < 0 || t.nbt > 2) complain("nbt must be 0, 1 or 2");
        if (t.ks < 0 || t.ks > 32) complain("split factor outside 0..32");
        if (t.pxw == 0 && t.nbt == 0 && t.ks == 0) complain("entry changes nothing");
        const bool s1_3x3 = !d->transposed && d->k == 3 && d->sh == 1 && d->sw == 1;
        if ((t.pxw == 1 || t.pxw == 4) && !s1_3x3) complain("128- / 512-pixel tiles exist for 3x3 stride-1 layers only");
        if (t.pxw == 4 && d->cout > 32) complain("512-pixel tiles exist for <= 32 output channels only");
        if (t.nbt == 2 && d->cout < 64) complain("64-cout blocks need >= 64 output channels");
        if (d->k == 7) complain("the first layer runs on conv7, not conv3");
        for (size_t j = 0; j < i; ++j)
            if (!strcmp(kTileTable[j].layer, t.layer) && kTileTable[j].bucket == t.bucket) complain("duplicate entry");
    }
    return bad;
}

void apply_tile_table_impl(std::vector<Layer>& layers) {
    for (const TileEntry& t : kTileTable)
        for (Layer& L : layers)
            if (L.name == t.layer) { L.tile[t.bucket].pxw = (signed char)t.pxw; L.tile[t.bucket].nbt = (signed char)t.nbt; L.tile[t.bucket].ks = (signed char)t.ks; }
}


// `hint_hw`: pixels per image of the layer's input map.  `flat_ld` > 0: the k x k "valid" conv that collapses a
// k x k map to 1x1 (face_encoder_blocks.7.0) is run as a 1x1 conv over the map viewed as ONE pixel of
// k*k*cin channels (a channel-blocked k x k map is contiguous per channel block).
// `map_w` > 0: the input map is map_w x map_w (face encoder / decoder): 3x3 layers whose OUTPUT map is at most 8 x 8 also get a rowconv plan.
int build_layer_impl(ltk_engine* e, const LayerDef& d, const ltk_named_tensor* sd, int n, Layer* L, int hint_hw, int flat_ld, int map_w) {
    const std::string p = d.prefix;
    const size_t wcount = (size_t)d.cin * d.cout * d.k * d.k;
    SD dict{sd, n, ""};
    const float* w = dict.get(p + ".conv_block.0.weight", wcount);
    const float* b = dict.get(p + ".conv_block.0.bias", d.cout);
    const float* g = dict.get(p + ".conv_block.1.weight", d.cout);
    const float* beta = dict.get(p + ".conv_block.1.bias", d.cout);
    const float* mean = dict.get(p + ".conv_block.1.running_mean", d.cout);
    const float* var = dict.get(p + ".conv_block.1.running_var", d.cout);
    if (!w || !b || !g || !beta || !mean || !var)
        return fail(LTK_E_INVALID, "state_dict is missing (or has a wrong shape for) tensors of layer " + p);
    std::vector<float> sc(d.cout), sf(d.cout);
    fold_bn(g, beta, mean, var, b, kBnEps, d.cout, sc.data(), sf.data());
    std::string err;
    int rc;
    // Residual blocks (conv.py:16-17: out = relu(bn(conv(x)) + x), x = the block's own input): with
    // y = s*conv(x) + t + x the identity is the centre tap of a k x k kernel, w[co][co][c][c] += 1/s[co].
    // The accumulation is fp32 and the fp16 rounding of (w + 1/s) perturbs the identity term by one fp16 ulp of
    // x - the same error x already carries - while the separate residual read (one extra pass over the
    // activation) disappears.  Not applied when a scale is too small for 1/s to be a sane fp16 weight.
    std::vector<float> wfold;
    L->res_folded = false;
    if (d.residual && !d.transposed && d.cin == d.cout && (d.k & 1) && d.sh == 1 && d.sw == 1 && d.pad == d.k / 2) {
        bool ok = true;
        for (int c = 0; c < d.cout; ++c) ok = ok && fabsf(sc[c]) >= 1e-3f;
        if (ok) {
            wfold.assign(w, w + wcount);
            const int kk = d.k * d.k, ctr = (d.k / 2) * d.k + d.k / 2;
            for (int c = 0; c < d.cout; ++c) wfold[((size_t)c * d.cin + c) * kk + ctr] += 1.0f / sc[c];
            w = wfold.data();
            L->res_folded = true;
        }
    }
    if (flat_ld > 0) {
        // channel-blocked map [n][cb][k*k][16] read as ONE pixel of cin*k*k channels: flat channel = ((cb*kk + t)*16 + c16)
        const int kk = d.k * d.k;
        const int cin_flat = kk * d.cin;
        std::vector<float> wf((size_t)d.cout * cin_flat, 0.f);
        for (int co = 0; co < d.cout; ++co)
            for (int ci = 0; ci < d.cin; ++ci)
                for (int t = 0; t < kk; ++t)
                    wf[(size_t)co * cin_flat + ((size_t)(ci >> 4) * kk + t) * 16 + (ci & 15)] = w[((size_t)co * d.cin + ci) * kk + t];
        rc = conv_plan_create(&L->plan, wf.data(), cin_flat, d.cout, 1, 1, 1, 1, 0, 0, false, 0, sc.data(), sf.data(), &err);
    } else {
        rc = conv_plan_create(&L->plan, w, d.cin, d.cout, d.k, d.k, d.sh, d.sw, d.pad, d.pad, d.transposed, d.out_pad,
                              sc.data(), sf.data(), &err);
    }
    if (rc) return conv_status(rc, p + ": " + err);
    // one pixel per frame on both sides: a plain GEMM with as many rows as frames (rowgemm.hip, used for launches of <= 32 frames).
    // Not built (45 MB of duplicated weights) when the process starts with the paths switched off.
    const bool want_rowgemm = knob(K_ROWGEMM) && knob(K_SPLITK), want_rowconv = knob(K_ROWCONV) > 0 && knob(K_SPLITK);
    {
        std::vector<float> we, se, fe;
        int J = 0, K = 0;
        if (flat_ld > 0) {                                            // k x k valid conv collapsing the k x k map: W = the flattened weights above
            const int kk = d.k * d.k;
            J = d.cout; K = kk * d.cin;
            we.assign((size_t)J * K, 0.f);
            for (int co = 0; co < d.cout; ++co)
                for (int ci = 0; ci < d.cin; ++ci)
                    for (int t = 0; t < kk; ++t)
                        we[(size_t)co * K + ((size_t)(ci >> 4) * kk + t) * 16 + (ci & 15)] = w[((size_t)co * d.cin + ci) * kk + t];
            se = sc; fe = sf;
        } else if (!d.transposed && d.k == 1 && hint_hw == 1 && d.cin % 32 == 0 && d.cout % 16 == 0) {
            J = d.cout; K = d.cin;
            we.assign(w, w + (size_t)J * K);
            se = sc; fe = sf;
        } else if (d.transposed && hint_hw == 1 && d.sh == 1 && d.pad == 0 && d.out_pad == 0 && d.cin % 32 == 0 && d.cout % 16 == 0) {
            // ConvTranspose2d(k, 1, 0) on a 1x1 map: output channel-blocked k x k map [cout block][position][16] = k*k*Cout columns
            const int kk = d.k * d.k;
            J = kk * d.cout; K = d.cin;
            we.assign((size_t)J * K, 0.f); se.assign(J, 0.f); fe.assign(J, 0.f);
            for (int j = 0; j < J; ++j) {
                const int c16 = j & 15, tt = j >> 4, pos = tt % kk, co = (tt / kk) * 16 + c16;
                for (int ci = 0; ci < d.cin; ++ci) we[(size_t)j * K + ci] = w[((size_t)ci * d.cout + co) * kk + pos];
                se[j] = sc[co]; fe[j] = sf[co];
            }
        }
        if (J > 0 && !want_rowgemm) {
            // conv3 + split-K finish serves the layer
        } else if (J > 0) {
            rc = rowgemm_plan_create(&L->rg, we.data(), J, K, se.data(), fe.data(), &err);
            if (rc) return conv_status(rc, p + ": " + err);
            L->rg_y_ld = (d.transposed ? J : 0);
        } else if (want_rowconv && flat_ld == 0 && !d.transposed && d.k == 3 && d.pad == 1 && (d.cout % 256 == 0 || (map_w < 0 && d.cout == 128)) &&
                   ((map_w > 0 && d.sh == d.sw && (d.sh == 1 || d.sh == 2) && map_w % d.sh == 0 && map_w / d.sh <= 8 && (d.cin == 256 || d.cin == 512)) ||
                    // round 5: the audio encoder's last two 3 x 3 layers (audio_encoder.9: 128 -> 256, stride (3, 2), 9 x 6 -> 3 x 3; .10: 256 -> 256 on
                    // 3 x 3): 144 output pixels per 16-frame launch behind 0.6 / 1.2 MB of weights (map_w < 0: the caller vouches for a small map)
                    (map_w < 0 && d.cin % 32 == 0))) {
            // 3x3 conv whose output map is at most 8 x 8: W_eff[j][tap * Cin + c], tap = ky * 3 + kx (`w` carries the folded identity
            // of a residual layer, exactly as the conv3 plan above does)
            J = d.cout; K = 9 * d.cin;
            rowconv_weff(w, d.cin, d.cout, &we);
            rc = rowgemm_plan_create(&L->rg, we.data(), J, K, sc.data(), sf.data(), &err);
            if (rc) return conv_status(rc, p + ": " + err);
            L->rowconv = true;
            L->rc_stride = d.sh;
            L->rc_stride_w = d.sw;
        } else if (want_rowconv && map_w > 0 && map_w <= 8 && d.transposed && d.k == 3 && d.sh == 2 && d.sw == 2 && d.pad == 1 && d.out_pad == 1 &&
                   (d.cin == 256 || d.cin == 512 || d.cin == 1024) && d.cout % 256 == 0) {
            // stride-2 transposed conv on the 4x4 / 8x8 maps: one plan per output phase (rowconvT_weff, rowgemm.hip)
            for (int gph = 0; gph < 4; ++gph) {
                J = d.cout; K = (1 + (gph >> 1)) * (1 + (gph & 1)) * d.cin;
                rowconvT_weff(w, d.cin, d.cout, gph, &we);
                rc = rowgemm_plan_create(&L->rgT[gph], we.data(), J, K, sc.data(), sf.data(), &err);
                if (rc) return conv_status(rc, p + ": " + err);
            }
        }
    }
    if (!d.transposed && d.k == 7 && d.cin == 6 && d.cout == 16 && d.sh == 1 && d.pad == 3 && !e->c7) {
        rc = conv7_plan_create(&e->c7, w, sc.data(), sf.data(), &err);
        if (rc) return fail(LTK_E_HIP, p + ": " + err);
    }
    if (!d.transposed && d.k == 3 && d.cin == 1 && d.cout == 32 && d.sh == 1 && d.sw == 1 && d.pad == 1 && !d.residual && (knob(K_AUDIO0) & 1) && !e->a0) {
        rc = audio0_plan_create(&e->a0, w, sc.data(), sf.data(), &err);
        if (rc) return fail(LTK_E_HIP, p + ": " + err);
    }
    if (!d.transposed && d.k == 3 && d.cin == 32 && d.cout == 64 && d.sh == 3 && d.sw == 1 && d.pad == 1 && !d.residual && (knob(K_AUDIO0) & 2) && !e->a3) {
        rc = audio3_plan_create(&e->a3, w, sc.data(), sf.data(), &err);
        if (rc) return fail(LTK_E_HIP, p + ": " + err);
        L->special = 3;
    }
    if (!d.transposed && d.k == 3 && d.sh == 2 && d.sw == 2 && d.pad == 1 && !d.residual && (d.cin == 16 || d.cin == 32) && d.cout % 32 == 0 &&
        knob(K_CONV_S2D) && !L->s2d) {
        rc = convs2d_plan_create(&L->s2d, w, d.cin, d.cout, sc.data(), sf.data(), &err);
        if (rc) return conv_status(rc, p + ": " + err);
    }
    L->name = p;
    L->cin_real = d.cin;
    L->residual = d.residual;
    return 0;
}


// A Layer is pushed into e->layers only after it is complete: on a failure the device plans built so far go here (a failed load
// that is retried would otherwise leak the packed weights each time)
int build_layer(ltk_engine* e, const LayerDef& d, const ltk_named_tensor* sd, int n, Layer* L, int hint_hw = 0, int flat_ld = 0, int map_w = 0) {
    const int rc = build_layer_impl(e, d, sd, n, L, hint_hw, flat_ld, map_w);
    if (rc) {
        conv_plan_destroy(&L->plan); rowgemm_plan_destroy(&L->rg);
        for (RowGemmPlan& q : L->rgT) rowgemm_plan_destroy(&q);
        convs2d_plan_destroy(L->s2d); L->s2d = nullptr;
    }
    return rc;
}

void bump(size_t* cur, size_t v) { if (v > *cur) *cur = v; }

}  // namespace

namespace ltk {

// Everything ltk_wav2lip_load creates (layer plans, head weights, first-layer plan, activation arena): a failed load leaves
// the engine as it found it, and can be retried.
void wav2lip_unload(ltk_engine* e) {
    (void)drain_pending(e);                                  // knob DEFER: a pass still in flight works in the buffers that go away below
    if (e->aux2) (void)hipStreamSynchronize(e->aux2);        // an outstanding prefetch writes them too
    e->graphs.drop();
    e->hw_w2l.release(); e->w2l_scan = nullptr;
    if (e->d_tab) { (void)hipFree(e->d_tab); e->d_tab = nullptr; }
    for (Layer& L : e->layers) {
        conv_plan_destroy(&L.plan); rowgemm_plan_destroy(&L.rg);
        for (RowGemmPlan& q : L.rgT) rowgemm_plan_destroy(&q);
        convs2d_plan_destroy(L.s2d); L.s2d = nullptr;
    }
    e->layers.clear();
    for (int i = 0; i < B_COUNT; ++i) {
        if (e->buf[i]) { (void)hipFree(e->buf[i]); e->buf[i] = nullptr; }
        if (e->pf_tmp[i]) { (void)hipFree(e->pf_tmp[i]); e->pf_tmp[i] = nullptr; }
        for (ltk_engine::PfSlot& sl : e->pfs)
            if (sl.cat[i]) { (void)hipFree(sl.cat[i]); sl.cat[i] = nullptr; }
    }
    for (ltk_engine::PfSlot& sl : e->pfs) {
        if (sl.ev_done) (void)hipEventDestroy(sl.ev_done);
        if (sl.ev_read) (void)hipEventDestroy(sl.ev_read);
        sl = ltk_engine::PfSlot();
    }
    e->alt_frames = 0;
    for (ltk_engine::SoloSeq& q : e->solo_seq) q = ltk_engine::SoloSeq();
    if (e->d_tab_next) { (void)hipFree(e->d_tab_next); e->d_tab_next = nullptr; }
    if (e->d_head) { (void)hipFree(e->d_head); e->d_head = nullptr; }
    conv7_plan_destroy(e->c7);
    e->c7 = nullptr;
    audio0_plan_destroy(e->a0);
    e->a0 = nullptr;
    audio3_plan_destroy(e->a3);
    e->a3 = nullptr;
    e->loaded = false;
}

// Wire the layer program: buffers, channel offsets (torch.cat), spatial dims.
int build_program(ltk_engine* e, const ltk_named_tensor* sd, int n) {
    wav2lip_unload(e);
    size_t* bh = e->buf_halfs;
    for (int i = 0; i < B_COUNT; ++i) bh[i] = 0;
    bh[B_MEL] = 80 * 16 * 8;
    bh[B_X0] = 65536 * 8;
    bh[B_OUT32] = 65536 * 32;
    for (int k = 0; k < 8; ++k) {
        const int hw = kFeatHW[7 - k];
        bh[B_CAT0 + k] = (size_t)hw * hw * (kDecCh[k] + kFeatCh[7 - k]);
    }
    int rc;
    // ---- audio encoder (wav2lip_v2.py:132): MEL -> AT0/AT1 ping-pong
    {
        int H = 80, W = 16, in_buf = B_MEL, in_ld = 8, pp = 0;
        for (const LayerDef& d : kAudio) {
            Layer L;
            // audio_encoder.11: the 3x3 "valid" conv on the 3x3 map = a GEMM over the flattened map with one row per frame (K = 2304),
            // like face_encoder_blocks.7.0: rowgemm for launches of <= 32 frames (16 blocks of the first-generation kernel streamed its
            // 2.4 MB of weights in 26 us - the longest launch of the audio branch, which heads the critical path under knob PREFETCH)
            const bool flat = !d.transposed && d.pad == 0 && d.k > 1 && d.k == H && d.k == W && d.cin % 64 == 0;
            const int oh = (H + 2 * d.pad - d.k) / d.sh + 1, ow = (W + 2 * d.pad - d.k) / d.sw + 1;
            // audio_encoder.6 .. .10 (output maps 9 x 6 and 3 x 3: <= 864 rows per 16-frame launch): rowconv (build_layer) in launches of
            // <= ROWCONV rows, instead of the first-generation kernel / conv3 + split-K finish of rounds 1-4
            constexpr int kAudioRowconvMaxPixels = 54;
            const bool small = !flat && d.k == 3 && d.pad == 1 && oh * ow <= kAudioRowconvMaxPixels && d.cin % 32 == 0;
            if ((rc = build_layer(e, d, sd, n, &L, H * W, flat ? in_ld : 0, small ? -1 : 0))) return rc;
            L.audio = true;
            L.in_buf = in_buf; L.in_ld = in_ld; L.in_coff = 0; L.H = H; L.W = W;
            if (flat) { L.Ho = 1; L.Wo = 1; L.H = 1; L.W = 1; L.in_ld = d.k * d.k * in_ld; }
            else
            L.plan.out_dims(H, W, &L.Ho, &L.Wo);
            L.out_buf = B_AT0 + pp; L.out_ld = d.cout; L.out_coff = 0;
            bump(&bh[L.out_buf], (size_t)L.Ho * L.Wo * d.cout);
            L.macs = (double)d.cin * d.cout * d.k * d.k * L.Ho * L.Wo;
            e->layers.push_back(L);
            in_buf = L.out_buf; in_ld = d.cout; H = L.Ho; W = L.Wo; pp ^= 1;
        }
    }
    const int audio_emb_buf = e->layers.back().out_buf;
    // ---- face encoder (wav2lip_v2.py:136-140): block i ends in CAT[7-i] at channel offset dec_ch
    {
        int H = 256, W = 256, in_buf = B_X0, in_ld = 8, in_coff = 0, pp = 0;
        const int nl = (int)(sizeof(kFaceEnc) / sizeof(kFaceEnc[0]));
        for (int li = 0; li < nl; ++li) {
            const BlockLayer& bl = kFaceEnc[li];
            const bool last = (li + 1 == nl) || kFaceEnc[li + 1].block != bl.block;
            Layer L;
            // the 4x4 "valid" conv on the 4x4 map: a 1x1 conv over the flattened map (needs in_ld % 64 == 0)
            const bool flat = !bl.d.transposed && bl.d.pad == 0 && bl.d.k > 1 && bl.d.k == H && bl.d.k == W && bl.d.cin % 64 == 0;
            if ((rc = build_layer(e, bl.d, sd, n, &L, H * W, flat ? in_ld : 0, H == W ? W : 0))) return rc;
            L.in_buf = in_buf; L.in_ld = in_ld; L.in_coff = in_coff; L.H = H; L.W = W;
            if (flat) {
                L.Ho = 1; L.Wo = 1;
                L.H = 1; L.W = 1;                                      // one "pixel" per image
                L.in_ld = bl.d.k * bl.d.k * in_ld; L.in_coff = bl.d.k * bl.d.k * in_coff;
            } else {
                L.plan.out_dims(H, W, &L.Ho, &L.Wo);
            }
            if (last) {
                const int k = 7 - bl.block;
                L.out_buf = B_CAT0 + k; L.out_ld = kDecCh[k] + kFeatCh[bl.block]; L.out_coff = kDecCh[k];
                if (L.Ho != kFeatHW[bl.block] || bl.d.cout != kFeatCh[bl.block]) return fail(LTK_E_INVALID, "encoder geometry mismatch");
            } else {
                L.out_buf = B_T0 + pp; L.out_ld = bl.d.cout; L.out_coff = 0; pp ^= 1;
                bump(&bh[L.out_buf], (size_t)L.Ho * L.Wo * bl.d.cout);
            }
            L.macs = (double)bl.d.cin * bl.d.cout * bl.d.k * bl.d.k * L.Ho * L.Wo;
            L.face_enc = true;
            e->layers.push_back(L);
            in_buf = L.out_buf; in_ld = L.out_ld; in_coff = L.out_coff; H = L.Ho; W = L.Wo;
        }
    }
    // ---- decoder (wav2lip_v2.py:142-152): block k reads CAT[k-1] (all channels), ends in CAT[k][0:dec_ch)
    {
        int H = 1, W = 1, in_buf = audio_emb_buf, in_ld = 512, in_coff = 0, pp = 0;
        const int nl = (int)(sizeof(kFaceDec) / sizeof(kFaceDec[0]));
        for (int li = 0; li < nl; ++li) {
            const BlockLayer& bl = kFaceDec[li];
            const bool last = (li + 1 == nl) || kFaceDec[li + 1].block != bl.block;
            Layer L;
            if ((rc = build_layer(e, bl.d, sd, n, &L, H * W, 0, H == W ? W : 0))) return rc;
            L.in_buf = in_buf; L.in_ld = in_ld; L.in_coff = in_coff; L.H = H; L.W = W;
            L.plan.out_dims(H, W, &L.Ho, &L.Wo);
            if (last) {
                const int k = bl.block;
                L.out_buf = B_CAT0 + k; L.out_ld = kDecCh[k] + kFeatCh[7 - k]; L.out_coff = 0;
                if (L.Ho != kFeatHW[7 - k] || bl.d.cout != kDecCh[k]) return fail(LTK_E_INVALID, "decoder geometry mismatch");
            } else {
                L.out_buf = B_T0 + pp; L.out_ld = bl.d.cout; L.out_coff = 0; pp ^= 1;
                bump(&bh[L.out_buf], (size_t)L.Ho * L.Wo * bl.d.cout);
            }
            if (bl.d.transposed) L.macs = (double)bl.d.cin * bl.d.cout * bl.d.k * bl.d.k * H * W;
            else L.macs = (double)bl.d.cin * bl.d.cout * bl.d.k * bl.d.k * L.Ho * L.Wo;
            e->layers.push_back(L);
            in_buf = L.out_buf; in_ld = L.out_ld; in_coff = L.out_coff; H = L.Ho; W = L.Wo;
        }
    }
    // ---- output block conv (wav2lip_v2.py:89,154)
    {
        Layer L;
        if ((rc = build_layer(e, kOutConv, sd, n, &L, 65536))) return rc;
        L.in_buf = B_CAT0 + 7; L.in_ld = 80; L.in_coff = 0; L.H = 256; L.W = 256; L.Ho = 256; L.Wo = 256;
        L.out_buf = B_OUT32; L.out_ld = 32; L.out_coff = 0;
        L.macs = 80.0 * 32 * 9 * 65536;
        e->layers.push_back(L);
    }
    // head: plain nn.Conv2d(32,3,1) (wav2lip_v2.py:90)
    SD dict{sd, n, ""};
    const float* hw = dict.get("output_block.1.weight", 96);
    const float* hb = dict.get("output_block.1.bias", 3);
    if (!hw || !hb) return fail(LTK_E_INVALID, "state_dict is missing output_block.1.{weight,bias}");
    std::vector<float> h(99);
    memcpy(h.data(), hw, 96 * sizeof(float));
    memcpy(h.data() + 96, hb, 3 * sizeof(float));
    CHK(hipMalloc((void**)&e->d_head, 99 * sizeof(float)));
    CHK(hipMemcpy(e->d_head, h.data(), 99 * sizeof(float), hipMemcpyHostToDevice));
    e->macs_per_frame = 32.0 * 3 * 65536;
    for (const Layer& L : e->layers) e->macs_per_frame += L.macs;
    apply_tile_table_impl(e->layers);
    return 0;
}

// Enqueue the 54 conv/convT layers for frames [0, nf) of the arena on `s`.  The audio encoder has no
// dependency on the face encoder until decoder block 0 (wav2lip_v2.py:132-142): its 13 small launches run on
// the aux stream beside the face encoder instead of in front of it.
// `head_outs` != nullptr (a DEVICE table): the last layer (output_block.0) also applies the 1x1 head + sigmoid and writes the
// uint8 frames (one launch and one 4 MB/frame round trip of the 32-channel map less); the caller then skips launch_head.
// `evs` != nullptr (measurement): everything on `s`, one event in front of every layer and one behind the last.
// `faces` != nullptr (a DEVICE table): the first layer reads the uint8 bank crops itself (the caller then skips launch_pack_faces).
// Knob DF_FRAMES > 0: the decoder blocks >= DF_BLOCK and the output conv run depth-first over sub-batches of that many frames
// (all their layers for frames [f0, f0 + df), then the next sub-batch), so that a producer's output is still in the 256 MiB
// Infinity Cache when its consumer reads it; every layer sees the same frames with the same weights, only the launch size changes.
// `part`: 0 the whole network; 1 the face encoder only (builds the skip cache of knob FACE_CACHE: no audio branch, no decoder);
// 2 everything but the face encoder (its skip tensors are already in the concat buffers).
int run_convs(ltk_engine* e, int nf, hipStream_t s, const OutPtrs* head_outs, std::vector<hipEvent_t>* evs, const FacePtrs* faces, int part, int par,
              bool pf_enc) {
    // `par`: which set of concat buffers the launched layers use (0 = the arena's own, 1..kPfSlots = a prefetch slot, knob PREFETCH);
    // `pf_enc`: the launched layers are a prefetched face encoder running beside another call's decoder, with temporaries of its own
    auto B = [&](int id) -> f16* {
        if (id >= B_CAT0) return par ? e->pfs[par].cat[id] : e->buf[id];
        if (pf_enc && (id == B_X0 || id == B_T0 || id == B_T1)) return e->pf_tmp[id];
        return e->buf[id];
    };
    std::string err;
    const bool fork = !e->capture && e->aux && !evs && part != 1;
    size_t evi = 0;
    bool joined = !fork;
    if (fork) {
        CHK(hipEventRecord(e->ev_fork, s));
        CHK(hipStreamWaitEvent(e->aux, e->ev_fork, 0));
    }
    // enqueue order: the first two face-encoder launches go out before the 13 audio launches, so the main
    // stream is busy while the host is still issuing the small audio kernels (each launch costs the host
    // a few microseconds); stream order per stream is unchanged
    std::vector<Layer*> order;
    if (fork) {
        size_t first_face = 0;
        while (first_face < e->layers.size() && e->layers[first_face].audio) ++first_face;
        const size_t head = std::min(e->layers.size(), first_face + 2);
        for (size_t i = first_face; i < head; ++i) order.push_back(&e->layers[i]);
        for (size_t i = 0; i < first_face; ++i) order.push_back(&e->layers[i]);
        for (size_t i = head; i < e->layers.size(); ++i) order.push_back(&e->layers[i]);
    } else {
        for (Layer& L : e->layers) order.push_back(&L);
    }
    if (part != 0) {
        std::vector<Layer*> kept;
        for (Layer* L : order)
            if ((part == 1) == L->face_enc) kept.push_back(L);
        order.swap(kept);
    }
    constexpr int kRowConvTMaxRows = 512;      // measured (profiles/r04_rowconvT_ab.txt): 256 rows -7.5 us, 1024 rows +-0
    // one layer on frames [f0, f0 + n) of the arena
    auto launch_layer = [&](Layer& L, int f0, int n, bool on_aux) -> int {
        const int bucket = frame_bucket(n);
        ConvIO io;
        io.x = B(L.in_buf) + (size_t)f0 * L.in_ld * L.H * L.W; io.N = n; io.H = L.H; io.W = L.W; io.x_ld = L.in_ld; io.x_coff = L.in_coff;
        io.y = B(L.out_buf) + (size_t)f0 * L.out_ld * L.Ho * L.Wo; io.y_ld = L.out_ld; io.y_coff = L.out_coff;
        io.res = (L.residual && !L.res_folded) ? io.x : nullptr; io.res_ld = L.in_ld; io.res_coff = L.in_coff;
        io.relu = 1;
        io.partial = pf_enc ? e->d_partial_pf : on_aux ? e->d_partial_aux : e->d_partial;
        io.partial_cap = pf_enc ? e->partial_pf_cap : on_aux ? e->partial_aux_cap : e->partial_cap;
        if (head_outs && &L == &e->layers.back()) { io.head_w = e->d_head; io.head_outs = reinterpret_cast<const uint8_t* const*>(head_outs) + f0; }
        if (knob(K_TILE_TABLE)) { io.force_pxw = L.tile[bucket].pxw; io.force_nbt = L.tile[bucket].nbt; io.force_ksplit = L.tile[bucket].ks; }
        int rc;
        if (e->c7 && L.in_buf == B_X0)       // face_encoder_blocks.0.0
            rc = conv7_launch(e->c7, faces ? reinterpret_cast<const FacePtrs*>(reinterpret_cast<const uint8_t* const*>(faces) + f0) : nullptr,
                              B(B_X0) + (size_t)f0 * 65536 * 8, n, io.y, L.out_ld, L.out_coff, s, &err);
        else if (L.s2d && knob(K_CONV_S2D) && !(L.H & 1) && !(L.W & 63))                          // face_encoder_blocks.1.0 / 2.0
            rc = convs2d_launch(L.s2d, io.x, L.in_ld, L.in_coff, n, L.H, L.W, io.y, L.out_ld, L.out_coff, on_aux ? e->aux : s, &err);
        else if (e->a3 && (knob(K_AUDIO0) & 2) && L.special == 3 && L.H == 80 && L.W == 16)      // audio_encoder.3
            rc = audio3_launch(e->a3, io.x, L.in_ld, L.in_coff, n, io.y, L.out_ld, L.out_coff, on_aux ? e->aux : s, &err);
        else if (e->a0 && (knob(K_AUDIO0) & 1) && L.in_buf == B_MEL)  // audio_encoder.0: reads the float32 mel windows of the pass's table itself
            rc = audio0_launch(e->a0, reinterpret_cast<const MelPtrs*>(e->d_tab->mels.p + f0), n, io.y, L.out_ld, L.out_coff, on_aux ? e->aux : s, &err);
        // one-pixel maps: a skinny GEMM, no split-K finish launch.  Not under LTK_SPLITK=0, whose promise is ONE summation order per
        // output element whatever the launch's frame count (larger launches run these layers on conv3)
        else if (L.rowconv && L.rg.d_w && (long long)n * L.Ho * L.Wo <= std::min(knob(K_ROWCONV), kRowConvMaxRows) && knob(K_SPLITK)) {
            // 3x3 layers on the 4x4 / 8x8 maps: the same weight-streaming GEMM over gathered im2col rows (same LTK_SPLITK=0 rule)
            RowConvIO rio;
            rio.x = io.x; rio.x_ld = L.in_ld; rio.x_coff = L.in_coff; rio.H = L.H; rio.W = L.W;
            rio.y = io.y; rio.y_ld = L.out_ld; rio.y_coff = L.out_coff; rio.Ho = L.Ho; rio.Wo = L.Wo;
            rio.res = io.res; rio.res_ld = io.res_ld; rio.res_coff = io.res_coff;
            rio.N = n; rio.KW = 3; rio.stride = L.rc_stride; rio.stride_w = L.rc_stride_w; rio.pad = 1; rio.relu = 1;
            rc = rowconv_launch(L.rg, rio, on_aux ? e->aux : s, &err);
        } else if (L.rgT[0].d_w && (long long)n * L.H * L.W <= kRowConvTMaxRows && knob(K_ROWCONV) > 0 && knob(K_SPLITK)) {
            // stride-2 transposed convs on the 4x4 / 8x8 maps: four per-phase weight-streaming GEMMs in one launch (no split-K finish)
            // instead of conv3's merged-phase items, in launches of at most kRowConvTMaxRows SOURCE pixels (frames x H x W)
            RowConvIO rio;
            rio.x = io.x; rio.x_ld = L.in_ld; rio.x_coff = L.in_coff; rio.H = L.H; rio.W = L.W;
            rio.y = io.y; rio.y_ld = L.out_ld; rio.y_coff = L.out_coff; rio.Ho = L.Ho; rio.Wo = L.Wo;
            rio.N = n; rio.relu = 1;
            rc = rowconvT_launch(L.rgT, rio, on_aux ? e->aux : s, &err);
        } else if (!L.rowconv && L.rg.d_w && n <= kRowGemmMaxFrames && knob(K_ROWGEMM) && knob(K_SPLITK) &&
                   // the k x k expansion of a one-pixel map writes k*k*Cout contiguous columns per frame: only into a dense output
                   // (a CAT buffer's skip channels would be overwritten)
                   (L.rg_y_ld == 0 || (L.out_coff == 0 && L.out_ld * L.Ho * L.Wo == L.rg_y_ld)))
            rc = rowgemm_launch(L.rg, io.x, L.in_ld, L.in_coff, io.y, L.rg_y_ld ? L.rg_y_ld : L.out_ld, L.out_coff, n, 1,
                                on_aux ? e->aux : s, &err);
        else
            rc = conv_launch(L.plan, io, on_aux ? e->aux : s, &err);
        if (rc) return conv_status(rc, L.name + ": " + err);
        // a watched call (ltk_health_watch): this layer's record, on the layer's stream.  The fused head's 32-channel map never reaches
        // memory: that layer stays unobserved
        if (e->w2l_scan && !(io.head_w && io.head_outs))
            e->w2l_scan->scan((int)(&L - e->layers.data()), io.y, n, L.out_ld / 16, L.out_coff / 16, (L.plan.Cout + 15) / 16, (long long)L.Ho * L.Wo, 0,
                              on_aux ? e->aux : s);
        return 0;
    };
    // depth-first region: [df_first, end) of `order`
    const int df = (!e->capture && !evs && nf >= std::max(1, knob(K_DF_MIN))) ? knob(K_DF_FRAMES) : 0;
    size_t df_first = order.size();
    if (df > 0 && df < nf) {
        const std::string first_name = "face_decoder_blocks." + std::to_string(std::max(1, std::min(7, knob(K_DF_BLOCK)))) + ".0";
        for (size_t i = 0; i < order.size(); ++i)
            if (order[i]->name == first_name) { df_first = i; break; }
    }
    for (size_t oi = 0; oi < df_first; ++oi) {
        Layer& L = *order[oi];
        const bool on_aux = fork && L.audio;
        if (!on_aux && !joined && !L.audio && L.in_buf >= B_AT0 && L.in_buf <= B_AT1 && L.name.rfind("face_decoder", 0) == 0) {
            CHK(hipEventRecord(e->ev_join, e->aux));
            CHK(hipStreamWaitEvent(s, e->ev_join, 0));
            joined = true;
        }
        if (evs) CHK(hipEventRecord((*evs)[evi++], s));
        const int rc = launch_layer(L, 0, nf, on_aux);
        if (rc) return rc;
        if (e->capture) {
            const int C = L.plan.Cout;
            std::vector<float>& t = e->taps[L.name];
            t.resize((size_t)nf * C * L.Ho * L.Wo);
            float* d_tmp = nullptr;
            CHK(hipMalloc((void**)&d_tmp, t.size() * sizeof(float)));
            launch_nhwc_to_nchw_f32(e->buf[L.out_buf], nf, L.Ho, L.Wo, L.out_ld, L.out_coff, C, d_tmp, s);
            CHK(hipStreamSynchronize(s));
            CHK(hipMemcpy(t.data(), d_tmp, t.size() * sizeof(float), hipMemcpyDeviceToHost));
            CHK(hipFree(d_tmp));
            e->tap_shape[L.name] = {nf, C, L.Ho, L.Wo};
        }
    }
    if (!joined) {
        CHK(hipEventRecord(e->ev_join, e->aux));
        CHK(hipStreamWaitEvent(s, e->ev_join, 0));
    }
    for (int f0 = 0; df_first < order.size() && f0 < nf; f0 += df)
        for (size_t oi = df_first; oi < order.size(); ++oi) {
            const int rc = launch_layer(*order[oi], f0, std::min(df, nf - f0), false);
            if (rc) return rc;
        }
    if (evs) CHK(hipEventRecord((*evs)[evi++], s));
    return 0;
}

}  // namespace ltk

extern "C" {

int ltk_wav2lip_load(ltk_engine* e, const ltk_named_tensor* sd, int n, int max_frames) {
    if (!e || !sd || n <= 0) return fail(LTK_E_INVALID, "bad arguments");
    if (max_frames < 1 || max_frames > 4096) return fail(LTK_E_INVALID, "max_frames must be in [1, 4096]");
    std::lock_guard<std::mutex> g(e->mu);
    if (e->loaded) return fail(LTK_E_STATE, "a model is already loaded in this engine");
    CHK(enter_device(e->device));
    const int rc = [&]() -> int {
        const int brc = build_program(e, sd, n);
        if (brc) return brc;
        e->micro_batch = knob(K_MICROBATCH);
        if (e->micro_batch <= 0 || e->micro_batch > max_frames) e->micro_batch = max_frames;
        e->max_frames = max_frames;
        if (hipMalloc((void**)&e->d_tab, sizeof(DevTables)) != hipSuccess) return fail(LTK_E_NOMEM, "pointer table allocation failed");
        CHK(hipMemset(e->d_tab, 0, sizeof(DevTables)));
        const int arena_frames = e->micro_batch;
        for (int i = 0; i < B_COUNT; ++i) {
            if (!e->buf_halfs[i]) continue;
            const size_t bytes = e->buf_halfs[i] * arena_frames * sizeof(f16) + 4096;
            if (hipMalloc((void**)&e->buf[i], bytes) != hipSuccess) return fail(LTK_E_NOMEM, "activation arena allocation failed");
            CHK(hipMemset(e->buf[i], 0, bytes));
        }
        if (knob(K_PREFETCH)) {       // the prefetch slots (8 x 0.13 GB of concat buffers at 32 frames) + the prefetched encoder's temporaries
            e->alt_frames = std::min(arena_frames, kPrefetchMaxFrames);
            for (int i = 0; i < B_COUNT; ++i) {
                if (!e->buf_halfs[i] || !(i >= B_CAT0 || i == B_X0 || i == B_T0 || i == B_T1)) continue;
                const size_t bytes = e->buf_halfs[i] * e->alt_frames * sizeof(f16) + 4096;
                if (i < B_CAT0) {
                    if (hipMalloc((void**)&e->pf_tmp[i], bytes) != hipSuccess) return fail(LTK_E_NOMEM, "prefetch arena allocation failed");
                    CHK(hipMemset(e->pf_tmp[i], 0, bytes));
                    continue;
                }
                for (int k = 1; k <= ltk_engine::kPfSlots; ++k) {
                    if (hipMalloc((void**)&e->pfs[k].cat[i], bytes) != hipSuccess) return fail(LTK_E_NOMEM, "prefetch arena allocation failed");
                    CHK(hipMemset(e->pfs[k].cat[i], 0, bytes));
                }
            }
            for (int k = 1; k <= ltk_engine::kPfSlots; ++k) {
                CHK(hipEventCreateWithFlags(&e->pfs[k].ev_done, hipEventDisableTiming));
                CHK(hipEventCreateWithFlags(&e->pfs[k].ev_read, hipEventDisableTiming));
            }
            if (hipMalloc((void**)&e->d_tab_next, sizeof(DevTables)) != hipSuccess) return fail(LTK_E_NOMEM, "pointer table allocation failed");
            CHK(hipMemset(e->d_tab_next, 0, sizeof(DevTables)));
        }
        if (e->hw_w2l.alloc((int)e->layers.size())) return fail(LTK_E_NOMEM, "health table allocation failed");
        return LTK_OK;
    }();
    if (rc) { wav2lip_unload(e); return rc; }       // nothing half-built stays behind (the error text is already set)
    e->loaded = true;
    return LTK_OK;
}

int ltk_debug_tile_table_check(char* msg, int cap) {
    std::string m;
    const int bad = check_tile_table_impl(m);
    if (msg && cap > 0) { strncpy(msg, m.c_str(), (size_t)cap - 1); msg[cap - 1] = 0; }
    return bad;
}

}  // extern "C"

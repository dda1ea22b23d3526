// MtGraph (mt_graph.h): how ops are added to a program, its activations allocated, and the executor that turns every op into launches of the
// conv kernels (conv3_mfma.hip / conv_mfma.hip / rowgemm.hip), nn_kernels.hip and hubert_kernels.hip; and the model-independent mt_* wrappers of
// musetalk.h.  The models' builders are musetalk.hip (U-Net, VAE decoder / encoder), whisper.hip and hubert.hip.
#include <string.h>

#include <algorithm>

#include "mt_graph.h"
#include "tune.h"
#include "nn_kernels.h"
#include "misc_kernels.h"
#include "hubert_kernels.h"
#include "parse_kernels.h"
#include "s3fd_kernels.h"

namespace ltk {

MtTensor MtGraph::alloc(int C, int H, int W) {
    MtTensor t;
    t.buf = (int)buf_halfs.size();
    t.C = up16(C); t.ld = t.C; t.coff = 0; t.H = H; t.W = W;
    buf_halfs.push_back((size_t)t.C * H * W);
    return t;
}
MtTensor MtGraph::alloc_q8(int C, int H, int W) {          // C % 32 == 0
    MtTensor t;
    t.buf = (int)buf_halfs.size();
    t.C = C; t.ld = C; t.coff = 0; t.H = H; t.W = W; t.q8 = true;
    buf_halfs.push_back((size_t)(C / 2) * H * W);
    return t;
}
MtTensor MtGraph::view(const MtTensor& b, int coff, int C) {
    MtTensor t = b;
    t.coff = b.coff + coff; t.C = C;
    return t;
}
int MtGraph::add_vec(const float* host, int n, int pad_to) {
    const int m = std::max(n, pad_to);
    std::vector<float> tmp(m, 0.f);
    memcpy(tmp.data(), host, n * sizeof(float));
    float* d = nullptr;
    if (hipMalloc((void**)&d, m * sizeof(float)) != hipSuccess) { err = "hipMalloc failed"; return -1; }
    (void)hipMemcpy(d, tmp.data(), m * sizeof(float), hipMemcpyHostToDevice);
    vecs.push_back(d);
    return (int)vecs.size() - 1;
}
int MtGraph::add_named_vec(const std::string& name, const void* host, size_t bytes) {
    if (share) {
        auto it = share->vec_of.find(name);
        if (it == share->vec_of.end()) { err = "the shared weights have no " + name; return -1; }
        vecs.push_back(share->vecs[it->second]);
        return (int)vecs.size() - 1;
    }
    float* d = nullptr;
    if (hipMalloc((void**)&d, bytes) != hipSuccess) { err = "hipMalloc failed"; return -1; }
    (void)hipMemcpy(d, host, bytes, hipMemcpyHostToDevice);
    vecs.push_back(d);
    vec_of[name] = (int)vecs.size() - 1;
    return (int)vecs.size() - 1;
}
int MtGraph::add_conv(const std::string& name, const float* w, const float* bias, int Cin, int Cout, int k, int stride, int pad,
             const MtTensor& x, const MtTensor& y, const MtTensor* res, int act, int ups, const float* scale) {
    return add_conv2(name, w, bias, Cin, Cout, k, k, stride, stride, pad, pad, x, y, res, act, ups, 0, scale);
}
int MtGraph::alloc_ln_stats(int C, int H, int W) {
    const int b = (int)buf_halfs.size();
    buf_halfs.push_back((size_t)H * W * (C / 32) * 4);          // float2 = 4 halfs
    return b;
}
int MtGraph::add_conv_down_asym(const std::string& name, const float* w, const float* bias, int C, const MtTensor& x, const MtTensor& y) {
    return add_conv2(name, w, bias, C, C, 3, 3, 2, 2, 0, 0, x, y, nullptr, 0, 0, 1);
}
int MtGraph::add_conv2(const std::string& name, const float* w, const float* bias, int Cin, int Cout, int kh, int kw, int sh, int sw,
              int ph, int pw, const MtTensor& x, const MtTensor& y, const MtTensor* res, int act, int ups, int pad_br,
              const float* scale) {
    const int k = kh, stride = sh;
    const int kk = kh * kw;
    (void)k;
    if (share) return add_conv_shared(name, Cin, Cout, kh, kw, sh, x, y, res, act);
    const int CoutP = up16(Cout);
    const int CinR = Cin;
    Cin = up16(Cin);                    // whole channel blocks on both sides (zero weights for the padding)
    std::vector<float> wp;
    const float* wuse = w;
    if (CoutP != Cout || Cin != CinR) {
        wp.assign((size_t)CoutP * Cin * kk, 0.f);
        for (int co = 0; co < Cout; ++co)
            for (int ci = 0; ci < CinR; ++ci)
                memcpy(&wp[((size_t)co * Cin + ci) * kk], &w[((size_t)co * CinR + ci) * kk], (size_t)kk * sizeof(float));
        wuse = wp.data();
    }
    macs += (double)CinR * Cout * kk * (stride == 2 ? y.P() : (ups ? x.P() : y.P()));
    if (x.q8) macs_fp8 += (double)CinR * Cout * kk * y.P();
    std::vector<float> sc(CoutP, 1.f), sf(CoutP, 0.f);
    if (bias) memcpy(sf.data(), bias, Cout * sizeof(float));
    if (scale) memcpy(sc.data(), scale, Cout * sizeof(float));
    ConvPlan p;
    std::string e;
    int rc = conv_plan_create(&p, wuse, Cin, CoutP, kh, kw, sh, sw, ph, pw, false, pad_br, sc.data(), sf.data(), &e,
                              x.q8 ? conv_fp8_quant(CinR) : 0, fp8_ascale, ups ? 1 : 0);
    if (rc) { err = name + ": " + e; return -1; }
    plans.push_back(p);
    MtOp op;
    op.type = OP_CONV; op.name = name; op.x = x; op.y = y; op.plan = (int)plans.size() - 1; op.act = act; op.ups = ups;
    op.unet3x3 = !x.q8 && !ups && kh == 3 && kw == 3 && sh == 1 && sw == 1 && ph == 1 && pw == 1 && pad_br == 0 && x.P() <= 1024 && Cin >= 320 &&
                 name.rfind("decoder.", 0) != 0 && name.rfind("encoder.", 0) != 0;
    // The 1x1 / linear layers on maps of <= 64 pixels or tokens per frame (the U-Net's 8x8 and 4x4 levels: projections of the transformer
    // blocks, resnet shortcuts, the 50-token context projections; 1..13 MB of weights each behind 1024 / 256 rows of a 16-frame pass) also get
    // a rowconv plan: conv3 runs them as ~160 items of 40..160 chunks each behind a two-stage DMA pipe (30 us for a 1280 x 1280 linear layer
    // whose weights stream in 0.5 us); the weight-streaming GEMM over gathered rows pays one round trip per trip instead (mt_graph_run picks
    // it by the launch's row count).
    // Only the 1x1 / linear layers with <= 2560 outputs: a row block re-gathers its rows for every 32-output slab and every weight slab is
    // re-read by every row group, so the 3x3 layers (K = 11 520..23 040: ~1.4 GB of L2 -> CU traffic per layer at 1024 rows) and the
    // 10 240-output GEGLU projection would lose to conv3.
    if (!no_rowgemm && !x.q8 && !ups && act == 0 && sh == 1 && sw == 1 && kh == 1 && kw == 1 && ph == 0 && pw == 0 && pad_br == 0 &&
        Cin % 32 == 0 && Cin <= 5120 && CoutP % 256 == 0 && CoutP <= 2560 && x.P() <= 64 && x.P() == y.P()) {
        const size_t K = (size_t)kk * Cin;
        std::vector<float> we((size_t)CoutP * K);
        for (int co = 0; co < CoutP; ++co) {
            const float* src = wuse + (size_t)co * Cin * kk;
            float* dst = we.data() + (size_t)co * K;
            for (int t = 0; t < kk; ++t)
                for (int ci = 0; ci < Cin; ++ci) dst[(size_t)t * Cin + ci] = src[(size_t)ci * kk + t];
        }
        RowGemmPlan rg;
        rc = rowgemm_plan_create(&rg, we.data(), CoutP, (int)K, sc.data(), sf.data(), &e);
        if (rc) { err = name + ": " + e; return -1; }
        rplans.push_back(rg);
        op.rplan = (int)rplans.size() - 1;
        op.ksz = kh;
    }
    if (res) op.r = *res;
    // act 4 = GEGLU in the epilogue (conv3_mfma.hip): the output is half as wide as the projection
    if (up16(Cin) != x.C || (act == 4 ? CoutP / 2 : CoutP) != y.C) { err = name + ": channel mismatch (" + std::to_string(Cin) + "->" + std::to_string(Cout) + ")"; return -1; }
    ops.push_back(op);
    named[name] = y;
    plan_of[name] = op.plan;
    if (op.rplan >= 0) rplan_of[name] = op.rplan;
    return 0;
}
int MtGraph::add_conv_shared(const std::string& name, int Cin, int Cout, int kh, int kw, int stride, const MtTensor& x, const MtTensor& y,
                    const MtTensor* res, int act) {
    auto it = share->plan_of.find(name);
    if (it == share->plan_of.end()) { err = "the shared weights have no " + name; return -1; }
    plans.push_back(share->plans[it->second]);
    macs += (double)Cin * Cout * kh * kw * y.P();
    MtOp op;
    op.type = OP_CONV; op.name = name; op.x = x; op.y = y; op.plan = (int)plans.size() - 1; op.act = act;
    auto rt = share->rplan_of.find(name);
    if (rt != share->rplan_of.end() && act == 0 && stride == 1 && kh == 1 && kw == 1 && x.P() <= 64 && x.P() == y.P()) {
        rplans.push_back(share->rplans[rt->second]);
        op.rplan = (int)rplans.size() - 1;
        op.ksz = kh;
    }
    if (res) op.r = *res;
    if (up16(Cin) != x.C || up16(Cout) != y.C) { err = name + ": channel mismatch (" + std::to_string(Cin) + "->" + std::to_string(Cout) + ")"; return -1; }
    ops.push_back(op);
    named[name] = y;
    return 0;
}
int MtGraph::add_gn(const std::string& name, SD& sd, const std::string& prefix, const MtTensor& x, const MtTensor& y, float eps, int silu) {
    const float* g = sd.get(prefix + ".weight", x.C);
    const float* b = sd.get(prefix + ".bias", x.C);
    if (!g || !b) { err = sd.err; return -1; }
    // the kernels read a group's shift from x while other blocks already store y (nn_kernels.hip: gn_shift)
    if (x.buf == y.buf && x.coff < y.coff + y.C && y.coff < x.coff + x.C) { err = "GroupNorm " + name + " in place"; return -1; }
    MtOp op;
    op.type = OP_GN; op.name = name; op.x = x; op.y = y; op.eps = eps; op.silu = silu; op.groups = 32;
    op.gamma = add_vec(g, x.C); op.beta = add_vec(b, x.C);
    ops.push_back(op);
    if (!y.q8) named[name] = y;
    return 0;
}
int MtGraph::add_ln(const std::string& name, SD& sd, const std::string& prefix, const MtTensor& x, const MtTensor& y, float eps) {
    const float* g = sd.get(prefix + ".weight", x.C);
    const float* b = sd.get(prefix + ".bias", x.C);
    if (!g || !b) { err = sd.err; return -1; }
    MtOp op;
    op.type = OP_LN; op.name = name; op.x = x; op.y = y; op.eps = eps;
    op.gamma = add_vec(g, x.C); op.beta = add_vec(b, x.C);
    ops.push_back(op);
    named[name] = y;
    return 0;
}
void MtGraph::add_attn(const std::string& name, const MtTensor& q, const MtTensor& k, const MtTensor& v, const MtTensor& o, int heads, int d16,
              int vt_buf) {
    MtOp op;
    op.type = OP_ATTN; op.name = name; op.x = q; op.k = k; op.v = v; op.y = o; op.heads = heads; op.d16 = d16; op.Tk = k.P();
    op.vt_buf = vt_buf;
    if (vt_buf < 0) vt_halfs = std::max(vt_halfs, (size_t)heads * attn_dv32(d16) * attn_tkp(k.P()));
    ops.push_back(op);
    named[name + ".attn"] = o;
}
void MtGraph::add_geglu(const std::string& name, const MtTensor& x, const MtTensor& y) {
    MtOp op;
    op.type = OP_GEGLU; op.name = name; op.x = x; op.y = y;
    ops.push_back(op);
    named[name] = y;
}

// ------------------------------------------------------------------------------------------ allocate / run / free
int mt_graph_alloc(MtGraph& g, int frames) {
    g.frames = frames;
    g.bufs.assign(g.buf_halfs.size(), nullptr);
    for (size_t i = 0; i < g.buf_halfs.size(); ++i) {
        const size_t bytes = g.buf_halfs[i] * frames * sizeof(f16) + 256;
        if (hipMalloc((void**)&g.bufs[i], bytes) != hipSuccess) { g.err = "activation allocation failed"; return -4; }
        (void)hipMemset(g.bufs[i], 0, bytes);
    }
    // GroupNorm partial stats: [N][C/16][segs][32] floats, C <= 2560, segs <= 256 -> bound by the op list
    size_t need = 0;
    for (const MtOp& op : g.ops)
        if (op.type == OP_GN) need = std::max(need, (size_t)frames * (op.x.C / 16) * gn_segments(frames, op.x.C, op.x.P()) * 32);
    // the segment count is chosen per launch from the launch's frame count: size for the worst case (1 frame)
    for (const MtOp& op : g.ops)
        if (op.type == OP_GN) need = std::max(need, (size_t)frames * (op.x.C / 16) * 256 * 32);
    g.gn_partial_floats = need;
    if (hipMalloc((void**)&g.gn_partial, need * sizeof(float)) != hipSuccess) { g.err = "allocation failed"; return -4; }
    // gn_coop_kernel: 8 words per block, a region per op (a launch of nf <= frames images uses the head of its region)
    g.gn_slot_words = 0;
    for (MtOp& op : g.ops) {
        op.gn_slot_off = -1;
        if (op.type != OP_GN || gn_group_fits(op.x.C, op.x.P(), op.groups)) continue;
        const int M = gn_coop_members(op.x.C, op.x.P(), op.groups);
        if (!M) continue;
        op.gn_slot_off = (long long)g.gn_slot_words;
        g.gn_slot_words += (size_t)frames * (op.x.C / 16) * (op.x.P() / 2048) * 8;      // sized for 2048-pixel slices, the smallest the kernel uses
    }
    if (g.gn_slot_words) {
        if (hipMalloc((void**)&g.gn_slots, g.gn_slot_words * sizeof(unsigned)) != hipSuccess) { g.err = "allocation failed"; return -4; }
        if (hipHostMalloc((void**)&g.gn_err_host, sizeof(unsigned), hipHostMallocMapped) != hipSuccess) { g.err = "allocation failed"; return -4; }
        *g.gn_err_host = 0u;
        if (hipHostGetDevicePointer((void**)&g.gn_err_dev, g.gn_err_host, 0) != hipSuccess) { g.err = "allocation failed"; return -4; }
    }
    if (g.vt_halfs) {
        if (hipMalloc((void**)&g.vt, g.vt_halfs * frames * sizeof(f16)) != hipSuccess) { g.err = "allocation failed"; return -4; }
    }
    return 0;
}

void mt_graph_free(MtGraph& g) {
    for (f16* b : g.bufs) if (b) (void)hipFree(b);
    if (!g.share) {                                   // a graph over shared weights holds copies of the owner's handles
        for (ConvPlan& p : g.plans) conv_plan_destroy(&p);
        for (RowGemmPlan& p : g.rplans) rowgemm_plan_destroy(&p);
        for (float* v : g.vecs) if (v) (void)hipFree(v);
    }
    if (g.gn_partial) (void)hipFree(g.gn_partial);
    if (g.gn_slots) (void)hipFree(g.gn_slots);
    if (g.gn_err_host) (void)hipHostFree(g.gn_err_host);
    g.gn_slots = nullptr; g.gn_err_host = nullptr; g.gn_err_dev = nullptr;
    if (g.vt) (void)hipFree(g.vt);
    g.bufs.clear(); g.plans.clear(); g.rplans.clear(); g.vecs.clear();
}

// one op on stream `s`
static int mt_run_op_body(MtGraph& g, const MtOp& op, int nf, float* partial, size_t partial_cap, hipStream_t s) {
    switch (op.type) {
        case OP_CONV: {
            ConvIO io;
            io.x = g.bufs[op.x.buf]; io.N = nf; io.H = op.x.H; io.W = op.x.W; io.x_ld = op.x.ld; io.x_coff = op.x.coff;
            if (op.x.q8) { io.x_ld /= 2; io.x_coff /= 2; }      // 16-bit units of the fp8 tensor (conv_mfma.h: ConvPlan::q8)
            io.y = g.bufs[op.y.buf]; io.y_ld = op.y.ld; io.y_coff = op.y.coff;
            io.res = op.r.buf >= 0 ? g.bufs[op.r.buf] : nullptr; io.res_ld = op.r.ld; io.res_coff = op.r.coff;
            io.relu = 0; io.act = op.act; io.ups = op.ups;
            io.partial = partial; io.partial_cap = partial_cap;
            if (op.ln_out_buf >= 0) { io.ln_out = reinterpret_cast<float*>(g.bufs[op.ln_out_buf]); io.ln_out_tiles = op.y.C / 32; }
            if (op.ln_in_buf >= 0) { io.ln_in = reinterpret_cast<const float*>(g.bufs[op.ln_in_buf]); io.ln_in_tiles = op.ln_in_tiles; io.ln_eps = op.ln_eps; }
            // U-Net resnet convs of a <= 16-frame pass: conv3's items-per-CU rule settles on tiles that re-read weights (8x8, 32x32 levels) or
            // under-fill the chip (16x16 level); measured per level with the tile forced for every 3x3 launch (profiles/r02_mt_tile_force_ab.txt:
            // 8x8 1280..2560 ch 116 -> 89 us at 256-px tiles, 16x16 640 ch 67 -> 49 us at 128-px tiles, 32x32 320 ch 55 -> 44 us at 256-px tiles).
            // The VAE decoder keeps the rule (it wants its 512-px tiles).
            // (The 4x4 level keeps the rule: forced 256-px tiles measured 31 -> 37 us there, profiles/r04_mt_rowconv_tile_ab.txt.)
            if (op.unet3x3 && nf <= 16 && op.x.P() >= 64) io.force_pxw = op.x.P() == 256 ? 1 : 2;
            std::string e;
            int rc;
            // (K = 1280 linear layers from kLinFkMinRows rows on - the 8^2 level of a 16-frame pass - take conv3_launch's lin_fk route)
            const bool lin_fk = knob(K_LIN_FK) && op.ksz == 1 && (long long)nf * op.y.P() >= kLinFkMinRows &&
                                (conv3_lin_fk_k(g.plans[op.plan].Cin) || conv3_lin_mp_nsl(g.plans[op.plan].Cin, (long long)nf * op.y.P(), g.plans[op.plan].lCout) > 0);
            constexpr int kMtRowConvMaxRows = 1024;      // rowconv plans (add_conv) in launches of at most this many rows (frames x pixels)
            if (op.rplan >= 0 && !lin_fk && (long long)nf * op.y.P() <= kMtRowConvMaxRows) {
                RowConvIO rio;
                rio.x = io.x; rio.x_ld = op.x.ld; rio.x_coff = op.x.coff; rio.H = op.x.H; rio.W = op.x.W;
                rio.y = io.y; rio.y_ld = op.y.ld; rio.y_coff = op.y.coff; rio.Ho = op.y.H; rio.Wo = op.y.W;
                rio.res = io.res; rio.res_ld = io.res_ld; rio.res_coff = io.res_coff;
                rio.N = nf; rio.KW = op.ksz; rio.stride = 1; rio.pad = op.ksz / 2; rio.relu = 0;
                rio.ln_out = io.ln_out; rio.ln_out_tiles = io.ln_out_tiles; rio.ln_in = io.ln_in; rio.ln_in_tiles = io.ln_in_tiles; rio.ln_eps = io.ln_eps;
                rc = rowconv_launch(g.rplans[op.rplan], rio, s, &e);
            } else if (op.own_split && nf > 1) {
                // The face detector's records must not depend on the images beside an image.  conv3 splits the channel loop of an
                // under-filled launch by a factor that follows the launch's frame count, and another factor (or another kernel family)
                // is another fp32 summation order: every image takes the order of its OWN one-image launch - in one launch over all
                // nf where the planner grants that factor to the same family at nf, else image by image.
                ConvReport r1, rn;
                memset(&r1, 0, sizeof(r1)); memset(&rn, 0, sizeof(rn));
                ConvIO d = io;
                d.N = 1; d.report = &r1;
                rc = conv_launch_dry(g.plans[op.plan], d, &e);
                const int ks1 = std::max(1, r1.ksplit);
                if (!rc) { d.N = nf; d.force_ksplit = ks1; d.report = &rn; rc = conv_launch_dry(g.plans[op.plan], d, &e); }
                auto family = [](const ConvReport& r) { return std::string(r.kernel, strcspn(r.kernel, "<")); };
                if (!rc && family(rn) == family(r1) && std::max(1, rn.ksplit) == ks1) {
                    io.force_ksplit = ks1;
                    rc = conv_launch(g.plans[op.plan], io, s, &e);
                } else if (!rc) {
                    const size_t xs = (size_t)op.x.P() * op.x.ld, ys = (size_t)op.y.P() * op.y.ld;
                    for (int f = 0; f < nf && !rc; ++f) {
                        ConvIO one = io;
                        one.N = 1; one.x = io.x + f * xs; one.y = io.y + f * ys;
                        rc = conv_launch(g.plans[op.plan], one, s, &e);
                    }
                }
            } else {
                rc = conv_launch(g.plans[op.plan], io, s, &e);
            }
            if (rc) { g.err = op.name + ": " + e; return rc; }
            break;
        }
        case OP_GN: {
            const int P = op.x.P();
            if (knob(K_MT_GN1) && gn_group_fits(op.x.C, P, op.groups)) {      // one launch: block = (image, group)
                launch_gn_group(g.bufs[op.x.buf], nf, op.x.ld / 16, op.x.coff / 16, op.x.C, P, op.groups, op.eps, g.vecs[op.gamma],
                                g.vecs[op.beta], op.silu, g.bufs[op.y.buf], op.y.q8 ? op.y.ld / 32 : op.y.ld / 16,
                                op.y.q8 ? op.y.coff / 32 : op.y.coff / 16, op.y.q8 ? 1 : 0, g.fp8_ascale, s);
                break;
            }
            if (knob(K_GN_COOP) && op.gn_slot_off >= 0 && g.gn_slots) {           // one tensor pass: slices in registers, partial sums exchanged between blocks
                launch_gn_coop(g.bufs[op.x.buf], nf, op.x.ld / 16, op.x.coff / 16, op.x.C, P, op.groups, op.eps, g.gn_slots + op.gn_slot_off, g.gn_err_dev,
                               g.vecs[op.gamma], g.vecs[op.beta], op.silu, g.bufs[op.y.buf], op.y.q8 ? op.y.ld / 32 : op.y.ld / 16,
                               op.y.q8 ? op.y.coff / 32 : op.y.coff / 16, op.y.q8 ? 1 : 0, g.fp8_ascale, s);
                break;
            }
            const int segs = gn_segments(nf, op.x.C, P);
            launch_gn_stats(g.bufs[op.x.buf], nf, op.x.ld / 16, op.x.coff / 16, op.x.C, P, op.groups, segs, g.gn_partial, s);
            if (op.y.q8)
                launch_gn_apply_fp8(g.bufs[op.x.buf], nf, op.x.ld / 16, op.x.coff / 16, op.x.C, P, op.groups, op.eps, g.gn_partial, segs,
                                    g.vecs[op.gamma], g.vecs[op.beta], op.silu, g.fp8_ascale, (unsigned char*)g.bufs[op.y.buf],
                                    op.y.ld / 32, op.y.coff / 32, s);
            else
                launch_gn_apply(g.bufs[op.x.buf], nf, op.x.ld / 16, op.x.coff / 16, op.x.C, P, op.groups, op.eps, g.gn_partial, segs,
                                g.vecs[op.gamma], g.vecs[op.beta], op.silu, g.bufs[op.y.buf], op.y.ld / 16, op.y.coff / 16, s);
            break;
        }
        case OP_LN:
            launch_layernorm(g.bufs[op.x.buf], nf, op.x.ld / 16, op.x.coff / 16, op.x.C, op.x.P(), op.eps, g.vecs[op.gamma],
                             g.vecs[op.beta], g.bufs[op.y.buf], op.y.ld / 16, op.y.coff / 16, s);
            break;
        case OP_VT: {
            VtMulti m;
            m.n = (int)g.vt_items.size(); m.Tk = g.vt_items.empty() ? 0 : g.vt_items[0].Tk; m.Tkp = 0;
            if (m.n > 16) { g.err = "too many hoisted value tensors"; return -1; }
            for (int i = 0; i < m.n; ++i) {
                const MtVtItem& it = g.vt_items[i];
                m.it[i] = {g.bufs[it.v.buf], g.bufs[it.vt_buf], it.v.ld / 16, it.v.coff / 16, it.heads, it.d16, 0, 0};
            }
            launch_v_transpose_multi(m, nf, s);
            break;
        }
        case OP_ATTN: {
            f16* vt = g.vt;
            if (op.vt_buf >= 0) vt = g.bufs[op.vt_buf];
            else launch_v_transpose(g.bufs[op.v.buf], nf, op.v.ld / 16, op.v.coff / 16, op.heads, op.d16, op.Tk, g.vt, s);
            const int rc = launch_attention(g.bufs[op.x.buf], op.x.ld / 16, op.x.coff / 16, op.x.P(), g.bufs[op.k.buf], op.k.ld / 16,
                                            op.k.coff / 16, op.Tk, vt, g.bufs[op.y.buf], op.y.ld / 16, op.y.coff / 16, nf, op.heads,
                                            op.d16, s);
            if (rc) { g.err = op.name + ": attention launch failed (head dim " + std::to_string(op.d16) + ")"; return rc; }
            break;
        }
        case OP_ADDPOS:
            launch_add_pos(g.bufs[op.x.buf], nf, op.x.ld / 16, op.x.coff / 16, op.x.C, op.x.P(), g.vecs[op.gamma], s);
            break;
        case OP_HB_L0:
            launch_hubert_layer0_n(reinterpret_cast<const float*>(g.bufs[g.hb_pcm_buf]), g.hb_samples, nf, g.vecs[op.wvec], g.vecs[op.bvec],
                                   g.vecs[op.gamma], g.vecs[op.beta], op.eps, g.bufs[op.y.buf], op.y.ld / 16, s);
            break;
        case OP_LNGELU:
            launch_ln_gelu512_n(g.bufs[op.x.buf], nf, op.x.ld / 16, op.x.coff / 16, op.x.P(), op.eps, g.vecs[op.gamma], g.vecs[op.beta],
                                g.bufs[op.y.buf], op.y.ld / 16, op.y.coff / 16, s);
            break;
        case OP_POSCONV:
            launch_hubert_posconv_n(g.bufs[op.x.buf], nf, op.x.ld / 16, op.x.coff / 16, op.x.P(), reinterpret_cast<const f16*>(g.vecs[op.wvec]),
                                    g.vecs[op.bvec], g.bufs[op.y.buf], op.y.ld / 16, op.y.coff / 16, s);
            break;
        case OP_GEGLU:
            launch_geglu(g.bufs[op.x.buf], nf, op.x.ld / 16, op.x.coff / 16, op.y.C, op.x.P(), g.bufs[op.y.buf], op.y.ld / 16,
                         op.y.coff / 16, s);
            break;
        // the face parser's own ops (parse_kernels.h): every launcher checks its views and refuses with its text, nothing enqueued
        case OP_FP_STEM:
        case OP_FP_MAXPOOL:
        case OP_FP_GAP:
        case OP_FP_GATE:
        case OP_FP_LABELS: {
            std::string e;
            int rc = -1;
            if (op.type == OP_FP_STEM)
                rc = launch_parse_stem(reinterpret_cast<const uint8_t*>(g.bufs[g.fp_img_buf]), nf, g.fp_size, g.fp_size,
                                       reinterpret_cast<const f16*>(g.vecs[op.wvec]), g.vecs[op.gamma], g.vecs[op.beta], g.bufs[op.y.buf],
                                       op.y.ld / 16, op.y.coff / 16, s, &e);
            else if (op.type == OP_FP_MAXPOOL)
                rc = launch_maxpool3x3s2(g.bufs[op.x.buf], nf, op.x.ld / 16, op.x.coff / 16, op.x.C, op.x.H, op.x.W, g.bufs[op.y.buf], op.y.ld / 16,
                                         op.y.coff / 16, s, &e);
            else if (op.type == OP_FP_GAP)
                rc = launch_gap(g.bufs[op.x.buf], nf, op.x.ld / 16, op.x.coff / 16, op.x.C, op.x.P(), g.bufs[op.y.buf], op.y.ld / 16, op.y.coff / 16, s, &e);
            else if (op.type == OP_FP_GATE)
                rc = launch_chan_gate(g.bufs[op.x.buf], nf, op.x.ld / 16, op.x.coff / 16, op.x.C, op.x.P(), g.bufs[op.ga.buf],
                                      op.gb.buf >= 0 ? g.bufs[op.gb.buf] : nullptr, op.r.buf >= 0 ? g.bufs[op.r.buf] : nullptr, op.r.ld / 16,
                                      op.r.coff / 16, op.plus1, g.bufs[op.y.buf], op.y.ld / 16, op.y.coff / 16, s, &e);
            else
                rc = launch_seg_argmax(g.bufs[op.x.buf], nf, op.x.H, op.x.W, reinterpret_cast<uint8_t*>(g.bufs[g.fp_label_buf]), s, &e);
            if (rc) { g.err = op.name + ": " + e; return rc; }
            break;
        }
        // the face detector's own ops (s3fd_kernels.h), refusing as the parser's do
        case OP_FD_STEM:
        case OP_FD_POOL:
        case OP_FD_L2NORM:
        case OP_FD_DETECT: {
            std::string e;
            int rc = -1;
            if (op.type == OP_FD_STEM)
                rc = launch_s3fd_stem(reinterpret_cast<const uint8_t*>(g.bufs[g.fd_img_buf]), nf, g.fd_H, g.fd_W, reinterpret_cast<const f16*>(g.vecs[op.wvec]),
                                      g.vecs[op.beta], g.bufs[op.y.buf], op.y.ld / 16, op.y.coff / 16, s, &e);
            else if (op.type == OP_FD_POOL)
                rc = launch_maxpool2x2s2(g.bufs[op.x.buf], nf, op.x.ld / 16, op.x.coff / 16, op.x.C, op.x.H, op.x.W, g.bufs[op.y.buf], op.y.ld / 16,
                                         op.y.coff / 16, s, &e);
            else if (op.type == OP_FD_L2NORM)
                rc = launch_l2norm(g.bufs[op.x.buf], nf, op.x.ld / 16, op.x.coff / 16, op.x.C, op.x.P(), g.vecs[op.gamma], g.bufs[op.y.buf], op.y.ld / 16,
                                   op.y.coff / 16, s, &e);
            else {
                char* base = reinterpret_cast<char*>(g.bufs[g.fd_rec_buf]);
                rc = launch_s3fd_detect(g.bufs[op.x.buf], nf, op.x.ld / 16, op.x.coff / 16, op.x.H, op.x.W, op.fd_maxout, op.fd_level, 0.f,
                                        reinterpret_cast<const float*>(base + kFdThreshAt), reinterpret_cast<uint32_t*>(base + kFdHeadBytes), g.fd_cap,
                                        reinterpret_cast<uint32_t*>(base), s, &e);
            }
            if (rc) { g.err = op.name + ": " + e; return rc; }
            break;
        }
    }
    return 0;
}

static int mt_run_op(MtGraph& g, const MtOp& op, int nf, float* partial, size_t partial_cap, hipStream_t s) {
    const int rc = mt_run_op_body(g, op, nf, partial, partial_cap, s);
    if (!rc && g.health && op.y.buf >= 0) {                            // a watched call: this op's record (an op without an output tensor stays unobserved)
        const int gran = op.y.q8 ? 32 : 16;
        const size_t oi = (size_t)(&op - g.ops.data());
        launch_health_scan(g.bufs[op.y.buf], nf, op.y.ld / gran, op.y.coff / gran, op.y.C / gran, op.y.P(), op.y.q8 ? 1 : 0, g.health + oi, s);
        if (g.health_obs) g.health_obs[oi] = 1;
    }
    return rc;
}


int mt_graph_run(MtGraph& g, int nf, float* partial, size_t partial_cap, hipStream_t s, int op_begin, int op_end,
                 std::vector<hipEvent_t>* evs) {
    if (nf > g.frames) { g.err = "more frames than the graph was sized for"; return -1; }
    if (op_end < 0) op_end = (int)g.ops.size();
    if (g.gn_slots && knob(K_GN_COOP)) {                 // the exchange slots of this range's cooperative GroupNorms back to the sentinel (one fill per pass)
        long long lo = -1, hi = -1;
        for (int oi = op_begin; oi < op_end; ++oi) {
            const MtOp& op = g.ops[oi];
            if (op.type != OP_GN || op.gn_slot_off < 0) continue;
            const long long words = (long long)g.frames * (op.x.C / 16) * (op.x.P() / 2048) * 8;
            if (lo < 0) lo = op.gn_slot_off;
            hi = op.gn_slot_off + words;
        }
        if (lo >= 0) launch_gn_coop_reset(g.gn_slots + lo, (size_t)(hi - lo), s);
    }
    for (int oi = op_begin; oi < op_end; ++oi) {
        if (evs) (void)hipEventRecord((*evs)[oi - op_begin], s);
        const int rc = mt_run_op(g, g.ops[oi], nf, partial, partial_cap, s);
        if (rc) return rc;
    }
    if (evs) (void)hipEventRecord((*evs)[op_end - op_begin], s);
    if (hipGetLastError() != hipSuccess) { g.err = "a MuseTalk kernel launch failed"; return -2; }
    return 0;
}

// ------------------------------------------------------------------------------------------ public wrappers
int mt_op_count(MtGraph* g) { return (int)g->ops.size(); }
const char* mt_op_name(MtGraph* g, int i, int* type) {
    if (i < 0 || i >= (int)g->ops.size()) return nullptr;
    if (type) *type = g->ops[i].fp_type >= 0 ? g->ops[i].fp_type : (int)g->ops[i].type;
    return g->ops[i].name.c_str();
}
int mt_run_head(MtGraph* g, int nf, float* partial, size_t partial_cap, hipStream_t s, int op_end) {
    return mt_graph_run(*g, nf, partial, partial_cap, s, 0, op_end);
}
int mt_run_timed(MtGraph* g, int nf, float* partial, size_t partial_cap, hipStream_t s, std::vector<hipEvent_t>* evs) {
    return mt_graph_run(*g, nf, partial, partial_cap, s, 0, -1, evs);
}
MtGraph* mt_graph_new() { return new MtGraph(); }
void mt_graph_delete(MtGraph* g) {
    if (!g) return;
    mt_graph_free(*g);
    delete g->t_latent; delete g->t_ctx; delete g->t_unet_out; delete g->t_vae_out;
    delete[] g->whisper_states;
    delete g->hb_out;
    delete g;
}
const char* mt_graph_error(const MtGraph* g) { return g->err.c_str(); }
int mt_gn_error(MtGraph* g) {
    if (!g || !g->gn_err_host || !*reinterpret_cast<volatile unsigned*>(g->gn_err_host)) return 0;
    *g->gn_err_host = 0u;
    g->err = "a cooperative GroupNorm block gave up waiting for its set (gn_coop_kernel): the pass's frames are invalid; LTK_GN_COOP=0 selects the two-pass kernels";
    return 1;
}

void mt_set_health(MtGraph* g, HealthRec* recs, unsigned char* observed) { g->health = recs; g->health_obs = observed; }
bool mt_health_on(const MtGraph* g) { return g->health != nullptr; }
const void* mt_op_out(MtGraph* g, const char* name, int* C, int* ld, int* coff, int* P, int* q8) {
    for (const MtOp& op : g->ops)
        if (op.name == name && op.y.buf >= 0) {
            *C = op.y.C; *ld = op.y.ld; *coff = op.y.coff; *P = op.y.P(); *q8 = op.y.q8 ? 1 : 0;
            return g->bufs[op.y.buf];
        }
    return nullptr;
}
int mt_op_out_q8(MtGraph* g, int i) { return i >= 0 && i < (int)g->ops.size() && g->ops[i].y.buf >= 0 && g->ops[i].y.q8 ? 1 : 0; }
void mt_set_fp8(MtGraph* g, int on, float act_scale) { g->fp8 = on != 0; if (act_scale > 0.f) g->fp8_ascale = act_scale; }
double mt_macs_fp8_per_frame(const MtGraph* g) { return g->macs_fp8; }
int mt_run(MtGraph* g, int nf, float* partial, size_t partial_cap, hipStream_t s) { return mt_graph_run(*g, nf, partial, partial_cap, s, 0, -1); }
f16* mt_named(MtGraph* g, const char* name, int* C, int* ld, int* coff, int* H, int* W) {
    auto it = g->named.find(name);
    if (it == g->named.end()) return nullptr;
    const MtTensor& t = it->second;
    *C = t.C; *ld = t.ld; *coff = t.coff; *H = t.H; *W = t.W;
    return g->bufs[t.buf];
}
double mt_macs_per_frame(const MtGraph* g) { return g->macs; }
size_t mt_activation_bytes(const MtGraph* g) {
    size_t b = 0;
    for (size_t h : g->buf_halfs) b += h * (size_t)std::max(g->frames, 1) * sizeof(f16);
    return b + g->vt_halfs * sizeof(f16);
}

}  // namespace ltk

// The Ultralight avatar (avatars/ultralight/unet.py Model(6, 'hubert'), avatars/ultralight_avatar.py): a MobileNet-style U-Net at
// 160x160 as a static launch program over a device activation arena.  Every inverted residual (unet.py:7-36) is three launches -
// 1x1 expand on conv3's 1x1 path, depthwise 3x3 and (where the block has one) the residual add in the 1x1 project's epilogue -
// eval-mode BatchNorm folded into scale / shift at register time; torch.cat is a channel-block range of a shared buffer, the
// bilinear upsample writes straight into it.  The model is per avatar (ultralight_avatar.py:69-70), so the program is built by
// ltk_ultralight_avatar_register and owned by the avatar; the activation arena and the pointer tables belong to the engine.
// Its VALU kernels are dw_kernels.hip; what the other engine sources call is declared in engine_internal.h.
#include "engine_internal.h"
#include "ul_gconv.h"
#include "ul_ir.h"

namespace ltk {

enum UlBuf { U_FEAT = 0, U_X0, U_E1, U_E2, U_P, U_Q, U_CAT1, U_CAT2, U_CAT3, U_CAT4, U_FCAT, U_COUNT };
static_assert(U_COUNT <= kUlBufs, "engine_internal.h kUlBufs");

enum UlOpType { UL_CONV = 0, UL_DW, UL_UP, UL_IN, UL_FEAT, UL_HEAD, UL_IR };      // UL_IR: only in the listing of a fused program (ul_listing)

struct UlOp {
    int type = UL_CONV;
    std::string name;               // state_dict prefix of the conv (tap name); "<block>.up" for an upsample
    ConvPlan plan;                  // UL_CONV
    float* d_dw = nullptr;          // UL_DW: [C/16][9][16] weights, then scale [C], shift [C]
    f16* d_gw = nullptr;            // UL_CONV, grouped path: the weights as ul_gconv_pack lays them out, then (d_gss) scale [C], shift [C]
    float* d_gss = nullptr;
    uint8_t* d_ir = nullptr;        // UL_CONV, the expand conv of an inverted residual the fused kernel takes (knob UL_FUSE_IR): the block's
    size_t ir_off[4] = {0, 0, 0, 0};   // operand image for ul_ir_kernel (ul_ir_pack) - this op, the depthwise conv and the project conv behind it
    int cin = 0, k = 1, pad = 0;    // UL_CONV geometry (the geometry-only program of the grouped path has no plan)
    int C = 0, Creal = 0;           // channels the op writes (layout) / of the reference's tensor
    int stride = 1, relu = 0;
    int in_buf = 0, in_ld = 0, in_coff = 0, H = 0, W = 0;
    int out_buf = 0, out_ld = 0, out_coff = 0, Ho = 0, Wo = 0;
    int res_buf = -1, res_ld = 0, res_coff = 0;
    double macs = 0;                // per frame
};

struct UlProgram {
    std::vector<UlOp> ops;
    UlInW inw;
    UlHeadW headw;
    size_t buf_halfs[U_COUNT] = {0};      // per frame
    double macs_per_frame = 0;
    size_t ir_bytes = 0;                  // operand images of the fused inverted residuals
    UlGroupW* d_group = nullptr;          // the avatar's record of the grouped path (ul_gconv.h): every op's operands by op index
};

void ul_program_delete(UlProgram* p) {
    if (!p) return;
    for (UlOp& op : p->ops) {
        conv_plan_destroy(&op.plan);
        if (op.d_dw) (void)hipFree(op.d_dw);
        if (op.d_gw) (void)hipFree(op.d_gw);
        if (op.d_gss) (void)hipFree(op.d_gss);
        if (op.d_ir) (void)hipFree(op.d_ir);
    }
    if (p->d_group) (void)hipFree(p->d_group);
    delete p;
}

double ul_macs_per_frame(const UlAvatar& a) { return a.prog ? a.prog->macs_per_frame : 0.0; }

// The program fuses the inverted residuals whose input map has at least this many pixels (32 x 32: the blocks on the 160^2 .. 40^2 maps and
// the audio tower's first two).  The blocks on the 20^2 maps and below have 512 to 2048 hidden channels and stream weights: ul_ir_kernel
// re-reads them per 8 x 8 tile, and fusing them was not tried.
constexpr int kUlIrMinMapPx = 32 * 32;

// ops[at] .. ops[at + 2] = expand, depthwise, project of an inverted residual that has a fused operand image: the fused launch over n
// frames, if the planner accepts it at that count (x, y, res: the arena's buffers, or null for the plan alone)
bool ul_ir_io(const UlProgram& p, size_t at, int n, f16* const* bufs, UlIrIO* io) {
    if (at + 2 >= p.ops.size() || !p.ops[at].d_ir) return false;
    const UlOp &ex = p.ops[at], &dw = p.ops[at + 1], &pr = p.ops[at + 2];
    *io = UlIrIO();
    io->N = n; io->H = ex.H; io->W = ex.W; io->Cin = ex.cin; io->mid = ex.C; io->Cout = pr.C; io->stride = dw.stride;
    io->x_ld = ex.in_ld; io->x_coff = ex.in_coff;
    io->y_ld = pr.out_ld; io->y_coff = pr.out_coff;
    io->has_res = pr.res_buf >= 0 ? 1 : 0; io->res_ld = pr.res_ld; io->res_coff = pr.res_coff;
    if (bufs) {
        io->x = bufs[ex.in_buf]; io->y = bufs[pr.out_buf];
        io->res = pr.res_buf >= 0 ? bufs[pr.res_buf] : nullptr;
    }
    UlIrPlan pl;
    std::string err;
    return ul_ir_plan(*io, false, &pl, &err) == 0;
}

// (name, type) of every launch of a per-avatar pass under the knob's current value: a fused inverted residual once, as UL_IR under
// its project conv's name
std::vector<std::pair<std::string, int>> ul_listing(const UlProgram& p) {
    std::vector<std::pair<std::string, int>> out;
    const bool fuse = knob(K_UL_FUSE_IR) != 0;
    UlIrIO io;
    for (size_t at = 0; at < p.ops.size(); ++at) {
        if (fuse && ul_ir_io(p, at, 1, nullptr, &io)) { at += 2; out.emplace_back(p.ops[at].name, (int)UL_IR); }
        else out.emplace_back(p.ops[at].name, p.ops[at].type);
    }
    return out;
}

namespace {

const float kUlBnEps = 1e-5f;     // nn.BatchNorm2d default (unet.py:17,26,29)

struct Tn { int buf, ld, coff, C, H, W; };     // a tensor = channels [coff, coff + C) of a buffer of ld channels

struct Builder {
    SD sd;              // (ltk_ultralight_avatar_register has checked that every entry has a name and data)
    UlProgram* p;

    // the BatchNorm2d `bn` behind a conv with `bias` (or null), folded (state_dict.h)
    int fold_bn(const std::string& bn, int C, const float* bias, std::vector<float>* sc, std::vector<float>* sf) {
        const float* g = sd.get(bn + ".weight", C);
        const float* b = sd.get(bn + ".bias", C);
        const float* m = sd.get(bn + ".running_mean", C);
        const float* v = sd.get(bn + ".running_var", C);
        if (!g || !b || !m || !v) return fail(LTK_E_INVALID, "state_dict is missing (or has a wrong shape for) the BatchNorm tensors " + bn + ".*");
        sc->resize(C); sf->resize(C);
        ltk::fold_bn(g, b, m, v, bias, kUlBnEps, C, sc->data(), sf->data());
        return 0;
    }
    void note(const UlOp& op) {
        size_t& h = p->buf_halfs[op.out_buf];
        h = std::max(h, (size_t)op.out_ld * op.Ho * op.Wo);
        p->macs_per_frame += op.macs;
    }
    // dense conv (1x1 or 3x3) + folded BN (+ conv bias) + optional ReLU / residual
    int conv(const std::string& wname, const std::string& bn, bool has_bias, const Tn& in, int cout, int k, int stride, int pad, int relu,
             const Tn* res, int out_buf, int out_ld, int out_coff, Tn* out) {
        const float* w = sd.get(wname + ".weight", (size_t)cout * in.C * k * k);
        const float* bias = has_bias ? sd.get(wname + ".bias", cout) : nullptr;
        if (!w || (has_bias && !bias)) return fail(LTK_E_INVALID, "state_dict is missing (or has a wrong shape for) " + wname + ".weight / .bias");
        std::vector<float> sc, sf;
        int rc = fold_bn(bn, cout, bias, &sc, &sf);
        if (rc) return rc;
        p->ops.emplace_back();
        UlOp& op = p->ops.back();
        op.type = UL_CONV; op.name = wname;
        std::string err;
        rc = conv_plan_create(&op.plan, w, in.C, cout, k, k, stride, stride, pad, pad, false, 0, sc.data(), sf.data(), &err);
        if (rc) return conv_status(rc, wname + ": " + err);
        op.C = op.Creal = cout; op.stride = stride; op.relu = relu;
        op.cin = (in.C + 15) / 16 * 16; op.k = k; op.pad = pad;      // layout channels (inc's project conv reads 12 of 16)
        {   // the grouped path's copy: fp16 weights in ul_gconv_kernel's operand layout (zeros behind channel in.C), fp32 scale / shift
            std::vector<f16> gw(ul_gconv_pack(w, in.C, cout, k, nullptr));
            ul_gconv_pack(w, in.C, cout, k, gw.data());
            CHK(hipMalloc((void**)&op.d_gw, gw.size() * sizeof(f16)));
            CHK(hipMemcpy(op.d_gw, gw.data(), gw.size() * sizeof(f16), hipMemcpyHostToDevice));
            CHK(hipMalloc((void**)&op.d_gss, (size_t)2 * cout * sizeof(float)));
            CHK(hipMemcpy(op.d_gss, sc.data(), (size_t)cout * sizeof(float), hipMemcpyHostToDevice));
            CHK(hipMemcpy(op.d_gss + cout, sf.data(), (size_t)cout * sizeof(float), hipMemcpyHostToDevice));
        }
        op.in_buf = in.buf; op.in_ld = in.ld; op.in_coff = in.coff; op.H = in.H; op.W = in.W;
        op.plan.out_dims(in.H, in.W, &op.Ho, &op.Wo);
        op.out_buf = out_buf; op.out_ld = out_ld; op.out_coff = out_coff;
        if (res) { op.res_buf = res->buf; op.res_ld = res->ld; op.res_coff = res->coff; }
        op.macs = (double)in.C * cout * k * k * op.Ho * op.Wo;
        note(op);
        *out = Tn{out_buf, out_ld, out_coff, cout, op.Ho, op.Wo};
        return 0;
    }
    // depthwise 3x3 + BN + ReLU over `Cpad` layout channels of which the first C are the reference's (the rest: zero weights)
    int dw(const std::string& wname, const std::string& bn, const Tn& in, int C, int stride, int out_buf, Tn* out) {
        const int Cpad = (C + 15) / 16 * 16;
        const float* w = sd.get(wname + ".weight", (size_t)C * 9);
        if (!w) return fail(LTK_E_INVALID, "state_dict is missing (or has a wrong shape for) " + wname + ".weight");
        std::vector<float> sc, sf;
        int rc = fold_bn(bn, C, nullptr, &sc, &sf);
        if (rc) return rc;
        std::vector<float> h((size_t)Cpad * 11);
        dw_pack(w, sc.data(), sf.data(), C, Cpad, h.data());
        p->ops.emplace_back();
        UlOp& op = p->ops.back();
        op.type = UL_DW; op.name = wname;
        CHK(hipMalloc((void**)&op.d_dw, h.size() * sizeof(float)));
        CHK(hipMemcpy(op.d_dw, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
        op.C = Cpad; op.Creal = C; op.stride = stride; op.relu = 1;
        op.in_buf = in.buf; op.in_ld = in.ld; op.in_coff = in.coff; op.H = in.H; op.W = in.W;
        op.Ho = (in.H - 1) / stride + 1; op.Wo = (in.W - 1) / stride + 1;
        op.out_buf = out_buf; op.out_ld = Cpad; op.out_coff = 0;
        op.macs = 9.0 * C * op.Ho * op.Wo;
        note(op);
        *out = Tn{out_buf, Cpad, 0, C, op.Ho, op.Wo};
        return 0;
    }
    // InvertedResidual(inp, oup, stride, use_res_connect, expand_ratio = 2), unet.py:7-36: `pre`.conv.{0,1} expand + BN + ReLU,
    // .conv.{3,4} depthwise + BN + ReLU, .conv.{6,7} project + BN (linear), + x where the block has the connection
    int ir(const std::string& pre, const Tn& in, int cout, int stride, bool res, int out_buf, int out_ld, int out_coff, Tn* out) {
        const int mid = in.C * 2;
        Tn e1, e2;
        int rc;
        if (in.C == 6) {        // inc: the expand conv reads the bank crop itself (UL_IN); 12 channels live in one 16-channel block
            const float* w = sd.get(pre + ".conv.0.weight", 72);
            if (!w) return fail(LTK_E_INVALID, "state_dict is missing (or has a wrong shape for) " + pre + ".conv.0.weight");
            std::vector<float> sc, sf;
            if ((rc = fold_bn(pre + ".conv.1", 12, nullptr, &sc, &sf))) return rc;
            memcpy(p->inw.w, w, 72 * sizeof(float));
            memcpy(p->inw.scale, sc.data(), 12 * sizeof(float));
            memcpy(p->inw.shift, sf.data(), 12 * sizeof(float));
            p->ops.emplace_back();
            UlOp& op = p->ops.back();
            op.type = UL_IN; op.name = pre + ".conv.0"; op.in_buf = -1;
            op.C = 16; op.Creal = 12; op.relu = 1; op.H = op.Ho = in.H; op.W = op.Wo = in.W;
            op.out_buf = U_X0; op.out_ld = 16; op.out_coff = 0;
            op.macs = 72.0 * in.H * in.W;
            note(op);
            e1 = Tn{U_X0, 16, 0, 12, in.H, in.W};
        } else {
            if ((rc = conv(pre + ".conv.0", pre + ".conv.1", false, in, mid, 1, 1, 0, 1, nullptr, U_E1, mid, 0, &e1))) return rc;
        }
        if ((rc = dw(pre + ".conv.3", pre + ".conv.4", e1, mid, stride, U_E2, &e2))) return rc;
        if ((rc = conv(pre + ".conv.6", pre + ".conv.7", false, e2, cout, 1, 1, 0, 0, res ? &in : nullptr, out_buf, out_ld, out_coff, out))) return rc;
        return in.C == 6 ? 0 : ir_fused(pre, in, mid, cout, stride, res, out_ld, out_coff);
    }
    // the same block's operands for ul_ir_kernel (knob UL_FUSE_IR, read at enqueue: the three ops above stay), where the program wants the
    // block fused and the planner accepts its geometry at some frame count
    int ir_fused(const std::string& pre, const Tn& in, int mid, int cout, int stride, bool res, int out_ld, int out_coff) {
        if (in.H * in.W < kUlIrMinMapPx) return 0;
        UlIrIO io;
        io.N = 1; io.H = in.H; io.W = in.W; io.Cin = in.C; io.mid = mid; io.Cout = cout; io.stride = stride;
        io.x_ld = in.ld; io.x_coff = in.coff; io.y_ld = out_ld; io.y_coff = out_coff;
        io.has_res = res ? 1 : 0; io.res_ld = in.ld; io.res_coff = in.coff;
        UlIrPlan pl;
        std::string err;
        if (ul_ir_plan(io, false, &pl, &err)) return 0;
        const float* w1 = sd.get(pre + ".conv.0.weight", (size_t)mid * in.C);
        const float* wd = sd.get(pre + ".conv.3.weight", (size_t)mid * 9);
        const float* w2 = sd.get(pre + ".conv.6.weight", (size_t)cout * mid);
        if (!w1 || !wd || !w2) return fail(LTK_E_INVALID, "state_dict is missing (or has a wrong shape for) " + pre + ".conv.{0,3,6}.weight");
        std::vector<float> s1, b1, s_d, b_d, s2, b2;
        int rc;
        if ((rc = fold_bn(pre + ".conv.1", mid, nullptr, &s1, &b1)) || (rc = fold_bn(pre + ".conv.4", mid, nullptr, &s_d, &b_d)) ||
            (rc = fold_bn(pre + ".conv.7", cout, nullptr, &s2, &b2)))
            return rc;
        UlOp& ex = p->ops[p->ops.size() - 3];
        std::vector<uint8_t> img(ul_ir_pack(nullptr, nullptr, nullptr, in.C, mid, cout, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, ex.ir_off));
        ul_ir_pack(w1, wd, w2, in.C, mid, cout, s1.data(), b1.data(), s_d.data(), b_d.data(), s2.data(), b2.data(), img.data(), ex.ir_off);
        CHK(hipMalloc((void**)&ex.d_ir, img.size()));
        CHK(hipMemcpy(ex.d_ir, img.data(), img.size(), hipMemcpyHostToDevice));
        p->ir_bytes += img.size();
        return 0;
    }
    // DoubleConvDW (unet.py:38-49): IR(in -> out, stride), IR(out -> out, 1, residual); the result lands at (out_buf, out_ld, out_coff)
    int dconv(const std::string& pre, const Tn& in, int cout, int stride, int out_buf, int out_ld, int out_coff, Tn* out) {
        const int tmp = (in.buf == U_P || out_buf == U_P) ? U_Q : U_P;
        if (tmp == in.buf || tmp == out_buf) return fail(LTK_E_INVALID, "ultralight program: no free temporary");
        Tn t;
        const int rc = ir(pre + ".double_conv.0", in, cout, stride, false, tmp, cout, 0, &t);
        if (rc) return rc;
        return ir(pre + ".double_conv.1", t, cout, 1, true, out_buf, out_ld, out_coff, out);
    }
    int up(const std::string& name, const Tn& in, int out_buf, int out_ld) {
        p->ops.emplace_back();
        UlOp& op = p->ops.back();
        op.type = UL_UP; op.name = name;
        op.C = op.Creal = in.C;
        op.in_buf = in.buf; op.in_ld = in.ld; op.in_coff = in.coff; op.H = in.H; op.W = in.W;
        op.Ho = 2 * in.H; op.Wo = 2 * in.W;
        op.out_buf = out_buf; op.out_ld = out_ld; op.out_coff = 0;
        note(op);
        return 0;
    }
};

// unet.py:168-215 Model.forward
int build_ul_program(UlProgram* p, const ltk_named_tensor* sd, int n) {
    Builder b{SD{sd, n, ""}, p};
    int rc;
    const int R = kUlRes;
    // ---- face path (unet.py:200-204): every level's output is the skip half of the matching Up's concat buffer
    Tn x1, x2, x3, x4, x5;
    if ((rc = b.ir("inc.inconv.0", Tn{-1, 0, 0, 6, R, R}, 32, 1, false, U_CAT4, 64, 32, &x1))) return rc;
    if ((rc = b.dconv("down1.maxpool_conv.0", x1, 64, 2, U_CAT3, 128, 64, &x2))) return rc;
    if ((rc = b.dconv("down2.maxpool_conv.0", x2, 128, 2, U_CAT2, 256, 128, &x3))) return rc;
    if ((rc = b.dconv("down3.maxpool_conv.0", x3, 256, 2, U_CAT1, 512, 256, &x4))) return rc;
    if ((rc = b.dconv("down4.maxpool_conv.0", x4, 512, 2, U_FCAT, 1024, 0, &x5))) return rc;
    // ---- audio tower (unet.py:132-166 AudioConvHubert): (16, 32, 32) -> 512 x 10 x 10, the second half of the fuse concat
    {
        p->ops.emplace_back();
        UlOp& op = p->ops.back();
        op.type = UL_FEAT; op.name = "audio_feat"; op.in_buf = -1;
        op.C = op.Creal = 16; op.H = op.Ho = 32; op.W = op.Wo = 32;
        op.out_buf = U_FEAT; op.out_ld = 16; op.out_coff = 0;
        b.note(op);
    }
    Tn a{U_FEAT, 16, 0, 16, 32, 32}, t;
    if ((rc = b.ir("audio_model.conv1", a, 64, 1, false, U_P, 64, 0, &t))) return rc;
    if ((rc = b.ir("audio_model.conv2", t, 128, 1, false, U_Q, 128, 0, &a))) return rc;
    if ((rc = b.conv("audio_model.conv3", "audio_model.bn3", true, a, 256, 3, 2, 1, 1, nullptr, U_P, 256, 0, &t))) return rc;
    if ((rc = b.ir("audio_model.conv4", t, 256, 1, true, U_Q, 256, 0, &a))) return rc;
    if ((rc = b.conv("audio_model.conv5", "audio_model.bn5", true, a, 512, 3, 2, 3, 1, nullptr, U_P, 512, 0, &t))) return rc;
    if (t.H != 10 || t.W != 10) return fail(LTK_E_INVALID, "ultralight program: audio tower geometry");
    if ((rc = b.ir("audio_model.conv6", t, 512, 1, true, U_Q, 512, 0, &a))) return rc;
    if ((rc = b.ir("audio_model.conv7", a, 512, 1, true, U_FCAT, 1024, 512, &t))) return rc;
    // ---- fuse (unet.py:207-208)
    Tn f{U_FCAT, 1024, 0, 1024, 10, 10}, g;
    if ((rc = b.dconv("fuse_conv.0", f, 512, 1, U_Q, 512, 0, &g))) return rc;
    if ((rc = b.dconv("fuse_conv.1", g, 256, 1, U_Q, 256, 0, &f))) return rc;
    // ---- decoder (unet.py:72-87, 209-212): cat([up(x), skip]); F.pad is a no-op at 160 x 160
    const struct { const char* name; int cat, cup, cout; } ups[4] = {{"up1", U_CAT1, 256, 128}, {"up2", U_CAT2, 128, 64}, {"up3", U_CAT3, 64, 32}, {"up4", U_CAT4, 32, 32}};
    for (int k = 0; k < 4; ++k) {
        if (f.C != ups[k].cup) return fail(LTK_E_INVALID, "ultralight program: decoder geometry");
        if ((rc = b.up(std::string(ups[k].name) + ".up", f, ups[k].cat, 2 * ups[k].cup))) return rc;
        const Tn c{ups[k].cat, 2 * ups[k].cup, 0, 2 * ups[k].cup, 2 * f.H, 2 * f.W};
        if ((rc = b.dconv(std::string(ups[k].name) + ".conv", c, ups[k].cout, 1, U_Q, ups[k].cout, 0, &f))) return rc;
    }
    if (f.H != R || f.C != 32) return fail(LTK_E_INVALID, "ultralight program: output geometry");
    // ---- outc + sigmoid (unet.py:213-214)
    const float* hw = b.sd.get("outc.conv.weight", 96);
    const float* hb = b.sd.get("outc.conv.bias", 3);
    if (!hw || !hb) return fail(LTK_E_INVALID, "state_dict is missing (or has a wrong shape for) outc.conv.{weight,bias}");
    memcpy(p->headw.w, hw, 96 * sizeof(float));
    memcpy(p->headw.b, hb, 3 * sizeof(float));
    p->ops.emplace_back();
    UlOp& op = p->ops.back();
    op.type = UL_HEAD; op.name = "outc.conv";
    op.C = op.Creal = 3; op.in_buf = f.buf; op.in_ld = 32; op.H = op.Ho = R; op.W = op.Wo = R;
    op.out_buf = f.buf;       // (writes the caller's frames, no arena buffer)
    op.macs = 96.0 * R * R;
    p->macs_per_frame += op.macs;
    // ---- the record the grouped kernels read this avatar's operands from
    if (p->ops.size() > (size_t)kUlMaxOps) return fail(LTK_E_INVALID, "ultralight program: more ops than a grouped record holds");
    std::vector<UlGroupW> rec(1);
    memset(&rec[0], 0, sizeof(UlGroupW));
    for (size_t i = 0; i < p->ops.size(); ++i) {
        const UlOp& o = p->ops[i];
        rec[0].op[i] = UlGroupOp{o.d_gw, o.d_gss, o.d_gss ? o.d_gss + o.C : nullptr, o.d_dw};
    }
    rec[0].inw = p->inw;
    rec[0].headw = p->headw;
    CHK(hipMalloc((void**)&p->d_group, sizeof(UlGroupW)));
    CHK(hipMemcpy(p->d_group, rec.data(), sizeof(UlGroupW), hipMemcpyHostToDevice));
    return 0;
}

// the grouped path's program: the ops' types, views and shapes of the one architecture, no weights (plans, d_dw, d_gw stay empty)
UlProgram* ul_geometry_of(const UlProgram& src) {
    UlProgram* p = new UlProgram();
    for (const UlOp& o : src.ops) {
        p->ops.emplace_back();
        UlOp& g = p->ops.back();
        g.type = o.type; g.name = o.name;
        g.C = o.C; g.Creal = o.Creal; g.stride = o.stride; g.relu = o.relu; g.cin = o.cin; g.k = o.k; g.pad = o.pad;
        g.in_buf = o.in_buf; g.in_ld = o.in_ld; g.in_coff = o.in_coff; g.H = o.H; g.W = o.W;
        g.out_buf = o.out_buf; g.out_ld = o.out_ld; g.out_coff = o.out_coff; g.Ho = o.Ho; g.Wo = o.Wo;
        g.res_buf = o.res_buf; g.res_ld = o.res_ld; g.res_coff = o.res_coff;
        g.macs = o.macs;
    }
    memcpy(p->buf_halfs, src.buf_halfs, sizeof(p->buf_halfs));
    p->macs_per_frame = src.macs_per_frame;
    return p;
}

// the split factor conv3's planner takes for `io` over n frames (force > 0: asked for that factor); 1 where the route has no split
// (the first-generation kernels, lin_fk_kernel).  Pure.
int ul_conv_split(const ConvPlan& plan, ConvIO io, int n, int force, int* ks, std::string* err) {
    ConvReport r;
    memset(&r, 0, sizeof(r));
    io.N = n; io.force_ksplit = force; io.report = &r;
    const int rc = conv_launch_dry(plan, io, err);
    *ks = std::max(1, r.ksplit);
    return rc;
}

// One dense conv of a merged per-avatar pass, `io` over all its frames.  conv3 splits the channel loop of an under-filled launch by a
// factor that follows the launch's frame count, and another factor is another fp32 summation order.  Here every frame takes the factor
// of its OWN call (own[i] frames): neighbouring frames of one factor share a launch that forces it (unsplit: always one launch; split:
// one launch where the planner grants the factor at that size, else launches of at most the own call's size, where it must).
int ul_conv_as_own_calls(const UlOp& op, const ConvIO& io, const std::vector<int>& own, hipStream_t s, std::string* err) {
    const int nf = io.N;
    const size_t xs = (size_t)op.H * op.W * op.in_ld, ys = (size_t)op.Ho * op.Wo * op.out_ld, rs = (size_t)op.Ho * op.Wo * op.res_ld;
    auto launch = [&](int at, int n, int ks) -> int {
        ConvIO sub = io;
        sub.N = n; sub.force_ksplit = ks;
        sub.x = io.x + (size_t)at * xs; sub.y = io.y + (size_t)at * ys;
        if (io.res) sub.res = io.res + (size_t)at * rs;
        return conv_launch(op.plan, sub, s, err);
    };
    std::map<int, int> split_of;              // own-call frame count -> its split factor
    for (int i = 0; i < nf; ++i)
        if (!split_of.count(own[i])) {
            int ks = 1;
            if (const int rc = ul_conv_split(op.plan, io, own[i], 0, &ks, err)) return rc;
            split_of[own[i]] = ks;
        }
    for (int at = 0; at < nf;) {
        const int n_own = own[at], ks = split_of[n_own];
        int end = at + 1;
        while (end < nf && split_of[own[end]] == ks && (ks == 1 || own[end] == n_own)) ++end;
        int step = end - at;
        if (ks > 1) {
            int got = 1;
            if (ul_conv_split(op.plan, io, step, ks, &got, err) || got != ks) step = std::min(step, n_own);
        }
        for (int f = at; f < end; f += step) {
            const int n = std::min(step, end - f);
            if (ks > 1 && n != end - at) {      // (a launch of at most the own call's size: the same scratch fits, the same route)
                int got = 1;
                if (const int rc = ul_conv_split(op.plan, io, n, ks, &got, err)) return rc;
                if (got != ks) { *err = "split factor " + std::to_string(ks) + " of a " + std::to_string(n_own) + "-frame call refused for " + std::to_string(n) + " frames"; return -1; }
            }
            if (const int rc = launch(f, n, ks)) return rc;
        }
        at = end;
    }
    return 0;
}

// the launches of one pass over frames [0, nf); tables in e->ul_tab.  gtab (grouped path): `p` is the geometry-only program and every
// op that has weights takes them per frame through the table (e->ul_gtab), by its index in the program.  own: see ul_pass
int ul_enqueue(ltk_engine* e, UlProgram& p, int nf, hipStream_t s, bool bank, const float* d_img6, bool u8_out, float* d_pred_f32,
               const UlGroupTab* gtab = nullptr, const std::vector<int>* own = nullptr) {
    std::string err;
    // knob UL_FUSE_IR: a per-avatar pass runs an inverted residual that has a fused operand image as ONE ul_ir_kernel launch over all its
    // frames (one summation order whatever the frame count: nothing for ul_conv_as_own_calls to do), from the expand conv's input view
    // into the project conv's output view; U_E1 / U_E2 are not touched.  The grouped path ignores the knob.
    const bool fuse = !gtab && knob(K_UL_FUSE_IR) != 0;
    for (size_t at = 0; at < p.ops.size(); ++at) {
        UlIrIO fio;
        const bool fused = fuse && ul_ir_io(p, at, nf, e->ul_buf, &fio);
        const UlOp& head = p.ops[at];
        if (fused) at += 2;
        UlOp& op = p.ops[at];              // fused: the project conv, whose name and output view the launch has
        const int opi = (int)at;
        const f16* x = op.in_buf >= 0 ? e->ul_buf[op.in_buf] : nullptr;
        f16* y = e->ul_buf[op.out_buf];
        if (fused) {
            const int rc = launch_ul_ir(ul_ir_weights(head.d_ir, head.ir_off), fio, s, nullptr, &err);
            if (rc) return conv_status(rc, op.name + ": " + err);
        } else switch (op.type) {
        case UL_IN:
            if (gtab) launch_ul_in_grouped(bank ? &e->ul_tab->faces : nullptr, d_img6, nf, gtab, y, s);
            else launch_ul_in(bank ? &e->ul_tab->faces : nullptr, d_img6, nf, p.inw, y, s);
            break;
        case UL_FEAT:
            launch_ul_pack_feat(&e->ul_tab->mels, nf, y, s);
            break;
        case UL_DW:
            if (gtab) launch_dwconv3x3_grouped(x, nf, op.in_ld / 16, op.in_coff / 16, op.C, op.H, op.W, op.stride, gtab, opi, op.relu, y,
                                               op.out_ld / 16, op.out_coff / 16, s);
            else launch_dwconv3x3(x, nf, op.in_ld / 16, op.in_coff / 16, op.C, op.H, op.W, op.stride, op.d_dw, op.d_dw + (size_t)op.C * 9,
                             op.d_dw + (size_t)op.C * 10, op.relu, y, op.out_ld / 16, op.out_coff / 16, s);
            break;
        case UL_UP:
            launch_upsample2x(x, nf, op.in_ld / 16, op.in_coff / 16, op.C, op.H, op.W, y, op.out_ld / 16, op.out_coff / 16, s);
            break;
        case UL_HEAD:
            if (gtab) launch_ul_head_grouped(x, nf, gtab, u8_out ? &e->ul_tab->outs : nullptr, d_pred_f32, s);
            else launch_ul_head(x, nf, p.headw, u8_out ? &e->ul_tab->outs : nullptr, d_pred_f32, s);
            break;
        default: if (gtab) {
            UlGconvIO io;
            io.x = x; io.N = nf; io.H = op.H; io.W = op.W; io.x_ld = op.in_ld; io.x_coff = op.in_coff; io.Cin = op.cin; io.Cout = op.C;
            io.y = y; io.y_ld = op.out_ld; io.y_coff = op.out_coff;
            io.res = op.res_buf >= 0 ? e->ul_buf[op.res_buf] : nullptr; io.res_ld = op.res_ld; io.res_coff = op.res_coff;
            io.k = op.k; io.stride = op.stride; io.pad = op.pad; io.relu = op.relu;
            const int rc = launch_ul_gconv(gtab, opi, io, s, &err);
            if (rc) return conv_status(rc, op.name + ": " + err);
        } else {
            ConvIO io;
            io.x = x; io.N = nf; io.H = op.H; io.W = op.W; io.x_ld = op.in_ld; io.x_coff = op.in_coff;
            io.y = y; io.y_ld = op.out_ld; io.y_coff = op.out_coff;
            io.res = op.res_buf >= 0 ? e->ul_buf[op.res_buf] : nullptr; io.res_ld = op.res_ld; io.res_coff = op.res_coff;
            io.relu = op.relu;
            io.partial = e->d_partial; io.partial_cap = e->partial_cap;
            const int rc = own ? ul_conv_as_own_calls(op, io, *own, s, &err) : conv_launch(op.plan, io, s, &err);
            if (rc) return conv_status(rc, op.name + ": " + err);
        }
        }
        CHK(hipGetLastError());
        if (e->capture) {           // ltk_debug_capture: every op's output as NCHW float32 under its name
            std::vector<float>& t = e->taps[op.name];
            t.resize((size_t)nf * op.Creal * op.Ho * op.Wo);
            if (op.type == UL_HEAD) {
                if (!d_pred_f32) { e->taps.erase(op.name); continue; }
                CHK(hipStreamSynchronize(s));
                CHK(hipMemcpy(t.data(), d_pred_f32, t.size() * sizeof(float), hipMemcpyDeviceToHost));
            } else {
                DevBuf tmp;
                CHK(hipMalloc(&tmp.p, t.size() * sizeof(float)));
                launch_nhwc_to_nchw_f32(y, nf, op.Ho, op.Wo, op.out_ld, op.out_coff, op.Creal, (float*)tmp.p, s);
                CHK(hipStreamSynchronize(s));
                CHK(hipMemcpy(t.data(), tmp.p, t.size() * sizeof(float), hipMemcpyDeviceToHost));
            }
            e->tap_shape[op.name] = {nf, op.Creal, op.Ho, op.Wo};
        }
    }
    return 0;
}

// key of a captured Ultralight pass in e->prog_graphs: avatar ids are never reused (a program's address could be)
const void* ul_graph_token(int avatar_id) { return reinterpret_cast<const void*>((uintptr_t)avatar_id); }
// ... of a merged pass whose frames come from own calls of other sizes (e->ul_comps numbers the compositions from 1): the avatar id
// stays in the low half
constexpr int kUlMaxComps = 1024;
const void* ul_comp_token(int avatar_id, int comp) { return reinterpret_cast<const void*>((uintptr_t)(uint32_t)avatar_id | ((uintptr_t)comp << 32)); }
bool ul_token_is_avatar(const void* tok, int avatar_id) {
    const uintptr_t t = reinterpret_cast<uintptr_t>(tok);
    return (uint32_t)t == (uint32_t)avatar_id && (t >> 32) <= (uintptr_t)kUlMaxComps;
}
// ... and of a grouped pass: it holds no avatar's address (the table is filled in front of it), so it outlives every avatar
const void* ul_group_token() { return reinterpret_cast<const void*>(~(uintptr_t)0); }

// the engine's arena serves every Ultralight avatar (one architecture): grown, never shrunk.  Under e->mu.
int ul_arena_reserve(ltk_engine* e, const UlProgram& p, int frames) {
    if (!e->ul_tab) {
        if (hipMalloc((void**)&e->ul_tab, sizeof(DevTables)) != hipSuccess) return fail(LTK_E_NOMEM, "pointer table allocation failed");
        CHK(hipMemset(e->ul_tab, 0, sizeof(DevTables)));
    }
    if (!e->ul_gtab) {
        if (hipMalloc((void**)&e->ul_gtab, sizeof(UlGroupTab)) != hipSuccess) return fail(LTK_E_NOMEM, "pointer table allocation failed");
        CHK(hipMemset(e->ul_gtab, 0, sizeof(UlGroupTab)));
    }
    if (frames <= e->ul_frames) return 0;
    CHK(hipStreamSynchronize(e->compute));
    // captured passes carry the old buffers' addresses
    std::vector<int> ids;
    {
        std::lock_guard<std::mutex> g(e->pool_mu);
        for (auto& kv : e->ul_avatars) ids.push_back(kv.first);
    }
    for (auto it = e->prog_graphs.graphs.begin(); it != e->prog_graphs.graphs.end();) {
        bool ul = it->first.first == ul_group_token();
        for (int id : ids) ul = ul || ul_token_is_avatar(it->first.first, id);
        if (ul) { if (it->second.exec) (void)hipGraphExecDestroy(it->second.exec); it = e->prog_graphs.graphs.erase(it); }
        else ++it;
    }
    for (int i = 0; i < U_COUNT; ++i) {
        if (e->ul_buf[i]) { (void)hipFree(e->ul_buf[i]); e->ul_buf[i] = nullptr; }
    }
    e->ul_frames = 0;
    for (int i = 0; i < U_COUNT; ++i) {
        if (!p.buf_halfs[i]) continue;
        const size_t bytes = p.buf_halfs[i] * (size_t)frames * sizeof(f16) + 4096;
        if (hipMalloc((void**)&e->ul_buf[i], bytes) != hipSuccess) { (void)hipGetLastError(); return fail(LTK_E_NOMEM, "ultralight activation arena allocation failed"); }
        CHK(hipMemset(e->ul_buf[i], 0, bytes));
    }
    e->ul_frames = frames;
    e->ul_frame_bytes = 0;
    for (int i = 0; i < U_COUNT; ++i) e->ul_frame_bytes += p.buf_halfs[i] * sizeof(f16);
    return 0;
}

}  // namespace

int ul_pass(ltk_engine* e, UlAvatar& a, int nf, bool bank, const float* d_img6, bool u8_out, float* d_pred_f32, const std::vector<int>* own) {
    if (nf <= 0 || nf > e->ul_frames || nf > kPackMaxFrames) return fail(LTK_E_INVALID, "ultralight pass: frame count outside the arena");
    if (own && (int)own->size() != nf) return fail(LTK_E_INVALID, "ultralight pass: one own-call frame count per frame");
    if (own && std::all_of(own->begin(), own->end(), [nf](int n) { return n == nf; })) own = nullptr;      // the plain pass, its graph
    hipStream_t s = e->compute;
    auto enq = [&]() -> int { return ul_enqueue(e, *a.prog, nf, s, bank, d_img6, u8_out, d_pred_f32, nullptr, own); };
    // the product configuration (bank crops in, uint8 frames out) has no per-call arguments: captured and replayed (knob GRAPH)
    if (knob(K_GRAPH) && bank && u8_out && !d_pred_f32 && !e->capture) {
        if (!own) return e->prog_graphs.run(e, std::make_pair(ul_graph_token(a.id), nf), s, "ultralight pass", nf, enq);
        // the launches follow the run lengths of `own` alone: one graph per (avatar, composition)
        std::vector<int> comp;
        for (int i = 0; i < nf; ++i) {
            if ((*own)[i] <= 0) return fail(LTK_E_INVALID, "ultralight pass: own-call frame count");
            if (comp.empty() || comp.back() != (*own)[i]) { comp.push_back(1); comp.push_back((*own)[i]); }
            else ++comp[comp.size() - 2];
        }
        auto it = e->ul_comps.find(comp);
        if (it == e->ul_comps.end() && (int)e->ul_comps.size() < kUlMaxComps) it = e->ul_comps.emplace(comp, (int)e->ul_comps.size() + 1).first;
        if (it != e->ul_comps.end())
            return e->prog_graphs.run(e, std::make_pair(ul_comp_token(a.id, it->second), nf), s, "ultralight merged pass", nf, enq);
    }
    return enq();
}

// one pass over frames [0, nf) of SEVERAL avatars: the tables, e->ul_gtab among them, are uploaded; `like`: any avatar's program (the
// geometry is the architecture's).  Captured per frame count under a token of its own.  Under e->mu.
int ul_pass_grouped(ltk_engine* e, const UlAvatar& like, int nf) {
    if (nf <= 0 || nf > e->ul_frames || nf > kPackMaxFrames) return fail(LTK_E_INVALID, "ultralight pass: frame count outside the arena");
    if (!e->ul_gtab || !like.prog) return fail(LTK_E_STATE, "no Ultralight arena");
    if (!e->ul_geo) e->ul_geo = ul_geometry_of(*like.prog);
    hipStream_t s = e->compute;
    auto enq = [&]() -> int { return ul_enqueue(e, *e->ul_geo, nf, s, true, nullptr, true, nullptr, e->ul_gtab); };
    if (knob(K_GRAPH) && !e->capture)
        return e->prog_graphs.run(e, std::make_pair(ul_group_token(), nf), s, "ultralight grouped pass", nf, enq);
    return enq();
}

void ul_drop_graphs(ltk_engine* e, int avatar_id) {
    bool synced = false;
    for (auto it = e->prog_graphs.graphs.begin(); it != e->prog_graphs.graphs.end();) {
        if (!ul_token_is_avatar(it->first.first, avatar_id)) { ++it; continue; }
        if (it->second.exec) {
            if (!synced) { (void)hipSetDevice(e->device); (void)hipStreamSynchronize(e->compute); synced = true; }
            (void)hipGraphExecDestroy(it->second.exec);
        }
        it = e->prog_graphs.graphs.erase(it);
    }
}

void ul_unload(ltk_engine* e) {
    e->ul_avatars.clear();
    for (int i = 0; i < kUlBufs; ++i)
        if (e->ul_buf[i]) { (void)hipFree(e->ul_buf[i]); e->ul_buf[i] = nullptr; }
    if (e->ul_tab) { (void)hipFree(e->ul_tab); e->ul_tab = nullptr; }
    if (e->ul_gtab) { (void)hipFree(e->ul_gtab); e->ul_gtab = nullptr; }
    ul_program_delete(e->ul_geo);
    e->ul_geo = nullptr;
    e->ul_frames = 0;
}

// The passes of one ltk_ultralight_infer_merged call (pure: no engine, no HIP).  Frames keep request order inside a pass; a request is a
// contiguous span, split only at a pass boundary; one request plans what ltk_ultralight_infer runs for it.
int ul_merge_plan(const int* avatar, const int* batch, int nreq, int cap, int mode, bool grouped_ok, bool grouped_knob,
                  std::vector<UlMergePass>* out, std::string* err) {
    out->clear();
    auto bad = [&](const char* m) { if (err) *err = m; return -1; };
    if (!avatar || !batch || nreq <= 0 || cap <= 0 || mode < 0 || mode > 2) return bad("merge plan: bad arguments");
    for (int r = 0; r < nreq; ++r)
        if (batch[r] <= 0) return bad("merge plan: a request without frames");
    std::vector<int> distinct;                 // in order of first appearance
    for (int r = 0; r < nreq; ++r)
        if (std::find(distinct.begin(), distinct.end(), avatar[r]) == distinct.end()) distinct.push_back(avatar[r]);
    if (mode == 2 && !grouped_ok) return bad("merge plan: the grouped path is not available");
    const bool grouped = mode == 2 || (mode == 0 && distinct.size() > 1 && grouped_knob && grouped_ok);
    auto cut = [&](const std::vector<int>& reqs, int path, int av) {
        UlMergePass cur{path, av, 0, {}};
        for (int r : reqs)
            for (int f = 0; f < batch[r];) {
                const int take = std::min(cap - cur.nf, batch[r] - f);
                cur.spans.push_back(UlMergeSpan{r, f, take, cur.nf});
                cur.nf += take; f += take;
                if (cur.nf == cap) { out->push_back(cur); cur = UlMergePass{path, av, 0, {}}; }
            }
        if (cur.nf) out->push_back(cur);
    };
    std::vector<int> reqs;
    if (grouped) {
        for (int r = 0; r < nreq; ++r) reqs.push_back(r);
        cut(reqs, UL_PATH_GROUPED, -1);
        return 0;
    }
    for (int av : distinct) {
        reqs.clear();
        for (int r = 0; r < nreq; ++r)
            if (avatar[r] == av) reqs.push_back(r);
        cut(reqs, UL_PATH_PER_AVATAR, av);
    }
    return 0;
}

}  // namespace ltk

extern "C" {

int ltk_ultralight_avatar_register(ltk_engine* e, const ltk_named_tensor* sd, int n_tensors, const uint8_t* face_bank, const uint8_t* full_bank,
                                   const int32_t* coords, int n, int H, int W, int max_frames, int* avatar_id) {
    if (!e || !sd || n_tensors <= 0 || !face_bank || !full_bank || !coords || !avatar_id || n <= 0 || H <= 0 || W <= 0)
        return fail(LTK_E_INVALID, "bad arguments");
    if (max_frames < 1 || max_frames > kPackMaxFrames) return fail(LTK_E_INVALID, "max_frames must be in [1, 256]");
    for (int i = 0; i < n_tensors; ++i)
        if (!sd[i].name || !sd[i].data || sd[i].ndim < 0 || (sd[i].ndim > 0 && !sd[i].shape)) return fail(LTK_E_INVALID, "state_dict entry without a name, data or shape");
    for (int i = 0; i < n; ++i) {
        const int32_t* c = coords + 4 * i;      // (x1, y1, x2, y2), ultralight_avatar.py:176
        if (c[0] < 0 || c[1] < 0 || c[2] > W || c[3] > H || c[2] <= c[0] || c[3] <= c[1]) return fail(LTK_E_INVALID, "coords box outside the frame");
    }
    CHK(enter_device(e->device));
    auto ap = std::make_shared<UlAvatar>();
    UlAvatar& a = *ap;
    a.device = e->device;
    a.n = n; a.H = H; a.W = W;
    a.boxes.assign(coords, coords + 4 * (size_t)n);
    a.prog = new UlProgram();
    int rc = build_ul_program(a.prog, sd, n_tensors);
    if (rc) return rc;                      // (the avatar's destructor frees the half-built program)
    const size_t fb = (size_t)n * kUlFace * kUlFace * 3, ub = (size_t)n * H * W * 3;
    CHK(hipMalloc((void**)&a.d_face, fb));
    CHK(hipMalloc((void**)&a.d_full, ub));
    CHK(hipMemcpy(a.d_face, face_bank, fb, hipMemcpyHostToDevice));
    CHK(hipMemcpy(a.d_full, full_bank, ub, hipMemcpyHostToDevice));
    {
        std::lock_guard<std::mutex> g(e->mu);
        if ((rc = ul_arena_reserve(e, *a.prog, max_frames))) return rc;
    }
    std::lock_guard<std::mutex> g(e->pool_mu);
    a.id = e->next_avatar++;
    e->ul_avatars[a.id] = ap;
    *avatar_id = a.id;
    return LTK_OK;
}

int ltk_ultralight_infer(ltk_engine* e, const ltk_ul_req* reqs, int nreq, void* stream) {
    if (!e || !reqs || nreq <= 0) return fail(LTK_E_INVALID, "bad arguments");
    std::vector<std::shared_ptr<UlAvatar>> hold;          // the banks and programs stay alive until this call has synchronised
    for (int r = 0; r < nreq; ++r) {
        if (reqs[r].batch <= 0 || reqs[r].index < 0 || !reqs[r].d_feat || !reqs[r].d_pred) return fail(LTK_E_INVALID, "bad request");
        hold.push_back(find_ul_avatar(e, reqs[r].avatar));
        if (!hold.back()) return fail(LTK_E_STATE, "unknown Ultralight avatar id");
    }
    CHK(enter_device(e->device));
    return infer_call(e, stream, [&]() -> int {
        const int cap = std::min(e->ul_frames, kPackMaxFrames);
        if (cap <= 0) return fail(LTK_E_STATE, "no Ultralight arena");
        // every request runs its own avatar's program (the weights are per avatar), in arena-sized launches, back to back on the
        // compute stream; the tables of a launch are uploaded in front of it in stream order
        for (int r = 0; r < nreq; ++r) {
            UlAvatar& a = *hold[r];
            for (int f0 = 0; f0 < reqs[r].batch; f0 += cap) {
                const int nf = std::min(cap, reqs[r].batch - f0);
                FacePtrs fp; MelPtrs mp; OutPtrs op;
                for (int i = 0; i < nf; ++i) {
                    const int idx = mirror_index(a.n, reqs[r].index + f0 + i);      // ultralight_avatar.py:150
                    fp.p[i] = a.d_face + (size_t)idx * kUlFace * kUlFace * 3;
                    mp.p[i] = (const float*)reqs[r].d_feat + (size_t)(f0 + i) * 16 * 1024;
                    op.p[i] = (uint8_t*)reqs[r].d_pred + (size_t)(f0 + i) * kUlRes * kUlRes * 3;
                }
                launch_upload_tables(&fp, &mp, &op, nf, e->ul_tab, e->compute);
                if (hipGetLastError() != hipSuccess) return fail(LTK_E_HIP, "pointer table upload failed");
                const int rc = ul_pass(e, a, nf, true, nullptr, true, nullptr);
                if (rc) return rc;
            }
        }
        return 0;
    });
}

int ltk_ultralight_infer_merged(ltk_engine* e, const ltk_ul_req* reqs, int nreq, int mode, void* stream, ltk_ul_merge_report* rep) {
    if (!reqs || nreq <= 0 || mode < 0 || mode > 2) return fail(LTK_E_INVALID, "bad arguments");
    // every request is checked before anything is launched: a caller that batched several sessions re-issues them one by one after a
    // failure and only the offender fails again (scheduler.py)
    for (int r = 0; r < nreq; ++r)
        if (reqs[r].batch <= 0 || reqs[r].index < 0 || !reqs[r].d_feat || !reqs[r].d_pred) return fail(LTK_E_INVALID, "bad request " + std::to_string(r));
    if (!e) return fail(LTK_E_INVALID, "bad arguments");
    std::vector<std::shared_ptr<UlAvatar>> hold;          // the banks, programs and records stay alive until this call has synchronised
    std::vector<int> av(nreq), nb(nreq);
    for (int r = 0; r < nreq; ++r) {
        hold.push_back(find_ul_avatar(e, reqs[r].avatar));
        if (!hold.back()) return fail(LTK_E_STATE, "unknown Ultralight avatar id (request " + std::to_string(r) + ")");
        av[r] = reqs[r].avatar; nb[r] = reqs[r].batch;
    }
    if (rep) memset(rep, 0, sizeof(*rep));
    CHK(enter_device(e->device));
    return infer_call(e, stream, [&]() -> int {
        const int cap = std::min(e->ul_frames, kPackMaxFrames);
        if (cap <= 0) return fail(LTK_E_STATE, "no Ultralight arena");
        std::vector<UlMergePass> plan;
        std::string err;
        if (ul_merge_plan(av.data(), nb.data(), nreq, cap, mode, e->ul_gtab != nullptr, knob(K_UL_GROUPED) != 0, &plan, &err)) return fail(LTK_E_STATE, err);
        if (rep) {
            std::vector<int> seen;
            for (int a : av)
                if (std::find(seen.begin(), seen.end(), a) == seen.end()) seen.push_back(a);
            rep->n_avatars = (int)seen.size();
        }
        for (const UlMergePass& ps : plan) {
            // the tables of a pass are uploaded in front of it in stream order; a frame's bank crop, features, destination and (grouped)
            // weight record are those of the request that owns it
            FacePtrs fp; MelPtrs mp; OutPtrs op;
            UlGroupTab gt;
            std::vector<int> own(ps.nf);        // the frame count of the ltk_ultralight_infer pass that would carry this frame
            for (const UlMergeSpan& sp : ps.spans) {
                const ltk_ul_req& q = reqs[sp.req];
                const UlAvatar& a = *hold[sp.req];
                for (int i = 0; i < sp.count; ++i) {
                    const int f = sp.first + i, at = sp.at + i;
                    const int idx = mirror_index(a.n, q.index + f);      // ultralight_avatar.py:150
                    fp.p[at] = a.d_face + (size_t)idx * kUlFace * kUlFace * 3;
                    mp.p[at] = (const float*)q.d_feat + (size_t)f * 16 * 1024;
                    op.p[at] = (uint8_t*)q.d_pred + (size_t)f * kUlRes * kUlRes * 3;
                    gt.w[at] = a.prog->d_group;
                    own[at] = std::min(cap, q.batch - f / cap * cap);
                }
            }
            launch_upload_tables(&fp, &mp, &op, ps.nf, e->ul_tab, e->compute);
            if (ps.path == UL_PATH_GROUPED) launch_upload_group_table(&gt, ps.nf, e->ul_gtab, e->compute);
            if (hipGetLastError() != hipSuccess) return fail(LTK_E_HIP, "pointer table upload failed");
            UlAvatar& first = *hold[ps.spans[0].req];
            const int rc = ps.path == UL_PATH_GROUPED ? ul_pass_grouped(e, first, ps.nf) : ul_pass(e, first, ps.nf, true, nullptr, true, nullptr, &own);
            if (rc) return rc;
            if (rep) {
                if (rep->n_passes < LTK_UL_MERGE_MAX_PASSES) {
                    rep->path[rep->n_passes] = ps.path; rep->nf[rep->n_passes] = ps.nf; rep->avatar[rep->n_passes] = ps.avatar;
                }
                rep->n_passes++;
                rep->grouped += ps.path == UL_PATH_GROUPED ? 1 : 0;
                rep->frames += ps.nf;
            }
        }
        return 0;
    });
}

int ltk_ultralight_info(ltk_engine* e, int* arena_frames, size_t* arena_bytes, size_t* bytes_per_frame, int* grouped) {
    if (!e) return fail(LTK_E_INVALID, "bad arguments");
    std::lock_guard<std::mutex> g(e->mu);
    if (arena_frames) *arena_frames = e->ul_frames;
    if (bytes_per_frame) *bytes_per_frame = e->ul_frame_bytes;
    if (arena_bytes) *arena_bytes = e->ul_frame_bytes * (size_t)e->ul_frames;
    if (grouped) *grouped = 1;             // ul_gconv.hip and the grouped kernels of dw_kernels.hip are part of every build
    return LTK_OK;
}

int ltk_debug_ul_merge_plan(const int* avatar, const int* batch, int nreq, int cap, int mode, int grouped_available, int grouped_knob,
                            int* pass_path, int* pass_avatar, int* pass_nf, int max_passes, int* n_passes,
                            int* span_pass, int* span_req, int* span_first, int* span_count, int* span_at, int max_spans, int* n_spans) {
    if (!avatar || !batch || nreq <= 0 || !pass_path || !pass_avatar || !pass_nf || !n_passes || !span_pass || !span_req || !span_first ||
        !span_count || !span_at || !n_spans || max_passes <= 0 || max_spans <= 0)
        return fail(LTK_E_INVALID, "bad arguments");
    std::vector<UlMergePass> plan;
    std::string err;
    const bool knob_on = grouped_knob < 0 ? knob(K_UL_GROUPED) != 0 : grouped_knob != 0;
    if (ul_merge_plan(avatar, batch, nreq, cap, mode, grouped_available != 0, knob_on, &plan, &err)) return fail(LTK_E_INVALID, err);
    int np = 0, ns = 0;
    for (const UlMergePass& ps : plan) {
        if (np >= max_passes) return fail(LTK_E_INVALID, "merge plan: more passes than the caller's arrays hold");
        pass_path[np] = ps.path; pass_avatar[np] = ps.avatar; pass_nf[np] = ps.nf;
        for (const UlMergeSpan& sp : ps.spans) {
            if (ns >= max_spans) return fail(LTK_E_INVALID, "merge plan: more spans than the caller's arrays hold");
            span_pass[ns] = np; span_req[ns] = sp.req; span_first[ns] = sp.first; span_count[ns] = sp.count; span_at[ns] = sp.at;
            ++ns;
        }
        ++np;
    }
    *n_passes = np; *n_spans = ns;
    return LTK_OK;
}

int ltk_ultralight_op_count(ltk_engine* e, int avatar_id) {
    if (!e) return 0;
    const std::shared_ptr<UlAvatar> ap = find_ul_avatar(e, avatar_id);
    return ap && ap->prog ? (int)ul_listing(*ap->prog).size() : 0;
}

int ltk_ultralight_op_name(ltk_engine* e, int avatar_id, int op, char* buf, int buf_len, int* type) {
    if (!e || !buf || buf_len <= 0) return fail(LTK_E_INVALID, "bad arguments");
    const std::shared_ptr<UlAvatar> ap = find_ul_avatar(e, avatar_id);
    if (!ap || !ap->prog) return fail(LTK_E_STATE, "unknown Ultralight avatar id");
    const std::vector<std::pair<std::string, int>> ls = ul_listing(*ap->prog);      // follows knob UL_FUSE_IR
    if (op < 0 || op >= (int)ls.size()) return fail(LTK_E_INVALID, "no such op");
    snprintf(buf, (size_t)buf_len, "%s", ls[op].first.c_str());
    if (type) *type = ls[op].second == UL_CONV ? 0 : 9 + ls[op].second;      // 0 as ltk_musetalk_op_name; 10.. its own
    return LTK_OK;
}

int ltk_ultralight_paste_back(ltk_engine* e, int avatar_id, int idx, const void* d_pred, void* out, int out_is_device, void* stream) {
    if (!e || !d_pred || !out) return fail(LTK_E_INVALID, "bad arguments");
    const std::shared_ptr<UlAvatar> ap = find_ul_avatar(e, avatar_id);
    if (!ap) return fail(LTK_E_STATE, "unknown Ultralight avatar id");
    const UlAvatar& a = *ap;
    if (idx < 0 || idx >= a.n) return fail(LTK_E_INVALID, "frame index outside the bank");
    CHK(enter_device(e->device));
    const int32_t* c = a.boxes.data() + 4 * (size_t)idx;
    const size_t bytes = (size_t)a.H * a.W * 3;
    StreamLease sl(e, stream);
    const uint8_t* full = a.d_full + (size_t)idx * bytes;
    const uint8_t* face = a.d_face + (size_t)idx * kUlFace * kUlFace * 3;
    if (out_is_device) {
        launch_ul_paste(full, a.H, a.W, face, (const uint8_t*)d_pred, c[0], c[1], c[2], c[3], (uint8_t*)out, sl.s);
        CHK(hipGetLastError());
        CHK(hipStreamSynchronize(sl.s));
        return LTK_OK;
    }
    ScratchLease sc(e, bytes);
    if (!sc.s.d) return fail(LTK_E_NOMEM, "scratch allocation failed");
    launch_ul_paste(full, a.H, a.W, face, (const uint8_t*)d_pred, c[0], c[1], c[2], c[3], (uint8_t*)sc.s.d, sl.s);
    const hipError_t pe = hipGetLastError();
    const hipError_t ce = pe == hipSuccess ? hipMemcpyAsync(out, sc.s.d, bytes, hipMemcpyDeviceToHost, sl.s) : pe;
    const hipError_t se = hipStreamSynchronize(sl.s);        // before the scratch goes back to the pool
    if (ce != hipSuccess || se != hipSuccess) return fail(LTK_E_HIP, std::string("ultralight_paste_back: ") + hipGetErrorString(ce != hipSuccess ? ce : se));
    return LTK_OK;
}

int ltk_ultralight_paste_back_batch(ltk_engine* e, int avatar_id, const int32_t* idx, const void* d_pred, int n, void* out, void* stream) {
    if (!e || !idx || !d_pred || !out || n <= 0) return fail(LTK_E_INVALID, "bad arguments");
    const std::shared_ptr<UlAvatar> ap = find_ul_avatar(e, avatar_id);      // held until the stream has been synchronised below
    if (!ap) return fail(LTK_E_STATE, "unknown Ultralight avatar id");
    const UlAvatar& a = *ap;
    for (int i = 0; i < n; ++i)
        if (idx[i] < 0 || idx[i] >= a.n) return fail(LTK_E_INVALID, "frame index outside the bank");
    CHK(enter_device(e->device));
    const size_t bytes = (size_t)a.H * a.W * 3;
    StreamLease sl(e, stream);
    ScratchLease sc(e, bytes * n);
    if (!sc.s.d) return fail(LTK_E_NOMEM, "scratch allocation failed");
    for (int i0 = 0; i0 < n; i0 += kPasteBatch) {          // one launch per 16 frames
        const int m = std::min(kPasteBatch, n - i0);
        UlPasteBatch pb;
        ul_fill_paste_batch(a, idx + i0, m, &pb);
        launch_ul_paste_batch(pb, m, a.H, a.W, (const uint8_t*)d_pred + (size_t)i0 * kUlRes * kUlRes * 3, (uint8_t*)sc.s.d + (size_t)i0 * bytes, bytes, sl.s);
    }
    // an error past this point must not hand the scratch back to the pool while earlier launches may still be writing it
    hipError_t pe = hipGetLastError();
    if (pe == hipSuccess) pe = hipMemcpyAsync(out, sc.s.d, bytes * n, hipMemcpyDeviceToHost, sl.s);
    const hipError_t se = hipStreamSynchronize(sl.s);
    if (pe != hipSuccess || se != hipSuccess) return fail(LTK_E_HIP, std::string("ultralight_paste_back_batch: ") + hipGetErrorString(pe != hipSuccess ? pe : se));
    return LTK_OK;
}

}  // extern "C"

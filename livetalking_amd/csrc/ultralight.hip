// The Ultralight avatar (avatars/ultralight/unet.py Model(6, 'hubert'), avatars/ultralight_avatar.py): a MobileNet-style U-Net at
// 160x160 as a static launch program over a device activation arena.  Every inverted residual (unet.py:7-36) is three launches -
// 1x1 expand on conv3's 1x1 path, depthwise 3x3 and (where the block has one) the residual add in the 1x1 project's epilogue -
// eval-mode BatchNorm folded into scale / shift at register time; torch.cat is a channel-block range of a shared buffer, the
// bilinear upsample writes straight into it.  The ARCHITECTURE (UlArch: ops, views, shapes, arena sizes) is the same for every avatar
// and is built once per process, without a state dict or a HIP call; the MODEL is per avatar (ultralight_avatar.py:69-70), so
// ltk_ultralight_avatar_register builds one operand record per op (UlProgram) that the avatar owns.  The activation arena and the
// pointer tables belong to the engine.  Its VALU kernels are dw_kernels.hip; what the other engine sources call is declared in
// engine_internal.h.
#include "engine_internal.h"
#include "ul_gconv.h"
#include "ul_ir.h"

namespace ltk {

enum UlBuf { U_FEAT = 0, U_X0, U_E1, U_E2, U_P, U_Q, U_CAT1, U_CAT2, U_CAT3, U_CAT4, U_FCAT, U_COUNT };
static_assert(U_COUNT <= kUlBufs, "engine_internal.h kUlBufs");

enum UlOpType { UL_CONV = 0, UL_DW, UL_UP, UL_IN, UL_FEAT, UL_HEAD, UL_IR };      // UL_IR: only in the listing of a fused program (ul_listing)

// one op of the architecture: what it is, what it reads and writes, and where the operand builder finds its tensors
struct UlOp {
    int type = UL_CONV;
    std::string name;               // state_dict prefix of the conv (tap name); "<block>.up" for an upsample
    std::string bn;                 // ... of the BatchNorm2d behind it
    bool bias = false;              // the conv has one (audio_model.conv3 / conv5)
    int cin = 0, cin_real = 0;      // input channels of the layout / of the reference's tensor (inc's project conv reads 12 of 16)
    int k = 1, pad = 0;
    int C = 0, Creal = 0;           // channels the op writes (layout) / of the reference's tensor
    int stride = 1, relu = 0;
    int in_buf = -1, in_ld = 0, in_coff = 0, H = 0, W = 0;
    int out_buf = -1, out_ld = 0, out_coff = 0, Ho = 0, Wo = 0;      // (the head writes the caller's frames: no arena buffer)
    int res_buf = -1, res_ld = 0, res_coff = 0;
    double macs = 0;                // per frame
    int block = -1;                 // the inverted residual it is part of (UlArch::blocks)
};
// an inverted residual: the indices of its three ops, and whether the program wants it as ONE ul_ir_kernel launch under knob UL_FUSE_IR
struct UlBlock { int expand, dw, project; bool fused; };

struct UlArch {
    std::vector<UlOp> ops;
    std::vector<UlBlock> blocks;
    size_t buf_halfs[U_COUNT] = {0};      // per frame
    double macs_per_frame = 0;
    std::string err;                      // non-empty: the tables below do not add up (nothing runs)
};

// The program fuses the inverted residuals whose input map has at least this many pixels (32 x 32: the blocks on the 160^2 .. 40^2 maps and
// the audio tower's first two).  The blocks on the 20^2 maps and below have 512 to 2048 hidden channels and stream weights: ul_ir_kernel
// re-reads them per 8 x 8 tile, and fusing them was not tried.
constexpr int kUlIrMinMapPx = 32 * 32;

namespace {

// the fused launch of block `b` over n frames: from the expand conv's input view into the project conv's output view (bufs: the arena,
// or null for the planner alone)
UlIrIO ul_ir_io(const UlArch& A, const UlBlock& b, int n, f16* const* bufs) {
    const UlOp &ex = A.ops[b.expand], &dw = A.ops[b.dw], &pr = A.ops[b.project];
    UlIrIO io;
    io.N = n; io.H = ex.H; io.W = ex.W; io.Cin = ex.cin; io.mid = ex.C; io.Cout = pr.C; io.stride = dw.stride;
    io.x_ld = ex.in_ld; io.x_coff = ex.in_coff;
    io.y_ld = pr.out_ld; io.y_coff = pr.out_coff;
    io.has_res = pr.res_buf >= 0 ? 1 : 0; io.res_ld = pr.res_ld; io.res_coff = pr.res_coff;
    if (bufs) {
        io.x = bufs[ex.in_buf]; io.y = bufs[pr.out_buf];
        io.res = pr.res_buf >= 0 ? bufs[pr.res_buf] : nullptr;
    }
    return io;
}

struct Tn { int buf, ld, coff, C, H, W; };     // a tensor = channels [coff, coff + C) of a buffer of ld channels

struct ArchBuilder {
    UlArch* a;

    UlOp& add(int type, const std::string& name, const Tn& in, const Tn& out, double macs) {
        a->ops.emplace_back();
        UlOp& op = a->ops.back();
        op.type = type; op.name = name;
        op.in_buf = in.buf; op.in_ld = in.ld; op.in_coff = in.coff; op.H = in.H; op.W = in.W;
        op.out_buf = out.buf; op.out_ld = out.ld; op.out_coff = out.coff; op.Ho = out.H; op.Wo = out.W;
        op.C = op.Creal = out.C; op.cin = op.cin_real = in.C; op.macs = macs;
        if (out.buf >= 0) a->buf_halfs[out.buf] = std::max(a->buf_halfs[out.buf], (size_t)out.ld * out.H * out.W);
        a->macs_per_frame += macs;
        return op;
    }
    // dense conv (1x1 or 3x3) + folded BN (+ conv bias) + optional ReLU / residual
    Tn conv(const std::string& name, const std::string& bn, bool bias, const Tn& in, int cout, int k, int stride, int pad, int relu, const Tn* res,
            int out_buf, int out_ld, int out_coff) {
        const Tn out{out_buf, out_ld, out_coff, cout, (in.H + 2 * pad - k) / stride + 1, (in.W + 2 * pad - k) / stride + 1};
        UlOp& op = add(UL_CONV, name, in, out, (double)in.C * cout * k * k * out.H * out.W);
        op.bn = bn; op.bias = bias; op.stride = stride; op.relu = relu;
        op.cin = (in.C + 15) / 16 * 16; op.k = k; op.pad = pad;
        if (res) { op.res_buf = res->buf; op.res_ld = res->ld; op.res_coff = res->coff; }
        return out;
    }
    // depthwise 3x3 + BN + ReLU over `Cpad` layout channels of which the first C are the reference's (the rest: zero weights)
    Tn dw(const std::string& name, const std::string& bn, const Tn& in, int C, int stride, int out_buf) {
        const int Cpad = (C + 15) / 16 * 16;
        const Tn out{out_buf, Cpad, 0, C, (in.H - 1) / stride + 1, (in.W - 1) / stride + 1};
        UlOp& op = add(UL_DW, name, in, out, 9.0 * C * out.H * out.W);
        op.bn = bn; op.C = op.cin = Cpad; op.cin_real = C; op.k = 3; op.pad = 1; op.stride = stride; op.relu = 1;
        return out;
    }
    // InvertedResidual(inp, oup, stride, use_res_connect, expand_ratio = 2), unet.py:7-36: `pre`.conv.{0,1} expand + BN + ReLU,
    // .conv.{3,4} depthwise + BN + ReLU, .conv.{6,7} project + BN (linear), + x where the block has the connection
    Tn ir(const std::string& pre, const Tn& in, int cout, int stride, bool res, int out_buf, int out_ld, int out_coff) {
        const int mid = in.C * 2, first = (int)a->ops.size();
        Tn e1;
        if (in.C == 6) {        // inc: the expand conv reads the bank crop itself (UL_IN); 12 channels live in one 16-channel block
            e1 = Tn{U_X0, 16, 0, 12, in.H, in.W};
            UlOp& op = add(UL_IN, pre + ".conv.0", in, e1, 72.0 * in.H * in.W);
            op.bn = pre + ".conv.1"; op.C = 16; op.relu = 1;
        } else {
            e1 = conv(pre + ".conv.0", pre + ".conv.1", false, in, mid, 1, 1, 0, 1, nullptr, U_E1, mid, 0);
        }
        const Tn e2 = dw(pre + ".conv.3", pre + ".conv.4", e1, mid, stride, U_E2);
        const Tn out = conv(pre + ".conv.6", pre + ".conv.7", false, e2, cout, 1, 1, 0, 0, res ? &in : nullptr, out_buf, out_ld, out_coff);
        UlBlock b{first, first + 1, first + 2, false};
        for (int i = first; i < first + 3; ++i) a->ops[i].block = (int)a->blocks.size();
        if (in.C != 6 && in.H * in.W >= kUlIrMinMapPx) {      // ... and the planner accepts its geometry
            UlIrPlan pl;
            std::string err;
            b.fused = ul_ir_plan(ul_ir_io(*a, b, 1, nullptr), false, &pl, &err) == 0;
        }
        a->blocks.push_back(b);
        return out;
    }
    // DoubleConvDW (unet.py:38-49): IR(in -> out, stride), IR(out -> out, 1, residual); the result lands at (out_buf, out_ld, out_coff)
    Tn dconv(const std::string& pre, const Tn& in, int cout, int stride, int out_buf, int out_ld, int out_coff) {
        const int tmp = (in.buf == U_P || out_buf == U_P) ? U_Q : U_P;
        if (tmp == in.buf || tmp == out_buf) a->err = "ultralight program: no free temporary";
        const Tn t = ir(pre + ".double_conv.0", in, cout, stride, false, tmp, cout, 0);
        return ir(pre + ".double_conv.1", t, cout, 1, true, out_buf, out_ld, out_coff);
    }
};

// unet.py:168-215 Model.forward
UlArch build_ul_arch() {
    UlArch A;
    ArchBuilder b{&A};
    const int R = kUlRes;
    // ---- face path (unet.py:200-204): every level's output is the skip half of the matching Up's concat buffer
    const Tn x1 = b.ir("inc.inconv.0", Tn{-1, 0, 0, 6, R, R}, 32, 1, false, U_CAT4, 64, 32);
    const Tn x2 = b.dconv("down1.maxpool_conv.0", x1, 64, 2, U_CAT3, 128, 64);
    const Tn x3 = b.dconv("down2.maxpool_conv.0", x2, 128, 2, U_CAT2, 256, 128);
    const Tn x4 = b.dconv("down3.maxpool_conv.0", x3, 256, 2, U_CAT1, 512, 256);
    b.dconv("down4.maxpool_conv.0", x4, 512, 2, U_FCAT, 1024, 0);
    // ---- audio tower (unet.py:132-166 AudioConvHubert): (16, 32, 32) -> 512 x 10 x 10, the second half of the fuse concat
    Tn a{U_FEAT, 16, 0, 16, 32, 32}, t;
    b.add(UL_FEAT, "audio_feat", Tn{-1, 0, 0, 16, 32, 32}, a, 0);
    t = b.ir("audio_model.conv1", a, 64, 1, false, U_P, 64, 0);
    a = b.ir("audio_model.conv2", t, 128, 1, false, U_Q, 128, 0);
    t = b.conv("audio_model.conv3", "audio_model.bn3", true, a, 256, 3, 2, 1, 1, nullptr, U_P, 256, 0);
    a = b.ir("audio_model.conv4", t, 256, 1, true, U_Q, 256, 0);
    t = b.conv("audio_model.conv5", "audio_model.bn5", true, a, 512, 3, 2, 3, 1, nullptr, U_P, 512, 0);
    if (t.H != 10 || t.W != 10) A.err = "ultralight program: audio tower geometry";
    a = b.ir("audio_model.conv6", t, 512, 1, true, U_Q, 512, 0);
    b.ir("audio_model.conv7", a, 512, 1, true, U_FCAT, 1024, 512);
    // ---- fuse (unet.py:207-208)
    Tn f = b.dconv("fuse_conv.0", Tn{U_FCAT, 1024, 0, 1024, 10, 10}, 512, 1, U_Q, 512, 0);
    f = b.dconv("fuse_conv.1", f, 256, 1, U_Q, 256, 0);
    // ---- decoder (unet.py:72-87, 209-212): cat([up(x), skip]); F.pad is a no-op at 160 x 160
    const struct { const char* name; int cat, cup, cout; } ups[4] = {{"up1", U_CAT1, 256, 128}, {"up2", U_CAT2, 128, 64}, {"up3", U_CAT3, 64, 32}, {"up4", U_CAT4, 32, 32}};
    for (int k = 0; k < 4; ++k) {
        if (f.C != ups[k].cup) A.err = "ultralight program: decoder geometry";
        const Tn c{ups[k].cat, 2 * ups[k].cup, 0, 2 * ups[k].cup, 2 * f.H, 2 * f.W};
        b.add(UL_UP, std::string(ups[k].name) + ".up", f, Tn{c.buf, c.ld, 0, f.C, c.H, c.W}, 0);
        f = b.dconv(std::string(ups[k].name) + ".conv", c, ups[k].cout, 1, U_Q, ups[k].cout, 0);
    }
    if (f.H != R || f.C != 32) A.err = "ultralight program: output geometry";
    // ---- outc + sigmoid (unet.py:213-214)
    b.add(UL_HEAD, "outc.conv", f, Tn{-1, 0, 0, 3, R, R}, 96.0 * R * R);
    if (A.ops.size() > (size_t)kUlMaxOps) A.err = "ultralight program: more ops than a grouped record holds";
    return A;
}

const UlArch& ul_arch() {
    static const UlArch A = build_ul_arch();
    return A;
}

// the block that op `at` opens as its expand conv, if the program wants that block fused
const UlBlock* ul_fused_block(const UlArch& A, size_t at) {
    const int b = A.ops[at].block;
    return b >= 0 && A.blocks[b].fused && A.blocks[b].expand == (int)at ? &A.blocks[b] : nullptr;
}

// every launch of a per-avatar pass with the fused route on or off (fuse < 0: as knob UL_FUSE_IR stands).  A fused inverted residual is
// listed once, as UL_IR under its project conv's name: the expand conv's input view and map, the depthwise conv's k / stride / pad,
// everything else the project conv's.  Type codes as ltk_ultralight_op_name documents them.
std::vector<ltk_ul_op_info> ul_listing(int fuse) {
    const UlArch& A = ul_arch();
    const bool fused = fuse < 0 ? knob(K_UL_FUSE_IR) != 0 : fuse != 0;
    std::vector<ltk_ul_op_info> out;
    for (size_t at = 0; at < A.ops.size(); ++at) {
        const UlBlock* b = fused ? ul_fused_block(A, at) : nullptr;
        const UlOp &in = A.ops[at], &op = A.ops[b ? b->project : at], &geo = A.ops[b ? b->dw : at];
        ltk_ul_op_info o;
        memset(&o, 0, sizeof(o));
        snprintf(o.name, sizeof(o.name), "%s", op.name.c_str());
        const int type = b ? (int)UL_IR : op.type;
        o.type = type == UL_CONV ? 0 : 9 + type;      // 0 as ltk_musetalk_op_name; 10.. its own
        o.in_buf = in.in_buf; o.in_ld = in.in_ld; o.in_coff = in.in_coff; o.H = in.H; o.W = in.W; o.cin = in.cin;
        o.out_buf = op.out_buf; o.out_ld = op.out_ld; o.out_coff = op.out_coff; o.Ho = op.Ho; o.Wo = op.Wo;
        o.res_buf = op.res_buf; o.res_ld = op.res_ld; o.res_coff = op.res_coff;
        o.C = op.C; o.Creal = op.Creal; o.relu = op.relu;
        o.k = geo.k; o.stride = geo.stride; o.pad = geo.pad;
        out.push_back(o);
        if (b) at = b->project;
    }
    return out;
}

}  // namespace

// a device allocation that is freed with its owner
template <class T>
struct Dev {
    T* p = nullptr;
    Dev() = default;
    Dev(const Dev&) = delete;
    Dev& operator=(const Dev&) = delete;
    ~Dev() { if (p) (void)hipFree(p); }
    int upload(const T* host, size_t n) {
        CHK(hipMalloc((void**)&p, n * sizeof(T)));
        CHK(hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice));
        return 0;
    }
};

// one avatar's operands of the op of the same index in ul_arch().ops
struct UlOperands {
    ConvPlan plan;                  // UL_CONV
    Dev<float> dw;                  // UL_DW: [C/16][9][16] weights, then scale [C], shift [C]
    Dev<f16> gw;                    // UL_CONV, grouped path: the weights as ul_gconv_pack lays them out, and (gss) scale [C], shift [C]
    Dev<float> gss;
    Dev<uint8_t> ir;                // the expand conv of a block the program wants fused: the block's operand image for ul_ir_kernel
    size_t ir_off[4] = {0, 0, 0, 0};   // (ul_ir_pack) - this op, the depthwise conv and the project conv behind it
    UlOperands() = default;
    ~UlOperands() { conv_plan_destroy(&plan); }
};

struct UlProgram {
    std::vector<UlOperands> w;            // by op index
    UlInW inw;
    UlHeadW headw;
    size_t ir_bytes = 0;                  // operand images of the fused inverted residuals
    Dev<UlGroupW> group;                  // the avatar's record of the grouped path (ul_gconv.h): every op's operands by op index
    UlProgram() : w(ul_arch().ops.size()) {}
};

UlAvatar::UlAvatar() = default;
UlAvatar::~UlAvatar() {
    (void)hipSetDevice(device);
    if (d_face) (void)hipFree(d_face);
    if (d_full) (void)hipFree(d_full);
}       // (the program's operands go behind this body, on the device it selected)

double ul_macs_per_frame() { return ul_arch().macs_per_frame; }

namespace {

const float kUlBnEps = 1e-5f;     // nn.BatchNorm2d default (unet.py:17,26,29)

// One walk over the architecture table: every conv's weights are fetched once and its BatchNorm is folded once (state_dict.h), then
// packed and uploaded in every form a route reads - conv3's plan and ul_gconv_kernel's image of a dense conv, dw_pack's of a depthwise
// one, and, where the program wants the block fused, ul_ir_kernel's image of all three, packed when the walk reaches the project conv.
// (ltk_ultralight_avatar_register has checked that every state_dict entry has a name and data.)
int build_ul_operands(UlProgram* p, const ltk_named_tensor* tensors, int n) {
    const UlArch& A = ul_arch();
    if (!A.err.empty()) return fail(LTK_E_INVALID, A.err);
    SD sd{tensors, n, ""};
    struct Folded { const float* w = nullptr; std::vector<float> sc, sf; };
    std::vector<Folded> host(A.ops.size());
    for (size_t i = 0; i < A.ops.size(); ++i) {
        const UlOp& op = A.ops[i];
        UlOperands& o = p->w[i];
        Folded& h = host[i];
        if (op.type == UL_FEAT || op.type == UL_UP) continue;
        if (op.type == UL_HEAD) {
            const float* hw = sd.get("outc.conv.weight", 96);
            const float* hb = sd.get("outc.conv.bias", 3);
            if (!hw || !hb) return fail(LTK_E_INVALID, "state_dict is missing (or has a wrong shape for) outc.conv.{weight,bias}");
            memcpy(p->headw.w, hw, 96 * sizeof(float));
            memcpy(p->headw.b, hb, 3 * sizeof(float));
            continue;
        }
        const int C = op.Creal;
        h.w = sd.get(op.name + ".weight", op.type == UL_DW ? (size_t)C * 9 : (size_t)C * op.cin_real * op.k * op.k);
        const float* bias = op.bias ? sd.get(op.name + ".bias", C) : nullptr;
        if (!h.w || (op.bias && !bias))
            return fail(LTK_E_INVALID, "state_dict is missing (or has a wrong shape for) " + op.name + (op.type == UL_CONV ? ".weight / .bias" : ".weight"));
        const float* g = sd.get(op.bn + ".weight", C);
        const float* b = sd.get(op.bn + ".bias", C);
        const float* m = sd.get(op.bn + ".running_mean", C);
        const float* v = sd.get(op.bn + ".running_var", C);
        if (!g || !b || !m || !v) return fail(LTK_E_INVALID, "state_dict is missing (or has a wrong shape for) the BatchNorm tensors " + op.bn + ".*");
        h.sc.resize(C); h.sf.resize(C);
        fold_bn(g, b, m, v, bias, kUlBnEps, C, h.sc.data(), h.sf.data());
        int rc = 0;
        if (op.type == UL_IN) {
            memcpy(p->inw.w, h.w, 72 * sizeof(float));
            memcpy(p->inw.scale, h.sc.data(), 12 * sizeof(float));
            memcpy(p->inw.shift, h.sf.data(), 12 * sizeof(float));
        } else if (op.type == UL_DW) {
            std::vector<float> img((size_t)op.C * 11);
            dw_pack(h.w, h.sc.data(), h.sf.data(), C, op.C, img.data());
            if ((rc = o.dw.upload(img.data(), img.size()))) return rc;
        } else {
            std::string err;
            rc = conv_plan_create(&o.plan, h.w, op.cin_real, C, op.k, op.k, op.stride, op.stride, op.pad, op.pad, false, 0, h.sc.data(), h.sf.data(), &err);
            if (rc) return conv_status(rc, op.name + ": " + err);
            // the grouped path's copy: fp16 weights in ul_gconv_kernel's operand layout (zeros behind channel cin_real), fp32 scale / shift
            std::vector<f16> gw(ul_gconv_pack(h.w, op.cin_real, C, op.k, nullptr));
            ul_gconv_pack(h.w, op.cin_real, C, op.k, gw.data());
            std::vector<float> ss(h.sc);
            ss.insert(ss.end(), h.sf.begin(), h.sf.end());
            if ((rc = o.gw.upload(gw.data(), gw.size())) || (rc = o.gss.upload(ss.data(), ss.size()))) return rc;
        }
        const UlBlock* blk = op.block >= 0 ? &A.blocks[op.block] : nullptr;
        if (blk && blk->fused && blk->project == (int)i) {
            const Folded &ex = host[blk->expand], &dw = host[blk->dw];
            const int cin = A.ops[blk->expand].cin_real, mid = A.ops[blk->dw].Creal;
            UlOperands& to = p->w[blk->expand];
            std::vector<uint8_t> img(ul_ir_pack(nullptr, nullptr, nullptr, cin, mid, C, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, to.ir_off));
            ul_ir_pack(ex.w, dw.w, h.w, cin, mid, C, ex.sc.data(), ex.sf.data(), dw.sc.data(), dw.sf.data(), h.sc.data(), h.sf.data(), img.data(), to.ir_off);
            if ((rc = to.ir.upload(img.data(), img.size()))) return rc;
            p->ir_bytes += img.size();
        }
    }
    // ---- the record the grouped kernels read this avatar's operands from
    std::vector<UlGroupW> rec(1);
    memset(&rec[0], 0, sizeof(UlGroupW));
    for (size_t i = 0; i < A.ops.size(); ++i) {
        const UlOperands& o = p->w[i];
        rec[0].op[i] = UlGroupOp{o.gw.p, o.gss.p, o.gss.p ? o.gss.p + A.ops[i].C : nullptr, o.dw.p};
    }
    rec[0].inw = p->inw;
    rec[0].headw = p->headw;
    return p->group.upload(rec.data(), 1);
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
int ul_conv_as_own_calls(const UlOp& op, const ConvPlan& plan, const ConvIO& io, const std::vector<int>& own, hipStream_t s, std::string* err) {
    const int nf = io.N;
    const size_t xs = (size_t)op.H * op.W * op.in_ld, ys = (size_t)op.Ho * op.Wo * op.out_ld, rs = (size_t)op.Ho * op.Wo * op.res_ld;
    auto launch = [&](int at, int n, int ks) -> int {
        ConvIO sub = io;
        sub.N = n; sub.force_ksplit = ks;
        sub.x = io.x + (size_t)at * xs; sub.y = io.y + (size_t)at * ys;
        if (io.res) sub.res = io.res + (size_t)at * rs;
        return conv_launch(plan, sub, s, err);
    };
    std::map<int, int> split_of;              // own-call frame count -> its split factor
    for (int i = 0; i < nf; ++i)
        if (!split_of.count(own[i])) {
            int ks = 1;
            if (const int rc = ul_conv_split(plan, io, own[i], 0, &ks, err)) return rc;
            split_of[own[i]] = ks;
        }
    for (int at = 0; at < nf;) {
        const int n_own = own[at], ks = split_of[n_own];
        int end = at + 1;
        while (end < nf && split_of[own[end]] == ks && (ks == 1 || own[end] == n_own)) ++end;
        int step = end - at;
        if (ks > 1) {
            int got = 1;
            if (ul_conv_split(plan, io, step, ks, &got, err) || got != ks) step = std::min(step, n_own);
        }
        for (int f = at; f < end; f += step) {
            const int n = std::min(step, end - f);
            if (ks > 1 && n != end - at) {      // (a launch of at most the own call's size: the same scratch fits, the same route)
                int got = 1;
                if (const int rc = ul_conv_split(plan, io, n, ks, &got, err)) return rc;
                if (got != ks) { *err = "split factor " + std::to_string(ks) + " of a " + std::to_string(n_own) + "-frame call refused for " + std::to_string(n) + " frames"; return -1; }
            }
            if (const int rc = launch(f, n, ks)) return rc;
        }
        at = end;
    }
    return 0;
}

// The launches of one pass over frames [0, nf): a walk over the architecture table, the per-frame tables in e->ul_tab.  Where an op
// has operands they are `w`'s, the avatar's, or (a.gtab, the grouped path: w is null) every frame's own through the table, by op index.
int ul_enqueue(ltk_engine* e, const UlProgram* w, int nf, hipStream_t s, const UlPassArgs& a) {
    const UlArch& A = ul_arch();
    std::string err;
    const FacePtrs* faces = a.d_img6 ? nullptr : &e->ul_tab->faces;
    const OutPtrs* outs = a.d_pred_f32 ? nullptr : &e->ul_tab->outs;
    // knob UL_FUSE_IR: a per-avatar pass runs an inverted residual the program wants fused as ONE ul_ir_kernel launch over all its frames
    // (one summation order whatever the frame count: nothing for ul_conv_as_own_calls to do), from the expand conv's input view into the
    // project conv's output view; U_E1 / U_E2 are not touched.  The grouped path ignores the knob.
    const bool fuse = !a.gtab && knob(K_UL_FUSE_IR) != 0;
    for (size_t at = 0; at < A.ops.size(); ++at) {
        const UlBlock* blk = fuse ? ul_fused_block(A, at) : nullptr;
        // -1: the op's own launch (no fused block opens here, or the planner, asked once by the launcher, refuses this frame count)
        int rc = blk ? launch_ul_ir(ul_ir_weights(w->w[at].ir.p, w->w[at].ir_off), ul_ir_io(A, *blk, nf, e->ul_buf), s, nullptr, &err) : -1;
        if (rc != -1) at = blk->project;   // the launch has the project conv's name and output view
        const UlOp& op = A.ops[at];
        const int opi = (int)at, ldb = op.in_ld / 16, cb = op.in_coff / 16, oldb = op.out_ld / 16, ocb = op.out_coff / 16;
        const f16* x = op.in_buf >= 0 ? e->ul_buf[op.in_buf] : nullptr;
        f16* y = op.out_buf >= 0 ? e->ul_buf[op.out_buf] : nullptr;
        f16* res = op.res_buf >= 0 ? e->ul_buf[op.res_buf] : nullptr;
        if (rc == -1) {
            rc = 0;
            if (op.type == UL_FEAT) launch_ul_pack_feat(&e->ul_tab->mels, nf, y, s);
            else if (op.type == UL_UP) launch_upsample2x(x, nf, ldb, cb, op.C, op.H, op.W, y, oldb, ocb, s);
            else if (a.gtab) switch (op.type) {
                case UL_IN: launch_ul_in_grouped(faces, a.d_img6, nf, a.gtab, y, s); break;
                case UL_DW: launch_dwconv3x3_grouped(x, nf, ldb, cb, op.C, op.H, op.W, op.stride, a.gtab, opi, op.relu, y, oldb, ocb, s); break;
                case UL_HEAD: launch_ul_head_grouped(x, nf, a.gtab, outs, a.d_pred_f32, s); break;
                default: {
                    UlGconvIO io;
                    io.x = x; io.N = nf; io.H = op.H; io.W = op.W; io.x_ld = op.in_ld; io.x_coff = op.in_coff; io.Cin = op.cin; io.Cout = op.C;
                    io.y = y; io.y_ld = op.out_ld; io.y_coff = op.out_coff;
                    io.res = res; io.res_ld = op.res_ld; io.res_coff = op.res_coff;
                    io.k = op.k; io.stride = op.stride; io.pad = op.pad; io.relu = op.relu;
                    rc = launch_ul_gconv(a.gtab, opi, io, s, &err);
                }
            } else switch (op.type) {
                case UL_IN: launch_ul_in(faces, a.d_img6, nf, w->inw, y, s); break;
                case UL_DW: {
                    const float* d = w->w[at].dw.p;
                    launch_dwconv3x3(x, nf, ldb, cb, op.C, op.H, op.W, op.stride, d, d + (size_t)op.C * 9, d + (size_t)op.C * 10, op.relu, y, oldb, ocb, s);
                    break;
                }
                case UL_HEAD: launch_ul_head(x, nf, w->headw, outs, a.d_pred_f32, s); break;
                default: {
                    ConvIO io;
                    io.x = x; io.N = nf; io.H = op.H; io.W = op.W; io.x_ld = op.in_ld; io.x_coff = op.in_coff;
                    io.y = y; io.y_ld = op.out_ld; io.y_coff = op.out_coff;
                    io.res = res; io.res_ld = op.res_ld; io.res_coff = op.res_coff;
                    io.relu = op.relu;
                    io.partial = e->d_partial; io.partial_cap = e->partial_cap;
                    rc = a.own ? ul_conv_as_own_calls(op, w->w[at].plan, io, *a.own, s, &err) : conv_launch(w->w[at].plan, io, s, &err);
                }
            }
        }
        if (rc) return conv_status(rc, op.name + ": " + err);
        CHK(hipGetLastError());
        // a watched call: what this launch left in the arena (the head writes bytes; a fused block's hidden tensors never exist)
        if (a.health && y && op.type != UL_HEAD) a.health->scan(opi, y, nf, oldb, ocb, op.C / 16, (long long)op.Ho * op.Wo, 0, s);
        if (e->capture) {           // ltk_debug_capture: every op's output as NCHW float32 under its name
            std::vector<float>& t = e->taps[op.name];
            t.resize((size_t)nf * op.Creal * op.Ho * op.Wo);
            if (op.type == UL_HEAD) {
                if (!a.d_pred_f32) { e->taps.erase(op.name); continue; }
                CHK(hipStreamSynchronize(s));
                CHK(hipMemcpy(t.data(), a.d_pred_f32, t.size() * sizeof(float), hipMemcpyDeviceToHost));
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

// under e->mu: the captured passes whose token `is_ul` accepts leave e->prog_graphs, the stream drained before the first is destroyed
template <class Pred>
void ul_erase_graphs(ltk_engine* e, Pred is_ul) {
    bool synced = false;
    for (auto it = e->prog_graphs.graphs.begin(); it != e->prog_graphs.graphs.end();) {
        if (!is_ul(it->first.first)) { ++it; continue; }
        if (it->second.exec) {
            if (!synced) { (void)hipSetDevice(e->device); (void)hipStreamSynchronize(e->compute); synced = true; }
            (void)hipGraphExecDestroy(it->second.exec);
        }
        it = e->prog_graphs.graphs.erase(it);
    }
}

// the engine's arena serves every Ultralight avatar (one architecture): grown, never shrunk.  Under e->mu.
int ul_arena_reserve(ltk_engine* e, int frames) {
    const UlArch& A = ul_arch();
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
    ul_erase_graphs(e, [&](const void* tok) {
        return tok == ul_group_token() || std::any_of(ids.begin(), ids.end(), [tok](int id) { return ul_token_is_avatar(tok, id); });
    });
    for (int i = 0; i < U_COUNT; ++i) {
        if (e->ul_buf[i]) { (void)hipFree(e->ul_buf[i]); e->ul_buf[i] = nullptr; }
    }
    e->ul_frames = 0;
    for (int i = 0; i < U_COUNT; ++i) {
        if (!A.buf_halfs[i]) continue;
        const size_t bytes = A.buf_halfs[i] * (size_t)frames * sizeof(f16) + 4096;
        if (hipMalloc((void**)&e->ul_buf[i], bytes) != hipSuccess) { (void)hipGetLastError(); return fail(LTK_E_NOMEM, "ultralight activation arena allocation failed"); }
        CHK(hipMemset(e->ul_buf[i], 0, bytes));
    }
    e->ul_frames = frames;
    e->ul_frame_bytes = 0;
    for (int i = 0; i < U_COUNT; ++i) e->ul_frame_bytes += A.buf_halfs[i] * sizeof(f16);
    return 0;
}

}  // namespace

int ul_pass(ltk_engine* e, const UlAvatar& av, int nf, UlPassArgs a) {
    if (nf <= 0 || nf > e->ul_frames || nf > kPackMaxFrames) return fail(LTK_E_INVALID, "ultralight pass: frame count outside the arena");
    if (a.own && (int)a.own->size() != nf) return fail(LTK_E_INVALID, "ultralight pass: one own-call frame count per frame");
    if (a.own && std::all_of(a.own->begin(), a.own->end(), [nf](int n) { return n == nf; })) a.own = nullptr;      // the plain pass, its graph
    hipStream_t s = e->compute;
    auto enq = [&]() -> int { return ul_enqueue(e, av.prog.get(), nf, s, a); };
    // the product configuration (bank crops in, uint8 frames out) has no per-call arguments: captured and replayed (knob GRAPH)
    if (knob(K_GRAPH) && !a.d_img6 && !a.d_pred_f32 && !e->capture && !a.health) {
        if (!a.own) return e->prog_graphs.run(e, std::make_pair(ul_graph_token(av.id), nf), s, "ultralight pass", nf, enq);
        // the launches follow the run lengths of `own` alone: one graph per (avatar, composition)
        std::vector<int> comp;
        for (int i = 0; i < nf; ++i) {
            if ((*a.own)[i] <= 0) return fail(LTK_E_INVALID, "ultralight pass: own-call frame count");
            if (comp.empty() || comp.back() != (*a.own)[i]) { comp.push_back(1); comp.push_back((*a.own)[i]); }
            else ++comp[comp.size() - 2];
        }
        auto it = e->ul_comps.find(comp);
        if (it == e->ul_comps.end() && (int)e->ul_comps.size() < kUlMaxComps) it = e->ul_comps.emplace(comp, (int)e->ul_comps.size() + 1).first;
        if (it != e->ul_comps.end())
            return e->prog_graphs.run(e, std::make_pair(ul_comp_token(av.id, it->second), nf), s, "ultralight merged pass", nf, enq);
    }
    return enq();
}

namespace {

// one pass over frames [0, nf) of SEVERAL avatars: the tables, e->ul_gtab among them, are uploaded.  Captured per frame count under a
// token of its own.  Under e->mu.
int ul_pass_grouped(ltk_engine* e, int nf) {
    if (nf <= 0 || nf > e->ul_frames || nf > kPackMaxFrames) return fail(LTK_E_INVALID, "ultralight pass: frame count outside the arena");
    if (!e->ul_gtab) return fail(LTK_E_STATE, "no Ultralight arena");
    hipStream_t s = e->compute;
    UlPassArgs a;
    a.gtab = e->ul_gtab;
    auto enq = [&]() -> int { return ul_enqueue(e, nullptr, nf, s, a); };
    if (knob(K_GRAPH) && !e->capture)
        return e->prog_graphs.run(e, std::make_pair(ul_group_token(), nf), s, "ultralight grouped pass", nf, enq);
    return enq();
}

}  // namespace

void ul_health_listing(std::vector<std::string>* names, std::vector<int>* types, std::vector<int>* arch_index) {
    const UlArch& A = ul_arch();
    const bool fused = knob(K_UL_FUSE_IR) != 0;
    const std::vector<ltk_ul_op_info> ls = ul_listing(fused ? 1 : 0);
    size_t li = 0;
    for (size_t at = 0; at < A.ops.size() && li < ls.size(); ++at, ++li) {      // ul_listing's walk
        const UlBlock* b = fused ? ul_fused_block(A, at) : nullptr;
        if (b) at = b->project;
        names->push_back(ls[li].name); types->push_back(ls[li].type); arch_index->push_back((int)at);
    }
}

void ul_drop_graphs(ltk_engine* e, int avatar_id) {
    ul_erase_graphs(e, [avatar_id](const void* tok) { return ul_token_is_avatar(tok, avatar_id); });
}

void ul_unload(ltk_engine* e) {
    e->ul_avatars.clear();
    for (int i = 0; i < kUlBufs; ++i)
        if (e->ul_buf[i]) { (void)hipFree(e->ul_buf[i]); e->ul_buf[i] = nullptr; }
    if (e->ul_tab) { (void)hipFree(e->ul_tab); e->ul_tab = nullptr; }
    if (e->ul_gtab) { (void)hipFree(e->ul_gtab); e->ul_gtab = nullptr; }
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

namespace {

// The body of both infer entries, under e->mu: the passes ul_merge_plan cuts `nreq` checked requests into (hold[r]: request r's avatar,
// kept alive until the call has synchronised), each behind its tables in stream order, and the report (or null).
// `watched`: the avatars whose headroom watch counts this engine call (ul_health_begin); their per-avatar passes are scanned.
int ul_run_requests(ltk_engine* e, const ltk_ul_req* reqs, const std::shared_ptr<UlAvatar>* hold, int nreq, int mode, ltk_ul_merge_report* rep,
                    const std::vector<const UlAvatar*>& watched) {
    const int cap = std::min(e->ul_frames, kPackMaxFrames);
    if (cap <= 0) return fail(LTK_E_STATE, "no Ultralight arena");
    std::vector<int> av(nreq), nb(nreq);
    for (int r = 0; r < nreq; ++r) { av[r] = reqs[r].avatar; nb[r] = reqs[r].batch; }
    std::vector<UlMergePass> plan;
    std::string err;
    if (ul_merge_plan(av.data(), nb.data(), nreq, cap, mode, e->ul_gtab != nullptr, knob(K_UL_GROUPED) != 0, &plan, &err)) return fail(LTK_E_STATE, err);
    if (rep) {
        std::sort(av.begin(), av.end());
        rep->n_avatars = (int)(std::unique(av.begin(), av.end()) - av.begin());
    }
    for (const UlMergePass& ps : plan) {
        // a frame's bank crop, features, destination and (grouped) weight record are those of the request that owns it
        FacePtrs fp; MelPtrs mp; OutPtrs op;
        UlGroupTab gt;
        std::vector<int> own(ps.nf);        // the frame count of the pass that would carry this frame if its request came alone
        for (const UlMergeSpan& sp : ps.spans) {
            const ltk_ul_req& q = reqs[sp.req];
            const UlAvatar& a = *hold[sp.req];
            for (int i = 0; i < sp.count; ++i) {
                const int f = sp.first + i, at = sp.at + i;
                const int idx = mirror_index(a.n, q.index + f);      // ultralight_avatar.py:150
                fp.p[at] = a.d_face + (size_t)idx * kUlFace * kUlFace * 3;
                mp.p[at] = (const float*)q.d_feat + (size_t)f * 16 * 1024;
                op.p[at] = (uint8_t*)q.d_pred + (size_t)f * kUlRes * kUlRes * 3;
                gt.w[at] = a.prog->group.p;
                own[at] = std::min(cap, q.batch - f / cap * cap);
            }
        }
        launch_upload_tables(&fp, &mp, &op, ps.nf, e->ul_tab, e->compute);
        if (ps.path == UL_PATH_GROUPED) launch_upload_group_table(&gt, ps.nf, e->ul_gtab, e->compute);
        if (hipGetLastError() != hipSuccess) return fail(LTK_E_HIP, "pointer table upload failed");
        UlPassArgs a;
        a.own = &own;
        if (ps.path != UL_PATH_GROUPED && std::find(watched.begin(), watched.end(), hold[ps.spans[0].req].get()) != watched.end())
            a.health = hold[ps.spans[0].req]->health.get();
        const int rc = ps.path == UL_PATH_GROUPED ? ul_pass_grouped(e, ps.nf) : ul_pass(e, *hold[ps.spans[0].req], ps.nf, a);
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
}

// under e->mu, once per engine call: every avatar of the call whose watch is armed counts the call
std::vector<const UlAvatar*> ul_health_begin(const std::shared_ptr<UlAvatar>* hold, int nreq) {
    std::vector<const UlAvatar*> watched;
    for (int r = 0; r < nreq; ++r) {
        const UlAvatar* a = hold[r].get();
        if (std::find(watched.begin(), watched.end(), a) != watched.end() || !a->health || a->health->left <= 0) continue;
        if (a->health->begin()) watched.push_back(a);
    }
    return watched;
}

}  // namespace

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
    a.prog.reset(new UlProgram());
    int rc = build_ul_operands(a.prog.get(), sd, n_tensors);
    if (rc) return rc;                      // (the avatar's destructor frees the half-built program)
    a.health.reset(new HealthWatch());
    if (a.health->alloc((int)ul_arch().ops.size())) return fail(LTK_E_NOMEM, "health table allocation failed");
    const size_t fb = (size_t)n * kUlFace * kUlFace * 3, ub = (size_t)n * H * W * 3;
    CHK(hipMalloc((void**)&a.d_face, fb));
    CHK(hipMalloc((void**)&a.d_full, ub));
    CHK(hipMemcpy(a.d_face, face_bank, fb, hipMemcpyHostToDevice));
    CHK(hipMemcpy(a.d_full, full_bank, ub, hipMemcpyHostToDevice));
    {
        std::lock_guard<std::mutex> g(e->mu);
        if ((rc = ul_arena_reserve(e, max_frames))) return rc;
    }
    std::lock_guard<std::mutex> g(e->pool_mu);
    a.id = e->next_avatar++;
    e->ul_avatars[a.id] = ap;
    *avatar_id = a.id;
    return LTK_OK;
}

// every request on its own, in order: the per-avatar plan of that request alone (arena-sized passes back to back on the compute stream)
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
        int rc = 0;
        const std::vector<const UlAvatar*> watched = ul_health_begin(hold.data(), nreq);
        for (int r = 0; r < nreq && !rc; ++r) rc = ul_run_requests(e, reqs + r, hold.data() + r, 1, /* mode: per avatar */ 1, nullptr, watched);
        return rc;
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
    for (int r = 0; r < nreq; ++r) {
        hold.push_back(find_ul_avatar(e, reqs[r].avatar));
        if (!hold.back()) return fail(LTK_E_STATE, "unknown Ultralight avatar id (request " + std::to_string(r) + ")");
    }
    if (rep) memset(rep, 0, sizeof(*rep));
    CHK(enter_device(e->device));
    return infer_call(e, stream, [&]() -> int { return ul_run_requests(e, reqs, hold.data(), nreq, mode, rep, ul_health_begin(hold.data(), nreq)); });
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

int ltk_debug_ultralight_program(int fuse, ltk_ul_op_info* ops, int max_ops, int* n_ops, uint64_t* buf_halfs, int max_bufs, int* n_bufs) {
    if (!ops || !n_ops || !buf_halfs || !n_bufs || fuse < -1 || fuse > 1) return fail(LTK_E_INVALID, "bad arguments");
    if (!ul_arch().err.empty()) return fail(LTK_E_STATE, ul_arch().err);
    const std::vector<ltk_ul_op_info> ls = ul_listing(fuse);
    if (max_ops < (int)ls.size() || max_bufs < (int)U_COUNT) return fail(LTK_E_INVALID, "ultralight program: more ops or buffers than the caller's arrays hold");
    std::copy(ls.begin(), ls.end(), ops);
    for (int i = 0; i < U_COUNT; ++i) buf_halfs[i] = ul_arch().buf_halfs[i];
    *n_ops = (int)ls.size(); *n_bufs = U_COUNT;
    return LTK_OK;
}

int ltk_ultralight_op_count(ltk_engine* e, int avatar_id) {
    return e && find_ul_avatar(e, avatar_id) ? (int)ul_listing(-1).size() : 0;
}

int ltk_ultralight_op_name(ltk_engine* e, int avatar_id, int op, char* buf, int buf_len, int* type) {
    if (!e || !buf || buf_len <= 0) return fail(LTK_E_INVALID, "bad arguments");
    if (!find_ul_avatar(e, avatar_id)) return fail(LTK_E_STATE, "unknown Ultralight avatar id");
    const std::vector<ltk_ul_op_info> ls = ul_listing(-1);      // follows knob UL_FUSE_IR
    if (op < 0 || op >= (int)ls.size()) return fail(LTK_E_INVALID, "no such op");
    snprintf(buf, (size_t)buf_len, "%s", ls[op].name);
    if (type) *type = ls[op].type;
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

// fp_program and fp_plan: see faceparse.h.  Host code only.
#include "faceparse.h"

#include <string.h>

#include <map>

namespace ltk {

std::vector<FpOp> fp_program(int S) {
    std::vector<FpOp> ops;
    if (S < 64 || S > 512 || S % 32) return ops;
    auto add = [&](const std::string& name, int type, int cin, int cout, int H, int Ho) -> FpOp& {
        FpOp op;
        op.name = name; op.type = type; op.cin = cin; op.cout = cout; op.H = op.W = H; op.Ho = op.Wo = Ho;
        ops.push_back(op);
        return ops.back();
    };
    auto conv = [&](const std::string& name, int cin, int cout, int k, int stride, int H, int relu, int has_res = 0, int ups = 0) {
        FpOp& op = add(name, 0, cin, cout, H, H / stride);
        op.k = k; op.stride = stride; op.pad = k / 2; op.relu = relu; op.has_res = has_res; op.ups = ups;
    };
    {   // cp.resnet (resnet.py:71-80)
        FpOp& st = add("cp.resnet.conv1", 10, 3, 64, S, S / 2);
        st.k = 7; st.stride = 2; st.pad = 3; st.relu = 1;
        FpOp& mp = add("cp.resnet.maxpool", 11, 64, 64, S / 2, S / 4);
        mp.k = 3; mp.stride = 2; mp.pad = 1;
    }
    const int chans[4] = {64, 128, 256, 512};
    int C = 64, H = S / 4;
    for (int l = 0; l < 4; ++l)
        for (int b = 0; b < 2; ++b) {                      // BasicBlock (resnet.py:36-48): the shortcut is the second conv's residual
            const std::string p = "cp.resnet.layer" + std::to_string(l + 1) + "." + std::to_string(b);
            const bool down = l > 0 && b == 0;
            const int st = down ? 2 : 1;
            conv(p + ".conv1", C, chans[l], 3, st, H, 1);
            if (down) conv(p + ".downsample.0", C, chans[l], 1, st, H, 0);
            H /= st; C = chans[l];
            conv(p + ".conv2", C, C, 3, 1, H, 1, 1);
        }
    const int h8 = S / 8, h16 = S / 16, h32 = S / 32;
    auto arm = [&](const std::string& p, int cin, int h) {   // AttentionRefinementModule up to its pre-sigmoid attention (model.py:76-80)
        conv(p + ".conv", cin, 128, 3, 1, h, 1);
        add(p + ".avg", 12, 128, 128, h, 1);
        conv(p + ".conv_atten", 128, 128, 1, 1, 1, 0);
    };
    // ContextPath.forward (model.py:111-123)
    add("cp.avg", 12, 512, 512, h32, 1);
    conv("cp.conv_avg", 512, 128, 1, 1, 1, 1);
    arm("cp.arm32", 512, h32);
    add("cp.feat32_sum", 13, 128, 128, h32, h32);            // arm32 * sigmoid + avg_up
    conv("cp.conv_head32", 128, 128, 3, 1, h16, 1, 0, 1);
    arm("cp.arm16", 256, h16);
    add("cp.feat16_sum", 13, 128, 128, h16, h16).has_res = 1; // arm16 * sigmoid + feat32_up
    conv("cp.conv_head16", 128, 128, 3, 1, h8, 1, 0, 1);
    // FeatureFusionModule.forward (model.py:200-210) over cat(feat8, feat_cp8)
    conv("ffm.convblk", 256, 256, 1, 1, h8, 1);
    add("ffm.avg", 12, 256, 256, h8, 1);
    conv("ffm.conv1", 256, 64, 1, 1, 1, 1);
    conv("ffm.conv2", 64, 256, 1, 1, 1, 0);
    add("ffm", 13, 256, 256, h8, h8).plus1 = 1;              // feat * atten + feat
    // BiSeNetOutput (model.py:44-47), then labels
    conv("conv_out.conv", 256, 256, 3, 1, h8, 1);
    conv("conv_out.conv_out", 256, 19, 1, 1, h8, 0);
    add("labels", 14, 19, 1, h8, S);
    return ops;
}

int fp_plan(int S, int max_images, FpPlan* out, std::string* err) {
    FpPlan pl;
    pl.ops = fp_program(S);
    if (pl.ops.empty()) { if (err) *err = "face parser: size must be a multiple of 32 in [64, 512]"; return -1; }
    if (max_images < 1 || max_images > kFpMaxImages) { if (err) *err = "face parser: max_images must be in [1, " + std::to_string(kFpMaxImages) + "]"; return -1; }
    pl.size = S; pl.max_images = max_images;
    auto up16 = [](int c) { return (c + 15) / 16 * 16; };
    auto alloc = [&](int C, int H, int W) {
        FpView v;
        v.buf = (int)pl.buf_elems.size(); v.ld = v.C = up16(C); v.coff = 0; v.H = H; v.W = W;
        pl.buf_elems.push_back((size_t)v.C * H * W);
        return v;
    };
    auto sub = [](FpView v, int coff, int C) { v.coff += coff; v.C = C; return v; };
    FpView image, labels;
    image.buf = pl.image_buf = (int)pl.buf_elems.size(); image.ld = image.C = 3; image.H = image.W = S;
    pl.buf_elems.push_back((size_t)S * S * 3);
    labels.buf = pl.label_buf = (int)pl.buf_elems.size(); labels.ld = labels.C = 1; labels.H = labels.W = S;
    pl.buf_elems.push_back((size_t)S * S);
    // ffm.convblk's input, torch.cat([feat8, feat_cp8], 1) (model.py:201): one buffer, its two producers write their halves
    const FpView cat = alloc(256, S / 8, S / 8);
    std::map<std::string, FpView> outs;
    outs["cat"] = cat;
    // operands of everything behind the ResNet, by producer (tests/faceparse_ref.py walk; model.py:76-83,111-123,200-210,44-47)
    struct In { const char *op, *x, *r, *a, *b; };
    static const In kIn[] = {
        {"cp.avg", "cp.resnet.layer4.1.conv2", nullptr, nullptr, nullptr},
        {"cp.conv_avg", "cp.avg", nullptr, nullptr, nullptr},
        {"cp.arm32.conv", "cp.resnet.layer4.1.conv2", nullptr, nullptr, nullptr},
        {"cp.arm32.avg", "cp.arm32.conv", nullptr, nullptr, nullptr},
        {"cp.arm32.conv_atten", "cp.arm32.avg", nullptr, nullptr, nullptr},
        {"cp.feat32_sum", "cp.arm32.conv", nullptr, "cp.arm32.conv_atten", "cp.conv_avg"},
        {"cp.conv_head32", "cp.feat32_sum", nullptr, nullptr, nullptr},
        {"cp.arm16.conv", "cp.resnet.layer3.1.conv2", nullptr, nullptr, nullptr},
        {"cp.arm16.avg", "cp.arm16.conv", nullptr, nullptr, nullptr},
        {"cp.arm16.conv_atten", "cp.arm16.avg", nullptr, nullptr, nullptr},
        {"cp.feat16_sum", "cp.arm16.conv", "cp.conv_head32", "cp.arm16.conv_atten", nullptr},
        {"cp.conv_head16", "cp.feat16_sum", nullptr, nullptr, nullptr},
        {"ffm.convblk", "cat", nullptr, nullptr, nullptr},
        {"ffm.avg", "ffm.convblk", nullptr, nullptr, nullptr},
        {"ffm.conv1", "ffm.avg", nullptr, nullptr, nullptr},
        {"ffm.conv2", "ffm.conv1", nullptr, nullptr, nullptr},
        {"ffm", "ffm.convblk", nullptr, "ffm.conv2", nullptr},
        {"conv_out.conv", "ffm", nullptr, nullptr, nullptr},
        {"conv_out.conv_out", "conv_out.conv", nullptr, nullptr, nullptr},
        {"labels", "conv_out.conv_out", nullptr, nullptr, nullptr},
    };
    auto ends_with = [](const std::string& s, const char* t) { const size_t n = strlen(t); return s.size() >= n && s.compare(s.size() - n, n, t) == 0; };
    FpView cur, mid, shortcut;            // BasicBlock: the block's input, conv1's output, downsample.0's output
    bool down = false;
    for (const FpOp& op : pl.ops) {
        FpBind b;
        auto need = [&](const char* name, FpView* v) {
            auto it = outs.find(name);
            if (it == outs.end()) return false;
            *v = it->second;
            return true;
        };
        if (op.name == "cp.resnet.layer2.1.conv2") b.y = sub(cat, 0, 128);            // feat8: channels 0..127 of the concat
        else if (op.name == "cp.conv_head16") b.y = sub(cat, 128, 128);              // feat_cp8: channels 128..255
        else if (op.type == 14) b.y = labels;
        else b.y = alloc(op.cout, op.Ho, op.Wo);
        if (op.type == 10) {
            b.x = image;
        } else if (op.type == 11) {
            b.x = cur;
        } else if (op.name.rfind("cp.resnet.layer", 0) == 0) {
            if (ends_with(op.name, ".conv1")) { b.x = cur; mid = b.y; down = false; }
            else if (ends_with(op.name, ".downsample.0")) { b.x = cur; shortcut = b.y; down = true; }
            else { b.x = mid; b.r = down ? shortcut : cur; }
        } else {
            const In* in = nullptr;
            for (const In& k : kIn) if (op.name == k.op) in = &k;
            bool ok = in && need(in->x, &b.x);
            if (ok && in->r) ok = need(in->r, &b.r);
            if (ok && in->a) ok = need(in->a, &b.a);
            if (ok && in->b) ok = need(in->b, &b.b);
            if (!ok) { if (err) *err = "face parser: no binding for " + op.name; return -1; }
        }
        // the block input of what follows: the stem, the pool, and every BasicBlock's second conv
        if (op.type == 10 || op.type == 11 || (op.name.rfind("cp.resnet.layer", 0) == 0 && ends_with(op.name, ".conv2"))) cur = b.y;
        outs[op.name] = b.y;
        pl.bind.push_back(b);
    }
    pl.buf_bytes.resize(pl.buf_elems.size());
    for (size_t i = 0; i < pl.buf_elems.size(); ++i) {
        const bool bytes = (int)i == pl.image_buf || (int)i == pl.label_buf;
        pl.buf_bytes[i] = pl.buf_elems[i] * (size_t)max_images * (bytes ? 1 : 2);
    }
    *out = std::move(pl);
    return 0;
}

}  // namespace ltk

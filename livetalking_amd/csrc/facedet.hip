// fd_program and fd_plan: see facedet.h.  Host code only.
#include "facedet.h"

#include "s3fd_kernels.h"

#include <map>

namespace ltk {

std::vector<FdOp> fd_program(int H, int W) {
    std::vector<FdOp> ops;
    if (H < 32 || W < 32 || H > 16384 || W > 16384) return ops;
    int h = H, w = W, C = 3;
    std::map<std::string, FdOp> made;
    auto add = [&](const std::string& name, int type, int cin, int cout, int hi, int wi, int ho, int wo) -> FdOp& {
        FdOp op;
        op.name = name; op.type = type; op.cin = cin; op.cout = cout; op.H = hi; op.W = wi; op.Ho = ho; op.Wo = wo;
        ops.push_back(op);
        return ops.back();
    };
    auto conv = [&](const std::string& name, int cout, int k, int stride, int pad) {      // the trunk: every conv is followed by a ReLU
        const int ho = (h + 2 * pad - k) / stride + 1, wo = (w + 2 * pad - k) / stride + 1;
        FdOp& op = add(name, 0, C, cout, h, w, ho, wo);
        op.k = k; op.stride = stride; op.pad = pad; op.relu = 1;
        h = ho; w = wo; C = cout;
        made[name] = op;
    };
    auto pool = [&](const std::string& name) {                                            // F.max_pool2d(h, 2, 2): floor mode
        FdOp& op = add(name, 21, C, C, h, w, h / 2, w / 2);
        op.k = 2; op.stride = 2;
        h /= 2; w /= 2;
    };
    {   // net_s3fd.py:71 on the frame itself
        FdOp& st = add("conv1_1", 20, 3, 64, H, W, H, W);
        st.k = 3; st.pad = 1; st.relu = 1;
        C = 64;
    }
    conv("conv1_2", 64, 3, 1, 1);
    pool("pool1");
    conv("conv2_1", 128, 3, 1, 1); conv("conv2_2", 128, 3, 1, 1);
    pool("pool2");
    conv("conv3_1", 256, 3, 1, 1); conv("conv3_2", 256, 3, 1, 1); conv("conv3_3", 256, 3, 1, 1);
    pool("pool3");
    conv("conv4_1", 512, 3, 1, 1); conv("conv4_2", 512, 3, 1, 1); conv("conv4_3", 512, 3, 1, 1);
    pool("pool4");
    conv("conv5_1", 512, 3, 1, 1); conv("conv5_2", 512, 3, 1, 1); conv("conv5_3", 512, 3, 1, 1);
    pool("pool5");
    conv("fc6", 1024, 3, 1, 3);                      // pad 3: the map grows by 4 (net_s3fd.py:43)
    conv("fc7", 1024, 1, 1, 0);
    conv("conv6_1", 256, 1, 1, 0); conv("conv6_2", 512, 3, 2, 1);
    conv("conv7_1", 128, 1, 1, 0); conv("conv7_2", 256, 3, 2, 1);
    // net_s3fd.py:107-122: three sources go through L2Norm, three are read as they are
    const char* src[6] = {"conv3_3", "conv4_3", "conv5_3", "fc7", "conv6_2", "conv7_2"};
    for (int i = 0; i < 3; ++i) {
        const FdOp& s = made[src[i]];
        add(std::string(src[i]) + "_norm", 22, s.cout, s.cout, s.Ho, s.Wo, s.Ho, s.Wo);
    }
    for (int i = 0; i < 6; ++i) {
        const FdOp& s = made[src[i]];
        FdOp& op = add(std::string(src[i]) + (i < 3 ? "_norm_mbox" : "_mbox"), 0, s.cout, 16, s.Ho, s.Wo, s.Ho, s.Wo);
        op.k = 3; op.pad = 1; op.level = i; op.maxout = i == 0;
    }
    for (int i = 0; i < 6; ++i) {
        const FdOp& s = made[src[i]];
        FdOp& op = add("detect" + std::to_string(i), 23, 16, 0, s.Ho, s.Wo, s.Ho, s.Wo);
        op.level = i; op.maxout = i == 0;
    }
    return ops;
}

int fd_plan(int H, int W, int max_images, FdPlan* out, std::string* err) {
    FdPlan pl;
    pl.ops = fd_program(H, W);
    if (pl.ops.empty()) { if (err) *err = "face detector: H and W must be in [32, 16384]"; return -1; }
    if (max_images < 1 || max_images > kFdMaxImages) { if (err) *err = "face detector: max_images must be in [1, " + std::to_string(kFdMaxImages) + "]"; return -1; }
    pl.H = H; pl.W = W; pl.max_images = max_images;
    auto view = [&](int buf, int C, int h, int w) {
        FdView v;
        v.buf = buf; v.ld = v.C = C; v.coff = 0; v.H = h; v.W = w;
        const size_t n = (size_t)C * h * w;
        if (pl.buf_elems[buf] < n) pl.buf_elems[buf] = n;
        return v;
    };
    auto fresh = [&]() { pl.buf_elems.push_back(0); return (int)pl.buf_elems.size() - 1; };
    pl.image_buf = fresh();
    const FdView image = view(pl.image_buf, 3, H, W);
    const int trunk[2] = {fresh(), fresh()};
    int turn = 0;
    std::map<std::string, FdView> outs;
    auto tapped = [](const std::string& n) { return n == "conv3_3" || n == "conv4_3" || n == "conv5_3" || n == "fc7" || n == "conv6_2" || n == "conv7_2"; };
    FdView cur = image;
    for (const FdOp& op : pl.ops) {
        FdBind b;
        if (op.type == 22 || op.level >= 0) {             // a norm, a head, a detect: named sources
            const char* src[6] = {"conv3_3", "conv4_3", "conv5_3", "fc7", "conv6_2", "conv7_2"};
            std::string from;
            if (op.type == 22) from = op.name.substr(0, op.name.size() - 5);                          // "<source>_norm"
            else if (op.type == 0) from = op.name.substr(0, op.name.size() - 5);                      // "<source>[_norm]_mbox"
            else from = std::string(src[op.level]) + (op.level < 3 ? "_norm_mbox" : "_mbox");
            auto it = outs.find(from);
            if (it == outs.end()) { if (err) *err = "face detector: no binding for " + op.name; return -1; }
            b.x = it->second;
            if (op.type != 23) b.y = view(fresh(), op.cout, op.Ho, op.Wo);
        } else {                                          // the trunk: a chain
            b.x = cur;
            if (tapped(op.name)) b.y = view(fresh(), op.cout, op.Ho, op.Wo);
            else { b.y = view(trunk[turn], op.cout, op.Ho, op.Wo); turn ^= 1; }
            cur = b.y;
        }
        if (b.y.buf >= 0) outs[op.name] = b.y;
        pl.bind.push_back(b);
    }
    pl.rec_buf = fresh();
    pl.buf_elems[pl.rec_buf] = (size_t)kFdDevCap * kFdRecWords * 2 + kFdHeadBytes / 2;      // halfs per image: its records, and room for the head
    pl.buf_bytes.resize(pl.buf_elems.size());
    for (size_t i = 0; i < pl.buf_elems.size(); ++i) {
        pl.buf_bytes[i] = pl.buf_elems[i] * (size_t)max_images * ((int)i == pl.image_buf ? 1 : 2);
        pl.total_bytes += pl.buf_bytes[i];
    }
    if (pl.total_bytes >= kFdMaxBytes) {
        if (err) *err = "face detector: the program needs " + std::to_string(pl.total_bytes) + " bytes at " + std::to_string(max_images) +
                        " images of " + std::to_string(H) + " x " + std::to_string(W) + ", the limit is " + std::to_string(kFdMaxBytes);
        return -1;
    }
    *out = std::move(pl);
    return 0;
}

}  // namespace ltk

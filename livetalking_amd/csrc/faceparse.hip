// fp_program: see faceparse.h.  Host code only.
#include "faceparse.h"

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

}  // namespace ltk

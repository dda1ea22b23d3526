// Grouped kernels of the Ultralight render path: ONE launch over the frames of several avatars, every image taking the weights of
// its own avatar.  The model is per avatar (avatars/ultralight_avatar.py:69-70) but the architecture is one, so sessions of
// different avatars can share a launch sequence as soon as a kernel picks its weights per image: each avatar owns a device record
// (UlGroupW) with the operands of every op of the program, and a per-frame device table (UlGroupTab, uploaded in stream order in
// front of the pass like the bank / feature / output tables) names each frame's record.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "dw_kernels.h"

namespace ltk {

constexpr int kUlMaxOps = 96;          // ops of the Ultralight program (86: ultralight.hip build_ul_arch)

struct UlGroupOp {
    const f16* w;                      // dense conv: packed fp16 weights (ul_gconv_pack)
    const float* scale;                // dense conv: folded BatchNorm scale [Cout]
    const float* shift;                //             ... shift [Cout]
    const float* dw;                   // depthwise conv: [C/16][9][16] weights, then scale [C], shift [C] (dw_pack)
};
struct UlGroupW {
    UlGroupOp op[kUlMaxOps];
    UlInW inw;
    UlHeadW headw;
};
struct UlGroupTab {
    const UlGroupW* w[kPackMaxFrames];
};

// host image -> device table entries [0, nframes), in stream order (kernel arguments: no host memory is read after the call returns)
void launch_upload_group_table(const UlGroupTab* host, int nframes, UlGroupTab* d_tab, hipStream_t s);

// Weights of a dense conv, torch layout [Cout][Cin][k][k] fp32 -> fp16 [Cout/16][k*k][ceil(Cin/32)][64 lanes][8]: the A operand of
// v_mfma_f32_16x16x32_f16 as a lane loads it (lane l: output channel l & 15, channels (l >> 4) * 8 .. + 8 of the 32-channel step);
// channels past Cin (Cin % 32 == 16) are zeros.  Returns the number of halfs; out == nullptr: only that.
size_t ul_gconv_pack(const float* weight, int Cin, int Cout, int k, f16* out);

// Dense conv on channel-blocked fp16 maps with per-image weights: y = clamp(relu?(acc * scale + shift + res)).  k = 1 (stride 1,
// pad 0) or k = 3 stride 2 (pad 1 or 3).  Views: channels [coff, coff + C) of a buffer of ld channels, both multiples of 16.
struct UlGconvIO {
    const f16* x = nullptr; int x_ld = 0, x_coff = 0;
    f16* y = nullptr; int y_ld = 0, y_coff = 0;
    const f16* res = nullptr; int res_ld = 0, res_coff = 0;
    int N = 0, H = 0, W = 0, Cin = 0, Cout = 0;
    int k = 1, stride = 1, pad = 0, relu = 0;
};
struct UlGconvGeom {
    int Ho = 0, Wo = 0, tile_px = 0, tile_co = 0, grid_x = 0, grid_y = 0, grid_z = 0, blocks = 0, ksteps = 0, threads = 0;
};
// checks the arguments and derives the launch geometry on the host alone; 0, or -1 with *err set
int ul_gconv_geom(const UlGconvIO& io, UlGconvGeom* g, std::string* err);
// op: index into UlGroupW::op of the record each frame's table entry names.  0 / -1 (arguments) / -2 (launch)
int launch_ul_gconv(const UlGroupTab* d_tab, int op, const UlGconvIO& io, hipStream_t s, std::string* err);
const char* ul_gconv_kernel_name();

// dw_kernels.hip: the grouped twins of launch_dwconv3x3 / launch_ul_in / launch_ul_head read their weights through the table
void launch_dwconv3x3_grouped(const f16* x, int N, int x_cbt, int x_cb0, int C, int H, int W, int stride, const UlGroupTab* d_tab, int op,
                              int relu, f16* y, int y_cbt, int y_cb0, hipStream_t s);
void launch_ul_in_grouped(const FacePtrs* faces, const float* img6, int N, const UlGroupTab* d_tab, f16* y, hipStream_t s);
void launch_ul_head_grouped(const f16* x, int N, const UlGroupTab* d_tab, const OutPtrs* outs, float* out_f32, hipStream_t s);

}  // namespace ltk

// ul_ir: one inverted residual of the Ultralight program (avatars/ultralight/unet.py:7-36: 1x1 expand + BN + ReLU, depthwise 3x3 + BN
// + ReLU, 1x1 project + BN, + x where the block has the connection) as ONE launch, the two hidden tensors kept in LDS (ul_ir.hip).
// The pure planner (no HIP call), the weight image the kernel reads, and the launcher, which launches what the planner says.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "dw_kernels.h"

namespace ltk {

constexpr int kIrTH = 8, kIrTW = 8;        // a block's tile of OUTPUT pixels (of one image)
constexpr int kIrMC = 64;                  // hidden channels per chunk
constexpr int kIrThreads = 256;
constexpr int kIrMaxJT = 16;               // 16-channel output tiles whose accumulators a block keeps (Cout <= 256)
constexpr int kIrLdsLimit = 64 * 1024;     // dynamic LDS a launch may take without an attribute (the CU has 160 KiB)
constexpr int kIrParamFloats = 13 * kIrMC; // fp32 record of a chunk: scale1, shift1, dw [MC/16][9][16], scale_d, shift_d

struct UlIrIO {
    const f16* x = nullptr; int x_ld = 0, x_coff = 0;
    f16* y = nullptr; int y_ld = 0, y_coff = 0;
    const f16* res = nullptr; int res_ld = 0, res_coff = 0;
    int has_res = 0;
    int N = 0, H = 0, W = 0, Cin = 0, mid = 0, Cout = 0, stride = 1;
    f16* e1 = nullptr;                     // tap buffers (both or none): [N][mid/16][H][W][16] / [N][mid/16][Ho][Wo][16]
    f16* e2 = nullptr;
};

struct UlIrPlan {
    char kernel[64];
    int Ho, Wo;
    int TH, TW, MC, chunks;
    int hid_h, hid_w, hidden_px;           // the hidden tile a block expands (tile + halo, at input resolution)
    int lds_bytes, lds_limit;
    int grid_x, grid_y, grid_z, blocks, threads;
    int JT;
};

// accept (0, *p filled) or refuse (-1, *err = the reason) on the host alone; `tap`: the instantiation that also stores e1 / e2
int ul_ir_plan(const UlIrIO& io, bool tap, UlIrPlan* p, std::string* err);

// The block's operands as the kernel reads them, one device allocation:
//   w1 fp16 [chunks * MC/16][ceil(Cin/32)][64 lanes][8]  (ul_gconv_pack's A-operand image of [mid][Cin], zero rows behind mid)
//   w2 fp16 [Cout/16][chunks * MC/32][64][8]             (... of [Cout][mid], zero columns behind mid)
//   par fp32 [chunks][kIrParamFloats], then scale2 [Cout], shift2 [Cout]
// Hidden channels behind mid carry zero weights, scales and shifts: they expand to 0, convolve to 0 and project 0.
struct UlIrW {
    const f16* w1 = nullptr;
    const f16* w2 = nullptr;
    const float* par = nullptr;
    const float* ss2 = nullptr;
};
// bytes of the image; out (or null): the image, and *off the byte offsets of w1, w2, par, ss2 in it.  Weights in torch layout:
// w1 [mid][Cin], wd [mid][3][3], w2 [Cout][mid]; scale / shift pairs fp32 (null: 1 / 0)
size_t ul_ir_pack(const float* w1, const float* wd, const float* w2, int Cin, int mid, int Cout, const float* s1, const float* b1,
                  const float* sd, const float* bd, const float* s2, const float* b2, uint8_t* out, size_t off[4]);
inline UlIrW ul_ir_weights(const uint8_t* d_base, const size_t off[4]) {
    return UlIrW{(const f16*)(d_base + off[0]), (const f16*)(d_base + off[1]), (const float*)(d_base + off[2]), (const float*)(d_base + off[3])};
}

// 0 / -1 (the planner refused: *err) / -2 (launch).  plan (or null): what was launched
int launch_ul_ir(const UlIrW& w, const UlIrIO& io, hipStream_t s, UlIrPlan* plan, std::string* err);

}  // namespace ltk

// VALU / HBM-bound kernels of the Ultralight render path (avatars/ultralight/unet.py): depthwise 3x3 convolution, bilinear x2
// upsample into a concat buffer, the input layer with the bank gather fused, the HuBERT feature pack and the output head.
// Host launch interface; tensors are channel-blocked fp16 [N][C/16][H][W][16] (conv_mfma.h), addressed as a block range
// [cb0, cb0 + C/16) of a buffer of `cbt` channel blocks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "misc_kernels.h"

namespace ltk {

constexpr int kUlFace = 168;       // bank face crop (face_imgs/), ultralight_avatar.py:152
constexpr int kUlRes = 160;        // network resolution: the crop's [4:164, 4:164]
constexpr int kUlCropOff = 4;
// cv2.rectangle(img, (5, 5, 150, 145), 0, -1) (ultralight_avatar.py:154): Rect(x, y, w, h), both corners inclusive
constexpr int kUlMaskX0 = 5, kUlMaskX1 = 154, kUlMaskY0 = 5, kUlMaskY1 = 149;

// nn.Conv2d(C, C, 3, stride, 1, groups=C, bias=False) + folded BatchNorm + optional ReLU (unet.py:19-27).
// w: DEVICE fp32 [C/16][9][16] (tap-major inside a channel block), scale / shift: DEVICE fp32 [C].  stride 1 or 2, zero padding.
// fp32 accumulation, one fp16 rounding.  C % 16 == 0.
void launch_dwconv3x3(const f16* x, int N, int x_cbt, int x_cb0, int C, int H, int W, int stride, const float* w, const float* scale,
                      const float* shift, int relu, f16* y, int y_cbt, int y_cb0, hipStream_t s);
// The host image of those three arrays, back to back: weight fp32 [C][3][3] -> out[Cpad / 16][9][16], then scale [Cpad] (null: 1) and shift
// [Cpad] (null: 0); the layout channels behind the first C get zero weights, scale and shift.  out: Cpad * 11 floats.
void dw_pack(const float* weight, const float* scale, const float* shift, int C, int Cpad, float* out);

// nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True) (unet.py:76): source coordinate of output pixel o is
// o * (h - 1) / (2h - 1), formed from integers; the interpolation itself runs in fp64 (the kernel moves 5 tensor elements per
// 3 fp64 FMAs: memory bound on gfx950), one rounding to fp16.  Written into blocks [y_cb0, y_cb0 + C/16) of the concat buffer.
void launch_upsample2x(const f16* x, int N, int x_cbt, int x_cb0, int C, int h, int w, f16* y, int y_cbt, int y_cb0, hipStream_t s);

// inc.inconv.0.conv.0/1/2 (unet.py:16-18 with inp = 6): 1x1 conv 6 -> 12 + folded BN + ReLU with the input fused:
// faces != nullptr (DEVICE table): bank crops uint8 [168][168][3] BGR; channels 0..2 = crop[4:164, 4:164] / 255, channels 3..5 the
// same with the mask rectangle zeroed (ultralight_avatar.py:150-161); else img6: DEVICE float32 NCHW [N][6][160][160].
// y: [N][1][160][160][16], channels 12..15 zero.
struct UlInW {
    float w[12][6];
    float scale[12], shift[12];
};
void launch_ul_in(const FacePtrs* faces, const float* img6, int N, const UlInW& w, f16* y, hipStream_t s);

// HuBERT chunks float32 [16][32][32] per frame (DEVICE table; ultralight_avatar.py:164) -> [N][1][32][32][16]
void launch_ul_pack_feat(const MelPtrs* feats, int N, f16* y, hipStream_t s);

// outc (unet.py:92, 1x1 conv 32 -> 3 + bias) + sigmoid (unet.py:214); x: [N][2][160][160][16].  outs (DEVICE table, or null): uint8
// [160][160][3] per frame = trunc(sigmoid * 255) (ultralight_avatar.py:170,181); out_f32 (or null): float32 NCHW sigmoid.
struct UlHeadW {
    float w[3][32];
    float b[3];
};
void launch_ul_head(const f16* x, int N, const UlHeadW& w, const OutPtrs* outs, float* out_f32, hipStream_t s);

// ultralight_avatar.py:173-184 paste_back_frame: the 168x168 bank face with the prediction at [4:164, 4:164], cv2.resize'd
// (INTER_LINEAR, as launch_paste) to the box (x1, y1, x2, y2) and pasted into a copy of the full frame (misc_kernels.hip).
void launch_ul_paste(const uint8_t* full, int H, int W, const uint8_t* face168, const uint8_t* pred160, int x1, int y1, int x2, int y2,
                     uint8_t* out, hipStream_t s);

}  // namespace ltk

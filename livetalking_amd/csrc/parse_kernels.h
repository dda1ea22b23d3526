// Kernels of the BiSeNet face parser (avatars/musetalk/utils/face_parsing/model.py, resnet.py) that the convolution library has no
// kernel for: the 7x7 stride-2 stem on uint8 RGB, the 3x3 stride-2 max pool, the global average pool, the channel gate of the
// attention-refinement / feature-fusion modules and the segmentation head (bilinear x8 upsample + argmax).
// Host launch interface; tensors are channel-blocked fp16 [N][C/16][H][W][16] (conv_mfma.h), addressed as a block range
// [cb0, cb0 + C/16) of a buffer of `cbt` channel blocks.  Every launcher returns 0, or -1 with the refusal in *err (nothing enqueued).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

#include "conv_mfma.h"

namespace ltk {

constexpr int kStemCout = 64;
constexpr int kStemK = 147, kStemKPad = 160;      // 7 x 7 x 3 products, ten K-steps of v_mfma_f32_32x32x16_f16
constexpr int kStemTH = 8, kStemTW = 16;          // output tile of a block: 4 waves x (2 rows x 16 columns)
// the operand image of the stem's weights: fp16 [2 cout tiles][10 K-steps][64 lanes][8], k = (ky * 7 + kx) * 3 + c (zero from 147 on),
// then nothing; scale / shift stay fp32 [64] + [64].  weight: fp32 [64][3][7][7] (torch layout, c = 0 is R).
constexpr size_t kStemWHalfs = (size_t)2 * (kStemKPad / 16) * 64 * 8;
void parse_stem_pack(const float* weight, f16* out);

// cp.resnet.conv1 + bn1 + ReLU (resnet.py:61-62,72-73) with the input transform fused (face_parsing/__init__.py:72-75: ToTensor +
// Normalize): rgb DEVICE uint8 [N][H][W][3], H and W even; each tap is f16((v / 255 - mean_c) / std_c) INSIDE the image and 0 outside
// it (the reference pads the normalised tensor); fp32 accumulation, fp32 scale / shift (DEVICE [64] each), ReLU, one fp16 rounding.
// y: 64 channels at [y_cb0, y_cb0 + 4) of [N][y_cbt][H/2][W/2][16].
int launch_parse_stem(const uint8_t* rgb, int N, int H, int W, const f16* wq, const float* scale, const float* shift, f16* y, int y_cbt,
                      int y_cb0, hipStream_t s, std::string* err);

// nn.MaxPool2d(kernel_size=3, stride=2, padding=1) (resnet.py:64,74): padding is -inf, Ho = (H - 1) / 2 + 1.  Exact.
int launch_maxpool3x3s2(const f16* x, int N, int x_cbt, int x_cb0, int C, int H, int W, f16* y, int y_cbt, int y_cb0, hipStream_t s,
                        std::string* err);

constexpr int kGapMaxP = 4096;
// F.avg_pool2d(x, x.size()[2:]) (model.py:78,111,203): [N][C][P] -> [N][C][1], P <= 4096.  One block per (image, channel block); the
// P values of a channel are summed in fp32 as ONE fixed binary tree (5 levels in a thread over pixels q + 128 i, 7 levels across the
// block; absent pixels are exact zeros), so a channel's bytes depend on nothing but its own P values; sum / P, one fp16 rounding.
int launch_gap(const f16* x, int N, int x_cbt, int x_cb0, int C, int P, f16* y, int y_cbt, int y_cb0, hipStream_t s, std::string* err);

// y = x * (sigmoid(a) [+ 1]) [+ b] [+ r]: a (pre-sigmoid attention) and b (or null) are dense [N][C/16][1][16], r (or null) a full map.
// sigmoid, product and sums in fp32, one fp16 rounding.  ARM32: b = avg_up (model.py:82,116); ARM16: r = feat32_up (:121); FFM: plus1,
// feat * atten + feat (:208-209).
int launch_chan_gate(const f16* x, int N, int x_cbt, int x_cb0, int C, int P, const f16* a, const f16* b, const f16* r, int r_cbt,
                     int r_cb0, int plus1, f16* y, int y_cbt, int y_cb0, hipStream_t s, std::string* err);

constexpr int kSegClasses = 19;
// F.interpolate(feat_out, (8h, 8w), mode='bilinear', align_corners=True) (model.py:251) + argmax(0) (face_parsing/__init__.py:90):
// x [N][2][h][w][16] logits (classes 0..18 of 32 layout channels), labels DEVICE uint8 [N][8h][8w].  Source coordinate of output
// pixel o = o * (h - 1) / (8h - 1), integer quotient and remainder; interpolation and comparison in fp32; the lowest class wins a tie.
int launch_seg_argmax(const f16* x, int N, int h, int w, uint8_t* labels, hipStream_t s, std::string* err);

}  // namespace ltk

// Kernels of the S3FD face detector (avatars/wav2lip/face_detection/detection/sfd/net_s3fd.py, detect.py, bbox.py) that the
// convolution library has no kernel for: conv1_1 on the uint8 frame itself, the 2x2 stride-2 max pool, L2Norm, and what batch_detect
// does behind the network for one detection level (two-way softmax, threshold, box decode, append to the image's candidate list).
// Host launch interface; tensors are channel-blocked fp16 [N][C/16][H][W][16] (conv_mfma.h), addressed as a block range
// [cb0, cb0 + C/16) of a buffer of `cbt` channel blocks.  Every launcher returns 0, or -1 with the refusal in *err (nothing enqueued).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

#include "conv_mfma.h"

namespace ltk {

constexpr int kFdStemCout = 64;
constexpr int kFdStemK = 27, kFdStemKPad = 32;    // 3 x 3 x 3 products: ONE K-step of v_mfma_f32_16x16x32_f16
constexpr int kFdStemTH = 16, kFdStemTW = 16;     // output tile of a block: 4 waves x (4 rows x 16 columns)
// the operand image of conv1_1's weights: fp16 [4 cout tiles][64 lanes][8], lane l element j = W[cout 16 t + (l & 15)][k = 8 (l >> 4) + j],
// k = (ky * 3 + kx) * 3 + c (zero from 27 on).  weight: fp32 [64][3][3][3] (torch layout; c = 0 is the channel the network sees first).
constexpr size_t kFdStemWHalfs = (size_t)4 * 64 * 8;
void s3fd_stem_pack(const float* weight, f16* out);

// conv1_1 + ReLU (net_s3fd.py:71) with the input transform of api.py:65 + detect.py:59 fused: bgr DEVICE uint8 [N][H][W][3] as
// cv2.imread gives it; the network's channel c is byte 2 - c of the pixel (the reversal) minus (104, 117, 123)[c] - the means in
// the order the reference applies them to the REVERSED image.  Integers in [-123, 151]: exact in fp16.  Outside the image a tap is 0
// (the padding of the mean-subtracted tensor).  fp32 accumulation, fp32 bias (DEVICE [64]), ReLU, one fp16 rounding.  Any H, W >= 1.
// y: 64 channels at [y_cb0, y_cb0 + 4) of [N][y_cbt][H][W][16].
int launch_s3fd_stem(const uint8_t* bgr, int N, int H, int W, const f16* wq, const float* bias, f16* y, int y_cbt, int y_cb0, hipStream_t s,
                     std::string* err);

// F.max_pool2d(h, 2, 2) (net_s3fd.py:73,77,83,89,95): floor mode, Ho = H / 2, Wo = W / 2, an odd last row / column is dropped.  Exact.
int launch_maxpool2x2s2(const f16* x, int N, int x_cbt, int x_cb0, int C, int H, int W, f16* y, int y_cbt, int y_cb0, hipStream_t s,
                        std::string* err);

// L2Norm (net_s3fd.py:16-19): y = x / (sqrt(sum_c x^2) + 1e-10) * weight[c] per pixel.  The sum of squares is fp32, channels in
// ascending order (fp16 would overflow at 256^2); y = f16(x * (1 / norm) * weight[c]), fp32 products, one fp16 rounding.  weight DEVICE fp32 [C].
int launch_l2norm(const f16* x, int N, int x_cbt, int x_cb0, int C, int P, const float* weight, f16* y, int y_cbt, int y_cb0, hipStream_t s,
                  std::string* err);

constexpr int kFdLevels = 6;
constexpr int kFdRecWords = 6;                    // a candidate: {uint32 key, float x1, y1, x2, y2, score}
constexpr int kFdKeyBits = 14;                    // key = level << 28 | h << 14 | w
// the candidate buffer of a device program (MtGraph::fd_rec_buf): a head of kFdHeadBytes - the images' counters from byte 0, the
// threshold at kFdThreshAt - and kFdDevCap records per image behind it
constexpr int kFdHeadBytes = 256, kFdThreshAt = 128, kFdDevCap = 4096;
// detect.py:71-89 + bbox.py:111-129 for level i of the merged head map x (16 layout channels: conf at 0..1, or 0..3 with maxout - then
// conf = [max(c0, c1, c2), c3], net_s3fd.py:125-127 -, loc at 4..7): per position the two-way softmax in fp32; where score > thresh
// the box is decoded (stride 2^(i+2), prior centre stride / 2 + index * stride, prior size 4 stride, variances 0.1 / 0.2) and one
// record is appended to image n's list recs[n][cap][6] through the counter counts[n] (atomicAdd).  The counter is NOT reset here (the
// six levels share it) and keeps counting past `cap`: records beyond it are dropped, the host sees counts[n] > cap.  Arrival order is
// arbitrary; the key orders a list.  d_thresh (or null): the threshold is read from this DEVICE float when the kernel runs, so that a
// captured launch follows the value of the call that replays it; `thresh` is then ignored.
int launch_s3fd_detect(const f16* x, int N, int x_cbt, int x_cb0, int H, int W, int maxout, int level, float thresh, const float* d_thresh,
                       uint32_t* recs, int cap, uint32_t* counts, hipStream_t s, std::string* err);

}  // namespace ltk

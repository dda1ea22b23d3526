// Kernels of the HuBERT-large audio front end of the Ultralight avatar (gfx950) that the MuseTalk / Whisper kernel set does not have:
// waveform statistics and normalisation, the one-channel first conv layer with its LayerNorm and GELU, LayerNorm + GELU over 512
// channels, the grouped positional convolution on MFMA, and the chunk gather.  Activations are CB16 fp16 ([N][C/16][T][16]: image
// stride cbt * T * 16 halfs, as the executor lays out frames > 1), see nn_kernels.h.  Host launch interface.  Every kernel has an
// image dimension (the `_n` forms: N clips of ONE length in one launch, nothing shared between clips); the forms without it are
// N = 1 and run the same kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "conv_mfma.h"

namespace ltk {

// ---- Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm: (x - mean) / sqrt(var + 1e-7), population variance over the WHOLE input.
// stats[0] = mean, stats[1] = variance of pcm[0, n): fp32, two passes (the second one centred, with the first-order correction of
// the mean's own rounding), one block, fixed summation order.
void launch_hubert_stats(const float* pcm, long long n, float* stats, hipStream_t s);
// y[i] = (pcm[i] - stats[0]) * rsqrt(stats[1] + 1e-7), i < n
void launch_hubert_normalise(const float* pcm, int n, const float* stats, float* y, hipStream_t s);
// N clips: pcm / y fp32 [N][n], stats [N][2]; one block per clip with the same two-pass sums in the same order, each clip normalised
// with its own pair.  resid [N] (may be null: the forms above) = what the fp32 rounding of each stored mean left out; the
// normalisation takes it off the centred sample, y = ((pcm - mean) - resid) * rstd, so that a DC offset does not cost the waveform
// its last digits (half an ulp of a mean of 100 is 3.8e-6, on a deviation of a few tenths)
void launch_hubert_stats_n(const float* pcm, long long n, int N, float* stats, float* resid, hipStream_t s);
void launch_hubert_normalise_n(const float* pcm, int n, int N, const float* stats, const float* resid, float* y, hipStream_t s);

// ---- feature_extractor.conv_layers.0: Conv1d(1, 512, k 10, stride 5, bias) + LayerNorm(512) + GELU in one kernel.
// x fp32 [n]; w fp32 [512][10]; bias / gamma / beta fp32 [512]; y CB16 [32][L0][16], L0 = (n - 10) / 5 + 1
void launch_hubert_layer0(const float* x, int n, const float* w, const float* bias, const float* gamma, const float* beta, float eps,
                          f16* y, hipStream_t s);
// x fp32 [N][n]; y CB16 [N][y_cbt][L0][16]
void launch_hubert_layer0_n(const float* x, int n, int N, const float* w, const float* bias, const float* gamma, const float* beta, float eps,
                            f16* y, int y_cbt, hipStream_t s);

// ---- LayerNorm over the 512 channels of every time step + GELU (conv_layers.1-6).  ONE image: x / y are CB16 buffers whose block
// stride is T rows ([blocks][T][16]); the tensor is blocks [cb0, cb0 + 32) of its buffer
void launch_ln_gelu512(const f16* x, int x_cb0, int T, float eps, const float* gamma, const float* beta, f16* y, int y_cb0, hipStream_t s);
void launch_ln_gelu512_n(const f16* x, int N, int x_cbt, int x_cb0, int T, float eps, const float* gamma, const float* beta, f16* y, int y_cbt,
                         int y_cb0, hipStream_t s);

// ---- encoder.pos_conv_embed: y = x + GELU(Conv1d(1024, 1024, k 128, pad 64, groups 16)(x)[:, :, :-1]) on T rows.
// Weights packed by hubert_posconv_pack ([1024][64][128] fp32 -> MFMA fragments, kPosConvPackHalfs halfs); bias fp32 [1024].
// x and y are distinct CB16 tensors of one image (block stride T rows), 64 channel blocks each from x_cb0 / y_cb0.
constexpr size_t kPosConvPackHalfs = (size_t)1024 * 64 * 128;
void hubert_posconv_pack(const float* w, f16* packed);
void launch_hubert_posconv(const f16* x, int x_cb0, int T, const f16* w_packed, const float* bias, f16* y, int y_cb0, hipStream_t s);
// N images of T rows each: a tap that leaves [0, T) of its own image is padding
void launch_hubert_posconv_n(const f16* x, int N, int x_cbt, int x_cb0, int T, const f16* w_packed, const float* bias, f16* y, int y_cbt,
                             int y_cb0, hipStream_t s);

// ---- feature2chunks: frame f takes rows [first_row + f * row_step, + rows), every index clamped into [0, T) -> out fp32
// [batch][rows][1024].  x CB16 of one image (block stride T rows), 64 blocks from x_cb0.
void launch_hubert_chunks(const f16* x, int x_cb0, int T, int batch, int first_row, int row_step, int rows, float* out, hipStream_t s);
// ... of image `img` of a batched tensor (x_cbt channel blocks per image), clamped into that image's own [0, T)
void launch_hubert_chunks_img(const f16* x, int img, int x_cbt, int x_cb0, int T, int batch, int first_row, int row_step, int rows, float* out,
                              hipStream_t s);

}  // namespace ltk

// HuBERT-large front-end kernels (hubert_kernels.h): transformers HubertModel with feat_extract_norm="layer",
// do_stable_layer_norm=True as avatars/ultralight/audio2feature.py calls it.  The linear layers, the stride-2 convs of layers 1-6,
// the LayerNorms of the encoder and the attention are the MuseTalk / Whisper kernels (hubert.hip mt_build_hubert); what is here
// is the rest.
#include "hubert_kernels.h"

#include <string.h>

namespace ltk {

typedef f16 f16x8 __attribute__((ext_vector_type(8)));
typedef f16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

// sum over the 64 lanes of a wave, the same value (and the same summation tree) in every lane
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// sum over a 1024-thread block in a fixed order: wave tree, then the 16 wave sums in wave order
__device__ __forceinline__ float block_sum_1024(float v, float* red /*[16]*/) {
    v = wave_sum(v);
    __syncthreads();                                   // red may still be read from the previous call
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) s += red[w];
    return s;
}

}  // namespace

// =============================================================================================== waveform statistics
// One block per clip (blockIdx.x = clip; never a sum over the batch): a live step has 16 640 samples.  An offline utterance has a few million, which one block reads twice at one CU's
// bandwidth: not measured, and not on a session's path (a multi-block first stage with a fixed-order second one is the lever there).
// Pass 1: mean0 = sum x / n.  Pass 2, centred on mean0: D = sum (x - mean0), Q = sum (x - mean0)^2; mean = mean0 + D / n takes the
// rounding of pass 1 out of the mean, var = (Q - D^2 / n) / n out of the variance.  E[x^2] - E[x]^2 is not used anywhere: with a DC
// offset of 100 on unit-variance noise both terms are 1e4 and their fp32 roundings alone are 1e-3 of the variance they leave.
// The mean itself is stored in fp32: near 100 that is half an ulp of 7.6e-6, which x - mean would carry whole into a waveform whose
// deviation is a few tenths.  resid (optional) = (mean0 - stats[0]) + dm: what the rounding of stats[0] left out, for the normalisation.
__global__ __launch_bounds__(1024) void hubert_stats_kernel(const float* __restrict__ x, long long n, float* __restrict__ stats,
                                                             float* __restrict__ resid) {
    __shared__ float red[16];
    x += (size_t)blockIdx.x * (size_t)n;               // clip blockIdx.x of [N][n], its pair in [N][2]
    stats += 2 * blockIdx.x;
    float s = 0.f;
    for (long long i = threadIdx.x; i < n; i += 1024) s += x[i];
    const float mean0 = block_sum_1024(s, red) / (float)n;
    float d = 0.f, q = 0.f;
    for (long long i = threadIdx.x; i < n; i += 1024) { const float c = x[i] - mean0; d += c; q = fmaf(c, c, q); }
    const float D = block_sum_1024(d, red);
    const float Q = block_sum_1024(q, red);
    if (threadIdx.x == 0) {
        const float dm = D / (float)n;
        const float mean = mean0 + dm;
        stats[0] = mean;
        stats[1] = fmaxf(Q / (float)n - dm * dm, 0.f);
        if (resid) resid[blockIdx.x] = (mean0 - mean) + dm;
    }
}

void launch_hubert_stats_n(const float* pcm, long long n, int N, float* stats, float* resid, hipStream_t s) {
    hipLaunchKernelGGL(hubert_stats_kernel, dim3(N), dim3(1024), 0, s, pcm, n, stats, resid);
}
void launch_hubert_stats(const float* pcm, long long n, float* stats, hipStream_t s) { launch_hubert_stats_n(pcm, n, 1, stats, nullptr, s); }

// (x - mean) is exact where x and mean are within a factor of two of each other, so with resid the centred sample is good to its own
// last bit whatever the offset; where the mean is small resid is below half an ulp of nearly every x - mean and changes nothing.
__global__ __launch_bounds__(256) void hubert_normalise_kernel(const float* __restrict__ x, int n, const float* __restrict__ stats,
                                                                const float* __restrict__ resid, float* __restrict__ y) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t o = (size_t)blockIdx.y * n;             // clip blockIdx.y, normalised with its own pair
    const float mean = stats[2 * blockIdx.y], rstd = 1.0f / sqrtf(stats[2 * blockIdx.y + 1] + 1e-7f);
    const float e = resid ? resid[blockIdx.y] : 0.f;
    y[o + i] = ((x[o + i] - mean) - e) * rstd;
}

void launch_hubert_normalise_n(const float* pcm, int n, int N, const float* stats, const float* resid, float* y, hipStream_t s) {
    hipLaunchKernelGGL(hubert_normalise_kernel, dim3((n + 255) / 256, N), dim3(256), 0, s, pcm, n, stats, resid, y);
}
void launch_hubert_normalise(const float* pcm, int n, const float* stats, float* y, hipStream_t s) {
    launch_hubert_normalise_n(pcm, n, 1, stats, nullptr, y, s);
}

// =============================================================================================== layer 0
// Conv1d(1, 512, 10, stride 5) + LayerNorm(512) + GELU: 10 MACs per output, VALU work (as audio0_kernel).  A wave owns a time
// step: lane l holds channels 8l .. 8l+7 (half a channel block: one 16-byte store), their 80 weights stay in registers across the
// kTimePerWave steps the wave walks, the 10 samples of a step are the same address in every lane (one broadcast load each).  The
// LayerNorm is two wave sums (mean, then the centred squares); the [L0][512] map is written once.  blockIdx.y = image: a block's
// time steps end at L0 of ITS image (the waveform of image i starts at i * n samples, its map at i * y_cbt * L0 * 16 halfs).
constexpr int kL0TimePerWave = 8;

__global__ __launch_bounds__(256) void hubert_layer0_kernel(const float* __restrict__ x, int n, int L0, const float* __restrict__ w,
                                                             const float* __restrict__ bias, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float eps, f16* __restrict__ y, int y_cbt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    x += (size_t)blockIdx.y * n;
    y += (size_t)blockIdx.y * y_cbt * L0 * 16;
    const int c0 = lane * 8;
    float wr[8][10], br[8], gr[8], er[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
#pragma unroll
        for (int k = 0; k < 10; ++k) wr[c][k] = w[(c0 + c) * 10 + k];
        br[c] = bias[c0 + c]; gr[c] = gamma[c0 + c]; er[c] = beta[c0 + c];
    }
    const int t0 = (blockIdx.x * 4 + wave) * kL0TimePerWave;
    for (int t = t0; t < min(t0 + kL0TimePerWave, L0); ++t) {
        float xs[10];
#pragma unroll
        for (int k = 0; k < 10; ++k) xs[k] = x[(size_t)t * 5 + k];          // 5 t + 9 <= n - 1 by the definition of L0
        float v[8], s = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            float a = br[c];
#pragma unroll
            for (int k = 0; k < 10; ++k) a = fmaf(wr[c][k], xs[k], a);
            v[c] = a; s += a;
        }
        const float mean = wave_sum(s) * (1.f / 512.f);
        float q = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) { v[c] -= mean; q = fmaf(v[c], v[c], q); }
        const float rstd = rsqrtf(wave_sum(q) * (1.f / 512.f) + eps);
        f16x8 o;
#pragma unroll
        for (int c = 0; c < 8; ++c) o[c] = (f16)gelu_as(fmaf(v[c] * rstd, gr[c], er[c]));
        *reinterpret_cast<f16x8*>(y + ((size_t)(lane >> 1) * L0 + t) * 16 + (lane & 1) * 8) = o;
    }
}

void launch_hubert_layer0_n(const float* x, int n, int N, const float* w, const float* bias, const float* gamma, const float* beta, float eps,
                            f16* y, int y_cbt, hipStream_t s) {
    const int L0 = (n - 10) / 5 + 1;
    const int per_block = 4 * kL0TimePerWave;
    hipLaunchKernelGGL(hubert_layer0_kernel, dim3((L0 + per_block - 1) / per_block, N), dim3(256), 0, s, x, n, L0, w, bias, gamma, beta, eps, y,
                       y_cbt);
}
void launch_hubert_layer0(const float* x, int n, const float* w, const float* bias, const float* gamma, const float* beta, float eps,
                          f16* y, hipStream_t s) {
    launch_hubert_layer0_n(x, n, 1, w, bias, gamma, beta, eps, y, 32, s);
}

// =============================================================================================== LayerNorm + GELU over 512 channels
// layernorm_kernel's tiling (16 time steps x 16 channel slices per block, nn_kernels.hip) with the 32 values of a thread kept in
// registers between the passes, so the variance is a sum of centred squares, and the GELU behind the affine.  blockIdx.y = image
// (x_cbt / y_cbt channel blocks per image): the 16 rows of a block end at T of its own image.
__global__ __launch_bounds__(256) void ln_gelu512_kernel(const f16* __restrict__ x, int x_cbt, int x_cb0, int T, float eps,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          f16* __restrict__ y, int y_cbt, int y_cb0) {
    __shared__ float red[2][16][17];
    const int tid = threadIdx.x;
    const int tok = tid & 15, part = tid >> 4;
    const int p = blockIdx.x * 16 + tok;
    const bool ok = p < T;
    const f16* xb = x + ((size_t)blockIdx.y * x_cbt + x_cb0) * T * 16;
    float v[4][8];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = part + 16 * j;                 // 8-channel item 0..63
        f16x8 h = {0, 0, 0, 0, 0, 0, 0, 0};
        if (ok) h = *reinterpret_cast<const f16x8*>(xb + ((size_t)(i >> 1) * T + p) * 16 + (i & 1) * 8);
#pragma unroll
        for (int c = 0; c < 8; ++c) { v[j][c] = (float)h[c]; s += v[j][c]; }
    }
    red[0][tok][part] = s;
    __syncthreads();
    float S = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) S += red[0][tok][i];
    const float mean = S * (1.f / 512.f);
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < 8; ++c) { v[j][c] -= mean; q = fmaf(v[j][c], v[j][c], q); }
    red[1][tok][part] = q;
    __syncthreads();
    float Q = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) Q += red[1][tok][i];
    const float rstd = rsqrtf(Q * (1.f / 512.f) + eps);
    if (!ok) return;
    f16* yb = y + ((size_t)blockIdx.y * y_cbt + y_cb0) * T * 16;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = part + 16 * j;
        f16x8 o;
#pragma unroll
        for (int c = 0; c < 8; ++c) o[c] = (f16)gelu_as(fmaf(v[j][c] * rstd, gamma[i * 8 + c], beta[i * 8 + c]));
        *reinterpret_cast<f16x8*>(yb + ((size_t)(i >> 1) * T + p) * 16 + (i & 1) * 8) = o;
    }
}

void launch_ln_gelu512_n(const f16* x, int N, int x_cbt, int x_cb0, int T, float eps, const float* gamma, const float* beta, f16* y, int y_cbt,
                         int y_cb0, hipStream_t s) {
    hipLaunchKernelGGL(ln_gelu512_kernel, dim3((T + 15) / 16, N), dim3(256), 0, s, x, x_cbt, x_cb0, T, eps, gamma, beta, y, y_cbt, y_cb0);
}
void launch_ln_gelu512(const f16* x, int x_cb0, int T, float eps, const float* gamma, const float* beta, f16* y, int y_cb0, hipStream_t s) {
    launch_ln_gelu512_n(x, 1, 0, x_cb0, T, eps, gamma, beta, y, 0, y_cb0, s);
}

// =============================================================================================== positional convolution
// Conv1d(1024, 1024, k 128, pad 64, groups 16), last output dropped, GELU, + x.  Per group a GEMM of T rows x 64 outputs over
// K = 128 taps x 64 channels, with row t of tap k reading input row t + k - 64 (zero outside [0, T)).
//
// A block owns 32 rows (two 16-row tiles) x 16 outputs of one group; its 8 waves split the taps.  Both operands go from global
// memory straight into v_mfma_f32_16x16x32_f16 (rowgemm.hip's scheme): the weight fragments [group][16-output tile][tap][32-channel
// half][lane][8] are used once per block and stream through registers (non-temporal), the activations (T x 1024 halfs: 100 KB at
// the live length) live in L2.  Only the taps that touch a row of the tile are walked: tap k reaches rows [t0, t1) iff
// 64 - (t1 - 1) <= k <= T + 63 - t0, which at T = 51 leaves 101 of 128 taps for the first tile and 69 for the second.  The 8 partial
// tiles meet in LDS and are summed in wave order: the same input gives the same bytes, no atomics.  Bias, GELU and the residual
// are the epilogue.  blockIdx.z = image: rows, taps and the tap-skipping bounds are those of the block's own image, so a tap that
// leaves [0, T) is padding even where the neighbouring image's rows lie next to it in memory.
constexpr int kPcRows = 32;

struct PosConvArgs {
    const f16* x; f16* y; const f16* w; const float* bias;
    int x_cbt, x_cb0, y_cbt, y_cb0, T;
};

__global__ __launch_bounds__(512) void hubert_posconv_kernel(const PosConvArgs a) {
    __shared__ f32x4 red[8][2][64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int T = a.T;
    const int t0 = blockIdx.x * kPcRows, t1 = min(t0 + kPcRows, T);
    const int grp = blockIdx.y >> 2, jt = blockIdx.y & 3;
    const int i16 = lane & 15, g = lane >> 4;
    const int klo = max(0, 64 - (t1 - 1)), khi = min(127, T + 63 - t0);        // taps that reach a row of this tile (klo <= khi: t0 < T)
    const int ntap = khi - klo + 1, per = (ntap + 7) >> 3;
    const int k0 = klo + wave * per, k1 = min(khi + 1, k0 + per);
    // lane (i16, g) of the weight fragment: output jt * 16 + i16, channels ks * 32 + g * 8 .. + 8 of the group
    const f16x8* wp = reinterpret_cast<const f16x8*>(a.w) + ((size_t)(grp * 4 + jt) * 128) * 2 * 64 + lane;
    // lane (i16, g) of the activation fragment: row t0 + ft * 16 + i16, the same 8 channels: channel block grp * 4 + ks * 2 + (g >> 1)
    const f16* ximg = a.x + ((size_t)blockIdx.z * a.x_cbt + a.x_cb0) * T * 16;
    const f16* xg = ximg + ((size_t)(grp * 4 + (g >> 1)) * T) * 16 + (g & 1) * 8;
    f32x4 acc[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
    const f16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = k0; k < k1; ++k) {
        f16x8 wa[2], xb[2][2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) wa[ks] = __builtin_nontemporal_load(wp + ((size_t)k * 2 + ks) * 64);
#pragma unroll
        for (int ft = 0; ft < 2; ++ft) {
            const int t = t0 + ft * 16 + i16, tr = t + k - 64;
            const bool ok = t < T && tr >= 0 && tr < T;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
                xb[ks][ft] = ok ? *reinterpret_cast<const f16x8*>(xg + ((size_t)(ks * 2) * T + tr) * 16) : zero;
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int ft = 0; ft < 2; ++ft) acc[ft] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[ks], xb[ks][ft], acc[ft], 0, 0, 0);
    }
    red[wave][0][lane] = acc[0];
    red[wave][1][lane] = acc[1];
    __syncthreads();
    if (wave >= 2) return;                                     // wave ft finishes row tile ft
    const int ft = wave;
    f32x4 s = red[0][ft][lane];
#pragma unroll
    for (int w = 1; w < 8; ++w) {                              // fixed order
        const f32x4 t = red[w][ft][lane];
        s[0] += t[0]; s[1] += t[1]; s[2] += t[2]; s[3] += t[3];
    }
    // D layout of the 16x16 MFMA: lane holds outputs 4g .. 4g+3 of row i16
    const int t = t0 + ft * 16 + i16;
    if (t >= T) return;
    const int j0 = jt * 16 + 4 * g;                            // output channel inside the group
    const f32x4 b = *reinterpret_cast<const f32x4*>(a.bias + grp * 64 + j0);
    const size_t off = ((size_t)(grp * 4 + jt) * T + t) * 16 + 4 * g;
    const f16x4 r = *reinterpret_cast<const f16x4*>(ximg + off);
    f16x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = (f16)__builtin_amdgcn_fmed3f((float)r[i] + gelu_as(s[i] + b[i]), -65504.f, 65504.f);
    *reinterpret_cast<f16x4*>(a.y + ((size_t)blockIdx.z * a.y_cbt + a.y_cb0) * T * 16 + off) = o;
}

// w [1024][64][128] (output, channel of the group, tap) -> [group 16][tile 4][tap 128][half 2][lane 64][8]
void hubert_posconv_pack(const float* w, f16* packed) {
    for (int grp = 0; grp < 16; ++grp)
        for (int jt = 0; jt < 4; ++jt)
            for (int k = 0; k < 128; ++k)
                for (int ks = 0; ks < 2; ++ks)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int co = grp * 64 + jt * 16 + (lane & 15), c = ks * 32 + (lane >> 4) * 8;
                        f16* dst = packed + ((((size_t)(grp * 4 + jt) * 128 + k) * 2 + ks) * 64 + lane) * 8;
                        for (int e = 0; e < 8; ++e) dst[e] = (f16)w[((size_t)co * 64 + c + e) * 128 + k];
                    }
}

void launch_hubert_posconv_n(const f16* x, int N, int x_cbt, int x_cb0, int T, const f16* w_packed, const float* bias, f16* y, int y_cbt,
                             int y_cb0, hipStream_t s) {
    PosConvArgs a{x, y, w_packed, bias, x_cbt, x_cb0, y_cbt, y_cb0, T};
    hipLaunchKernelGGL(hubert_posconv_kernel, dim3((T + kPcRows - 1) / kPcRows, 64, N), dim3(512), 0, s, a);
}
void launch_hubert_posconv(const f16* x, int x_cb0, int T, const f16* w_packed, const float* bias, f16* y, int y_cb0, hipStream_t s) {
    launch_hubert_posconv_n(x, 1, 0, x_cb0, T, w_packed, bias, y, 0, y_cb0, s);
}

// =============================================================================================== chunk gather
__global__ __launch_bounds__(256) void hubert_chunks_kernel(const f16* __restrict__ x, int x_cb0, int T, int batch, int first_row,
                                                             int row_step, int rows, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;          // (frame, row, c8)
    const int total = batch * rows * 128;
    if (i >= total) return;
    const int c8 = i & 127, r = (i >> 7) % rows, f = (i >> 7) / rows;
    int row = first_row + f * row_step + r;
    row = min(max(row, 0), T - 1);
    const f16x8 v = *reinterpret_cast<const f16x8*>(x + ((size_t)(x_cb0 + (c8 >> 1)) * T + row) * 16 + (c8 & 1) * 8);
    float* o = out + ((size_t)f * rows + r) * 1024 + c8 * 8;
#pragma unroll
    for (int c = 0; c < 8; ++c) o[c] = (float)v[c];
}

void launch_hubert_chunks(const f16* x, int x_cb0, int T, int batch, int first_row, int row_step, int rows, float* out, hipStream_t s) {
    const int total = batch * rows * 128;
    hipLaunchKernelGGL(hubert_chunks_kernel, dim3((total + 255) / 256), dim3(256), 0, s, x, x_cb0, T, batch, first_row, row_step, rows, out);
}
// one request of a batched run: the kernel sees image `img` alone, so its clamp is that clip's own [0, T)
void launch_hubert_chunks_img(const f16* x, int img, int x_cbt, int x_cb0, int T, int batch, int first_row, int row_step, int rows, float* out,
                              hipStream_t s) {
    launch_hubert_chunks(x + (size_t)img * x_cbt * T * 16, x_cb0, T, batch, first_row, row_step, rows, out, s);
}

}  // namespace ltk

// Ultralight (MobileNet-style U-Net, avatars/ultralight/unet.py) kernels that are not implicit GEMMs: see dw_kernels.h.
// All of them move far more bytes than they compute on: one item = 8 channels of one pixel = one 16-byte load / store, consecutive
// lanes on consecutive 16-byte items of the channel-blocked tensor.
#include "dw_kernels.h"
#include "ul_gconv.h"

namespace ltk {

void dw_pack(const float* weight, const float* scale, const float* shift, int C, int Cpad, float* out) {
    for (int c = 0; c < Cpad; ++c) {
        for (int t = 0; t < 9; ++t) out[((size_t)(c >> 4) * 9 + t) * 16 + (c & 15)] = c < C ? weight[(size_t)c * 9 + t] : 0.f;
        out[(size_t)Cpad * 9 + c] = c < C ? (scale ? scale[c] : 1.f) : 0.f;
        out[(size_t)Cpad * 10 + c] = c < C && shift ? shift[c] : 0.f;
    }
}

namespace {

union H8 {
    uint4 u;
    f16 h[8];
};

__device__ __forceinline__ f16 to_f16_sat(float t) { return (f16)__builtin_amdgcn_fmed3f(t, -65504.f, 65504.f); }

// block = 256 items of ONE (image, channel block): its 144 weights and 32 scale / shift values sit in LDS (two addresses per wave)
__device__ __forceinline__ void dwconv3x3_body(const f16* __restrict__ x, int x_cbt, int x_cb0, int cb, int n, int H, int W, int Ho, int Wo,
                                               int stride, const float* __restrict__ w, const float* __restrict__ scale,
                                               const float* __restrict__ shift, int relu, f16* __restrict__ y, int y_cbt, int y_cb0) {
    __shared__ float sw[9 * 16 + 32];
    const int t = threadIdx.x;
    if (t < 144) sw[t] = w[cb * 144 + t];
    else if (t < 160) sw[t] = scale[cb * 16 + t - 144];
    else if (t < 176) sw[t] = shift[cb * 16 + t - 160];
    __syncthreads();
    const int item = blockIdx.x * 256 + t;
    if (item >= Ho * Wo * 2) return;
    const int hh = item & 1, p = item >> 1;
    const int oy = p / Wo, ox = p - oy * Wo;
    const f16* xb = x + ((size_t)n * x_cbt + x_cb0 + cb) * H * W * 16 + hh * 8;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy * stride - 1 + ky;
        if ((unsigned)iy >= (unsigned)H) continue;          // zero padding
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = ox * stride - 1 + kx;
            if ((unsigned)ix >= (unsigned)W) continue;
            H8 v;
            v.u = *reinterpret_cast<const uint4*>(xb + ((size_t)iy * W + ix) * 16);
            const float* wt = sw + (ky * 3 + kx) * 16 + hh * 8;
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = fmaf((float)v.h[j], wt[j], acc[j]);
        }
    }
    H8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float r = fmaf(acc[j], sw[144 + hh * 8 + j], sw[160 + hh * 8 + j]);
        if (relu) r = fmaxf(r, 0.f);
        o.h[j] = to_f16_sat(r);
    }
    *reinterpret_cast<uint4*>(y + (((size_t)n * y_cbt + y_cb0 + cb) * Ho * Wo + p) * 16 + hh * 8) = o.u;
}

__global__ __launch_bounds__(256) void dwconv3x3_kernel(const f16* __restrict__ x, int x_cbt, int x_cb0, int CB, int H, int W, int Ho, int Wo,
                                                         int stride, const float* __restrict__ w, const float* __restrict__ scale,
                                                         const float* __restrict__ shift, int relu, f16* __restrict__ y, int y_cbt, int y_cb0) {
    dwconv3x3_body(x, x_cbt, x_cb0, blockIdx.y % CB, blockIdx.y / CB, H, W, Ho, Wo, stride, w, scale, shift, relu, y, y_cbt, y_cb0);
}

// the same with the image's own weights: its record's [CB][9][16] weights, scale [16 CB] and shift [16 CB] of op `op` (ul_gconv.h; the
// image, and with it the record pointer, is one per block)
__global__ __launch_bounds__(256) void dwconv3x3_grouped_kernel(const f16* __restrict__ x, int x_cbt, int x_cb0, int CB, int H, int W, int Ho,
                                                                 int Wo, int stride, const UlGroupTab* __restrict__ tab, int op, int relu,
                                                                 f16* __restrict__ y, int y_cbt, int y_cb0) {
    const int n = blockIdx.y / CB;
    const float* const dw = tab->w[n]->op[op].dw;
    dwconv3x3_body(x, x_cbt, x_cb0, blockIdx.y % CB, n, H, W, Ho, Wo, stride, dw, dw + (size_t)CB * 144, dw + (size_t)CB * 160, relu, y, y_cbt, y_cb0);
}

__global__ __launch_bounds__(256) void upsample2x_kernel(const f16* __restrict__ x, int x_cbt, int x_cb0, int CB, int h, int w,
                                                          f16* __restrict__ y, int y_cbt, int y_cb0) {
    const int cb = blockIdx.y % CB, n = blockIdx.y / CB;
    const int Ho = 2 * h, Wo = 2 * w;
    const int item = blockIdx.x * 256 + threadIdx.x;
    if (item >= Ho * Wo * 2) return;
    const int hh = item & 1, p = item >> 1;
    const int oy = p / Wo, ox = p - oy * Wo;
    // align_corners: src = o * (in - 1) / (out - 1), exact quotient and remainder (a one-pixel axis maps everything to pixel 0)
    const int ny = oy * (h - 1), dy = Ho - 1, nx = ox * (w - 1), dx = Wo - 1;
    const int y0 = ny / dy, x0 = nx / dx;
    const double ly = (double)(ny - y0 * dy) / (double)dy, lx = (double)(nx - x0 * dx) / (double)dx;
    const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
    const f16* xb = x + ((size_t)n * x_cbt + x_cb0 + cb) * h * w * 16 + hh * 8;
    H8 a, b, c, d, o;
    a.u = *reinterpret_cast<const uint4*>(xb + ((size_t)y0 * w + x0) * 16);
    b.u = *reinterpret_cast<const uint4*>(xb + ((size_t)y0 * w + x1) * 16);
    c.u = *reinterpret_cast<const uint4*>(xb + ((size_t)y1 * w + x0) * 16);
    d.u = *reinterpret_cast<const uint4*>(xb + ((size_t)y1 * w + x1) * 16);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const double top = (double)a.h[j] + lx * ((double)b.h[j] - (double)a.h[j]);
        const double bot = (double)c.h[j] + lx * ((double)d.h[j] - (double)c.h[j]);
        o.h[j] = (f16)(top + ly * (bot - top));
    }
    *reinterpret_cast<uint4*>(y + (((size_t)n * y_cbt + y_cb0 + cb) * Ho * Wo + p) * 16 + hh * 8) = o.u;
}

// one thread = one pixel: 6 inputs, 12 outputs (+ 4 zero channels), weights as kernel arguments (scalar registers)
__global__ __launch_bounds__(256) void ul_in_kernel(const FacePtrs* __restrict__ faces, const float* __restrict__ img6, const UlInW wt,
                                                     f16* __restrict__ y) {
    const int n = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    constexpr int P = kUlRes * kUlRes;
    if (p >= P) return;
    float in[6];
    if (faces) {
        const int py = p / kUlRes, px = p - py * kUlRes;
        const uint8_t* f = faces->p[n] + ((size_t)(py + kUlCropOff) * kUlFace + px + kUlCropOff) * 3;
        const bool masked = py >= kUlMaskY0 && py <= kUlMaskY1 && px >= kUlMaskX0 && px <= kUlMaskX1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            in[c] = (float)f[c] / 255.0f;
            in[3 + c] = masked ? 0.f : in[c];
        }
    } else {
#pragma unroll
        for (int c = 0; c < 6; ++c) in[c] = img6[((size_t)n * 6 + c) * P + p];
    }
    H8 o[2];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        float r = 0.f;
        if (k < 12) {
#pragma unroll
            for (int c = 0; c < 6; ++c) r = fmaf(in[c], wt.w[k][c], r);
            r = fmaxf(fmaf(r, wt.scale[k], wt.shift[k]), 0.f);
        }
        o[k >> 3].h[k & 7] = to_f16_sat(r);
    }
    uint4* dst = reinterpret_cast<uint4*>(y + ((size_t)n * P + p) * 16);
    dst[0] = o[0].u;
    dst[1] = o[1].u;
}

// the same with the image's own weights: the block (one image) copies the 120 floats of its record's UlInW into LDS, every thread then
// reads them at wave-uniform addresses (ul_in_kernel's own text stays as it is: its weights are kernel arguments, and sharing a body
// through a reference changed its register allocation)
__global__ __launch_bounds__(256) void ul_in_grouped_kernel(const FacePtrs* __restrict__ faces, const float* __restrict__ img6,
                                                             const UlGroupTab* __restrict__ tab, f16* __restrict__ y) {
    __shared__ UlInW wt;
    const int n = blockIdx.y;
    {
        const float* src = reinterpret_cast<const float*>(&tab->w[n]->inw);
        float* dst = reinterpret_cast<float*>(&wt);
        if (threadIdx.x < sizeof(UlInW) / sizeof(float)) dst[threadIdx.x] = src[threadIdx.x];
    }
    __syncthreads();
    const int p = blockIdx.x * 256 + threadIdx.x;
    constexpr int P = kUlRes * kUlRes;
    if (p >= P) return;
    float in[6];
    if (faces) {
        const int py = p / kUlRes, px = p - py * kUlRes;
        const uint8_t* f = faces->p[n] + ((size_t)(py + kUlCropOff) * kUlFace + px + kUlCropOff) * 3;
        const bool masked = py >= kUlMaskY0 && py <= kUlMaskY1 && px >= kUlMaskX0 && px <= kUlMaskX1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            in[c] = (float)f[c] / 255.0f;
            in[3 + c] = masked ? 0.f : in[c];
        }
    } else {
#pragma unroll
        for (int c = 0; c < 6; ++c) in[c] = img6[((size_t)n * 6 + c) * P + p];
    }
    H8 o[2];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        float r = 0.f;
        if (k < 12) {
#pragma unroll
            for (int c = 0; c < 6; ++c) r = fmaf(in[c], wt.w[k][c], r);
            r = fmaxf(fmaf(r, wt.scale[k], wt.shift[k]), 0.f);
        }
        o[k >> 3].h[k & 7] = to_f16_sat(r);
    }
    uint4* dst = reinterpret_cast<uint4*>(y + ((size_t)n * P + p) * 16);
    dst[0] = o[0].u;
    dst[1] = o[1].u;
}

__global__ __launch_bounds__(256) void ul_pack_feat_kernel(const MelPtrs* __restrict__ feats, f16* __restrict__ y) {
    const int n = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;      // 1024 pixels
    const float* f = feats->p[n];
    H8 o[2];
#pragma unroll
    for (int c = 0; c < 16; ++c) o[c >> 3].h[c & 7] = to_f16_sat(f[c * 1024 + p]);
    uint4* dst = reinterpret_cast<uint4*>(y + ((size_t)n * 1024 + p) * 16);
    dst[0] = o[0].u;
    dst[1] = o[1].u;
}

__device__ __forceinline__ void ul_head_body(const f16* __restrict__ x, const UlHeadW& wt, const OutPtrs* __restrict__ outs,
                                             float* __restrict__ out_f32) {
    const int n = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    constexpr int P = kUlRes * kUlRes;
    if (p >= P) return;
    float acc[3] = {wt.b[0], wt.b[1], wt.b[2]};
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
        const uint4* src = reinterpret_cast<const uint4*>(x + (((size_t)n * 2 + cb) * P + p) * 16);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            H8 v;
            v.u = src[q];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float xv = (float)v.h[j];
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] = fmaf(xv, wt.w[c][cb * 16 + q * 8 + j], acc[c]);
            }
        }
    }
    uint8_t* o8 = outs ? outs->p[n] : nullptr;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float sg = 1.0f / (1.0f + expf(-acc[c]));
        if (o8) o8[(size_t)p * 3 + c] = (uint8_t)(sg * 255.0f);       // pred * 255 then astype(uint8): truncation
        if (out_f32) out_f32[((size_t)n * 3 + c) * P + p] = sg;
    }
}

__global__ __launch_bounds__(256) void ul_head_kernel(const f16* __restrict__ x, const UlHeadW wt, const OutPtrs* __restrict__ outs,
                                                       float* __restrict__ out_f32) {
    ul_head_body(x, wt, outs, out_f32);
}

__global__ __launch_bounds__(256) void ul_head_grouped_kernel(const f16* __restrict__ x, const UlGroupTab* __restrict__ tab,
                                                               const OutPtrs* __restrict__ outs, float* __restrict__ out_f32) {
    __shared__ UlHeadW wt;              // the image's 99 floats, read at wave-uniform addresses
    {
        const float* src = reinterpret_cast<const float*>(&tab->w[blockIdx.y]->headw);
        float* dst = reinterpret_cast<float*>(&wt);
        if (threadIdx.x < sizeof(UlHeadW) / sizeof(float)) dst[threadIdx.x] = src[threadIdx.x];
    }
    __syncthreads();
    ul_head_body(x, wt, outs, out_f32);
}

}  // namespace

void launch_dwconv3x3(const f16* x, int N, int x_cbt, int x_cb0, int C, int H, int W, int stride, const float* w, const float* scale,
                      const float* shift, int relu, f16* y, int y_cbt, int y_cb0, hipStream_t s) {
    const int CB = C / 16, Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    const unsigned gx = (unsigned)((Ho * Wo * 2 + 255) / 256);
    hipLaunchKernelGGL(dwconv3x3_kernel, dim3(gx, (unsigned)(N * CB)), dim3(256), 0, s, x, x_cbt, x_cb0, CB, H, W, Ho, Wo, stride, w, scale,
                       shift, relu, y, y_cbt, y_cb0);
}

void launch_dwconv3x3_grouped(const f16* x, int N, int x_cbt, int x_cb0, int C, int H, int W, int stride, const UlGroupTab* d_tab, int op,
                              int relu, f16* y, int y_cbt, int y_cb0, hipStream_t s) {
    const int CB = C / 16, Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    const unsigned gx = (unsigned)((Ho * Wo * 2 + 255) / 256);
    hipLaunchKernelGGL(dwconv3x3_grouped_kernel, dim3(gx, (unsigned)(N * CB)), dim3(256), 0, s, x, x_cbt, x_cb0, CB, H, W, Ho, Wo, stride,
                       d_tab, op, relu, y, y_cbt, y_cb0);
}

void launch_upsample2x(const f16* x, int N, int x_cbt, int x_cb0, int C, int h, int w, f16* y, int y_cbt, int y_cb0, hipStream_t s) {
    const int CB = C / 16;
    const unsigned gx = (unsigned)((4 * h * w * 2 + 255) / 256);
    hipLaunchKernelGGL(upsample2x_kernel, dim3(gx, (unsigned)(N * CB)), dim3(256), 0, s, x, x_cbt, x_cb0, CB, h, w, y, y_cbt, y_cb0);
}

void launch_ul_in(const FacePtrs* faces, const float* img6, int N, const UlInW& w, f16* y, hipStream_t s) {
    hipLaunchKernelGGL(ul_in_kernel, dim3((kUlRes * kUlRes + 255) / 256, (unsigned)N), dim3(256), 0, s, faces, img6, w, y);
}

void launch_ul_in_grouped(const FacePtrs* faces, const float* img6, int N, const UlGroupTab* d_tab, f16* y, hipStream_t s) {
    hipLaunchKernelGGL(ul_in_grouped_kernel, dim3((kUlRes * kUlRes + 255) / 256, (unsigned)N), dim3(256), 0, s, faces, img6, d_tab, y);
}

void launch_ul_pack_feat(const MelPtrs* feats, int N, f16* y, hipStream_t s) {
    hipLaunchKernelGGL(ul_pack_feat_kernel, dim3(4, (unsigned)N), dim3(256), 0, s, feats, y);
}

void launch_ul_head(const f16* x, int N, const UlHeadW& w, const OutPtrs* outs, float* out_f32, hipStream_t s) {
    hipLaunchKernelGGL(ul_head_kernel, dim3((kUlRes * kUlRes + 255) / 256, (unsigned)N), dim3(256), 0, s, x, w, outs, out_f32);
}

void launch_ul_head_grouped(const f16* x, int N, const UlGroupTab* d_tab, const OutPtrs* outs, float* out_f32, hipStream_t s) {
    hipLaunchKernelGGL(ul_head_grouped_kernel, dim3((kUlRes * kUlRes + 255) / 256, (unsigned)N), dim3(256), 0, s, x, d_tab, outs, out_f32);
}

}  // namespace ltk

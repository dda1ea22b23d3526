// Kernels of the BiSeNet face parser that are not library convolutions: see parse_kernels.h.  The stem is an implicit GEMM on
// v_mfma_f32_32x32x16_f16 with the operand map of conv7_mfma.hip's audio3_kernel (weights = A, pixels = B); the other four move more
// bytes than they compute on: one item = 8 channels of one pixel = one 16-byte load / store, as in dw_kernels.hip.
#include "parse_kernels.h"

#include <math.h>

namespace ltk {

void parse_stem_pack(const float* weight, f16* out) {
    for (int nt = 0; nt < 2; ++nt)
        for (int s = 0; s < kStemKPad / 16; ++s)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int co = 32 * nt + (lane & 31), k = 16 * s + 8 * (lane >> 5) + j;
                    const int tap = k / 3, c = k - 3 * tap;
                    out[(((size_t)nt * (kStemKPad / 16) + s) * 64 + lane) * 8 + j] = k < kStemK ? (f16)weight[((size_t)co * 3 + c) * 49 + tap] : (f16)0.f;
                }
}

namespace {

typedef f16 f16x8 __attribute__((ext_vector_type(8)));
typedef f16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

union H8 {
    uint4 u;
    f16 h[8];
};

struct F8 {
    float v[8];
};

__device__ __forceinline__ f16 to_f16_sat(float t) { return (f16)__builtin_amdgcn_fmed3f(t, -65504.f, 65504.f); }

// ------------------------------------------------------------------------------------------ stem
constexpr int kStemPR = 2 * kStemTH + 5, kStemPC = 2 * kStemTW + 5;      // input patch of a tile: 21 x 37 pixels
constexpr int kStemRow = kStemPC * 3;                                     // 111 values per patch row
constexpr int kStemPatch = kStemPR * kStemRow;                            // 2331

// patch offset of product k = (ky * 7 + kx) * 3 + c from the window's corner: a window row is 21 consecutive values
__host__ __device__ constexpr int stem_off(int k) { return k < kStemK ? (k / 21) * kStemRow + k % 21 : 0; }

// A block owns an 8 x 16 output tile of one image and all 64 channels; wave w its rows 2w, 2w + 1 (32 pixels = the MFMA's columns).
// The 21 x 37 x 3 input patch is normalised ONCE into LDS as fp16 - 0 outside the image, which is the reference's padding of the
// normalised tensor (a zero BYTE would be -2.1) - and every lane assembles its B operands from it: 8 two-byte reads per K-step.
// The 20 weight operands of a lane (host-packed, 20 KB, L2 resident) are loaded before the patch is staged.
__global__ __launch_bounds__(256) void parse_stem_kernel(const uint8_t* __restrict__ rgb, const int H, const int W, const int Ho, const int Wo,
                                                          const f16x8* __restrict__ wq, const float* __restrict__ scale,
                                                          const float* __restrict__ shift, f16* __restrict__ y, const int y_cbt, const int y_cb0) {
    __shared__ f16 patch[kStemPatch + 5];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, kh = lane >> 5;
    const int n = blockIdx.z, oy0 = blockIdx.y * kStemTH, ox0 = blockIdx.x * kStemTW;
    f16x8 av[2][kStemKPad / 16];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int s = 0; s < kStemKPad / 16; ++s) av[nt][s] = wq[(nt * (kStemKPad / 16) + s) * 64 + lane];
    const int iy0 = 2 * oy0 - 3, ix0 = 2 * ox0 - 3;
    for (int i = t; i < kStemPatch; i += 256) {
        const int row = i / kStemRow, rem = i - row * kStemRow, col = rem / 3, c = rem - 3 * col;
        const int iy = iy0 + row, ix = ix0 + col;
        f16 v = (f16)0.f;
        if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) {
            const float mean = c == 0 ? 0.485f : c == 1 ? 0.456f : 0.406f, sd = c == 0 ? 0.229f : c == 1 ? 0.224f : 0.225f;
            v = (f16)(((float)rgb[(((size_t)n * H + iy) * W + ix) * 3 + c] / 255.0f - mean) / sd);
        }
        patch[i] = v;
    }
    __syncthreads();
    const int py = 2 * wave + (l31 >> 4), px = l31 & 15;
    const f16* win = patch + (2 * py) * kStemRow + (2 * px) * 3;         // + stem_off(146) = 686 <= 2330
    f32x16 acc[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[nt][v] = 0.f;
#pragma unroll
    for (int s = 0; s < kStemKPad / 16; ++s) {
        f16x8 bv;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            // lane half kh holds products 16 s + 8 kh + j; from 147 on the operand is 0 (and so is the weight)
            const int k0 = 16 * s + j, k1 = k0 + 8;
            const f16 xv = win[kh ? stem_off(k1) : stem_off(k0)];
            bv[j] = (kh ? k1 < kStemK : k0 < kStemK) ? xv : (f16)0.f;
        }
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av[nt][s], bv, acc[nt], 0, 0, 0);
    }
    // accumulator v of a lane: output channel 32 nt + 8 (v / 4) + 4 kh + (v % 4) of pixel l31
    const int oy = oy0 + py, ox = ox0 + px;
    if (oy < Ho && ox < Wo) {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int co = 32 * nt + 8 * q + 4 * kh;
                const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + co), sf = *reinterpret_cast<const f32x4*>(shift + co);
                f16x4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] = (f16)__builtin_amdgcn_fmed3f(fmaf(acc[nt][4 * q + r], sc[r], sf[r]), 0.f, 65504.f);
                *reinterpret_cast<f16x4*>(y + ((((size_t)n * y_cbt + y_cb0 + (co >> 4)) * Ho + oy) * Wo + ox) * 16 + (co & 15)) = o;
            }
    }
}

// ------------------------------------------------------------------------------------------ max pool
__global__ __launch_bounds__(256) void maxpool3x3s2_kernel(const f16* __restrict__ x, int x_cbt, int x_cb0, int CB, int H, int W, int Ho, int Wo,
                                                            f16* __restrict__ y, int y_cbt, int y_cb0) {
    const int cb = blockIdx.y % CB, n = blockIdx.y / CB;
    const int item = blockIdx.x * 256 + threadIdx.x;
    if (item >= Ho * Wo * 2) return;
    const int hh = item & 1, p = item >> 1;
    const int oy = p / Wo, ox = p - oy * Wo;
    const f16* xb = x + ((size_t)n * x_cbt + x_cb0 + cb) * H * W * 16 + hh * 8;
    float m[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = -INFINITY;       // the padding; the centre tap is always inside
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = 2 * oy - 1 + ky;
        if ((unsigned)iy >= (unsigned)H) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = 2 * ox - 1 + kx;
            if ((unsigned)ix >= (unsigned)W) continue;
            H8 v;
            v.u = *reinterpret_cast<const uint4*>(xb + ((size_t)iy * W + ix) * 16);
#pragma unroll
            for (int j = 0; j < 8; ++j) m[j] = fmaxf(m[j], (float)v.h[j]);
        }
    }
    H8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o.h[j] = (f16)m[j];
    *reinterpret_cast<uint4*>(y + (((size_t)n * y_cbt + y_cb0 + cb) * Ho * Wo + p) * 16 + hh * 8) = o.u;
}

// ------------------------------------------------------------------------------------------ global average pool
// the binary tree over pixels q + 128 i, i in [LO, LO + CNT): absent pixels are zeros, so its shape does not depend on P
template <int LO, int CNT>
__device__ __forceinline__ F8 gap_tree(const f16* __restrict__ xb, int q, int P) {
    F8 r;
    if constexpr (CNT == 1) {
        const int p = q + 128 * LO;
        if (p < P) {
            H8 v;
            v.u = *reinterpret_cast<const uint4*>(xb + (size_t)p * 16);
#pragma unroll
            for (int j = 0; j < 8; ++j) r.v[j] = (float)v.h[j];
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) r.v[j] = 0.f;
        }
    } else {
        r = gap_tree<LO, CNT / 2>(xb, q, P);
        const F8 b = gap_tree<LO + CNT / 2, CNT / 2>(xb, q, P);
#pragma unroll
        for (int j = 0; j < 8; ++j) r.v[j] += b.v[j];
    }
    return r;
}

// block = one (image, channel block); thread t: channels 8 (t & 1) .. + 7, pixels (t >> 1) + 128 i
__global__ __launch_bounds__(256) void gap_kernel(const f16* __restrict__ x, int x_cbt, int x_cb0, int P, f16* __restrict__ y, int y_cbt, int y_cb0) {
    __shared__ float sm[256 * 8];
    const int cb = blockIdx.x, n = blockIdx.y, t = threadIdx.x, hh = t & 1, q = t >> 1;
    const f16* xb = x + ((size_t)n * x_cbt + x_cb0 + cb) * P * 16 + hh * 8;
    // the tree's two halves one after the other (16 loads in flight each); the upper one is all zeros up to 2048 pixels, and x + 0 = x
    constexpr int kHalf = kGapMaxP / 256;
    F8 acc = gap_tree<0, kHalf>(xb, q, P);
    if (P > kHalf * 128) {
        __builtin_amdgcn_sched_barrier(0);
        const F8 up = gap_tree<kHalf, kHalf>(xb, q, P);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc.v[j] += up.v[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) sm[t * 8 + j] = acc.v[j];
    __syncthreads();
    for (int s = 64; s >= 1; s >>= 1) {
        if (q < s) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                acc.v[j] += sm[(t + 2 * s) * 8 + j];
                sm[t * 8 + j] = acc.v[j];
            }
        }
        __syncthreads();
    }
    if (q == 0) {
        H8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o.h[j] = to_f16_sat(acc.v[j] / (float)P);
        *reinterpret_cast<uint4*>(y + ((size_t)n * y_cbt + y_cb0 + cb) * 16 + hh * 8) = o.u;
    }
}

// ------------------------------------------------------------------------------------------ channel gate
__global__ __launch_bounds__(256) void chan_gate_kernel(const f16* __restrict__ x, int x_cbt, int x_cb0, int CB, int P, const f16* __restrict__ a,
                                                         const f16* __restrict__ b, const f16* __restrict__ r, int r_cbt, int r_cb0, int plus1,
                                                         f16* __restrict__ y, int y_cbt, int y_cb0) {
    const int cb = blockIdx.y % CB, n = blockIdx.y / CB;
    const int item = blockIdx.x * 256 + threadIdx.x;
    if (item >= P * 2) return;
    const int hh = item & 1, p = item >> 1;
    H8 xv, av, bv, rv, o;
    xv.u = *reinterpret_cast<const uint4*>(x + (((size_t)n * x_cbt + x_cb0 + cb) * P + p) * 16 + hh * 8);
    av.u = *reinterpret_cast<const uint4*>(a + ((size_t)n * CB + cb) * 16 + hh * 8);
    if (b) bv.u = *reinterpret_cast<const uint4*>(b + ((size_t)n * CB + cb) * 16 + hh * 8);
    if (r) rv.u = *reinterpret_cast<const uint4*>(r + (((size_t)n * r_cbt + r_cb0 + cb) * P + p) * 16 + hh * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float g = 1.0f / (1.0f + expf(-(float)av.h[j]));
        if (plus1) g += 1.0f;
        float v = (float)xv.h[j] * g;
        if (b) v += (float)bv.h[j];
        if (r) v += (float)rv.h[j];
        o.h[j] = to_f16_sat(v);
    }
    *reinterpret_cast<uint4*>(y + (((size_t)n * y_cbt + y_cb0 + cb) * P + p) * 16 + hh * 8) = o.u;
}

// ------------------------------------------------------------------------------------------ segmentation head
// one thread = one output pixel: the four source pixels' 19 logits (3 x 16-byte loads each; the 64 outputs of a source cell share
// them through the L1), 19 interpolations, a running first-wins maximum, one byte
__global__ __launch_bounds__(256) void seg_argmax_kernel(const f16* __restrict__ x, int h, int w, uint8_t* __restrict__ labels) {
    const int n = blockIdx.y;
    const int Ho = 8 * h, Wo = 8 * w;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= Ho * Wo) return;
    const int oy = p / Wo, ox = p - oy * Wo;
    // align_corners: src = o * (in - 1) / (out - 1), exact quotient and remainder (a one-pixel axis maps everything to pixel 0)
    const int ny = oy * (h - 1), dy = Ho - 1, nx = ox * (w - 1), dx = Wo - 1;
    const int y0 = ny / dy, x0 = nx / dx;
    const float ly = (float)(ny - y0 * dy) / (float)dy, lx = (float)(nx - x0 * dx) / (float)dx;
    const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
    const size_t hw = (size_t)h * w;
    const f16* xn = x + (size_t)n * 2 * hw * 16;
    const size_t o00 = ((size_t)y0 * w + x0) * 16, o01 = ((size_t)y0 * w + x1) * 16, o10 = ((size_t)y1 * w + x0) * 16, o11 = ((size_t)y1 * w + x1) * 16;
    float best = -INFINITY;
    int label = 0;
#pragma unroll
    for (int g = 0; g < 3; ++g) {                       // classes 8 g .. 8 g + 7 (16 .. 18 of the second channel block)
        const f16* xg = xn + (g >> 1) * hw * 16 + (g & 1) * 8;
        H8 a, b, c, d;
        a.u = *reinterpret_cast<const uint4*>(xg + o00);
        b.u = *reinterpret_cast<const uint4*>(xg + o01);
        c.u = *reinterpret_cast<const uint4*>(xg + o10);
        d.u = *reinterpret_cast<const uint4*>(xg + o11);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (8 * g + j >= kSegClasses) break;
            const float top = fmaf(lx, (float)b.h[j] - (float)a.h[j], (float)a.h[j]);
            const float bot = fmaf(lx, (float)d.h[j] - (float)c.h[j], (float)c.h[j]);
            const float v = fmaf(ly, bot - top, top);
            if (v > best) {
                best = v;
                label = 8 * g + j;
            }
        }
    }
    labels[(size_t)n * Ho * Wo + p] = (uint8_t)label;
}

int refuse(std::string* err, const char* msg) {
    if (err) *err = msg;
    return -1;
}

// the checks every channel-blocked launch shares: a view inside its buffer, a grid the launch can address, 31-bit element counts
bool view_ok(int cbt, int cb0, int CB) { return cbt > 0 && cb0 >= 0 && cb0 + CB <= cbt; }
bool size_ok(int N, int cbt, double pixels) { return (double)N * cbt * 16.0 * pixels < 2147483647.0; }

}  // namespace

int launch_parse_stem(const uint8_t* rgb, int N, int H, int W, const f16* wq, const float* scale, const float* shift, f16* y, int y_cbt,
                      int y_cb0, hipStream_t s, std::string* err) {
    if (!rgb || !wq || !scale || !shift || !y || N <= 0 || H <= 0 || W <= 0) return refuse(err, "parse stem: bad arguments");
    if ((H | W) & 1) return refuse(err, "parse stem: H and W must be even");
    if (!view_ok(y_cbt, y_cb0, kStemCout / 16)) return refuse(err, "parse stem: the output view leaves its buffer");
    const int Ho = H / 2, Wo = W / 2;
    const unsigned gx = (unsigned)((Wo + kStemTW - 1) / kStemTW), gy = (unsigned)((Ho + kStemTH - 1) / kStemTH);
    if (N > 65535 || gy > 65535 || !size_ok(N, y_cbt, (double)Ho * Wo) || (double)N * H * W * 3.0 >= 2147483647.0)
        return refuse(err, "parse stem: tensor too large");
    hipLaunchKernelGGL(parse_stem_kernel, dim3(gx, gy, (unsigned)N), dim3(256), 0, s, rgb, H, W, Ho, Wo, reinterpret_cast<const f16x8*>(wq), scale,
                       shift, y, y_cbt, y_cb0);
    return 0;
}

int launch_maxpool3x3s2(const f16* x, int N, int x_cbt, int x_cb0, int C, int H, int W, f16* y, int y_cbt, int y_cb0, hipStream_t s,
                        std::string* err) {
    if (!x || !y || N <= 0 || C <= 0 || H <= 0 || W <= 0) return refuse(err, "maxpool: bad arguments");
    if (C % 16) return refuse(err, "maxpool: C % 16 == 0");
    const int CB = C / 16, Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    if (!view_ok(x_cbt, x_cb0, CB) || !view_ok(y_cbt, y_cb0, CB)) return refuse(err, "maxpool: a channel view leaves its buffer");
    if ((long long)N * CB > 65535 || !size_ok(N, x_cbt, (double)H * W) || !size_ok(N, y_cbt, (double)Ho * Wo)) return refuse(err, "maxpool: tensor too large");
    const unsigned gx = (unsigned)((Ho * Wo * 2 + 255) / 256);
    hipLaunchKernelGGL(maxpool3x3s2_kernel, dim3(gx, (unsigned)(N * CB)), dim3(256), 0, s, x, x_cbt, x_cb0, CB, H, W, Ho, Wo, y, y_cbt, y_cb0);
    return 0;
}

int launch_gap(const f16* x, int N, int x_cbt, int x_cb0, int C, int P, f16* y, int y_cbt, int y_cb0, hipStream_t s, std::string* err) {
    if (!x || !y || N <= 0 || C <= 0 || P <= 0) return refuse(err, "global average pool: bad arguments");
    if (C % 16) return refuse(err, "global average pool: C % 16 == 0");
    if (P > kGapMaxP) return refuse(err, "global average pool: at most 4096 pixels");
    const int CB = C / 16;
    if (!view_ok(x_cbt, x_cb0, CB) || !view_ok(y_cbt, y_cb0, CB)) return refuse(err, "global average pool: a channel view leaves its buffer");
    if (N > 65535 || !size_ok(N, x_cbt, (double)P)) return refuse(err, "global average pool: tensor too large");
    hipLaunchKernelGGL(gap_kernel, dim3((unsigned)CB, (unsigned)N), dim3(256), 0, s, x, x_cbt, x_cb0, P, y, y_cbt, y_cb0);
    return 0;
}

int launch_chan_gate(const f16* x, int N, int x_cbt, int x_cb0, int C, int P, const f16* a, const f16* b, const f16* r, int r_cbt,
                     int r_cb0, int plus1, f16* y, int y_cbt, int y_cb0, hipStream_t s, std::string* err) {
    if (!x || !a || !y || N <= 0 || C <= 0 || P <= 0) return refuse(err, "channel gate: bad arguments");
    if (C % 16) return refuse(err, "channel gate: C % 16 == 0");
    const int CB = C / 16;
    if (!view_ok(x_cbt, x_cb0, CB) || !view_ok(y_cbt, y_cb0, CB) || (r && !view_ok(r_cbt, r_cb0, CB)))
        return refuse(err, "channel gate: a channel view leaves its buffer");
    if ((long long)N * CB > 65535 || !size_ok(N, x_cbt, (double)P) || !size_ok(N, y_cbt, (double)P) || (r && !size_ok(N, r_cbt, (double)P)))
        return refuse(err, "channel gate: tensor too large");
    const unsigned gx = (unsigned)((P * 2 + 255) / 256);
    hipLaunchKernelGGL(chan_gate_kernel, dim3(gx, (unsigned)(N * CB)), dim3(256), 0, s, x, x_cbt, x_cb0, CB, P, a, b, r, r_cbt, r_cb0, plus1 ? 1 : 0, y,
                       y_cbt, y_cb0);
    return 0;
}

int launch_seg_argmax(const f16* x, int N, int h, int w, uint8_t* labels, hipStream_t s, std::string* err) {
    if (!x || !labels || N <= 0 || h <= 0 || w <= 0) return refuse(err, "seg argmax: bad arguments");
    if (N > 65535 || (double)N * 64.0 * h * w >= 2147483647.0) return refuse(err, "seg argmax: tensor too large");
    const unsigned gx = (unsigned)((64 * h * w + 255) / 256);
    hipLaunchKernelGGL(seg_argmax_kernel, dim3(gx, (unsigned)N), dim3(256), 0, s, x, h, w, labels);
    return 0;
}

}  // namespace ltk

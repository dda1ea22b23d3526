// Kernels of the S3FD face detector that are not library convolutions: see s3fd_kernels.h.  The stem is an implicit GEMM on
// v_mfma_f32_16x16x32_f16 (weights = A, pixels = B: K = 27 of 32, one MFMA per 16 pixels x 16 outputs); the pool and the norm move
// more bytes than they compute on; the detect kernel reads one 32-byte pixel of the merged head map per thread.
#include "s3fd_kernels.h"

#include <math.h>

namespace ltk {

void s3fd_stem_pack(const float* weight, f16* out) {
    for (int nt = 0; nt < 4; ++nt)
        for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < 8; ++j) {
                const int co = 16 * nt + (lane & 15), k = 8 * (lane >> 4) + j;
                const int tap = k / 3, c = k - 3 * tap;
                out[((size_t)nt * 64 + lane) * 8 + j] = k < kFdStemK ? (f16)weight[((size_t)co * 3 + c) * 9 + tap] : (f16)0.f;
            }
}

namespace {

typedef f16 f16x8 __attribute__((ext_vector_type(8)));
typedef f16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

union H8 {
    uint4 u;
    f16 h[8];
};

__device__ __forceinline__ f16 to_f16_sat(float t) { return (f16)__builtin_amdgcn_fmed3f(t, -65504.f, 65504.f); }

// ------------------------------------------------------------------------------------------ stem
constexpr int kFdPR = kFdStemTH + 2, kFdPC = kFdStemTW + 2;              // input patch of a tile: 18 x 18 pixels
constexpr int kFdRow = kFdPC * 3;                                         // 54 values per patch row
constexpr int kFdPatch = kFdPR * kFdRow;                                  // 972

// A block owns a 16 x 16 output tile of one image and all 64 channels; wave w its rows 4w .. 4w + 3, one row of 16 pixels = the MFMA's
// columns at a time.  The 18 x 18 x 3 patch goes into LDS ONCE as fp16, reversed and mean-subtracted - 0 outside the image, the
// reference's padding of the mean-subtracted tensor (a zero BYTE would be -104) -; a lane's 8 products k = 8 (lane >> 4) + j sit at
// (k / 9) * 54 + k % 9 from its pixel's corner (k % 9 = kx * 3 + c: a window row is 9 consecutive values).
__global__ __launch_bounds__(256) void s3fd_stem_kernel(const uint8_t* __restrict__ bgr, const int H, const int W, const f16x8* __restrict__ wq,
                                                         const float* __restrict__ bias, f16* __restrict__ y, const int y_cbt, const int y_cb0) {
    __shared__ f16 patch[kFdPatch];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, px = lane & 15, kq = lane >> 4;
    const int n = blockIdx.z, oy0 = blockIdx.y * kFdStemTH, ox0 = blockIdx.x * kFdStemTW;
    f16x8 av[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) av[nt] = wq[nt * 64 + lane];
    for (int i = t; i < kFdPatch; i += 256) {
        const int row = i / kFdRow, rem = i - row * kFdRow, col = rem / 3, c = rem - 3 * col;
        const int iy = oy0 - 1 + row, ix = ox0 - 1 + col;
        f16 v = (f16)0.f;
        if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) {
            const float mean = c == 0 ? 104.f : c == 1 ? 117.f : 123.f;
            v = (f16)((float)bgr[(((size_t)n * H + iy) * W + ix) * 3 + (2 - c)] - mean);
        }
        patch[i] = v;
    }
    __syncthreads();
    int off[8];
    bool live[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = 8 * kq + j;
        live[j] = k < kFdStemK;
        off[j] = live[j] ? (k / 9) * kFdRow + k % 9 : 0;                  // <= 2 * 54 + 8
    }
    const int ox = ox0 + px;
    f32x4 bv[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) bv[nt] = *reinterpret_cast<const f32x4*>(bias + 16 * nt + 4 * kq);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int py = 4 * wave + r, oy = oy0 + py;
        if (oy >= H) break;                                               // wave-uniform
        const f16* win = patch + py * kFdRow + px * 3;                    // + off <= 15 * 54 + 45 + 116 = 971
        f16x8 xv;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const f16 v = win[off[j]];
            xv[j] = live[j] ? v : (f16)0.f;
        }
        // accumulator q of a lane: output channel 16 nt + 4 kq + q of pixel px
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[nt], xv, acc, 0, 0, 0);
            if (ox < W) {
                f16x4 o;
#pragma unroll
                for (int q = 0; q < 4; ++q) o[q] = (f16)__builtin_amdgcn_fmed3f(acc[q] + bv[nt][q], 0.f, 65504.f);
                *reinterpret_cast<f16x4*>(y + ((((size_t)n * y_cbt + y_cb0 + nt) * H + oy) * W + ox) * 16 + 4 * kq) = o;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ max pool
// one item = 8 channels of one output pixel: four 16-byte loads, one store
__global__ __launch_bounds__(256) void maxpool2x2s2_kernel(const f16* __restrict__ x, int x_cbt, int x_cb0, int CB, int H, int W, int Ho, int Wo,
                                                            f16* __restrict__ y, int y_cbt, int y_cb0) {
    const int cb = blockIdx.y % CB, n = blockIdx.y / CB;
    const int item = blockIdx.x * 256 + threadIdx.x;
    if (item >= Ho * Wo * 2) return;
    const int hh = item & 1, p = item >> 1;
    const int oy = p / Wo, ox = p - oy * Wo;
    const f16* xb = x + ((size_t)n * x_cbt + x_cb0 + cb) * H * W * 16 + hh * 8;
    H8 a, b, c, d, o;
    a.u = *reinterpret_cast<const uint4*>(xb + ((size_t)(2 * oy) * W + 2 * ox) * 16);          // 2 oy + 1 < H and 2 ox + 1 < W: floor mode
    b.u = *reinterpret_cast<const uint4*>(xb + ((size_t)(2 * oy) * W + 2 * ox + 1) * 16);
    c.u = *reinterpret_cast<const uint4*>(xb + ((size_t)(2 * oy + 1) * W + 2 * ox) * 16);
    d.u = *reinterpret_cast<const uint4*>(xb + ((size_t)(2 * oy + 1) * W + 2 * ox + 1) * 16);
#pragma unroll
    for (int j = 0; j < 8; ++j) o.h[j] = (f16)fmaxf(fmaxf((float)a.h[j], (float)b.h[j]), fmaxf((float)c.h[j], (float)d.h[j]));
    *reinterpret_cast<uint4*>(y + (((size_t)n * y_cbt + y_cb0 + cb) * Ho * Wo + p) * 16 + hh * 8) = o.u;
}

// ------------------------------------------------------------------------------------------ L2Norm
// one thread = one pixel: a first walk over its C / 16 channel blocks (stride P * 16 halfs; the 32 bytes of neighbouring pixels are
// neighbours) sums the squares in fp32, channel 0 first; a second one, out of the L2, scales and stores
__global__ __launch_bounds__(256) void l2norm_kernel(const f16* __restrict__ x, int x_cbt, int x_cb0, int CB, int P, const float* __restrict__ weight,
                                                      f16* __restrict__ y, int y_cbt, int y_cb0) {
    const int n = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const f16* xp = x + (((size_t)n * x_cbt + x_cb0) * P + p) * 16;
    f16* yp = y + (((size_t)n * y_cbt + y_cb0) * P + p) * 16;
    const size_t cs = (size_t)P * 16;
    float ss = 0.f;
    for (int cb = 0; cb < CB; ++cb) {
        H8 lo, hi;
        lo.u = *reinterpret_cast<const uint4*>(xp + cb * cs);
        hi.u = *reinterpret_cast<const uint4*>(xp + cb * cs + 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) ss = fmaf((float)lo.h[j], (float)lo.h[j], ss);
#pragma unroll
        for (int j = 0; j < 8; ++j) ss = fmaf((float)hi.h[j], (float)hi.h[j], ss);
    }
    const float inv = 1.0f / (sqrtf(ss) + 1e-10f);          // an all-zero pixel: 1e10 times 0
    for (int cb = 0; cb < CB; ++cb) {
        H8 lo, hi;
        lo.u = *reinterpret_cast<const uint4*>(xp + cb * cs);
        hi.u = *reinterpret_cast<const uint4*>(xp + cb * cs + 8);
        const f32x4 w0 = *reinterpret_cast<const f32x4*>(weight + cb * 16), w1 = *reinterpret_cast<const f32x4*>(weight + cb * 16 + 4);
        const f32x4 w2 = *reinterpret_cast<const f32x4*>(weight + cb * 16 + 8), w3 = *reinterpret_cast<const f32x4*>(weight + cb * 16 + 12);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            lo.h[j] = to_f16_sat((float)lo.h[j] * inv * w0[j]);
            lo.h[4 + j] = to_f16_sat((float)lo.h[4 + j] * inv * w1[j]);
            hi.h[j] = to_f16_sat((float)hi.h[j] * inv * w2[j]);
            hi.h[4 + j] = to_f16_sat((float)hi.h[4 + j] * inv * w3[j]);
        }
        *reinterpret_cast<uint4*>(yp + cb * cs) = lo.u;
        *reinterpret_cast<uint4*>(yp + cb * cs + 8) = hi.u;
    }
}

// ------------------------------------------------------------------------------------------ detect
__global__ __launch_bounds__(256) void s3fd_detect_kernel(const f16* __restrict__ x, int x_cbt, int x_cb0, int H, int W, int maxout, int level,
                                                           float thresh, const float* __restrict__ d_thresh, uint32_t* __restrict__ recs, int cap,
                                                           uint32_t* __restrict__ counts) {
    const int n = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= H * W) return;
    H8 v;
    v.u = *reinterpret_cast<const uint4*>(x + (((size_t)n * x_cbt + x_cb0) * H * W + p) * 16);     // channels 0 .. 7: conf and loc
    float c0 = (float)v.h[0], c1 = (float)v.h[1];
    if (maxout) {
        c0 = fmaxf(fmaxf(c0, c1), (float)v.h[2]);
        c1 = (float)v.h[3];
    }
    // F.softmax(dim=1) over two channels, as torch states it: exp(c - max) / sum
    const float m = fmaxf(c0, c1), e0 = expf(c0 - m), e1 = expf(c1 - m);
    const float score = e1 / (e0 + e1);
    if (!(score > (d_thresh ? *d_thresh : thresh))) return;
    const int h = p / W, w = p - h * W;
    const float stride = (float)(1 << (level + 2)), size = 4.f * stride;
    const float axc = 0.5f * stride + (float)w * stride, ayc = 0.5f * stride + (float)h * stride;
    // batch_decode: centre = prior + loc * 0.1 * size, extent = size * exp(loc * 0.2); corner = centre - extent / 2, far corner = extent + corner
    const float cx = axc + (float)v.h[4] * 0.1f * size, cy = ayc + (float)v.h[5] * 0.1f * size;
    const float bw = size * expf((float)v.h[6] * 0.2f), bh = size * expf((float)v.h[7] * 0.2f);
    const float x1 = cx - bw / 2.f, y1 = cy - bh / 2.f;
    const uint32_t slot = atomicAdd(counts + n, 1u);
    if (slot >= (uint32_t)cap) return;
    uint32_t* r = recs + ((size_t)n * cap + slot) * kFdRecWords;
    r[0] = ((uint32_t)level << 28) | ((uint32_t)h << kFdKeyBits) | (uint32_t)w;
    r[1] = __float_as_uint(x1);
    r[2] = __float_as_uint(y1);
    r[3] = __float_as_uint(bw + x1);
    r[4] = __float_as_uint(bh + y1);
    r[5] = __float_as_uint(score);
}

int refuse(std::string* err, const char* msg) {
    if (err) *err = msg;
    return -1;
}

// the checks every channel-blocked launch shares: a view inside its buffer, 31-bit element counts
bool view_ok(int cbt, int cb0, int CB) { return cbt > 0 && cb0 >= 0 && cb0 + CB <= cbt; }
bool size_ok(int N, int cbt, double pixels) { return (double)N * cbt * 16.0 * pixels < 2147483647.0; }

}  // namespace

int launch_s3fd_stem(const uint8_t* bgr, int N, int H, int W, const f16* wq, const float* bias, f16* y, int y_cbt, int y_cb0, hipStream_t s,
                     std::string* err) {
    if (!bgr || !wq || !bias || !y || N <= 0 || H <= 0 || W <= 0) return refuse(err, "s3fd stem: bad arguments");
    if (!view_ok(y_cbt, y_cb0, kFdStemCout / 16)) return refuse(err, "s3fd stem: the output view leaves its buffer");
    const unsigned gx = (unsigned)((W + kFdStemTW - 1) / kFdStemTW), gy = (unsigned)((H + kFdStemTH - 1) / kFdStemTH);
    if (N > 65535 || gy > 65535 || !size_ok(N, y_cbt, (double)H * W) || (double)N * H * W * 3.0 >= 2147483647.0)
        return refuse(err, "s3fd stem: tensor too large");
    hipLaunchKernelGGL(s3fd_stem_kernel, dim3(gx, gy, (unsigned)N), dim3(256), 0, s, bgr, H, W, reinterpret_cast<const f16x8*>(wq), bias, y, y_cbt,
                       y_cb0);
    return 0;
}

int launch_maxpool2x2s2(const f16* x, int N, int x_cbt, int x_cb0, int C, int H, int W, f16* y, int y_cbt, int y_cb0, hipStream_t s,
                        std::string* err) {
    if (!x || !y || N <= 0 || C <= 0 || H <= 0 || W <= 0) return refuse(err, "maxpool 2x2: bad arguments");
    if (C % 16) return refuse(err, "maxpool 2x2: C % 16 == 0");
    if (H < 2 || W < 2) return refuse(err, "maxpool 2x2: the map is smaller than the window");
    const int CB = C / 16, Ho = H / 2, Wo = W / 2;
    if (!view_ok(x_cbt, x_cb0, CB) || !view_ok(y_cbt, y_cb0, CB)) return refuse(err, "maxpool 2x2: a channel view leaves its buffer");
    if ((long long)N * CB > 65535 || !size_ok(N, x_cbt, (double)H * W) || !size_ok(N, y_cbt, (double)Ho * Wo))
        return refuse(err, "maxpool 2x2: tensor too large");
    const unsigned gx = (unsigned)(((long long)Ho * Wo * 2 + 255) / 256);
    hipLaunchKernelGGL(maxpool2x2s2_kernel, dim3(gx, (unsigned)(N * CB)), dim3(256), 0, s, x, x_cbt, x_cb0, CB, H, W, Ho, Wo, y, y_cbt, y_cb0);
    return 0;
}

int launch_l2norm(const f16* x, int N, int x_cbt, int x_cb0, int C, int P, const float* weight, f16* y, int y_cbt, int y_cb0, hipStream_t s,
                  std::string* err) {
    if (!x || !weight || !y || N <= 0 || C <= 0 || P <= 0) return refuse(err, "l2norm: bad arguments");
    if (C % 16) return refuse(err, "l2norm: C % 16 == 0");
    const int CB = C / 16;
    if (!view_ok(x_cbt, x_cb0, CB) || !view_ok(y_cbt, y_cb0, CB)) return refuse(err, "l2norm: a channel view leaves its buffer");
    if (N > 65535 || !size_ok(N, x_cbt, (double)P) || !size_ok(N, y_cbt, (double)P)) return refuse(err, "l2norm: tensor too large");
    const unsigned gx = (unsigned)((P + 255) / 256);
    hipLaunchKernelGGL(l2norm_kernel, dim3(gx, (unsigned)N), dim3(256), 0, s, x, x_cbt, x_cb0, CB, P, weight, y, y_cbt, y_cb0);
    return 0;
}

int launch_s3fd_detect(const f16* x, int N, int x_cbt, int x_cb0, int H, int W, int maxout, int level, float thresh, const float* d_thresh,
                       uint32_t* recs, int cap, uint32_t* counts, hipStream_t s, std::string* err) {
    if (!x || !recs || !counts || N <= 0 || H <= 0 || W <= 0 || cap <= 0) return refuse(err, "s3fd detect: bad arguments");
    if (level < 0 || level >= kFdLevels) return refuse(err, "s3fd detect: level must be in [0, 6)");
    if (!d_thresh && !(thresh >= 0.f && thresh < 1.f)) return refuse(err, "s3fd detect: thresh must be in [0, 1)");
    if (!view_ok(x_cbt, x_cb0, 1)) return refuse(err, "s3fd detect: the head view leaves its buffer");
    if (H >= (1 << kFdKeyBits) || W >= (1 << kFdKeyBits)) return refuse(err, "s3fd detect: a map side must be below 16384 (the key's 14 bits)");
    if (N > 65535 || !size_ok(N, x_cbt, (double)H * W) || (double)N * cap * kFdRecWords >= 2147483647.0)
        return refuse(err, "s3fd detect: tensor too large");
    const unsigned gx = (unsigned)((H * W + 255) / 256);
    hipLaunchKernelGGL(s3fd_detect_kernel, dim3(gx, (unsigned)N), dim3(256), 0, s, x, x_cbt, x_cb0, H, W, maxout ? 1 : 0, level, thresh, d_thresh, recs,
                       cap, counts);
    return 0;
}

}  // namespace ltk

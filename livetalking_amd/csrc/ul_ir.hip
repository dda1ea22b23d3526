// ul_ir_kernel: an inverted residual of the Ultralight program (ul_ir.h) in one launch.  A block of four waves owns ONE image's tile of
// 8 x 8 OUTPUT pixels and walks the hidden channels in chunks of 64:
//   expand     e1 = f16_sat(relu(W1 . x * scale1 + shift1)) for every hidden pixel the tile's depthwise windows touch (the tile and its
//              halo at input resolution: 10 x 10 at stride 1, 17 x 17 at stride 2), v_mfma_f32_16x16x32_f16 with both operands as 16-byte
//              loads from global memory (ul_gconv.hip's scheme; weights as A, pixels as B); wave w takes the 16-pixel tiles w, w + 4, ..
//              and all four 16-channel tiles of the chunk.  A hidden pixel outside the map is ZERO (the depthwise conv pads the hidden
//              map; relu(shift1) is not zero).  The chunk's e1 goes to LDS as [4 channel blocks][hidden pixel][16].
//   depthwise  dwconv3x3_body's arithmetic from LDS: fp32 weights, taps in ky, kx order, one fmaf each, out-of-map taps skipped, then
//              fmaf(acc, scale, shift), ReLU, to_f16_sat; one item = 8 channels of one output pixel.  e2 goes to LDS as [4][64 pixels][16].
//   project    acc2 += W2[:, chunk] . e2 on the MFMAs, two k-steps per chunk, the accumulators in registers across the chunks: the
//              (output channel tile j, pixel tile p) pairs are dealt round over the waves, JT = Cout / 16 pairs each.
// After the last chunk y = f16_sat(acc2 * scale2 + shift2 + res): the residual behind the affine, no ReLU.
//
// One summation order per element: channel blocks ascend, one accumulator, no split of K, no atomics; what a lane sums does not depend
// on the image count, the tile or the pixel's place in it, so a halo pixel a neighbouring block recomputes carries the owner's bits.
// Rounding points are those of the three launches it replaces: e1 and e2 are fp16 values, the output is rounded once.
// The tap instantiation also stores e1 / e2, every element by the one block that owns it (e2: its output pixels; e1: the input pixels
// [S oy, S oy + S) x [S ox, S ox + S) of its output pixels, clipped to the map).
#include "ul_ir.h"

#include <hip/hip_fp16.h>

#include <algorithm>
#include <cstdio>
#include <cstring>

namespace ltk {

typedef f16 f16x8 __attribute__((ext_vector_type(8)));
typedef f16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kIrPx = kIrTH * kIrTW;              // 64 output pixels = four 16-pixel MFMA tiles
constexpr int kIrCB = kIrMC / 16;                 // channel blocks per chunk
static_assert(kIrPx == 64 && kIrTW == 8 && kIrCB == 4 && kIrThreads == 256, "the index arithmetic below");
// offsets into a chunk's fp32 record
constexpr int kPS1 = 0, kPB1 = kIrMC, kPDW = 2 * kIrMC, kPSD = kPDW + kIrCB * 144, kPBD = kPSD + kIrMC;
static_assert(kPBD + kIrMC == kIrParamFloats, "ul_ir.h kIrParamFloats");

struct UlIrArgs {
    UlIrW w;
    const f16* x; int x_cbt, x_cb0;
    f16* y; int y_cbt, y_cb0;
    const f16* res; int res_cbt, res_cb0;
    f16* e1; f16* e2;
    int H, W, Ho, Wo, S;
    int CB;            // input channel blocks
    int KS1;           // k-steps of the expand: ceil(CB / 2)
    int MB;            // hidden channel blocks (mid / 16)
    int chunks;
    int hid_w, hid_px; // the hidden tile: width, pixels
    int NT;            // ... in 16-pixel tiles
};

union H8 {
    uint4 u;
    f16 h[8];
};

__device__ __forceinline__ f16 to_f16_sat(float t) { return (f16)__builtin_amdgcn_fmed3f(t, -65504.f, 65504.f); }

}  // namespace

template <int JT, bool TAP>
__global__ __launch_bounds__(kIrThreads) void ul_ir_kernel(const UlIrArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ir_smem[];
    float* const par = reinterpret_cast<float*>(ir_smem);
    f16* const e2s = reinterpret_cast<f16*>(ir_smem + kIrParamFloats * sizeof(float));
    f16* const e1s = e2s + kIrCB * kIrPx * 16;
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int i16 = lane & 15, g = lane >> 4;
    const int n = blockIdx.z;
    const int oy0 = blockIdx.y * kIrTH, ox0 = blockIdx.x * kIrTW;
    const int hy0 = oy0 * a.S - 1, hx0 = ox0 * a.S - 1;        // the hidden tile's first pixel, in map coordinates
    const int HWi = a.H * a.W, HWo = a.Ho * a.Wo;
    const int HPXP = a.NT * 16;
    const f16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    const f16* const xn = a.x + ((size_t)n * a.x_cbt + a.x_cb0) * HWi * 16 + (g & 1) * 8;
    f32x4 acc2[JT];
#pragma unroll
    for (int r = 0; r < JT; ++r) acc2[r] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int ch = 0; ch < a.chunks; ++ch) {
        for (int i = t; i < kIrParamFloats; i += kIrThreads) par[i] = a.w.par[(size_t)ch * kIrParamFloats + i];
        __syncthreads();
        // ---- expand: hidden pixel tiles wave, wave + 4, ..
        for (int pt = wave; pt < a.NT; pt += 4) {
            const int hp = pt * 16 + i16;
            const int hy = hp / a.hid_w, hx = hp - hy * a.hid_w;
            const int iy = hy0 + hy, ix = hx0 + hx;
            const bool in = hp < a.hid_px && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
            const f16* const xp = xn + (size_t)(in ? iy * a.W + ix : 0) * 16;
            const f16x8* const wp = reinterpret_cast<const f16x8*>(a.w.w1) + (size_t)ch * kIrCB * a.KS1 * 64 + lane;
            f32x4 acc[kIrCB];
#pragma unroll
            for (int c = 0; c < kIrCB; ++c) acc[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
            for (int ks = 0; ks < a.KS1; ++ks) {
                // channel block 2 ks + (g >> 1), half g & 1 of the step's 32 channels; zeros outside the map and behind the last block
                const int cb = 2 * ks + (g >> 1);
                const f16x8 xb = (in && cb < a.CB) ? *reinterpret_cast<const f16x8*>(xp + (size_t)cb * HWi * 16) : zero;
#pragma unroll
                for (int c = 0; c < kIrCB; ++c)
                    acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wp[((size_t)c * a.KS1 + ks) * 64], xb, acc[c], 0, 0, 0);
            }
            // D layout: this lane holds hidden channels 4 g .. 4 g + 3 of each 16-channel tile, pixel i16
            const bool own = TAP && in && hy >= 1 && hy <= a.S * kIrTH && hx >= 1 && hx <= a.S * kIrTW;
#pragma unroll
            for (int c = 0; c < kIrCB; ++c) {
                f16x4 o;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int ci = c * 16 + 4 * g + q;
                    const float v = acc[c][q] * par[kPS1 + ci] + par[kPB1 + ci];
                    o[q] = in ? (f16)__builtin_amdgcn_fmed3f(v, 0.f, 65504.f) : (f16)0.f;
                }
                *reinterpret_cast<f16x4*>(e1s + ((size_t)c * HPXP + hp) * 16 + 4 * g) = o;
                if (TAP) {
                    const int cbm = ch * kIrCB + c;
                    if (own && cbm < a.MB)
                        *reinterpret_cast<f16x4*>(a.e1 + (((size_t)n * a.MB + cbm) * HWi + iy * a.W + ix) * 16 + 4 * g) = o;
                }
            }
        }
        __syncthreads();
        // ---- depthwise: 4 channel blocks x 64 output pixels x 2 halves = 512 items
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int item = it * kIrThreads + t;
            const int hh = item & 1, px = (item >> 1) & (kIrPx - 1), c = item >> 7;
            const int oyl = px >> 3, oxl = px & 7;
            const int oy = oy0 + oyl, ox = ox0 + oxl;
            const f16* const eb = e1s + (size_t)c * HPXP * 16 + hh * 8;
            float acc[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int iy = oy * a.S - 1 + ky;
                if ((unsigned)iy >= (unsigned)a.H) continue;          // zero padding
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int ix = ox * a.S - 1 + kx;
                    if ((unsigned)ix >= (unsigned)a.W) continue;
                    H8 v;
                    v.u = *reinterpret_cast<const uint4*>(eb + ((oyl * a.S + ky) * a.hid_w + oxl * a.S + kx) * 16);
                    const float* wt = par + kPDW + (c * 9 + ky * 3 + kx) * 16 + hh * 8;
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] = fmaf((float)v.h[j], wt[j], acc[j]);
                }
            }
            H8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int ci = c * 16 + hh * 8 + j;
                o.h[j] = to_f16_sat(fmaxf(fmaf(acc[j], par[kPSD + ci], par[kPBD + ci]), 0.f));
            }
            *reinterpret_cast<uint4*>(e2s + ((size_t)c * kIrPx + px) * 16 + hh * 8) = o.u;
            if (TAP) {
                const int cbm = ch * kIrCB + c;
                if (oy < a.Ho && ox < a.Wo && cbm < a.MB)
                    *reinterpret_cast<uint4*>(a.e2 + (((size_t)n * a.MB + cbm) * HWo + oy * a.Wo + ox) * 16 + hh * 8) = o.u;
            }
        }
        __syncthreads();
        // ---- project: the chunk's two k-steps into the block's accumulators; pair r of this wave = (tile j, pixel tile p)
#pragma unroll
        for (int ks = 0; ks < kIrMC / 32; ++ks) {
#pragma unroll
            for (int r = 0; r < JT; ++r) {
                const int idx = r * 4 + wave, j = idx % JT, p = idx / JT;
                const f16x8 wa = reinterpret_cast<const f16x8*>(a.w.w2)[((size_t)j * (a.chunks * (kIrMC / 32)) + ch * (kIrMC / 32) + ks) * 64 + lane];
                const f16x8 eb = *reinterpret_cast<const f16x8*>(e2s + ((size_t)(2 * ks + (g >> 1)) * kIrPx + p * 16 + i16) * 16 + (g & 1) * 8);
                acc2[r] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa, eb, acc2[r], 0, 0, 0);
            }
        }
        // (the next chunk's first barrier stands between these reads of e2s and its depthwise stores)
    }

    // ---- output: lane holds output channels 4 g .. 4 g + 3 of tile j, pixel i16 of pixel tile p
#pragma unroll
    for (int r = 0; r < JT; ++r) {
        const int idx = r * 4 + wave, j = idx % JT, p = idx / JT;
        const int px = p * 16 + i16;
        const int oy = oy0 + (px >> 3), ox = ox0 + (px & 7);
        if (oy >= a.Ho || ox >= a.Wo) continue;                    // ragged tile: nothing stored
        const int j0 = j * 16 + 4 * g;
        const f32x4 sc = *reinterpret_cast<const f32x4*>(a.w.ss2 + j0), sf = *reinterpret_cast<const f32x4*>(a.w.ss2 + JT * 16 + j0);
        const size_t po = (size_t)oy * a.Wo + ox;
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = acc2[r][q] * sc[q] + sf[q];
        if (a.res) {                                               // behind the affine
            const f16x4 rv = *reinterpret_cast<const f16x4*>(a.res + (((size_t)n * a.res_cbt + a.res_cb0 + j) * HWo + po) * 16 + 4 * g);
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] += (float)rv[q];
        }
        f16x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = to_f16_sat(v[q]);
        *reinterpret_cast<f16x4*>(a.y + (((size_t)n * a.y_cbt + a.y_cb0 + j) * HWo + po) * 16 + 4 * g) = o;
    }
}

namespace {

template <int JT>
void launch_jt(bool tap, dim3 grid, int lds, hipStream_t s, const UlIrArgs& a) {
    if (tap) hipLaunchKernelGGL((ul_ir_kernel<JT, true>), grid, dim3(kIrThreads), lds, s, a);
    else hipLaunchKernelGGL((ul_ir_kernel<JT, false>), grid, dim3(kIrThreads), lds, s, a);
}

bool jt_built(int jt) { return jt == 1 || jt == 2 || jt == 3 || jt == 4 || jt == 8 || jt == 16; }

}  // namespace

int ul_ir_plan(const UlIrIO& io, bool tap, UlIrPlan* p, std::string* err) {
    auto bad = [&](const char* m) { if (err) *err = m; return -1; };
    memset(p, 0, sizeof(*p));
    if (io.N <= 0 || io.H <= 0 || io.W <= 0 || io.Cin <= 0 || io.mid <= 0 || io.Cout <= 0) return bad("ul_ir: bad arguments");
    if (io.N > kPackMaxFrames) return bad("ul_ir: at most 256 images per launch");
    if (io.Cin % 16 || io.mid % 16 || io.Cout % 16) return bad("ul_ir: Cin, mid and Cout must be multiples of 16");
    if (io.stride != 1 && io.stride != 2) return bad("ul_ir: stride 1 or 2");
    if (io.has_res && (io.Cin != io.Cout || io.stride != 1)) return bad("ul_ir: a residual needs Cin == Cout and stride 1");
    if (((io.x_ld | io.x_coff | io.y_ld | io.y_coff) & 15) || io.x_coff < 0 || io.y_coff < 0 || io.x_coff + io.Cin > io.x_ld ||
        io.y_coff + io.Cout > io.y_ld)
        return bad("ul_ir: a view leaves its buffer (channel pitch and offset: multiples of 16, offset + channels <= pitch)");
    if (io.has_res && (((io.res_ld | io.res_coff) & 15) || io.res_coff < 0 || io.res_coff + io.Cout > io.res_ld))
        return bad("ul_ir: a view leaves its buffer (the residual's)");
    const int JT = io.Cout / 16;
    if (JT > kIrMaxJT) return bad("ul_ir: the accumulators of more than 256 output channels do not fit a block's registers");
    if (!jt_built(JT)) return bad("ul_ir: the accumulators are built for Cout of 16, 32, 48, 64, 128 and 256");
    const int S = io.stride;
    p->Ho = (io.H - 1) / S + 1; p->Wo = (io.W - 1) / S + 1;
    const double big = 2147483647.0;
    if ((double)io.N * std::max(std::max(io.x_ld, io.mid) * (double)io.H * io.W, std::max(std::max(io.y_ld, io.res_ld), io.mid) * (double)p->Ho * p->Wo) >= big)
        return bad("ul_ir: tensor too large");
    p->TH = kIrTH; p->TW = kIrTW; p->MC = kIrMC;
    p->chunks = (io.mid + kIrMC - 1) / kIrMC;
    p->hid_h = S * (kIrTH - 1) + 3; p->hid_w = S * (kIrTW - 1) + 3;
    p->hidden_px = p->hid_h * p->hid_w;
    const int NT = (p->hidden_px + 15) / 16;
    p->lds_bytes = kIrParamFloats * (int)sizeof(float) + kIrCB * kIrPx * 16 * (int)sizeof(f16) + kIrCB * NT * 16 * 16 * (int)sizeof(f16);
    p->lds_limit = kIrLdsLimit;
    if (p->lds_bytes > p->lds_limit) return bad("ul_ir: the halo tile does not fit the LDS");
    p->grid_x = (p->Wo + kIrTW - 1) / kIrTW; p->grid_y = (p->Ho + kIrTH - 1) / kIrTH; p->grid_z = io.N;
    if (p->grid_y > 65535) return bad("ul_ir: map too tall");
    p->blocks = p->grid_x * p->grid_y * p->grid_z;
    p->threads = kIrThreads;
    p->JT = JT;
    snprintf(p->kernel, sizeof(p->kernel), "ul_ir_kernel<%d,%s>", JT, tap ? "true" : "false");
    return 0;
}

size_t ul_ir_pack(const float* w1, const float* wd, const float* w2, int Cin, int mid, int Cout, const float* s1, const float* b1,
                  const float* sd, const float* bd, const float* s2, const float* b2, uint8_t* out, size_t off[4]) {
    const int chunks = (mid + kIrMC - 1) / kIrMC, KS1 = (Cin + 31) / 32, KS2 = chunks * (kIrMC / 32), MT = chunks * kIrCB, JT = Cout / 16;
    const size_t n_w1 = (size_t)MT * KS1 * 512, n_w2 = (size_t)JT * KS2 * 512, n_par = (size_t)chunks * kIrParamFloats;
    size_t o[4];
    o[0] = 0;
    o[1] = o[0] + n_w1 * sizeof(f16);
    o[2] = o[1] + n_w2 * sizeof(f16);              // (both counts are multiples of 512 halfs: 16-byte alignment holds)
    o[3] = o[2] + n_par * sizeof(float);
    const size_t bytes = o[3] + (size_t)2 * Cout * sizeof(float);
    if (off) memcpy(off, o, sizeof(o));
    if (!out) return bytes;
    f16* p1 = reinterpret_cast<f16*>(out + o[0]);
    f16* p2 = reinterpret_cast<f16*>(out + o[1]);
    float* pp = reinterpret_cast<float*>(out + o[2]);
    float* ps = reinterpret_cast<float*>(out + o[3]);
    for (int mt = 0; mt < MT; ++mt)
        for (int ks = 0; ks < KS1; ++ks)
            for (int l = 0; l < 64; ++l)
                for (int e = 0; e < 8; ++e) {
                    const int m = mt * 16 + (l & 15), ci = ks * 32 + (l >> 4) * 8 + e;
                    p1[(((size_t)mt * KS1 + ks) * 64 + l) * 8 + e] = m < mid && ci < Cin ? (f16)w1[(size_t)m * Cin + ci] : (f16)0.f;
                }
    for (int jt = 0; jt < JT; ++jt)
        for (int ks = 0; ks < KS2; ++ks)
            for (int l = 0; l < 64; ++l)
                for (int e = 0; e < 8; ++e) {
                    const int co = jt * 16 + (l & 15), m = ks * 32 + (l >> 4) * 8 + e;
                    p2[(((size_t)jt * KS2 + ks) * 64 + l) * 8 + e] = m < mid ? (f16)w2[(size_t)co * mid + m] : (f16)0.f;
                }
    for (int ch = 0; ch < chunks; ++ch) {
        float* r = pp + (size_t)ch * kIrParamFloats;
        for (int i = 0; i < kIrMC; ++i) {
            const int m = ch * kIrMC + i;
            const bool live = m < mid;
            r[kPS1 + i] = live ? (s1 ? s1[m] : 1.f) : 0.f;
            r[kPB1 + i] = live && b1 ? b1[m] : 0.f;
            r[kPSD + i] = live ? (sd ? sd[m] : 1.f) : 0.f;
            r[kPBD + i] = live && bd ? bd[m] : 0.f;
            for (int tap = 0; tap < 9; ++tap) r[kPDW + ((i >> 4) * 9 + tap) * 16 + (i & 15)] = live ? wd[(size_t)m * 9 + tap] : 0.f;
        }
    }
    for (int c = 0; c < Cout; ++c) {
        ps[c] = s2 ? s2[c] : 1.f;
        ps[Cout + c] = b2 ? b2[c] : 0.f;
    }
    return bytes;
}

int launch_ul_ir(const UlIrW& w, const UlIrIO& io, hipStream_t s, UlIrPlan* plan, std::string* err) {
    UlIrPlan pl;
    const bool tap = io.e1 || io.e2;
    if (ul_ir_plan(io, tap, &pl, err)) return -1;
    if (!io.x || !io.y || !w.w1 || !w.w2 || !w.par || !w.ss2 || (tap && (!io.e1 || !io.e2)) || (io.has_res != 0) != (io.res != nullptr)) {
        if (err) *err = "ul_ir: bad arguments";
        return -1;
    }
    UlIrArgs a;
    a.w = w;
    a.x = io.x; a.x_cbt = io.x_ld >> 4; a.x_cb0 = io.x_coff >> 4;
    a.y = io.y; a.y_cbt = io.y_ld >> 4; a.y_cb0 = io.y_coff >> 4;
    a.res = io.res; a.res_cbt = io.res_ld >> 4; a.res_cb0 = io.res_coff >> 4;
    a.e1 = io.e1; a.e2 = io.e2;
    a.H = io.H; a.W = io.W; a.Ho = pl.Ho; a.Wo = pl.Wo; a.S = io.stride;
    a.CB = io.Cin / 16; a.KS1 = (io.Cin + 31) / 32; a.MB = io.mid / 16; a.chunks = pl.chunks;
    a.hid_w = pl.hid_w; a.hid_px = pl.hidden_px; a.NT = (pl.hidden_px + 15) / 16;
    const dim3 grid((unsigned)pl.grid_x, (unsigned)pl.grid_y, (unsigned)pl.grid_z);
    switch (pl.JT) {
    case 1: launch_jt<1>(tap, grid, pl.lds_bytes, s, a); break;
    case 2: launch_jt<2>(tap, grid, pl.lds_bytes, s, a); break;
    case 3: launch_jt<3>(tap, grid, pl.lds_bytes, s, a); break;
    case 4: launch_jt<4>(tap, grid, pl.lds_bytes, s, a); break;
    case 8: launch_jt<8>(tap, grid, pl.lds_bytes, s, a); break;
    case 16: launch_jt<16>(tap, grid, pl.lds_bytes, s, a); break;
    default: if (err) *err = "ul_ir: no instantiation"; return -1;
    }
    if (hipGetLastError() != hipSuccess) { if (err) *err = "ul_ir: launch failed"; return -2; }
    if (plan) *plan = pl;
    return 0;
}

}  // namespace ltk

// ul_gconv: the dense convs of the Ultralight program (avatars/ultralight/unet.py: the 1x1 expand / project convs of every
// InvertedResidual, the two biased 3x3 stride-2 audio convs) with weights, scale and shift chosen PER IMAGE (ul_gconv.h), so that
// frames of different avatars share one launch.  Same operand scheme as rowgemm.hip: v_mfma_f32_16x16x32_f16, both operands as
// 16-byte loads straight from global memory (weights as A: lane l holds output channel l & 15, channels (l >> 4) * 8 .. + 8 of the
// k-step; pixels as B), no LDS.  It differs in one way: a pixel's K is strided by channel block (block cb of the [N][C/16][H][W][16]
// map lies at cb * H * W * 16), so a k-step of 32 channels is two channel blocks - lane group g reads block 2 * step + (g >> 1),
// half g & 1 - and Cin % 32 == 16 leaves the upper two lane groups of a tap's last step with zeros (the packed weights have zeros
// there too, and the map is never read past its last block).
//
// A block is four waves over ONE image's tile of 32 output pixels: wave w owns output channels [16 (4 by + w), + 16) and all of K,
// so no partial sums cross waves (no LDS, no atomics, one summation order whatever the launch shape).  The four waves read the same
// pixels, which the second to fourth find in L1 / L2.  The image's record pointer comes from the per-frame table through blockIdx.z
// and is wave-uniform: the record's operand pointers are scalar loads.
#include "ul_gconv.h"

#include <hip/hip_fp16.h>

#include <algorithm>
#include <type_traits>

namespace ltk {

typedef f16 f16x8 __attribute__((ext_vector_type(8)));
typedef f16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kGcFT = 2;          // 16-pixel tiles per block
constexpr int kGcWaves = 4;       // 16-channel output tiles per block
constexpr int kGcU = 4;           // k-steps in flight per trip

struct UlGconvArgs {
    const UlGroupTab* tab; int op;
    const f16* x; int x_cbt, x_cb0;       // input  [N][x_cbt][H*W][16], this tensor's first channel block
    f16* y; int y_cbt, y_cb0;             // output [N][y_cbt][Ho*Wo][16]
    const f16* res; int res_cbt, res_cb0; // residual (y's geometry) or nullptr
    int H, W, Ho, Wo, S, pad, KW;
    int CB;                               // input channel blocks (Cin / 16)
    int KS;                               // k-steps per tap: ceil(CB / 2)
    int KT;                               // k-steps: taps * KS
    int JT;                               // output channel tiles (Cout / 16)
    int relu;
};

__global__ __launch_bounds__(64 * kGcWaves) void ul_gconv_kernel(const UlGconvArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int jt = blockIdx.y * kGcWaves + wave;
    if (jt >= a.JT) return;                                    // (no barrier below: a wave without a tile leaves)
    const int n = blockIdx.z;
    // wave-uniform: the table entry, and through it this op's operands, are scalar loads
    const UlGroupW* const rec = a.tab->w[n];
    const UlGroupOp gop = rec->op[a.op];
    const int i16 = lane & 15, g = lane >> 4;
    const int HWi = a.H * a.W, HWo = a.Ho * a.Wo;
    const f16x8* wp = reinterpret_cast<const f16x8*>(gop.w) + (size_t)jt * a.KT * 64 + lane;
    // this lane's pixel of each 16-pixel tile: top-left input pixel of its window
    int iy0[kGcFT], ix0[kGcFT];
    bool live[kGcFT];
#pragma unroll
    for (int ft = 0; ft < kGcFT; ++ft) {
        const int p = (blockIdx.x * kGcFT + ft) * 16 + i16;
        live[ft] = p < HWo;
        const int pp = live[ft] ? p : 0;
        const int oy = pp / a.Wo, ox = pp - oy * a.Wo;
        iy0[ft] = oy * a.S - a.pad; ix0[ft] = ox * a.S - a.pad;
    }
    // channel block (g >> 1) and half (g & 1) of a k-step's 32 channels belong to this lane
    const f16* const xn = a.x + (((size_t)n * a.x_cbt + a.x_cb0) * HWi) * 16 + (g & 1) * 8;
    f32x4 acc[kGcFT];
#pragma unroll
    for (int ft = 0; ft < kGcFT; ++ft) acc[ft] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const f16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    // operand of k-step k for pixel tile ft: tap = k / KS (wave-uniform), channel block 2 * (k % KS) + (g >> 1); zeros outside the
    // map, behind the last pixel and behind the last channel block (the K tail of Cin % 32 == 16)
    auto xload = [&](int k, int ft) -> f16x8 {
        const int tap = k / a.KS, cc = k - tap * a.KS;
        const int ky = tap / a.KW, kx = tap - ky * a.KW;
        const int iy = iy0[ft] + ky, ix = ix0[ft] + kx;
        const int cb = cc * 2 + (g >> 1);
        const bool ok = live[ft] && cb < a.CB && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
        return ok ? *reinterpret_cast<const f16x8*>(xn + ((size_t)cb * HWi + iy * a.W + ix) * 16) : zero;
    };
    // one trip = U k-steps: all of its loads are issued, then its MFMAs
    auto trip = [&](int kt, auto u_tag) {
        constexpr int U = decltype(u_tag)::value;
        f16x8 wa[U], xb[U][kGcFT];
#pragma unroll
        for (int u = 0; u < U; ++u) wa[u] = wp[(size_t)(kt + u) * 64];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int ft = 0; ft < kGcFT; ++ft) xb[u][ft] = xload(kt + u, ft);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int ft = 0; ft < kGcFT; ++ft) acc[ft] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[u], xb[u][ft], acc[ft], 0, 0, 0);
    };
    int kt = 0;
    for (; kt + kGcU <= a.KT; kt += kGcU) trip(kt, std::integral_constant<int, kGcU>{});
    for (; kt < a.KT; ++kt) trip(kt, std::integral_constant<int, 1>{});

    // D layout of the 16x16 MFMA: lane holds output channels 4g .. 4g+3 of pixel i16
    const int j0 = jt * 16 + 4 * g;
    const f32x4 sc = *reinterpret_cast<const f32x4*>(gop.scale + j0), sf = *reinterpret_cast<const f32x4*>(gop.shift + j0);
#pragma unroll
    for (int ft = 0; ft < kGcFT; ++ft) {
        const int p = (blockIdx.x * kGcFT + ft) * 16 + i16;
        if (p >= HWo) continue;                                // pixel tail: nothing stored
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = acc[ft][q] * sc[q] + sf[q];
        if (a.res) {                                           // behind the affine, in front of the ReLU
            const f16x4 rv = *reinterpret_cast<const f16x4*>(a.res + (((size_t)n * a.res_cbt + a.res_cb0 + jt) * HWo + p) * 16 + 4 * g);
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] += (float)rv[q];
        }
        f16x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            o[q] = (f16)(a.relu ? __builtin_amdgcn_fmed3f(v[q], 0.f, 65504.f) : __builtin_amdgcn_fmed3f(v[q], -65504.f, 65504.f));
        *reinterpret_cast<f16x4*>(a.y + (((size_t)n * a.y_cbt + a.y_cb0 + jt) * HWo + p) * 16 + 4 * g) = o;
    }
}

constexpr int kGtabChunk = 256;
struct GtabChunk {
    const UlGroupW* p[kGtabChunk];        // 2 KB of the 4 KB of kernel arguments HIP guarantees
};
static_assert(kGtabChunk >= kPackMaxFrames, "one launch uploads the whole table");
__global__ __launch_bounds__(kGtabChunk) void upload_group_table_kernel(const GtabChunk c, int n, UlGroupTab* __restrict__ t) {
    const int i = threadIdx.x;
    if (i < n) t->w[i] = c.p[i];
}

void launch_upload_group_table(const UlGroupTab* host, int nframes, UlGroupTab* d_tab, hipStream_t s) {
    GtabChunk c;
    const int n = std::min(nframes, kGtabChunk);
    for (int i = 0; i < kGtabChunk; ++i) c.p[i] = i < n ? host->w[i] : nullptr;
    hipLaunchKernelGGL(upload_group_table_kernel, dim3(1), dim3(kGtabChunk), 0, s, c, n, d_tab);
}

size_t ul_gconv_pack(const float* weight, int Cin, int Cout, int k, f16* out) {
    const int taps = k * k, KS = (Cin + 31) / 32, JT = Cout / 16;
    const size_t halfs = (size_t)JT * taps * KS * 64 * 8;
    if (!out) return halfs;
    for (int jt = 0; jt < JT; ++jt)
        for (int t = 0; t < taps; ++t)
            for (int ks = 0; ks < KS; ++ks)
                for (int l = 0; l < 64; ++l)
                    for (int e = 0; e < 8; ++e) {
                        const int co = jt * 16 + (l & 15), ci = ks * 32 + (l >> 4) * 8 + e;
                        out[((((size_t)jt * taps + t) * KS + ks) * 64 + l) * 8 + e] = ci < Cin ? (f16)weight[((size_t)co * Cin + ci) * taps + t] : (f16)0.f;
                    }
    return halfs;
}

const char* ul_gconv_kernel_name() { return "ul_gconv_kernel"; }

int ul_gconv_geom(const UlGconvIO& io, UlGconvGeom* g, std::string* err) {
    auto bad = [&](const char* m) { if (err) *err = m; return -1; };
    if (io.N <= 0 || io.H <= 0 || io.W <= 0 || io.Cin <= 0 || io.Cout <= 0) return bad("ul_gconv: bad arguments");
    if (io.N > kPackMaxFrames) return bad("ul_gconv: at most 256 images per launch (the per-frame table)");
    if (io.Cin % 16 || io.Cout % 16) return bad("ul_gconv: Cin % 16 == 0 and Cout % 16 == 0");
    const bool k1 = io.k == 1 && io.stride == 1 && io.pad == 0;
    const bool k3 = io.k == 3 && io.stride == 2 && (io.pad == 1 || io.pad == 3);
    if (!k1 && !k3) return bad("ul_gconv: 1x1 stride 1 pad 0, or 3x3 stride 2 pad 1 / 3");
    if (((io.x_ld | io.x_coff | io.y_ld | io.y_coff | io.res_ld | io.res_coff) & 15) || io.x_coff < 0 || io.y_coff < 0 || io.res_coff < 0)
        return bad("ul_gconv: channel pitch / offset must be multiples of 16");
    if (io.x_coff + io.Cin > io.x_ld || io.y_coff + io.Cout > io.y_ld || (io.res && io.res_coff + io.Cout > io.res_ld))
        return bad("ul_gconv: channel range outside the buffer's pitch");
    const int Ho = (io.H + 2 * io.pad - io.k) / io.stride + 1, Wo = (io.W + 2 * io.pad - io.k) / io.stride + 1;
    if (io.H + 2 * io.pad < io.k || io.W + 2 * io.pad < io.k || Ho <= 0 || Wo <= 0) return bad("ul_gconv: empty output map");
    if ((double)io.N * std::max(io.x_ld * (double)io.H * io.W, std::max(io.y_ld, io.res_ld) * (double)Ho * Wo) >= 2147483647.0)
        return bad("ul_gconv: tensor too large");
    g->Ho = Ho; g->Wo = Wo;
    g->tile_px = 16 * kGcFT; g->tile_co = 16 * kGcWaves; g->threads = 64 * kGcWaves;
    g->grid_x = (Ho * Wo + g->tile_px - 1) / g->tile_px;
    g->grid_y = (io.Cout / 16 + kGcWaves - 1) / kGcWaves;
    g->grid_z = io.N;
    g->blocks = g->grid_x * g->grid_y * g->grid_z;
    g->ksteps = io.k * io.k * ((io.Cin + 31) / 32);
    if (g->grid_y > 65535) return bad("ul_gconv: too many output channels");
    return 0;
}

int launch_ul_gconv(const UlGroupTab* d_tab, int op, const UlGconvIO& io, hipStream_t s, std::string* err) {
    UlGconvGeom g;
    if (!d_tab || op < 0 || op >= kUlMaxOps || !io.x || !io.y) { if (err) *err = "ul_gconv: bad arguments"; return -1; }
    if (ul_gconv_geom(io, &g, err)) return -1;
    UlGconvArgs a;
    a.tab = d_tab; a.op = op;
    a.x = io.x; a.x_cbt = io.x_ld >> 4; a.x_cb0 = io.x_coff >> 4;
    a.y = io.y; a.y_cbt = io.y_ld >> 4; a.y_cb0 = io.y_coff >> 4;
    a.res = io.res; a.res_cbt = io.res_ld >> 4; a.res_cb0 = io.res_coff >> 4;
    a.H = io.H; a.W = io.W; a.Ho = g.Ho; a.Wo = g.Wo; a.S = io.stride; a.pad = io.pad; a.KW = io.k;
    a.CB = io.Cin / 16; a.KS = (io.Cin + 31) / 32; a.KT = g.ksteps; a.JT = io.Cout / 16; a.relu = io.relu;
    hipLaunchKernelGGL(ul_gconv_kernel, dim3((unsigned)g.grid_x, (unsigned)g.grid_y, (unsigned)g.grid_z), dim3(64 * kGcWaves), 0, s, a);
    if (hipGetLastError() != hipSuccess) { if (err) *err = "ul_gconv: launch failed"; return -2; }
    return 0;
}

}  // namespace ltk

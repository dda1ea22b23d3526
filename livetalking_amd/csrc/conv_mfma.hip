// Implicit-GEMM fp16 convolution for gfx950 (CDNA4) on MFMA, first generation (register-staged); activations are
// channel-blocked CB16 ([N][C/16][H][W][16]), inputs of <= 8 channels [N][H][W][8].  Today it runs the 7x7, the
// shallow strided 3x3 and the valid-padding layers; conv3_mfma.hip runs the rest.  This file holds the kernel, its picker and its
// launcher (conv1_launch = conv1_plan_launch, pure, + the enqueue; what conv_launch calls for a plan that is not conv3's); plans are
// built in conv_plan.hip.
//
// Replaces the torch.nn.Conv2d / ConvTranspose2d + BatchNorm2d(eval) + residual
// + ReLU blocks of the reference generator (avatars/wav2lip/models/conv.py:5-44,
// instantiated at avatars/wav2lip/models/wav2lip_v2.py:12-91).
//
// Mapping (one workgroup = 4 waves = 256 output pixels x BN output channels):
//   * the input patch a tile needs ((TH-1)*s+k rows x (TW-1)*s+k cols, zero padded
//     at the image border) is staged ONCE per 16/32-channel chunk into LDS as
//     channel planes [c8][patch pixel][8 halfs]; all k*k taps then read their
//     operand from that patch at a shifted address, so a 3x3 layer reads its
//     input once from HBM/L2 instead of nine times;
//   * weights are pre-packed on the host in LDS image order
//     [cout tile][chunk][tap][c8][cout][8 halfs], so a chunk's slab is one
//     contiguous, fully coalesced copy;
//   * v_mfma_f32_32x32x16_f16 with the WEIGHTS as the row operand and the PIXELS
//     as the column operand: a lane's 16 accumulators then are 4 groups of 4
//     consecutive output channels of ONE pixel -> 8-byte stores into the pixel's channel block, and the
//     folded BN scale/shift, residual add and ReLU are applied in registers;
//   * channel-offset reads/writes (x_ld/x_coff, y_ld/y_coff) make the decoder's
//     torch.cat skip connections (wav2lip_v2.py:146) free;
//   * ConvTranspose2d(k3,s2,p1,op1) runs as its 4 sub-pixel phases (1/2/2/4
//     taps over a 2x2 input neighbourhood) in one launch: no zero-insertion.
//
// LDS (dynamic, one array - keeps hipcc from draining vmcnt per k-step):
//   [2 x A planes][2 x B slab][tap table]
#include "conv_host.h"
#include "tune.h"

#include <hip/hip_fp16.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

namespace ltk {

typedef f16 f16x8 __attribute__((ext_vector_type(8)));
typedef f16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct KArgs {
    const f16* x; const f16* w; const float* scale; const float* shift; const f16* res; f16* y;
    const PhaseMeta* phases;
    int N, H, W, x_cbt, x_cb0;        // channel-blocked [N][C/16][H][W][16]: blocks in the buffer, first block
    int Ho, Wo, y_cbt, y_cb0, HoA, WoA, osy, osx;
    int res_cbt, res_cb0;
    int Cin8, Cout;
    int sh, sw, pad_y, pad_x;
    int PH, PW, NPIXP;
    int log2TW, log2TH, NB;
    int tiles_x, tiles_y, tiles_n, n_ntiles;
    unsigned magicPW, magicPHW;
    int nchunks, Tp, relu;
    int lds_bytes;
    int s2half;                       // > 0: column-parity split of the patch rows (stride-2 3x3 layers): patch column px sits at slot
                                      // (px >> 1) + (px & 1) * s2half of its row, so the 16 lanes of a ds_read_b128 group - 16 consecutive
                                      // output pixels, i.e. every OTHER patch pixel - read 256 contiguous bytes instead of two 16-byte
                                      // items per 32 (a 2-way bank conflict on every A read: 30.7 % of this kernel's LDS cycles in round 5)
};

// A-patch staging registers per thread (16-byte items): the largest variant a configuration has.
constexpr int max_a_items(int NC8) { return NC8 == 4 ? 6 : (NC8 == 1 ? 5 : 10); }
constexpr int kTapTableBytes = 128;
constexpr int kLdsLimit = 160 * 1024;

// Single-buffered LDS + register prefetch: two barriers per chunk, several workgroups per CU overlap each other's
// load / epilogue phases.  (The double-buffered variant, one workgroup per CU, was last in commit fb7f771.)
template <int NC8, int NBT, bool TT9, int MAXA>
__global__ __launch_bounds__(256) void conv_mfma_kernel(const KArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int BN = NBT * 32;
    constexpr int MAXB = kMaxBItems;
    constexpr int LOG2NC8 = NC8 == 4 ? 2 : (NC8 == 2 ? 1 : 0);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int l31 = lane & 31;
    const int hh = lane >> 5;

    // ---- block -> (phase, image tile, y tile, x tile, cout tile); consecutive
    // logical ids (same pixel tile, different cout tiles) share an XCD's L2.
    int bid = blockIdx.x;
    {
        const int nblk = gridDim.x;
        const int q = nblk >> 3, r = nblk & 7;
        const int xcd = bid & 7, slot = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
    }
    const int ntile = bid % a.n_ntiles;
    int t0 = bid / a.n_ntiles;
    const int tx_t = t0 % a.tiles_x; t0 /= a.tiles_x;
    const int ty_t = t0 % a.tiles_y; t0 /= a.tiles_y;
    const int tn_t = t0 % a.tiles_n;
    const int phase = t0 / a.tiles_n;

    const PhaseMeta* __restrict__ pm = a.phases + phase;
    const int T = pm->T;
    const int ooy = pm->ooy, oox = pm->oox;

    const int A_BYTES = NC8 * a.NPIXP * 16;
    unsigned char* const smemA = smem;
    unsigned char* const smemB = smem + A_BYTES;
    // the tap table sits at the very end of the allocation (the epilogue reuses the front)
    short* const tapl = reinterpret_cast<short*>(smem + a.lds_bytes - kTapTableBytes);

    if (tid < kMaxTaps) {
        short v = 0;
        if (tid < T) v = (short)(pm->dy[tid] * a.PW + pm->dx[tid]);
        tapl[tid] = v;
    }

    const int TWm = (1 << a.log2TW) - 1, THm = (1 << a.log2TH) - 1;
    const int tx0 = tx_t << a.log2TW, ty0 = ty_t << a.log2TH, n0 = tn_t * a.NB;
    const int iy0 = ty0 * a.sh - a.pad_y, ix0 = tx0 * a.sw - a.pad_x;
    const int PHW = a.PH * a.PW;
    const int nitemsA = a.NB * PHW * NC8;

    // ---- A staging descriptors (chunk independent)
    int a_goff[MAXA];
    int a_slot[MAXA];                 // LDS pixel slot of the item (the identity unless s2half)
#pragma unroll
    for (int k = 0; k < MAXA; ++k) {
        const int i = tid + k * 256;
        const int pix = i >> LOG2NC8;
        const int c8 = i & (NC8 - 1);
        // exact for pix < 2^16; a divisor of 1 has no 32-bit magic
        const int b = (PHW == 1) ? pix : (int)__umulhi((unsigned)pix, a.magicPHW);
        const int rem = pix - b * PHW;
        const int py = (a.PW == 1) ? rem : (int)__umulhi((unsigned)rem, a.magicPW);
        const int px = rem - py * a.PW;
        const int n = n0 + b, iy = iy0 + py, ix = ix0 + px;
        a_slot[k] = a.s2half ? b * PHW + py * a.PW + (px >> 1) + (px & 1) * a.s2half : pix;
        const bool ok = (i < nitemsA) && (n < a.N) && ((unsigned)iy < (unsigned)a.H) && ((unsigned)ix < (unsigned)a.W);
        if constexpr (NC8 == 1)   // the two network inputs (packed face crops, mel windows) are plain [N][H][W][8]
            a_goff[k] = ok ? (((n * a.H + iy) * a.W + ix) * 8) : -1;
        else
            a_goff[k] = ok ? ((((n * a.x_cbt + a.x_cb0 + (c8 >> 1)) * a.H + iy) * a.W + ix) * 16 + (c8 & 1) * 8) : -1;
    }

    // weights are packed per 32-cout sub-slab: [cout/32][chunk][tap][plane][32][8 halfs]; a block
    // with BN = NBT*32 stages NBT sub-slabs -> LDS image [sub][tap][plane][32][16 B]
    const int slab32 = a.Tp * NC8 * 32;   // 16-byte items per (sub-slab, chunk)
    const int slab = slab32 * NBT;
    const uint4* __restrict__ wsrc = reinterpret_cast<const uint4*>(a.w) + pm->w_off16 + (size_t)(ntile * NBT) * a.nchunks * slab32;

    uint4 ra[MAXA];
    uint4 rb[MAXB];

    const int HW16 = a.H * a.W * 16;
    auto load_chunk = [&](int c) {
        const int cbase = c * NC8;
        const size_t coff = (size_t)c * (NC8 / 2) * HW16;     // chunk = NC8/2 channel blocks
#pragma unroll
        for (int k = 0; k < MAXA; ++k) {
            const int c8 = (tid + k * 256) & (NC8 - 1);
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (a_goff[k] >= 0 && cbase + c8 < a.Cin8)
                v = *reinterpret_cast<const uint4*>(a.x + a_goff[k] + coff);
            ra[k] = v;
        }
        const uint4* ws = wsrc + (size_t)c * slab32;
#pragma unroll
        for (int k = 0; k < MAXB; ++k) {
            const int i = tid + k * 256;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (i < slab) {
                int sub = 0;
                if constexpr (NBT > 1) sub = (i >= slab32) + (NBT > 2 ? ((i >= 2 * slab32) + (i >= 3 * slab32)) : 0);
                v = ws[(size_t)sub * a.nchunks * slab32 + (i - sub * slab32)];
            }
            rb[k] = v;
        }
    };
    auto store_chunk = [&]() {
        unsigned char* Ab = smemA;
        unsigned char* Bb = smemB;
#pragma unroll
        for (int k = 0; k < MAXA; ++k) {
            const int i = tid + k * 256;
            if (i < nitemsA) {
                const int c8 = i & (NC8 - 1);
                *reinterpret_cast<uint4*>(Ab + (c8 * a.NPIXP + a_slot[k]) * 16) = ra[k];
            }
        }
#pragma unroll
        for (int k = 0; k < MAXB; ++k) {
            const int i = tid + k * 256;
            if (i < slab) *reinterpret_cast<uint4*>(Bb + i * 16) = rb[k];
        }
    };

    // ---- per-lane operand bases: this lane's output pixel in each 32-pixel subtile
    int pixb[2];
    int obase[2], rbase[2];  // element offset of (output pixel, first channel block of this cout tile) in y / res, -1 = none
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int m = wave * 64 + j * 32 + l31;
        const int tx = m & TWm;
        const int ty = (m >> a.log2TW) & THm;
        const int b = m >> (a.log2TW + a.log2TH);
        const bool inb = b < a.NB;
        pixb[j] = inb ? ((b * a.PH + ty * a.sh) * a.PW + (a.s2half ? tx : tx * a.sw)) * 16 : 0;      // s2half: column 2 tx sits at slot tx
        const int n = n0 + b, oy = ty0 + ty, ox = tx0 + tx;
        const bool rowok = inb && n < a.N && oy < a.Ho && ox < a.Wo;
        const int opx = (oy * a.osy + ooy) * a.WoA + ox * a.osx + oox;
        const int cbo = (ntile * BN) >> 4;
        obase[j] = rowok ? (((n * a.y_cbt + a.y_cb0 + cbo) * (a.HoA * a.WoA) + opx) * 16) : -1;
        rbase[j] = rowok ? (((n * a.res_cbt + a.res_cb0 + cbo) * (a.HoA * a.WoA) + opx) * 16) : -1;
    }

    f32x16 acc[NBT][2];
#pragma unroll
    for (int i = 0; i < NBT; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int PS = a.NPIXP * 16;
    const int nchunks = a.nchunks;
    auto compute_chunk = [&](int c) {
        const unsigned char* Ab = smemA;
        const unsigned char* Bb = smemB;
        if constexpr (NC8 == 1) {
            // 8-channel input: one MFMA k16 step = two taps (lanes 0-31 tap 2s, lanes 32-63 tap 2s+1)
            const int nsteps = a.Tp >> 1;
            for (int s = 0; s < nsteps; ++s) {
                const int tp = 2 * s + hh;
                const int toff = (int)tapl[tp] * 16;
                f16x8 xa[2], wf[NBT];
#pragma unroll
                for (int j = 0; j < 2; ++j) xa[j] = *reinterpret_cast<const f16x8*>(Ab + pixb[j] + toff);
#pragma unroll
                for (int i = 0; i < NBT; ++i) wf[i] = *reinterpret_cast<const f16x8*>(Bb + (((i * a.Tp + tp) * 32) + l31) * 16);
#pragma unroll
                for (int i = 0; i < NBT; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[i], xa[j], acc[i][j], 0, 0, 0);
            }
        } else {
            const int planes = min(NC8, a.Cin8 - c * NC8);
            auto tap_body = [&](int t, int toff) {
#pragma unroll
                for (int q = 0; q < NC8 / 2; ++q) {
                    if (2 * q < planes) {
                        const int plane = 2 * q + hh;
                        f16x8 xa[2], wf[NBT];
#pragma unroll
                        for (int j = 0; j < 2; ++j) xa[j] = *reinterpret_cast<const f16x8*>(Ab + plane * PS + pixb[j] + toff);
#pragma unroll
                        for (int i = 0; i < NBT; ++i)
                            wf[i] = *reinterpret_cast<const f16x8*>(Bb + ((((i * a.Tp + t) * NC8 + plane) * 32) + l31) * 16);
#pragma unroll
                        for (int i = 0; i < NBT; ++i)
#pragma unroll
                            for (int j = 0; j < 2; ++j)
                                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[i], xa[j], acc[i][j], 0, 0, 0);
                    }
                }
            };
            if constexpr (TT9) {
                const int dxo1 = a.s2half ? a.s2half : 1, dxo2 = a.s2half ? 1 : 2;     // slot offset of patch column +1 / +2 (wave-uniform)
#pragma unroll
                for (int t = 0; t < 9; ++t) tap_body(t, ((t / 3) * a.PW + ((t % 3) == 0 ? 0 : (t % 3) == 1 ? dxo1 : dxo2)) * 16);
            } else {
                for (int t = 0; t < T; ++t) tap_body(t, (int)tapl[t] * 16);
            }
        }

    };

    load_chunk(0);
    for (int c = 0; c < nchunks; ++c) {
        if (c) __syncthreads();          // every wave is done reading chunk c-1
        store_chunk();
        __syncthreads();
        if (c + 1 < nchunks) load_chunk(c + 1);   // in flight under the MFMAs
        compute_chunk(c);
    }
    __syncthreads();

    // ---- epilogue: y = relu(acc*scale + shift + res) -> fp16, through a wave-private LDS
    // transpose so the residual is READ and the result WRITTEN as whole 16-byte channel
    // segments of a pixel row (8-byte scattered accesses from the MFMA C layout were
    // issue-bound).  The main loop ended with a barrier: the front of LDS is free.
    constexpr int ROWB = BN * 2 + 16;   // bytes per pixel row in the transpose region (+16: bank spread)
    constexpr int CBN = BN / 16;        // channel blocks per block (BN = 32: 2)
    unsigned char* const wreg = smem + wave * (64 * ROWB);
    const int cout0 = ntile * BN;
    const int ncb_valid = min(CBN, (a.Cout - cout0) >> 4);
    const bool has_res = a.res != nullptr;
    const int HWo16 = a.HoA * a.WoA * 16;

    if (has_res) {
#pragma unroll
        for (int it = 0; it < 2 * CBN; ++it) {
            const int idx = it * 64 + lane;
            const int cbl = idx >> 7, px = (idx >> 1) & 63, half = idx & 1;
            const int r0 = __shfl(rbase[0], px & 31), r1 = __shfl(rbase[1], px & 31);
            const int rb = (px & 32) ? r1 : r0;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (rb >= 0 && cbl < ncb_valid) v = *reinterpret_cast<const uint4*>(a.res + rb + cbl * HWo16 + half * 8);
            *reinterpret_cast<uint4*>(wreg + px * ROWB + (cbl * 16 + half * 8) * 2) = v;
        }
    }
#pragma unroll
    for (int i = 0; i < NBT; ++i) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int cl = i * 32 + 8 * g + 4 * hh;     // channel within the block's BN
            const f32x4 sc = *reinterpret_cast<const f32x4*>(a.scale + cout0 + cl);   // padded to CoutPad
            const f32x4 sf = *reinterpret_cast<const f32x4*>(a.shift + cout0 + cl);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                unsigned char* p = wreg + (j * 32 + l31) * ROWB + cl * 2;
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = acc[i][j][4 * g + r] * sc[r] + sf[r];
                if (has_res) {
                    const f16x4 rr = *reinterpret_cast<const f16x4*>(p);
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] += (float)rr[r];
                }
                f16x4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float t = v[r];
                    if (a.relu == 1) t = fmaxf(t, 0.f);
                    else if (a.relu >= 2) {      // rare (Whisper convs): keep the transcendental code out of the common path
                        if (a.relu == 2) t = 0.5f * t * (1.f + erff(t * 0.70710678118654752f));
                        else t = t / (1.f + __expf(-t));
                    }
                    t = fminf(fmaxf(t, -65504.f), 65504.f);
                    o[r] = (f16)t;
                }
                *reinterpret_cast<f16x4*>(p) = o;
            }
        }
    }
#pragma unroll
    for (int it = 0; it < 2 * CBN; ++it) {
        const int idx = it * 64 + lane;
        const int cbl = idx >> 7, px = (idx >> 1) & 63, half = idx & 1;
        const int o0 = __shfl(obase[0], px & 31), o1 = __shfl(obase[1], px & 31);
        const int ob = (px & 32) ? o1 : o0;
        const uint4 v = *reinterpret_cast<const uint4*>(wreg + px * ROWB + (cbl * 16 + half * 8) * 2);
        if (ob >= 0 && cbl < ncb_valid) *reinterpret_cast<uint4*>(a.y + ob + cbl * HWo16 + half * 8) = v;
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------

typedef void (*conv_kernel_t)(const KArgs);

// THE table of instantiations, X(NC8, NBT, TT9, MAXA), per (NC8, NBT, TT9) in ascending MAXA: pick_kernel and conv1_variant_names()
// (what a test has to see launched, ltk_debug_conv1_variants) are both made of it.  A launch runs blocks of at most 64 output channels
// (NBT <= 2, conv1_plan_launch).
#define K1_VARIANTS(X) \
    X(1, 1, false, 5) \
    X(4, 1, true, 6) X(4, 1, false, 6) X(4, 2, true, 6) X(4, 2, false, 6) \
    X(2, 1, true, 3) X(2, 1, false, 3) X(2, 2, true, 3) X(2, 2, false, 3) \
    X(2, 1, true, 10) X(2, 1, false, 10) X(2, 2, true, 10) X(2, 2, false, 10)

// `need` = 16-byte A items per thread this launch stages; returns the smallest instantiation that holds them (*maxa = its MAXA).
static conv_kernel_t pick_kernel(int NC8, int NBT, bool tt9, int need, int* maxa = nullptr) {
#define K1CASE(nc8, nbt, t9, ma) \
    if (NC8 == nc8 && NBT == nbt && tt9 == t9 && need <= ma) { if (maxa) *maxa = ma; return (conv_kernel_t)conv_mfma_kernel<nc8, nbt, t9, ma>; }
    K1_VARIANTS(K1CASE)
#undef K1CASE
    return nullptr;
}

static std::string k1_name(int NC8, int NBT, bool tt9, int maxa) {
    char b[64];
    snprintf(b, sizeof(b), "conv_mfma_kernel<%d,%d,%s,%d>", NC8, NBT, tt9 ? "true" : "false", maxa);
    return b;
}

std::string conv1_variant_names() {
    std::string out;
#define K1NAME(nc8, nbt, t9, ma) out += k1_name(nc8, nbt, t9, ma) + "\n";
    K1_VARIANTS(K1NAME)
#undef K1NAME
    return out;
}

bool conv1_has_kernel(int NC8, int NBT, bool tt9) { return pick_kernel(NC8, NBT, tt9, 1) != nullptr; }

// What conv1_plan_launch decides: the instantiation, the grid, the dynamic LDS and KArgs with everything but the pointers
// (conv1_launch fills those from the plan and the ConvIO)
struct K1Launch {
    conv_kernel_t kernel;
    unsigned grid;
    size_t lds;
    KArgs a;
};

// FNV-1a over every KArgs field behind the pointers (which the planner leaves null): one number a test can hold a launch's arguments to
static unsigned kargs_hash(const KArgs& a) {
    const unsigned char* b = reinterpret_cast<const unsigned char*>(&a);
    unsigned h = 2166136261u;
    for (size_t i = offsetof(KArgs, N); i < sizeof(KArgs); ++i) h = (h ^ b[i]) * 16777619u;
    return h;
}

int conv1_plan_launch(const ConvPlan& p, const ConvIO& io, K1Launch* k1, std::string* err) {
    K1Launch local;
    K1Launch& L = k1 ? *k1 : local;
    if (io.ups) { if (err) *err = "input upsampling is a conv3 feature (3x3 s1 p1 / 1x1 layers)"; return -1; }
    KArgs& a = L.a;
    memset(&a, 0, sizeof(a));
    const int NC8 = p.NC8;
    int HoA, WoA;
    p.out_dims(io.H, io.W, &HoA, &WoA);
    a.N = io.N; a.H = io.H; a.W = io.W; a.x_cbt = io.x_ld >> 4; a.x_cb0 = io.x_coff >> 4;
    a.res_cbt = io.res_ld >> 4; a.res_cb0 = io.res_coff >> 4;
    a.Cin8 = p.Cin / 8;
    a.relu = io.relu ? 1 : io.act;
    int y_ld = io.y_ld;
    int kext_y, kext_x;
    if (p.gemm_1x1_expand) {
        if (io.H != 1 || io.W != 1) { if (err) *err = "k x k transposed conv only supported on 1x1 maps"; return -1; }
        if (io.y_ld != p.Cout || io.y_coff != 0) { if (err) *err = "1x1-expand output must be contiguous"; return -1; }
        a.Ho = 1; a.Wo = 1; a.HoA = 1; a.WoA = 1; a.osy = 1; a.osx = 1;
        y_ld = p.kh * p.kw * p.Cout;
        a.Cout = p.kh * p.kw * p.Cout;
        a.sh = a.sw = 1; a.pad_y = a.pad_x = 0; kext_y = kext_x = 1;
    } else if (p.transposed) {
        a.Ho = io.H; a.Wo = io.W; a.HoA = HoA; a.WoA = WoA; a.osy = 2; a.osx = 2;
        a.Cout = p.Cout; a.sh = a.sw = 1; a.pad_y = a.pad_x = 0; kext_y = kext_x = 2;
    } else {
        a.Ho = HoA; a.Wo = WoA; a.HoA = HoA; a.WoA = WoA; a.osy = 1; a.osx = 1;
        a.Cout = p.Cout; a.sh = p.sh; a.sw = p.sw; a.pad_y = p.ph; a.pad_x = p.pw; kext_y = p.kh; kext_x = p.kw;
    }
    a.y_cbt = y_ld >> 4; a.y_cb0 = io.y_coff >> 4;
    if (((NC8 == 1 ? 0 : (io.x_ld | io.x_coff)) | y_ld | io.y_coff | a.Cout) & 15 || (NC8 == 1 && (io.x_ld != 8 || io.x_coff != 0))) {
        if (err) *err = "channel counts/offsets must be multiples of 16 (channel-blocked layout)";
        return -1;
    }
    if (io.res && ((io.res_ld | io.res_coff) & 15)) { if (err) *err = "residual channel count/offset must be a multiple of 16"; return -1; }

    // tile: TW x TH output pixels x NB images, 256 rows
    int l2w = std::min(5, ceil_log2(a.Wo));
    int l2h = std::min(8 - l2w, ceil_log2(a.Ho));
    int NBT = std::min(p.NBT, 2);
    const int maxpix = max_a_items(NC8) * 256 / NC8;
    int PH, PW, NB;
    for (;;) {
        PH = ((1 << l2h) - 1) * a.sh + kext_y;
        PW = ((1 << l2w) - 1) * a.sw + kext_x;
        NB = std::min(kConvBM >> (l2w + l2h), maxpix / (PH * PW));
        if (NB >= 1) break;
        if (l2h > 0) --l2h; else if (l2w > 0) --l2w; else { if (err) *err = "patch does not fit"; return -1; }
    }
    NB = std::min(NB, std::max(1, io.N));
    a.log2TW = l2w; a.log2TH = l2h; a.NB = NB; a.PH = PH; a.PW = PW;
    const int npix = NB * PH * PW;
    int NPIXP = npix;
    const int want = NC8 == 4 ? 2 : (NC8 == 2 ? 4 : 0);
    if (NC8 > 1) while ((NPIXP & 7) != want) ++NPIXP;
    a.NPIXP = NPIXP;
    a.magicPW = magic_u16(PW);
    a.magicPHW = magic_u16(PH * PW);
    a.tiles_x = (a.Wo + (1 << l2w) - 1) >> l2w;
    a.tiles_y = (a.Ho + (1 << l2h) - 1) >> l2h;
    a.tiles_n = (io.N + NB - 1) / NB;
    // block width: the widest (<= 64 couts) that still gives the chip >= kMinBlocks workgroups
    constexpr int kMinBlocks = 512;
    const long long mtiles = (long long)p.nphase * a.tiles_n * a.tiles_y * a.tiles_x;
    while (NBT > 1 && mtiles * ((p.lCout + 32 * NBT - 1) / (32 * NBT)) < kMinBlocks) NBT /= 2;
    const int BN = NBT * 32;
    a.n_ntiles = (p.lCout + BN - 1) / BN;
    a.nchunks = (a.Cin8 + NC8 - 1) / NC8;
    a.Tp = p.Tp;

    const size_t a_bytes = (size_t)NC8 * NPIXP * 16, b_bytes = (size_t)p.Tp * NC8 * BN * 16;
    const size_t epi_bytes = (size_t)4 * 64 * (BN * 2 + 16);
    size_t lds = a_bytes + b_bytes + kTapTableBytes;
    lds = std::max(lds, epi_bytes + kTapTableBytes);
    lds = (lds + 255) / 256 * 256;
    if (lds > (size_t)kLdsLimit) { if (err) *err = "LDS budget exceeded"; return -1; }
    a.lds_bytes = (int)lds;
    // stride-2 3x3 layers whose tile rows hold >= 16 output pixels: column-parity split of the patch rows (KArgs::s2half)
    a.s2half = (p.tt9 && a.sw == 2 && l2w >= 4) ? (PW + 1) / 2 : 0;
    // largest 32-bit element offset the kernel forms
    if ((double)io.N * io.H * io.W * io.x_ld >= 2147483647.0) { if (err) *err = "input tensor too large for 32-bit offsets"; return -1; }

    const int need = (npix * NC8 + 255) / 256;
    int maxa = 0;
    conv_kernel_t k = pick_kernel(NC8, NBT, p.tt9, need, &maxa);
    if (!k) { if (err) *err = "no kernel instantiation for this launch"; return -1; }
    const long long nblk = (long long)p.nphase * a.tiles_n * a.tiles_y * a.tiles_x * a.n_ntiles;
    if (nblk <= 0 || nblk > 0x7fffffffll) { if (err) *err = "bad grid"; return -1; }
    L.kernel = k; L.grid = (unsigned)nblk; L.lds = lds;
    if (io.report) {
        ConvReport& r = *io.report;
        r = ConvReport();
        snprintf(r.kernel, sizeof(r.kernel), "%s", k1_name(NC8, NBT, p.tt9, maxa).c_str());
        r.NC8 = NC8; r.NBT = NBT; r.T = p.Tp; r.S = a.sw; r.items = (int)nblk; r.grid = (int)nblk;
        r.l2w = l2w; r.l2h = l2h; r.NB = NB; r.s2half = a.s2half; r.phases = p.nphase; r.lds = (int)lds;
        r.args_hash = (int)(kargs_hash(a) & 0x7fffffffu);
    }
    return 0;
}

int conv1_launch(const ConvPlan& p, const ConvIO& io, hipStream_t stream, std::string* err) {
    K1Launch L;
    if (const int rc = conv1_plan_launch(p, io, &L, err)) return rc;
    KArgs& a = L.a;
    a.x = io.x; a.w = p.d_w; a.scale = p.d_scale; a.shift = p.d_shift; a.res = io.res; a.y = io.y;
    a.phases = reinterpret_cast<const PhaseMeta*>((const char*)p.d_w + (p.w_bytes + 15) / 16 * 16);
    HIPCHK((hipError_t)ensure_dyn_lds((const void*)L.kernel, kLdsLimit));
    hipLaunchKernelGGL(L.kernel, dim3(L.grid), dim3(256), L.lds, stream, a);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // namespace ltk

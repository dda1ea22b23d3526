// Conv plans, host only: which kernel family serves a layer and in what configuration (conv_route), its weights packed in LDS image
// order and uploaded with the folded scale / shift (conv_plan_create, a driver over the steps below), and the dispatch of a launch to
// the first-generation kernel (conv_mfma.hip) or conv3 (conv3_mfma.hip).  No device code in this file.
#include "conv_host.h"
#include "tune.h"

#include <string.h>

#include <algorithm>
#include <cmath>
#include <thread>
#include <vector>

namespace ltk {

void ConvPlan::out_dims(int H, int W, int* Ho, int* Wo) const {
    if (!transposed) {   // out_pad on a plain conv = extra zero rows/columns at the bottom/right (diffusers Downsample2D
                         // with padding=0: F.pad(x, (0,1,0,1)) then a stride-2 "valid" conv)
        *Ho = (H + 2 * ph + out_pad - kh) / sh + 1;
        *Wo = (W + 2 * pw + out_pad - kw) / sw + 1;
    } else {
        *Ho = (H - 1) * sh - 2 * ph + kh + out_pad;
        *Wo = (W - 1) * sw - 2 * pw + kw + out_pad;
    }
}

double ConvPlan::macs_per_image(int H, int W) const {
    int Ho, Wo;
    out_dims(H, W, &Ho, &Wo);
    if (!transposed) return (double)Cout * kh * kw * Ho * Wo;  // x real Cin applied by caller
    return (double)Cout * kh * kw * H * W;
}

unsigned char f32_to_e4m3(float v) {
    // OCP e4m3fn: 1-4-3, bias 7, max 448 (0x7E), no infinities; subnormal step 2^-9
    unsigned char sign = 0;
    if (v < 0.f) { sign = 0x80; v = -v; }
    if (!(v == v)) return 0x7F;                      // NaN
    if (v >= 448.f) return sign | 0x7E;              // saturate (incl. the half-way case above 448)
    if (v < 0.0009765625f) return sign;              // < 2^-10: rounds to zero (2^-10 itself is a tie -> even = 0)
    int e;
    (void)std::frexp(v, &e);                         // v = m * 2^e, m in [0.5, 1)
    int E = e - 1;                                   // v = 1.x * 2^E
    if (E < -6) E = -6;                              // subnormal range shares the exponent of the smallest normal
    const float q = std::ldexp(v, 3 - E);            // in units of the spacing 2^(E-3)
    float r = std::nearbyint(q);                     // round half to even (default rounding mode)
    int mant = (int)r;                               // normals: 8..16, subnormals: 0..8
    int be = E + 7;
    if (E == -6 && mant < 8) return sign | (unsigned char)mant;             // subnormal (biased exponent 0)
    if (mant == 16) { mant = 8; ++be; }
    if (be > 15 || (be == 15 && mant - 8 > 6)) return sign | 0x7E;
    return sign | (unsigned char)((be << 3) | (mant - 8));
}

// step 1: the route

// Upsample2D = F.interpolate(scale_factor=2, nearest) + Conv2d(3x3, pad 1).  Output pixel (2y+py, 2x+px) reads upsampled rows
// 2y+py+ky-1, i.e. source rows y + floor((py+ky-1)/2): phase py=0 sees rows {y-1 <- ky 0, y <- ky 1,2}, phase py=1 rows
// {y <- ky 0,1, y+1 <- ky 2} (columns alike).  So every phase is a 2x2 conv on the SOURCE map whose weights are sums of the
// 3x3 taps: 16 (operand, phase) products per source pixel instead of 36.  Operands (dy,dx) in 0..2 address the 3x3 source
// neighbourhood (patch origin y-1, x-1); the kernel walks them row-major and feeds phases g = (py<<1)|px in ascending order.
struct Ups4Pair { int dy, dx, py, px; };
static std::vector<Ups4Pair> ups4_pairs() {
    std::vector<Ups4Pair> out;
    for (int dy = 0; dy < 3; ++dy)
        for (int dx = 0; dx < 3; ++dx)
            for (int py = 0; py < 2; ++py)
                for (int px = 0; px < 2; ++px) {
                    if (dy != py && dy != py + 1) continue;
                    if (dx != px && dx != px + 1) continue;
                    out.push_back({dy, dx, py, px});
                }
    return out;
}

ConvPlanKnobs conv_plan_knobs() { return {knob(K_CONV_V3) != 0, knob(K_CONV3_NC8)}; }

int conv_route(ConvPlan* p, ConvRoute* r, int CinArg, int Cout, int kh, int kw, int sh, int sw, int ph, int pw, bool transposed, int out_pad,
               int quant, int ups4, const ConvPlanKnobs& knobs, std::string* err) {
    *p = ConvPlan();
    *r = ConvRoute();
    if (quant) {
        if (transposed || kh != 3 || kw != 3 || sh != 1 || sw != 1 || ph != 1 || pw != 1 || out_pad != 0 || CinArg % 32 != 0) {
            if (err) *err = "fp8 operands: 3x3 stride-1 pad-1 convs with Cin % 32 == 0 only";
            return -1;
        }
        p->q8 = true;
        if (quant == 2) {
            if (CinArg % 64 != 0) { if (err) *err = "MX fp8 operands: Cin % 64 == 0"; return -1; }
            p->mx = true;
        }
    }
    p->CinReal = CinArg;
    // fp8: two channels per 16-bit unit; everything below (chunking, pack order, launch geometry) sees CinArg / 2 "channels"
    const int CinReal = quant ? CinArg / 2 : CinArg;
    // channel-blocked layout: whole 16-channel blocks; inputs of <= 8 channels are plain [N][H][W][8]
    const int Cin = CinReal <= 8 ? 8 : (CinReal + 15) / 16 * 16;
    p->kh = kh; p->kw = kw; p->sh = sh; p->sw = sw; p->ph = ph; p->pw = pw;
    p->transposed = transposed; p->out_pad = out_pad;
    p->Cin = Cin; p->Cout = Cout;

    // logical conv the kernel executes
    int lCout = Cout;        // output channels of the executed conv
    int lsh = sh, lsw = sw;  // input stride
    std::vector<std::vector<ConvTap>>& phases = r->phases;
    std::vector<std::pair<int, int>>& phase_off = r->phase_off;
    const bool v3_on = knobs.v3_on;
    const bool is_convT_s2 = transposed && kh == 3 && kw == 3 && sh == 2 && sw == 2 && ph == 1 && pw == 1 && out_pad == 1;
    if (ups4 && v3_on && !transposed && !quant && kh == 3 && kw == 3 && sh == 1 && sw == 1 && ph == 1 && pw == 1 &&
        out_pad == 0 && Cin % 16 == 0) {
        // four-phase upsample-conv (ups4_pairs): ONE phase of 16 "taps" over a 4 x 4 weight, tap t = pair t of the pre-summed weights
        p->v3 = true; p->v3_G = 4; p->v3_T = 16; p->ups4 = true;
        lsh = lsw = 1;
        std::vector<ConvTap> taps;
        for (const Ups4Pair& q : ups4_pairs()) { const int t = (int)taps.size(); taps.push_back({t >> 2, t & 3, q.dy, q.dx}); }
        if (taps.size() != 16) { if (err) *err = "ups4 tap table"; return -1; }
        phases.push_back(taps);
        phase_off.push_back({0, 0});
    } else if (v3_on && is_convT_s2 && Cin % 16 == 0) {
        // conv3 merged transposed conv: ONE phase of 9 taps over a 2x2 input neighbourhood, in the tap order the
        // kernel's static table expects (offset (0,0): phases 0..3, (0,1): 1,3, (1,0): 2,3, (1,1): 3)
        p->v3 = true; p->v3_G = 4; p->v3_T = 9;
        lsh = lsw = 1;
        phases.push_back({{1, 1, 0, 0}, {1, 2, 0, 0}, {2, 1, 0, 0}, {2, 2, 0, 0},
                          {1, 0, 0, 1}, {2, 0, 0, 1}, {0, 1, 1, 0}, {0, 2, 1, 0}, {0, 0, 1, 1}});
        phase_off.push_back({0, 0});
    } else if (!transposed) {
        std::vector<ConvTap> taps;
        for (int y = 0; y < kh; ++y)
            for (int x = 0; x < kw; ++x) taps.push_back({y, x, y, x});
        phases.push_back(taps);
        phase_off.push_back({0, 0});
    } else if (sh == 1 && sw == 1 && ph == 0 && pw == 0 && out_pad == 0) {
        // k x k transposed conv: only the 1x1-input case is supported (a GEMM to k*k*Cout channels)
        p->gemm_1x1_expand = true;
        lCout = kh * kw * Cout;
        phases.push_back({{0, 0, 0, 0}});
        phase_off.push_back({0, 0});
    } else if (kh == 3 && kw == 3 && sh == 2 && sw == 2 && ph == 1 && pw == 1 && out_pad == 1) {
        lsh = lsw = 1;
        for (int py = 0; py < 2; ++py)
            for (int px = 0; px < 2; ++px) {
                std::vector<std::pair<int, int>> ys, xs;  // (k index, input offset)
                if (py == 0) ys = {{1, 0}}; else ys = {{0, 1}, {2, 0}};
                if (px == 0) xs = {{1, 0}}; else xs = {{0, 1}, {2, 0}};
                std::vector<ConvTap> taps;
                for (auto& yy : ys)
                    for (auto& xx : xs) taps.push_back({yy.first, xx.first, yy.second, xx.second});
                phases.push_back(taps);
                phase_off.push_back({py, px});
            }
    } else {
        if (err) *err = "unsupported transposed conv configuration";
        return -1;
    }

    if (v3_on && !p->v3 && !transposed && Cin % 16 == 0 && kh == 3 && kw == 3 && sh == 2 && sw == 2 &&
        ((ph == 1 && pw == 1 && out_pad == 0) || (ph == 0 && pw == 0 && out_pad == 1)) &&
        // measured in the pass (profiles/r04_s2_conflict_free.txt; conv3's stride-2 LDS image is bank-conflict free since round 4), register-
        // staged kernel -> conv3, 16 / 256 frames: 64->128 @64^2 16.9 -> 16.4 / 127 -> 94 us, 128->256 @32^2 20.4 -> 17.2 / 93 -> 69 us: conv3 from
        // 64 input channels on.  The wide, shallow ones stay register-staged: 16->32 @256^2 22.7 -> 30.5 / 249 -> 389 us (one 16-channel chunk per
        // item: 18 MFMAs per wave behind a 36-KB patch copy), 32->64 @128^2 15.0 -> 16.9 at 16 frames (-52 us at 256: a per-launch choice would
        // need both weight packs).  The asymmetric-pad form exists only in conv3.
        (Cin >= 64 || out_pad == 1)) {
        p->v3 = true; p->v3_G = 1; p->v3_T = 9; p->v3_S = 2;
    }
    if (v3_on && !p->v3 && Cin % 16 == 0 && lsh == 1 && lsw == 1) {
        if (!transposed && kh == 3 && kw == 3 && ph == 1 && pw == 1) { p->v3 = true; p->v3_G = 1; p->v3_T = 9; }
        if ((!transposed && kh == 1 && kw == 1 && ph == 0 && pw == 0) || p->gemm_1x1_expand) { p->v3 = true; p->v3_G = 1; p->v3_T = 1; }
    }
    const int Cin8 = Cin / 8;
    int NC8, NBT;
    const int Tmax = (int)std::max_element(phases.begin(), phases.end(),
                                           [](const std::vector<ConvTap>& a, const std::vector<ConvTap>& b) { return a.size() < b.size(); })->size();
    const bool strided = (lsh > 1 || lsw > 1);
    if (Cin8 == 1) {
        NC8 = 1; NBT = 1;
        if (lCout > 32) { if (err) *err = "Cin<=8 layers support Cout<=32"; return -1; }
    } else {
        if (Cin8 % 2) { if (err) *err = "Cin must be 8 or a multiple of 16"; return -1; }
        NBT = lCout >= 128 ? 4 : (lCout >= 64 ? 2 : 1);
        NC8 = (Cin8 >= 4) ? 4 : 2;
        if (strided || Tmax > 9) { NC8 = 2; NBT = std::min(NBT, 2); }   // large patches: 10 staging items, 2 planes
        // weight slab of one chunk must fit the staging registers (9 x 16 B per thread)
        while (((NC8 == 1) ? ((Tmax + 1) / 2 * 2) : Tmax) * NC8 * NBT * 32 > kMaxBItems * 256) {
            if (NC8 > 2) NC8 /= 2; else if (NBT > 1) NBT /= 2; else break;
        }
    }
    if (p->v3) {
        // 1x1: 64-channel chunks; wide outputs take 32-channel chunks so that a 128-cout block (conv3_plan_launch) still fits two
        // resident blocks per CU
        if (p->v3_T == 1) NC8 = (Cin % 32 == 0 && lCout >= 128 && lCout % 128 == 0) ? 4 : (Cin % 64 == 0) ? 8 : 2;
        else if (p->ups4) NC8 = 2;          // 16 weight matrices per chunk: 16-channel chunks keep two blocks per CU
        else if (p->v3_G == 4) NC8 = (Cin % 32 == 0) ? 4 : 2;
        // 16-channel chunks everywhere: measured (profiles/r02_conv_sweep.txt) equal or better than 32-channel chunks on
        // every 3x3 layer at 16 frames and 25-28 % better on the 256/512-channel 8^2..16^2 maps at 256 frames (the
        // smaller stage leaves room for two resident blocks and allows 512-pixel tiles); sweeps force 32 through knob CONV3_NC8
        else NC8 = (knobs.conv3_nc8 == 4 && Cin % 32 == 0) ? 4 : 2;
        if (p->v3_S == 2) NC8 = 2;
        if (p->mx) NC8 = 4;                 // 4 planes of 16 e4m3 channels = the 64 channels one MX MFMA contracts
        NBT = 2;
    }
    p->NC8 = NC8; p->NBT = NBT;      // NBT here = the widest block the staging registers allow
    p->tt9 = (!transposed && kh == 3 && kw == 3 && NC8 >= 2);
    p->nphase = (int)phases.size();
    const int Tp = (NC8 == 1) ? ((Tmax + 1) / 2 * 2) : Tmax;
    p->Tp = Tp;
    if (!p->v3) {
        if (Tp * NC8 * NBT * 32 > kMaxBItems * 256) { if (err) *err = "weight slab too large for staging registers"; return -1; }
        if (!conv1_has_kernel(NC8, std::min(NBT, 2), p->tt9)) { if (err) *err = "no kernel instantiation for this configuration"; return -1; }
    }
    p->CoutPad = (lCout + 127) / 128 * 128;   // any block width <= 128 tiles it evenly
    p->lCout = lCout;
    return 0;
}

// step 2: the weight view

// What the packer reads: element (co, ci, ky, kx) of the conv the kernel executes, as the 16 bits of one packed unit - an fp16 value,
// or two e4m3 channels under their output channel's scale.
struct ConvWeightView {
    const float* weight;          // the caller's, torch layout
    const float* wsrc;            // what wval reads: `weight`, or weff
    int wkh, wkw;                 // kernel extent of wsrc
    int CinArg, CinUnits, Cout;   // input channels; 16-bit units of them (fp8: two channels each)
    bool transposed;
    int quant;
    std::vector<float> weff;      // four-phase upsample-conv: [Cout][Cin][16] sums of the 3x3 taps per (operand, phase) pair
    std::vector<float> wq_scale;  // fp8: per-output-channel scale 224 / max|w|

    float wval(int co, int ci, int ky, int kx) const {
        if (ci >= CinUnits) return 0.f;
        if (!transposed) return wsrc[(((size_t)co * CinUnits + ci) * wkh + ky) * wkw + kx];
        return wsrc[(((size_t)ci * Cout + co) * wkh + ky) * wkw + kx];
    }
    // fp8: the 16-bit unit (two consecutive input channels, low byte first)
    uint16_t wbits(int co, int ci, int ky, int kx) const {
        if (!quant) { const f16 h = (f16)wval(co, ci, ky, kx); uint16_t u; memcpy(&u, &h, 2); return u; }
        if (ci >= CinUnits) return 0;
        const float s = wq_scale[co];
        const float lo = weight[(((size_t)co * CinArg + 2 * ci) * 3 + ky) * 3 + kx] * s;
        const float hi = weight[(((size_t)co * CinArg + 2 * ci + 1) * 3 + ky) * 3 + kx] * s;
        return (uint16_t)(f32_to_e4m3(lo) | (f32_to_e4m3(hi) << 8));
    }
};

static void conv_weight_view(ConvWeightView* v, const ConvPlan& p, const float* weight, int quant) {
    v->weight = v->wsrc = weight;
    v->wkh = p.kh; v->wkw = p.kw;
    v->CinArg = p.CinReal; v->CinUnits = quant ? p.CinReal / 2 : p.CinReal; v->Cout = p.Cout;
    v->transposed = p.transposed; v->quant = quant;
    if (p.ups4) {
        const int Cout = p.Cout, CinReal = v->CinUnits;
        v->weff.assign((size_t)Cout * CinReal * 16, 0.f);
        int t = 0;
        for (const Ups4Pair& q : ups4_pairs()) {
            // 3x3 taps of this phase that land on source offset (dy, dx)
            int kys[2], nky = 0, kxs[2], nkx = 0;
            for (int ky = 0; ky < 3; ++ky) if (1 + ((q.py + ky - 1) >> 1) == q.dy) kys[nky++] = ky;     // floor((py+ky-1)/2) + 1
            for (int kx = 0; kx < 3; ++kx) if (1 + ((q.px + kx - 1) >> 1) == q.dx) kxs[nkx++] = kx;
            for (int co = 0; co < Cout; ++co)
                for (int ci = 0; ci < CinReal; ++ci) {
                    float acc = 0.f;
                    for (int a = 0; a < nky; ++a)
                        for (int b = 0; b < nkx; ++b) acc += weight[(((size_t)co * CinReal + ci) * 3 + kys[a]) * 3 + kxs[b]];
                    v->weff[((size_t)co * CinReal + ci) * 16 + t] = acc;
                }
            ++t;
        }
        v->wsrc = v->weff.data(); v->wkh = 4; v->wkw = 4;
    }
    if (quant) {
        v->wq_scale.assign(p.Cout, 1.f);
        const size_t per = (size_t)p.CinReal * 9;
        for (int co = 0; co < p.Cout; ++co) {
            float m = 0.f;
            for (size_t i = 0; i < per; ++i) m = std::max(m, std::fabs(weight[(size_t)co * per + i]));
            if (m > 0.f) v->wq_scale[co] = 224.f / m;
        }
    }
}

// step 3: the packer

// The slab layout of a plan: [phase][cout/32][chunk][tap][plane][32][8 halfs]
struct ConvPackGeom {
    int Cin8, n_sub, nchunks;
    size_t phase_halfs;
    explicit ConvPackGeom(const ConvPlan& p) {
        Cin8 = p.Cin / 8;
        n_sub = p.CoutPad / 32;
        nchunks = (Cin8 + p.NC8 - 1) / p.NC8;
        phase_halfs = (size_t)n_sub * nchunks * ((size_t)p.Tp * p.NC8 * 32 * 8);
    }
};

// 32-cout sub-slabs [nt0, nt1) of one phase into `base`
static void pack_range(const ConvPlan& p, const ConvPackGeom& g, const ConvWeightView& v, const std::vector<ConvTap>& taps, f16* base, int nt0, int nt1) {
    const int NC8 = p.NC8, T = (int)taps.size();
    for (int nt = nt0; nt < nt1; ++nt)
        for (int c = 0; c < g.nchunks; ++c)
            for (int t = 0; t < T; ++t)
                for (int pl = 0; pl < NC8; ++pl) {
                    const int c8 = c * NC8 + pl;
                    if (c8 >= g.Cin8) continue;
                    for (int n = 0; n < 32; ++n) {
                        const int lco = nt * 32 + n;
                        if (lco >= p.lCout) continue;
                        int co = lco, ky = taps[t].ky, kx = taps[t].kx;
                        if (p.gemm_1x1_expand) {
                            // output channel order (cout block, position, 16): the result [N][k*k*Cout/16][1][1][16]
                            // IS the channel-blocked k x k map [N][Cout/16][k][k][16]
                            const int c16 = lco & 15, tt = lco >> 4, pos = tt % (p.kh * p.kw);
                            co = (tt / (p.kh * p.kw)) * 16 + c16; ky = pos / p.kw; kx = pos % p.kw;
                        }
                        f16* dst = base + ((((size_t)(nt * g.nchunks + c) * p.Tp + t) * NC8 + pl) * 32 + n) * 8;
                        for (int j = 0; j < 8; ++j) { const uint16_t u = v.wbits(co, c8 * 8 + j, ky, kx); memcpy(&dst[j], &u, 2); }
                    }
                }
}

// One phase.  The 32-cout sub-slabs are written to disjoint ranges: packed by a few host threads when the layer is large (a MuseTalk
// load packs 0.9 G weights: 16 s on one thread)
static void pack_phase(const ConvPlan& p, const ConvPackGeom& g, const ConvWeightView& v, const std::vector<ConvTap>& taps, f16* base) {
    const size_t work = (size_t)g.n_sub * g.nchunks * taps.size() * p.NC8 * 256;
    const int nthr = work < (size_t)4 << 20 ? 1 : std::max(1, std::min({(int)std::thread::hardware_concurrency(), 16, g.n_sub}));
    if (nthr <= 1) { pack_range(p, g, v, taps, base, 0, g.n_sub); return; }
    std::vector<std::thread> th;
    for (int k = 0; k < nthr; ++k)
        th.emplace_back([&, k] { pack_range(p, g, v, taps, base, (int)((long long)g.n_sub * k / nthr), (int)((long long)g.n_sub * (k + 1) / nthr)); });
    for (std::thread& t : th) t.join();
}

static void conv_pack(const ConvPlan& p, const ConvRoute& r, const ConvWeightView& v, std::vector<f16>* packed, std::vector<PhaseMeta>* metas) {
    const ConvPackGeom g(p);
    packed->assign(g.phase_halfs * r.phases.size(), (f16)0.f);
    metas->resize(r.phases.size());
    for (size_t pi = 0; pi < r.phases.size(); ++pi) {
        PhaseMeta& m = (*metas)[pi];
        memset(&m, 0, sizeof(m));
        m.T = (int)r.phases[pi].size();
        m.ooy = r.phase_off[pi].first;
        m.oox = r.phase_off[pi].second;
        m.w_off16 = (int)(pi * g.phase_halfs / 8);
        for (int t = 0; t < m.T; ++t) { m.dy[t] = (signed char)r.phases[pi][t].dy; m.dx[t] = (signed char)r.phases[pi][t].dx; }
        pack_phase(p, g, v, r.phases[pi], packed->data() + pi * g.phase_halfs);
    }
}

// step 4: folded BN parameters (padded to CoutPad; replicated per position for the 1x1-expand case)
static void conv_fold(const ConvPlan& p, const ConvWeightView& v, const float* scale, const float* shift, float act_scale,
                      std::vector<float>* sc, std::vector<float>* sf) {
    sc->assign(p.CoutPad, 0.f); sf->assign(p.CoutPad, 0.f);
    for (int i = 0; i < p.lCout; ++i) {
        const int co = p.gemm_1x1_expand ? ((i >> 4) / (p.kh * p.kw)) * 16 + (i & 15) : i;
        (*sc)[i] = scale ? scale[co] : 1.f; (*sf)[i] = shift ? shift[co] : 0.f;
        if (v.quant) (*sc)[i] /= v.wq_scale[co] * act_scale;        // acc = sum (w s_w)(x s_a)
    }
}

// step 5: upload
static int conv_upload(ConvPlan* p, const std::vector<f16>& packed, const std::vector<PhaseMeta>& metas, const std::vector<float>& sc,
                       const std::vector<float>& sf, std::string* err) {
    const int CoutPad = p->CoutPad;
    p->w_bytes = packed.size() * sizeof(f16);
    HIPCHK(hipMalloc((void**)&p->d_w, p->w_bytes + metas.size() * sizeof(PhaseMeta) + 256));
    HIPCHK(hipMemcpy(p->d_w, packed.data(), p->w_bytes, hipMemcpyHostToDevice));
    // phase metadata lives behind the weights (16-byte aligned)
    {
        const size_t off = (p->w_bytes + 15) / 16 * 16;
        HIPCHK(hipMemcpy((char*)p->d_w + off, metas.data(), metas.size() * sizeof(PhaseMeta), hipMemcpyHostToDevice));
    }
    HIPCHK(hipMalloc((void**)&p->d_scale, CoutPad * sizeof(float) * 2));
    p->d_shift = p->d_scale + CoutPad;
    HIPCHK(hipMemcpy(p->d_scale, sc.data(), CoutPad * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(p->d_shift, sf.data(), CoutPad * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

int conv_plan_create(ConvPlan* p, const float* weight, int Cin, int Cout, int kh, int kw,
                     int sh, int sw, int ph, int pw, bool transposed, int out_pad,
                     const float* scale, const float* shift, std::string* err, int quant, float act_scale, int ups4) {
    ConvRoute route;
    if (const int rc = conv_route(p, &route, Cin, Cout, kh, kw, sh, sw, ph, pw, transposed, out_pad, quant, ups4, conv_plan_knobs(), err)) return rc;
    ConvWeightView view;
    conv_weight_view(&view, *p, weight, quant);
    std::vector<f16> packed;
    std::vector<PhaseMeta> metas;
    conv_pack(*p, route, view, &packed, &metas);
    std::vector<float> sc, sf;
    conv_fold(*p, view, scale, shift, act_scale, &sc, &sf);
    return conv_upload(p, packed, metas, sc, sf, err);
}

void conv_plan_destroy(ConvPlan* p) {
    if (p->d_w) (void)hipFree(p->d_w);
    if (p->d_scale) (void)hipFree(p->d_scale);
    p->d_w = nullptr; p->d_scale = nullptr; p->d_shift = nullptr;
}

// launch dispatch

int conv_launch(const ConvPlan& p, const ConvIO& io, hipStream_t stream, std::string* err) {
    return p.v3 ? conv3_launch(p, io, stream, err) : conv1_launch(p, io, stream, err);
}

int conv_launch_dry(const ConvPlan& p, const ConvIO& io, std::string* err) {
    return p.v3 ? conv3_plan_launch(p, io, nullptr, err) : conv1_plan_launch(p, io, nullptr, err);
}

}  // namespace ltk

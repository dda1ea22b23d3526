// ------------------------------------------------------------------ test / measurement hooks of both models
#include "debug_util.h"
#include "facedet.h"
#include "faceparse.h"
#include "parse_kernels.h"
#include "s3fd_kernels.h"
#include "ul_gconv.h"
#include "ul_ir.h"

extern "C" {

// B frames from host tensors (warm_up, tests).  Runs as passes of at most one arena (micro-batch) each, so a start-up
// warm_up(batch_size) also works when LTK_MICROBATCH is smaller than the session batch.
int ltk_wav2lip_forward_host(ltk_engine* e, const float* mel, const float* face6, int B, float* pred) {
    if (!e || !mel || !face6 || !pred || B <= 0) return fail(LTK_E_INVALID, "bad arguments");
    if (!e->loaded) return fail(LTK_E_STATE, "ltk_wav2lip_load has not been called");
    if (B > e->max_frames) return fail(LTK_E_INVALID, "B exceeds max_frames");
    CHK(enter_device(e->device));
    { const int drc = drain_pending(e); if (drc) return drc; }      // knob DEFER: behind the pass in flight (as every hook below)
    const int mb = std::min(e->micro_batch, kPackMaxFrames);
    const int cap = std::min(B, mb);
    DevBuf d_mel, d_face, d_pred;
    CHK(hipMalloc(&d_mel.p, (size_t)cap * 80 * 16 * sizeof(float)));
    CHK(hipMalloc(&d_face.p, (size_t)cap * 6 * 65536 * sizeof(float)));
    CHK(hipMalloc(&d_pred.p, (size_t)cap * 3 * 65536 * sizeof(float)));
    for (int f0 = 0; f0 < B; f0 += mb) {
        const int nf = std::min(mb, B - f0);
        CHK(hipMemcpy(d_mel.p, mel + (size_t)f0 * 1280, (size_t)nf * 1280 * sizeof(float), hipMemcpyHostToDevice));
        CHK(hipMemcpy(d_face.p, face6 + (size_t)f0 * 6 * 65536, (size_t)nf * 6 * 65536 * sizeof(float), hipMemcpyHostToDevice));
        MelPtrs mp;
        for (int i = 0; i < nf; ++i) mp.p[i] = (float*)d_mel.p + (size_t)i * 1280;
        {
            std::lock_guard<std::mutex> g(e->mu);
            launch_upload_tables(nullptr, &mp, nullptr, nf, e->d_tab, e->compute);
            CHK(hipGetLastError());
            const int rc = launch_pass(e, nf, e->compute, false, (const float*)d_face.p, false, (float*)d_pred.p);
            if (rc) return rc;
            CHK(hipStreamSynchronize(e->compute));
        }
        CHK(hipMemcpy(pred + (size_t)f0 * 3 * 65536, d_pred.p, (size_t)nf * 3 * 65536 * sizeof(float), hipMemcpyDeviceToHost));
    }
    return LTK_OK;
}

int ltk_debug_capture(ltk_engine* e, int enable) {
    if (!e) return fail(LTK_E_INVALID, "engine is null");
    (void)hipSetDevice(e->device);
    { const int drc = drain_pending(e); if (drc) return drc; }
    std::lock_guard<std::mutex> g(e->mu);
    e->capture = enable != 0;
    if (!enable) { e->taps.clear(); e->tap_shape.clear(); }
    return LTK_OK;
}

int ltk_debug_set_knob(const char* name, int value) {
    if (knob_set(name, value)) return fail(LTK_E_INVALID, std::string("unknown knob ") + (name ? name : "(null)"));
    return LTK_OK;
}

int ltk_debug_get(ltk_engine* e, const char* layer, float* out, size_t n_floats) {
    if (!e || !layer || !out) return fail(LTK_E_INVALID, "bad arguments");
    (void)hipSetDevice(e->device);
    { const int drc = drain_pending(e); if (drc) return drc; }
    std::lock_guard<std::mutex> g(e->mu);
    auto it = e->taps.find(layer);
    if (it == e->taps.end()) return fail(LTK_E_STATE, std::string("no capture for layer ") + layer);
    if (it->second.size() != n_floats) return fail(LTK_E_INVALID, "size mismatch: captured " + std::to_string(it->second.size()));
    memcpy(out, it->second.data(), n_floats * sizeof(float));
    return LTK_OK;
}

// Dummy inputs of the timing hooks: every frame reads one zero bank crop and one zero mel window and writes its own scratch frame, so
// that the hooks run the pass exactly as ltk_wav2lip_infer does (bank crops in, fused head out, captured graph included).
namespace {
struct TimingIO {
    DevBuf face, mel, frames;
    int setup(ltk_engine* e, int nf) {
        CHK(hipMalloc(&face.p, 65536 * 3));
        CHK(hipMemset(face.p, 0, 65536 * 3));
        CHK(hipMalloc(&mel.p, 1280 * sizeof(float)));
        CHK(hipMemset(mel.p, 0, 1280 * sizeof(float)));
        CHK(hipMalloc(&frames.p, (size_t)nf * 65536 * 3));
        FacePtrs fp; MelPtrs mp; OutPtrs op;
        for (int i = 0; i < nf; ++i) { fp.p[i] = (const uint8_t*)face.p; mp.p[i] = (const float*)mel.p; op.p[i] = (uint8_t*)frames.p + (size_t)i * 65536 * 3; }
        launch_upload_tables(&fp, &mp, &op, nf, e->d_tab, e->compute);
        CHK(hipGetLastError());
        return 0;
    }
};
}  // namespace

int ltk_wav2lip_time_convs(ltk_engine* e, int frames, int iters, float* ms_per_pass, double* macs_per_pass) {
    if (!e || frames <= 0 || iters <= 0 || !ms_per_pass) return fail(LTK_E_INVALID, "bad arguments");
    if (!e->loaded) return fail(LTK_E_STATE, "ltk_wav2lip_load has not been called");
    if (frames > e->max_frames) return fail(LTK_E_INVALID, "frames exceeds max_frames");
    CHK(enter_device(e->device));
    { const int drc = drain_pending(e); if (drc) return drc; }
    std::lock_guard<std::mutex> g(e->mu);
    if (e->capture) return fail(LTK_E_STATE, "disable capture before timing");
    // the pass as ltk_wav2lip_infer runs it (pack_mel + conv stack with the bank gather and the output head fused, knob
    // HEAD_FUSED; replayed from the captured graph under knob GRAPH), same micro-batch schedule, frames going to a scratch buffer
    const int mbs = std::min(e->micro_batch, kPackMaxFrames);
    TimingIO tio;
    int rc = tio.setup(e, std::min(mbs, frames));
    if (rc) return rc;
    // knob PREFETCH: a session's consecutive <= 32-frame calls are pipelined across calls (tune.h); what is timed is then that steady
    // state - every pass finds its face-encoder outputs prefetched and prefetches the next pass's (dummy bank crops here) - which
    // is what the session's calls enqueue from the third call on
    for (ltk_engine::PfSlot& sl : e->pfs) sl.valid = false;        // the timing passes fill slots 1 and 2 with dummy crops
    const bool pipe = knob(K_PREFETCH) && e->alt_frames > 0 && frames <= std::min(e->alt_frames, mbs) && knob(K_HEAD_FUSED) && e->c7;
    if (pipe) {
        FacePtrs nx;
        for (int i = 0; i < frames; ++i) nx.p[i] = (const uint8_t*)tio.face.p;
        launch_upload_tables(&nx, nullptr, nullptr, frames, e->d_tab_next, e->aux2);
    }
    int cur = 0;              // slot this pass works in (0: the priming pass runs the whole network in the arena's own set)
    auto pass = [&]() -> int {
        int prc = 0;
        if (pipe) {
            if (cur) CHK(hipStreamWaitEvent(e->compute, e->pfs[cur].ev_done, 0));
            prc = launch_pass(e, frames, e->compute, true, nullptr, true, nullptr, false, cur, cur != 0);
            if (cur) {
                if (hipEventRecord(e->pfs[cur].ev_read, e->compute) != hipSuccess) { if (!prc) prc = fail(LTK_E_HIP, "hipEventRecord failed"); }
                else e->pfs[cur].read = true;
            }
            const int nxt = cur == 1 ? 2 : 1;
            if (!prc) prc = launch_prefetch(e, frames, nxt);
            cur = nxt;
            return prc;
        }
        for (int f0 = 0; f0 < frames && !prc; f0 += mbs) prc = launch_pass(e, std::min(mbs, frames - f0), e->compute, true, nullptr, true, nullptr);
        return prc;
    };
    if (pipe) { rc = pass(); if (!rc) rc = pass(); if (!rc) rc = pass(); if (rc) return rc; }     // prime, then both slots seen once (eager)
    rc = pass();              // warm (eager)
    if (!rc) rc = pass();     // warm (captures the graph under knob GRAPH)
    if (rc) return rc;
    float ms = 0.f;
    if ((rc = time_iters(e->compute, iters, pass, &ms))) return rc;
    *ms_per_pass = ms / iters;
    if (macs_per_pass) *macs_per_pass = (e->macs_per_frame - (knob(K_HEAD_FUSED) ? 0.0 : 32.0 * 3 * 65536)) * frames;
    return LTK_OK;
}

int ltk_wav2lip_prefetch_stats(ltk_engine* e, unsigned long long* hits, unsigned long long* misses, unsigned long long* issued) {
    if (!e) return fail(LTK_E_INVALID, "engine is null");
    (void)hipSetDevice(e->device);
    { const int drc = drain_pending(e); if (drc) return drc; }
    std::lock_guard<std::mutex> g(e->mu);
    if (hits) *hits = e->pf_hits;
    if (misses) *misses = e->pf_misses;
    if (issued) *issued = e->pf_issued;
    return LTK_OK;
}

int ltk_debug_solo_walk(int outstanding, int calls, int jump_at, int* slots_used) {
    if (outstanding < 0 || outstanding > 1 || calls <= 0) return -1;
    return solo_walk_last_capture(outstanding, calls, jump_at, slots_used);
}

int ltk_program_graph_count(ltk_engine* e) {
    if (!e) return 0;
    std::lock_guard<std::mutex> g(e->mu);
    return e->prog_graphs.live();
}

int ltk_wav2lip_graph_count(ltk_engine* e) {
    if (!e) return 0;
    (void)hipSetDevice(e->device);
    (void)drain_pending(e);
    std::lock_guard<std::mutex> g(e->mu);
    return e->graphs.live();
}

int ltk_wav2lip_layer_count(ltk_engine* e) {
    if (!e || !e->loaded) return 0;
    return (int)e->layers.size();
}

int ltk_wav2lip_layer_name(ltk_engine* e, int layer, char* buf, int buf_len) {
    if (!e || !e->loaded || layer < 0 || layer >= (int)e->layers.size() || !buf || buf_len <= 0) return fail(LTK_E_INVALID, "bad arguments");
    snprintf(buf, (size_t)buf_len, "%s", e->layers[layer].name.c_str());
    return LTK_OK;
}

int ltk_wav2lip_set_layer_tile(ltk_engine* e, int layer, int bucket, int pxw, int nbt, int ksplit) {
    if (!e || !e->loaded || layer < 0 || layer >= (int)e->layers.size() || bucket < 0 || bucket > 4) return fail(LTK_E_INVALID, "bad arguments");
    std::lock_guard<std::mutex> g(e->mu);
    Layer::Tile& t = e->layers[layer].tile[bucket];
    t.pxw = (signed char)pxw; t.nbt = (signed char)nbt; t.ks = (signed char)ksplit;
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->compute);
    e->graphs.drop();                  // captured passes carry the old tile choice
    return LTK_OK;
}

int ltk_wav2lip_time_layers(ltk_engine* e, int frames, int iters, float* ms_per_layer, int n_layers) {
    if (!e || frames <= 0 || iters <= 0 || !ms_per_layer) return fail(LTK_E_INVALID, "bad arguments");
    if (!e->loaded) return fail(LTK_E_STATE, "ltk_wav2lip_load has not been called");
    if (frames > e->micro_batch || frames > kPackMaxFrames) return fail(LTK_E_INVALID, "frames exceeds one arena pass");
    if (n_layers != (int)e->layers.size()) return fail(LTK_E_INVALID, "n_layers != ltk_wav2lip_layer_count");
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    if (e->capture) return fail(LTK_E_STATE, "disable capture before timing");
    const bool fused = knob(K_HEAD_FUSED) != 0;
    TimingIO tio;
    int rc = tio.setup(e, frames);
    if (rc) return rc;
    const OutPtrs* d_outs = fused ? &e->d_tab->outs : nullptr;
    const FacePtrs* d_faces = e->c7 ? &e->d_tab->faces : nullptr;
    if ((rc = run_convs(e, frames, e->compute, d_outs, nullptr, d_faces))) return rc;     // warm
    return time_intervals(n_layers, iters, [&](std::vector<hipEvent_t>* evs) { return run_convs(e, frames, e->compute, d_outs, evs, d_faces); },
                          ms_per_layer);
}

namespace {
// one conv layer on its own, fp16 operands (quant = 0) or e4m3 (conv_fp8_quant): plan, one launch, then `iters` timed ones
int conv2d_hook(ltk_engine* e, const void* d_x, int N, int H, int W, int Cin, const float* weight, int Cout, int kh, int kw, int sh, int sw,
                int ph, int pw, bool transposed, int out_pad, const float* scale, const float* shift, int quant, float act_scale,
                const void* d_res, int relu, int act, void* d_y, int iters, float* ms_avg) {
    if (!e || !d_x || !weight || !d_y) return fail(LTK_E_INVALID, "bad arguments");
    CHK(enter_device(e->device));
    ConvPlan plan;
    std::string err;
    int rc = conv_plan_create(&plan, weight, Cin, Cout, kh, kw, sh, sw, ph, pw, transposed, out_pad, scale, shift, &err, quant, act_scale);
    if (rc) return conv_status(rc, err);
    ConvIO io;
    io.partial = e->d_partial; io.partial_cap = e->partial_cap;
    io.x = (const f16*)d_x; io.N = N; io.H = H; io.W = W; io.x_ld = plan.Cin; io.x_coff = 0;   // (fp8: 16-bit units)
    io.y = (f16*)d_y; io.y_ld = Cout; io.y_coff = 0;
    io.res = (const f16*)d_res; io.res_ld = Cout; io.res_coff = 0;
    io.relu = relu; io.act = act;
    hipStream_t s = e->compute;
    std::lock_guard<std::mutex> g(e->mu);
    auto launch = [&]() -> int { const int lrc = conv_launch(plan, io, s, &err); return lrc ? conv_status(lrc, err) : 0; };
    rc = launch();
    if (!rc && iters > 0 && ms_avg) {
        float ms = 0.f;
        rc = time_iters(s, iters, launch, &ms);
        *ms_avg = ms / iters;
    }
    const hipError_t he = hipStreamSynchronize(s);
    conv_plan_destroy(&plan);
    if (rc) return rc;
    if (he != hipSuccess) return fail(LTK_E_HIP, std::string("conv kernel: ") + hipGetErrorString(he));
    return LTK_OK;
}
}  // namespace

int ltk_conv2d_f16(ltk_engine* e, const void* d_x, int N, int H, int W, int Cin, const float* weight, int Cout, int kh, int kw, int sh, int sw,
                   int ph, int pw, int transposed, int out_pad, const float* scale, const float* shift, const void* d_res, int relu, void* d_y,
                   int iters, float* ms_avg) {
    return conv2d_hook(e, d_x, N, H, W, Cin, weight, Cout, kh, kw, sh, sw, ph, pw, transposed != 0, out_pad, scale, shift, 0, 1.f, d_res, relu, 0,
                       d_y, iters, ms_avg);
}

namespace {
// plans of the hook below, freed on every return path
struct ConvPlanOwner { ConvPlan p; ~ConvPlanOwner() { conv_plan_destroy(&p); } };
struct RowPlansOwner { RowGemmPlan p[4]; ~RowPlansOwner() { for (RowGemmPlan& q : p) rowgemm_plan_destroy(&q); } };
}  // namespace

namespace {
// What ltk_conv2d_f16_ex / ltk_conv2d_fp8_ex and their host-only twins derive from their arguments
struct ConvHookCall {
    int act = 0, x_ld = 0, y_ld = 0, res_ld = 0;
    int quant = 0;               // the plan's: 0 fp16, 1 e4m3 MFMA, 2 MX
    ConvIO io;                   // family 0: the launch without its pointers and scratch
    int Ho = 0, Wo = 0;          // rowconv / rowconvT: the output map
};

void conv_report_copy(const ConvReport& cr, ltk_conv_report* rep) {
    memcpy(rep->kernel, cr.kernel, sizeof(rep->kernel));
    rep->G = cr.G; rep->NBT = cr.NBT; rep->PXW = cr.PXW; rep->NC8 = cr.NC8; rep->T = cr.T; rep->S = cr.S;
    rep->ksplit = cr.ksplit; rep->items = cr.items; rep->grid = cr.grid;
    rep->l2w = cr.l2w; rep->l2h = cr.l2h; rep->NB = cr.NB; rep->s2half = cr.s2half; rep->phases = cr.phases; rep->lds = cr.lds; rep->args_hash = cr.args_hash;
}

// Everything ltk_conv2d_f16_ex / ltk_conv2d_fp8_ex decide before they allocate or enqueue, on the host alone: the options and the
// channel views; family 0: conv_route and the launch planner (conv3_plan_launch with the split-K scratch taken as unbounded, or conv1_plan_launch); the row
// families: their shape refusals.  `quant`: 0 fp16 operands, 1 e4m3, 2 MX - x and its view then count fp8 channels (32 per block) and
// reach the launch in 16-bit units, as mt_graph.hip halves them.  *rep (may be NULL) = what a launch of this call reports.
int conv_hook_plan(int N, int H, int W, int Cin, int Cout, int kh, int kw, int sh, int sw, int ph, int pw, int transposed, int out_pad, bool has_res,
                   int relu, int quant, const ltk_conv_opts* opts, ltk_conv_report* rep, ConvHookCall* c) {
    if (!opts || N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || quant < 0 || quant > 2) return fail(LTK_E_INVALID, "bad arguments");
    const ltk_conv_opts& o = *opts;
    if (o.family < 0 || o.family > 3 || o.act < 0 || o.act > 3 || o.ups < 0 || o.ups > 2 || (relu && o.act > 1)) return fail(LTK_E_INVALID, "bad options");
    if (quant && (o.family != 0 || o.ups != 0)) return fail(LTK_E_INVALID, "fp8 operands: the conv kernels (family 0) without an upsample");
    if (rep) { memset(rep, 0, sizeof(*rep)); rep->family = o.family; }
    c->quant = quant;
    const int act = c->act = relu ? 1 : o.act;
    const int CinP = quant ? Cin : Cin <= 8 ? 8 : (Cin + 15) / 16 * 16;
    const int x_ld = c->x_ld = o.x_ld ? o.x_ld : CinP, y_ld = c->y_ld = o.y_ld ? o.y_ld : Cout, res_ld = c->res_ld = o.res_ld ? o.res_ld : Cout;
    if (o.x_coff < 0 || o.y_coff < 0 || o.res_coff < 0 || o.x_coff + CinP > x_ld || o.y_coff + Cout > y_ld || (has_res && o.res_coff + Cout > res_ld))
        return fail(LTK_E_INVALID, "channel view outside its buffer");
    std::string err;
    if (o.family == 0) {
        ConvPlan plan;
        ConvRoute route;
        const int rc = conv_route(&plan, &route, Cin, Cout, kh, kw, sh, sw, ph, pw, transposed != 0, out_pad, quant, o.ups == 2 ? 1 : 0, conv_plan_knobs(), &err);
        if (rc) return conv_status(rc, err);
        if (quant && ((x_ld | o.x_coff) & 31)) return fail(LTK_E_INVALID, "fp8 operands: the view of x is given in multiples of 32 channels");
        const int xdiv = quant ? 2 : 1;           // fp8: two channels per 16-bit unit
        if (o.ups == 2 && !plan.ups4) return fail(LTK_E_INVALID, "conv3: the four-phase upsample-conv serves 3x3 stride-1 pad-1 layers");
        static const f16 there = (f16)0.f;        // the planner asks whether a residual / a scratch exists, never what it holds
        ConvReport cr;
        memset(&cr, 0, sizeof(cr));
        ConvIO& io = c->io;
        io = ConvIO();
        io.x = nullptr; io.N = N; io.H = H; io.W = W; io.x_ld = x_ld / xdiv; io.x_coff = o.x_coff / xdiv;
        io.y = nullptr; io.y_ld = y_ld; io.y_coff = o.y_coff;
        io.res = has_res ? &there : nullptr; io.res_ld = res_ld; io.res_coff = o.res_coff;
        io.relu = act == 1; io.act = act == 1 ? 0 : act;
        io.ups = o.ups ? 1 : 0;
        io.force_pxw = o.force_pxw; io.force_nbt = o.force_nbt; io.force_ksplit = o.force_ksplit;
        io.partial = const_cast<float*>(reinterpret_cast<const float*>(&there)); io.partial_cap = ~(size_t)0;
        io.report = &cr;
        const int lrc = conv_launch_dry(plan, io, &err);
        io.res = nullptr; io.partial = nullptr; io.partial_cap = 0; io.report = nullptr;
        if (lrc) return conv_status(lrc, err);
        if (rep) conv_report_copy(cr, rep);
        return LTK_OK;
    }
    // the row kernels: plans over W_eff built from the torch-layout weight as w2l_program.hip builds them
    if (act > 1 || o.ups || o.force_pxw || o.force_nbt || o.force_ksplit) return fail(LTK_E_INVALID, "the row kernels take no activation but ReLU, no upsample and no tile");
    if (Cin % 32 || Cout % 16) return fail(LTK_E_INVALID, "the row kernels need Cin % 32 == 0 and Cout % 16 == 0");
    if (o.family == 1) {
        if (transposed || kh != 1 || kw != 1 || H != 1 || W != 1 || has_res) return fail(LTK_E_INVALID, "rowgemm: a 1x1 conv on a one-pixel map, no residual");
        if (rep) { snprintf(rep->kernel, sizeof(rep->kernel), "rowgemm_kernel<%d>", rowgemm_ft(N)); rep->FT = rowgemm_ft(N); rep->UB = rowgemm_ub(rep->FT); rep->grid = Cout / 16; }
        return LTK_OK;
    }
    if (o.family == 2) {
        if (transposed || kh != 3 || kw != 3 || ph != 1 || pw != 1 || sh < 1 || sw < 1) return fail(LTK_E_INVALID, "rowconv: a 3x3 pad-1 conv");
        c->Ho = (H + 2 - 3) / sh + 1; c->Wo = (W + 2 - 3) / sw + 1;
        if (rep) {
            rep->FT = rowconv_ft((long long)N * c->Ho * c->Wo, Cout); rep->UB = rowconv_ub(rep->FT);
            snprintf(rep->kernel, sizeof(rep->kernel), "rowconv_kernel<%d,%d>", rep->FT, rep->UB);
        }
        return LTK_OK;
    }
    if (!transposed || kh != 3 || kw != 3 || sh != 2 || sw != 2 || ph != 1 || pw != 1 || out_pad != 1 || has_res)
        return fail(LTK_E_INVALID, "rowconvT: ConvTranspose2d(k3, s2, p1, op1), no residual");
    c->Ho = 2 * H; c->Wo = 2 * W;
    if (rep) {
        rep->FT = rowconv_ft((long long)N * H * W, Cout); rep->UB = rowconv_ub(rep->FT);
        snprintf(rep->kernel, sizeof(rep->kernel), "rowconv_kernel<%d,%d> x 4 phases", rep->FT, rep->UB);
    }
    return LTK_OK;
}
}  // namespace

int ltk_debug_conv_plan(int N, int H, int W, int Cin, int Cout, int kh, int kw, int sh, int sw, int ph, int pw, int transposed, int out_pad,
                        int has_res, int relu, const ltk_conv_opts* opts, ltk_conv_report* rep) {
    ConvHookCall c;
    return conv_hook_plan(N, H, W, Cin, Cout, kh, kw, sh, sw, ph, pw, transposed, out_pad, has_res != 0, relu, 0, opts, rep, &c);
}

int ltk_debug_conv_fp8_plan(int N, int H, int W, int Cin, int Cout, int kh, int kw, int sh, int sw, int ph, int pw, int transposed, int out_pad,
                            int quant, int has_res, const ltk_conv_opts* opts, ltk_conv_report* rep) {
    if (quant < 0 || quant > 2) return fail(LTK_E_INVALID, "bad arguments");
    ConvHookCall c;
    return conv_hook_plan(N, H, W, Cin, Cout, kh, kw, sh, sw, ph, pw, transposed, out_pad, has_res != 0, 0, quant ? quant : conv_fp8_quant(Cin), opts, rep, &c);
}

namespace {
// family 0 of ltk_conv2d_f16_ex / ltk_conv2d_fp8_ex behind conv_hook_plan: the plan, one launch, the stream drained, the report of what ran
int conv_hook_launch(ltk_engine* e, const ConvHookCall& c, const void* d_x, const float* weight, int Cin, int Cout, int kh, int kw, int sh, int sw,
                     int ph, int pw, int transposed, int out_pad, const float* scale, const float* shift, float act_scale, int ups4,
                     const void* d_res, void* d_y, ltk_conv_report* rep) {
    std::string err;
    ConvPlanOwner po;
    int rc = conv_plan_create(&po.p, weight, Cin, Cout, kh, kw, sh, sw, ph, pw, transposed != 0, out_pad, scale, shift, &err, c.quant, act_scale, ups4);
    if (rc) return conv_status(rc, err);
    ConvReport cr;
    memset(&cr, 0, sizeof(cr));
    ConvIO io = c.io;
    io.partial = e->d_partial; io.partial_cap = e->partial_cap;
    io.x = (const f16*)d_x; io.y = (f16*)d_y; io.res = (const f16*)d_res;
    io.report = &cr;
    hipStream_t s = e->compute;
    std::lock_guard<std::mutex> g(e->mu);
    const int lrc = conv_launch(po.p, io, s, &err);
    const hipError_t he = hipStreamSynchronize(s);      // the launch's error wins; the stream is drained either way
    if (lrc) return conv_status(lrc, err);
    if (he != hipSuccess) return fail(LTK_E_HIP, std::string("conv kernel: ") + hipGetErrorString(he));
    if (rep) conv_report_copy(cr, rep);                 // what ran: the split under the engine's own scratch
    return LTK_OK;
}
}  // namespace

int ltk_conv2d_f16_ex(ltk_engine* e, const void* d_x, int N, int H, int W, int Cin, const float* weight, int Cout, int kh, int kw, int sh, int sw,
                      int ph, int pw, int transposed, int out_pad, const float* scale, const float* shift, const void* d_res, int relu, void* d_y,
                      const ltk_conv_opts* opts, ltk_conv_report* rep) {
    if (!e || !d_x || !weight || !d_y) return fail(LTK_E_INVALID, "bad arguments");
    ConvHookCall c;
    int rc = conv_hook_plan(N, H, W, Cin, Cout, kh, kw, sh, sw, ph, pw, transposed, out_pad, d_res != nullptr, relu, 0, opts, rep, &c);
    if (rc) return rc;
    const ltk_conv_opts& o = *opts;
    CHK(enter_device(e->device));
    std::vector<float> ones, zeros;
    if (!scale) { ones.assign(Cout, 1.f); scale = ones.data(); }
    if (!shift) { zeros.assign(Cout, 0.f); shift = zeros.data(); }
    std::string err;
    hipStream_t s = e->compute;
    auto done = [&](int lrc) -> int {       // the launch's error wins; the stream is drained either way
        const hipError_t he = hipStreamSynchronize(s);
        if (lrc) return conv_status(lrc, err);
        if (he != hipSuccess) return fail(LTK_E_HIP, std::string("conv kernel: ") + hipGetErrorString(he));
        return LTK_OK;
    };
    if (o.family == 0)
        return conv_hook_launch(e, c, d_x, weight, Cin, Cout, kh, kw, sh, sw, ph, pw, transposed, out_pad, scale, shift, 1.f, o.ups == 2 ? 1 : 0, d_res, d_y, rep);
    RowPlansOwner ro;
    std::vector<float> we;
    if (o.family == 1) {
        rc = rowgemm_plan_create(&ro.p[0], weight, Cout, Cin, scale, shift, &err);
        if (rc) return conv_status(rc, err);
        std::lock_guard<std::mutex> g(e->mu);
        return done(rowgemm_launch(ro.p[0], (const f16*)d_x, c.x_ld, o.x_coff, (f16*)d_y, c.y_ld, o.y_coff, N, c.act, s, &err));
    }
    RowConvIO rio;
    rio.x = (const f16*)d_x; rio.x_ld = c.x_ld; rio.x_coff = o.x_coff; rio.H = H; rio.W = W;
    rio.y = (f16*)d_y; rio.y_ld = c.y_ld; rio.y_coff = o.y_coff; rio.Ho = c.Ho; rio.Wo = c.Wo;
    rio.N = N; rio.relu = c.act;
    if (o.family == 2) {
        rowconv_weff(weight, Cin, Cout, &we);
        rc = rowgemm_plan_create(&ro.p[0], we.data(), Cout, 9 * Cin, scale, shift, &err);
        if (rc) return conv_status(rc, err);
        rio.res = (const f16*)d_res; rio.res_ld = c.res_ld; rio.res_coff = o.res_coff;
        rio.KW = 3; rio.stride = sh; rio.stride_w = sw; rio.pad = 1;
        std::lock_guard<std::mutex> g(e->mu);
        return done(rowconv_launch(ro.p[0], rio, s, &err));
    }
    for (int gph = 0; gph < 4; ++gph) {
        rowconvT_weff(weight, Cin, Cout, gph, &we);
        rc = rowgemm_plan_create(&ro.p[gph], we.data(), Cout, (1 + (gph >> 1)) * (1 + (gph & 1)) * Cin, scale, shift, &err);
        if (rc) return conv_status(rc, err);
    }
    std::lock_guard<std::mutex> g(e->mu);
    return done(rowconvT_launch(ro.p, rio, s, &err));
}

int ltk_debug_conv3_variants(char* buf, int cap) {
    const std::string names = conv3_variant_names();
    if (!buf || cap <= (int)names.size()) return fail(LTK_E_INVALID, "buffer too small: " + std::to_string(names.size() + 1) + " bytes needed");
    memcpy(buf, names.c_str(), names.size() + 1);
    return LTK_OK;
}

int ltk_debug_conv1_variants(char* buf, int cap) {
    const std::string names = conv1_variant_names();
    if (!buf || cap <= (int)names.size()) return fail(LTK_E_INVALID, "buffer too small: " + std::to_string(names.size() + 1) + " bytes needed");
    memcpy(buf, names.c_str(), names.size() + 1);
    return LTK_OK;
}

namespace {
// plans of ltk_w2l_head_f16, freed on every return path
struct HeadPlansOwner {
    Conv7Plan* c7 = nullptr; Audio0Plan* a0 = nullptr; Audio3Plan* a3 = nullptr; ConvS2dPlan* s2 = nullptr;
    ~HeadPlansOwner() { conv7_plan_destroy(c7); audio0_plan_destroy(a0); audio3_plan_destroy(a3); convs2d_plan_destroy(s2); }
};
}  // namespace

int ltk_w2l_head_f16(ltk_engine* e, int op, const void* const* frame_ptrs, const void* d_x, int N, int H, int W, int Cin, int Cout,
                     const float* weight, const float* scale, const float* shift, void* d_y, const ltk_norm_opts* opts) {
    if (!e || !weight || !scale || !shift || !d_y || !opts || N <= 0 || op < LTK_W2L_CONV7_BANK || op > LTK_W2L_CONVS2D)
        return fail(LTK_E_INVALID, "bad arguments");
    const bool table = op == LTK_W2L_CONV7_BANK || op == LTK_W2L_AUDIO0;       // the per-frame inputs come through a pointer table
    if (table ? !frame_ptrs : !d_x) return fail(LTK_E_INVALID, "bad arguments");
    // the layers' own channel counts; CONVS2D's are the caller's (its plan refuses what it has no kernel for)
    const int Ci = op == LTK_W2L_CONVS2D ? Cin : op == LTK_W2L_AUDIO3 ? 32 : 0;
    const int Co = op == LTK_W2L_CONVS2D ? Cout : op == LTK_W2L_AUDIO3 ? 64 : op == LTK_W2L_AUDIO0 ? 32 : 16;
    if (Ci < 0 || Co <= 0) return fail(LTK_E_INVALID, "bad arguments");
    const bool x_view = op == LTK_W2L_AUDIO3 || op == LTK_W2L_CONVS2D;
    const int x_ld = opts->x_ld ? opts->x_ld : Ci, y_ld = opts->y_ld ? opts->y_ld : Co;
    if (!x_view && (opts->x_ld || opts->x_coff)) return fail(LTK_E_INVALID, "this op's input is no channel-blocked tensor: no view of x");
    if (opts->x_coff < 0 || opts->y_coff < 0 || (x_view && opts->x_coff + Ci > x_ld) || opts->y_coff + Co > y_ld)
        return fail(LTK_E_INVALID, "channel view outside its buffer");
    CHK(enter_device(e->device));
    { const int drc = drain_pending(e); if (drc) return drc; }
    std::string err;
    HeadPlansOwner po;
    int rc = 0;
    switch (op) {
        case LTK_W2L_CONV7_BANK: case LTK_W2L_CONV7_PACKED: rc = conv7_plan_create(&po.c7, weight, scale, shift, &err); break;
        case LTK_W2L_AUDIO0: rc = audio0_plan_create(&po.a0, weight, scale, shift, &err); break;
        case LTK_W2L_AUDIO3: rc = audio3_plan_create(&po.a3, weight, scale, shift, &err); break;
        default: rc = convs2d_plan_create(&po.s2, weight, Cin, Cout, scale, shift, &err); break;
    }
    if (rc) return conv_status(rc, err);
    // the table as the bank gather builds it: entry i = frame i's input, any order, repeats allowed (entries past N, and past the
    // table's capacity when the launcher is about to refuse N, stay null)
    DevBuf d_tab;
    if (table) {
        FacePtrs fp;
        memset(&fp, 0, sizeof(fp));
        for (int i = 0; i < std::min(N, kPackMaxFrames); ++i) fp.p[i] = (const uint8_t*)frame_ptrs[i];
        static_assert(sizeof(FacePtrs) == sizeof(MelPtrs), "one upload serves both tables");
        const int urc = upload(&fp, sizeof(fp), &d_tab);
        if (urc) return urc;
    }
    hipStream_t s = e->compute;
    std::lock_guard<std::mutex> g(e->mu);
    int lrc = 0;
    switch (op) {
        case LTK_W2L_CONV7_BANK: lrc = conv7_launch(po.c7, (const FacePtrs*)d_tab.p, nullptr, N, (f16*)d_y, y_ld, opts->y_coff, s, &err); break;
        case LTK_W2L_CONV7_PACKED: lrc = conv7_launch(po.c7, nullptr, (const f16*)d_x, N, (f16*)d_y, y_ld, opts->y_coff, s, &err); break;
        case LTK_W2L_AUDIO0: lrc = audio0_launch(po.a0, (const MelPtrs*)d_tab.p, N, (f16*)d_y, y_ld, opts->y_coff, s, &err); break;
        case LTK_W2L_AUDIO3: lrc = audio3_launch(po.a3, (const f16*)d_x, x_ld, opts->x_coff, N, (f16*)d_y, y_ld, opts->y_coff, s, &err); break;
        default: lrc = convs2d_launch(po.s2, (const f16*)d_x, x_ld, opts->x_coff, N, H, W, (f16*)d_y, y_ld, opts->y_coff, s, &err); break;
    }
    const hipError_t he = hipStreamSynchronize(s);      // the launch's error wins; the stream is drained either way
    if (lrc) return conv_status(lrc, err);
    if (he != hipSuccess) return fail(LTK_E_HIP, std::string("w2l head kernel: ") + hipGetErrorString(he));
    return LTK_OK;
}

namespace {
// ltk_groupnorm_f16 and ltk_groupnorm_f16_ex: one body.  `o` (may be NULL): the channel views; `rep` (may be NULL): what was launched.
int groupnorm_hook(ltk_engine* e, const void* d_x, int N, int C, int P, int groups, float eps, const float* gamma, const float* beta, int silu,
                   int impl, int out_fp8, float out_scale, void* d_y, int iters, float* ms_avg, const ltk_norm_opts* o, ltk_norm_report* rep) {
    if (!e || !d_x || !d_y || !gamma || !beta || N <= 0 || C <= 0 || P <= 0 || groups <= 0 || C % groups || C % 16 || (out_fp8 && C % 32))
        return fail(LTK_E_INVALID, "bad arguments");
    if (rep) memset(rep, 0, sizeof(*rep));
    const int yb = out_fp8 ? 32 : 16;                    // channels per block of y
    const int x_ld = (o && o->x_ld) ? o->x_ld : C, x_coff = o ? o->x_coff : 0, y_ld = (o && o->y_ld) ? o->y_ld : C, y_coff = o ? o->y_coff : 0;
    if (x_ld % 16 || x_coff % 16 || y_ld % yb || y_coff % yb) return fail(LTK_E_INVALID, "channel views are multiples of 16 channels (of 32 for an e4m3 output)");
    if (x_coff < 0 || y_coff < 0 || x_coff + C > x_ld || y_coff + C > y_ld) return fail(LTK_E_INVALID, "channel view outside its buffer");
    {   // the kernels read their shift from x while other blocks already store y: no GroupNorm in place
        const char *xa = (const char*)d_x, *ya = (const char*)d_y;
        const size_t xn = (size_t)N * (x_ld / 16) * P * 32, yn = (size_t)N * (y_ld / yb) * P * yb * (out_fp8 ? 1 : 2);
        if (xa < ya + yn && ya < xa + xn) return fail(LTK_E_INVALID, "GroupNorm: x and y overlap");
    }
    CHK(enter_device(e->device));
    const bool fits_group = gn_group_fits(C, P, groups);
    const int members = gn_coop_members(C, P, groups);
    if (impl == 0) impl = (knob(K_MT_GN1) && fits_group) ? 2 : (knob(K_GN_COOP) && members) ? 3 : 1;
    if ((impl == 2 && !fits_group) || (impl == 3 && !members) || impl < 1 || impl > 3) return fail(LTK_E_INVALID, "this GroupNorm kernel does not serve the shape");
    DevBuf gamma_buf, beta_buf, partial_buf, slots_buf;
    HostWord errw;
    const int segs = gn_segments(N, C, P);
    const size_t slot_words = (size_t)N * (C / 16) * std::max(members, 1) * 8;
    hipStream_t s = e->compute;
    std::lock_guard<std::mutex> g(e->mu);
    if (hipMalloc(&gamma_buf.p, C * sizeof(float)) != hipSuccess || hipMalloc(&beta_buf.p, C * sizeof(float)) != hipSuccess ||
        hipMalloc(&partial_buf.p, (size_t)N * (C / 16) * segs * 32 * sizeof(float)) != hipSuccess ||
        hipMalloc(&slots_buf.p, slot_words * sizeof(unsigned)) != hipSuccess || errw.create() != hipSuccess)
        return fail(LTK_E_HIP, "allocation failed");
    float *d_gamma = (float*)gamma_buf.p, *d_beta = (float*)beta_buf.p, *d_partial = (float*)partial_buf.p;
    unsigned *d_slots = (unsigned*)slots_buf.p, *err_dev = errw.dev;
    (void)hipMemcpyAsync(d_gamma, gamma, C * sizeof(float), hipMemcpyHostToDevice, s);
    (void)hipMemcpyAsync(d_beta, beta, C * sizeof(float), hipMemcpyHostToDevice, s);
    const f16* x = (const f16*)d_x;
    const int xcbt = x_ld / 16, xcb0 = x_coff / 16, ycbt = y_ld / yb, ycb0 = y_coff / yb;
    auto run = [&]() {
        if (impl == 3) {
            launch_gn_coop_reset(d_slots, slot_words, s);
            launch_gn_coop(x, N, xcbt, xcb0, C, P, groups, eps, d_slots, err_dev, d_gamma, d_beta, silu, (f16*)d_y, ycbt, ycb0, out_fp8 ? 1 : 0, out_scale, s);
        } else if (impl == 2) {
            launch_gn_group(x, N, xcbt, xcb0, C, P, groups, eps, d_gamma, d_beta, silu, (f16*)d_y, ycbt, ycb0, out_fp8 ? 1 : 0, out_scale, s);
        } else {
            launch_gn_stats(x, N, xcbt, xcb0, C, P, groups, segs, d_partial, s);
            if (out_fp8) launch_gn_apply_fp8(x, N, xcbt, xcb0, C, P, groups, eps, d_partial, segs, d_gamma, d_beta, silu, out_scale, (unsigned char*)d_y, ycbt, ycb0, s);
            else launch_gn_apply(x, N, xcbt, xcb0, C, P, groups, eps, d_partial, segs, d_gamma, d_beta, silu, (f16*)d_y, ycbt, ycb0, s);
        }
    };
    run();
    int rc = LTK_OK;
    if (iters > 0 && ms_avg) {
        float ms = 0.f;
        rc = time_iters(s, iters, [&]() { run(); return 0; }, &ms);
        *ms_avg = ms / iters;
    }
    const hipError_t he = hipStreamSynchronize(s);
    if (rc) return rc;
    if (he != hipSuccess || hipGetLastError() != hipSuccess) return fail(LTK_E_HIP, std::string("GroupNorm kernel: ") + hipGetErrorString(he));
    if (*reinterpret_cast<volatile unsigned*>(errw.host)) return fail(LTK_E_HIP, "a cooperative GroupNorm block gave up waiting for its set (gn_coop_kernel)");
    if (rep) {
        const char* f8 = out_fp8 ? "true" : "false";
        rep->impl = impl;
        if (impl == 3) {
            snprintf(rep->kernel, sizeof(rep->kernel), "gn_coop_kernel<%s>", f8);
            rep->members = members; rep->grid = N * (C / 16) * members;
        } else if (impl == 2) {
            const GnGroupVariant v = gn_group_variant(C, P, groups);
            snprintf(rep->kernel, sizeof(rep->kernel), "gn_group_kernel<%d,%d,%s>", v.kmax, v.nt, f8);
            rep->grid = N * groups;
        } else {
            snprintf(rep->kernel, sizeof(rep->kernel), "gn_stats_kernel+gn_apply_kernel<%s>", f8);
            rep->segs = segs; rep->grid = N * (C / 16) * ((P + 1023) / 1024);
        }
    }
    return LTK_OK;
}
}  // namespace

int ltk_groupnorm_f16(ltk_engine* e, const void* d_x, int N, int C, int P, int groups, float eps, const float* gamma, const float* beta,
                      int silu, int impl, int out_fp8, float out_scale, void* d_y, int iters, float* ms_avg) {
    return groupnorm_hook(e, d_x, N, C, P, groups, eps, gamma, beta, silu, impl, out_fp8, out_scale, d_y, iters, ms_avg, nullptr, nullptr);
}

int ltk_groupnorm_f16_ex(ltk_engine* e, const void* d_x, int N, int C, int P, int groups, float eps, const float* gamma, const float* beta,
                         int silu, int impl, int out_fp8, float out_scale, void* d_y, const ltk_norm_opts* opts, ltk_norm_report* rep) {
    if (!opts) return fail(LTK_E_INVALID, "bad arguments");
    return groupnorm_hook(e, d_x, N, C, P, groups, eps, gamma, beta, silu, impl, out_fp8, out_scale, d_y, 0, nullptr, opts, rep);
}

int ltk_pointwise_f16(ltk_engine* e, int op, const void* d_x, void* d_y, int N, int C, int P, float eps, const float* v0, const float* v1,
                      const ltk_norm_opts* opts) {
    if (!e || !d_y || !opts || N <= 0 || C <= 0 || P <= 0 || op < LTK_PW_LAYERNORM || op > LTK_PW_VAE_POST) return fail(LTK_E_INVALID, "bad arguments");
    if (op != LTK_PW_ADD_POS && !d_x) return fail(LTK_E_INVALID, "bad arguments");
    const bool f16_in = op <= LTK_PW_ACT_SILU || op == LTK_PW_VAE_POST;        // x is a channel-blocked fp16 tensor
    const bool whole = op <= LTK_PW_ACT_SILU;                                  // kernels over whole 16-channel blocks
    if (whole && C % 16) return fail(LTK_E_INVALID, "C must be a multiple of 16");
    if ((op == LTK_PW_LAYERNORM && (!v0 || !v1)) || (op == LTK_PW_ADD_POS && !v0)) return fail(LTK_E_INVALID, "bad arguments");
    if (op == LTK_PW_VAE_POST && (C != 3 || N > 64)) return fail(LTK_E_INVALID, "vae_post: 3 channels, at most 64 frames");
    const int Cp = (C + 15) / 16 * 16, Cx = op == LTK_PW_GEGLU ? 2 * C : Cp;   // channels the view spans in y / in x
    const int x_ld = opts->x_ld ? opts->x_ld : Cx, y_ld = opts->y_ld ? opts->y_ld : Cp;
    if (x_ld % 16 || opts->x_coff % 16 || y_ld % 16 || opts->y_coff % 16) return fail(LTK_E_INVALID, "channel views are multiples of 16 channels");
    if (opts->x_coff < 0 || opts->y_coff < 0 || (f16_in && opts->x_coff + Cx > x_ld) || (op != LTK_PW_VAE_POST && opts->y_coff + Cp > y_ld))
        return fail(LTK_E_INVALID, "channel view outside its buffer");
    if (op == LTK_PW_VAE_POST && opts->x_coff) return fail(LTK_E_INVALID, "vae_post reads the first channel block");
    if (op == LTK_PW_VAE_POST && N > 1 && (P * 3) % 4) return fail(LTK_E_INVALID, "vae_post: frames are packed, so P * 3 must be a multiple of 4 (whole blocks are stored as dwords)");
    CHK(enter_device(e->device));
    const size_t n0 = op == LTK_PW_LAYERNORM ? (size_t)C : (size_t)P * C;     // gamma | pos / add table
    DevBuf b0, b1;
    const bool takes_v0 = op == LTK_PW_LAYERNORM || op == LTK_PW_ADD_POS || op == LTK_PW_TOKENS_TO_CB16;      // the others ignore v0 / v1
    if (v0 && takes_v0) { const int rc = upload(v0, n0 * sizeof(float), &b0); if (rc) return rc; }
    if (v1 && op == LTK_PW_LAYERNORM) { const int rc = upload(v1, (size_t)C * sizeof(float), &b1); if (rc) return rc; }
    const f16* x = (const f16*)d_x;
    f16* y = (f16*)d_y;
    const int xcbt = x_ld / 16, xcb0 = opts->x_coff / 16, ycbt = y_ld / 16, ycb0 = opts->y_coff / 16;
    hipStream_t s = e->compute;
    std::lock_guard<std::mutex> g(e->mu);
    switch (op) {
        case LTK_PW_LAYERNORM: launch_layernorm(x, N, xcbt, xcb0, C, P, eps, (const float*)b0.p, (const float*)b1.p, y, ycbt, ycb0, s); break;
        case LTK_PW_GEGLU: launch_geglu(x, N, xcbt, xcb0, C, P, y, ycbt, ycb0, s); break;
        case LTK_PW_ACT_GELU: launch_act(x, N, xcbt, xcb0, C, P, 2, y, ycbt, ycb0, s); break;
        case LTK_PW_ACT_SILU: launch_act(x, N, xcbt, xcb0, C, P, 3, y, ycbt, ycb0, s); break;
        case LTK_PW_ADD_POS: launch_add_pos(y, N, ycbt, ycb0, C, P, (const float*)b0.p, s); break;
        case LTK_PW_NCHW_TO_CB16: launch_nchw_to_cb16((const float*)d_x, N, C, P, y, ycbt, ycb0, s); break;
        case LTK_PW_TOKENS_TO_CB16: launch_tokens_to_cb16((const float*)d_x, N, P, C, (const float*)b0.p, y, ycbt, ycb0, s); break;
        default: {
            OutList64 outs;
            for (int i = 0; i < 64; ++i) outs.p[i] = i < N ? (uint8_t*)d_y + (size_t)i * P * 3 : nullptr;
            launch_vae_post(x, xcbt, N, P, outs, nullptr, s);
        }
    }
    const hipError_t le = hipGetLastError(), se = hipStreamSynchronize(s);       // before the uploaded vectors go
    if (le != hipSuccess || se != hipSuccess) return fail(LTK_E_HIP, std::string("pointwise kernel: ") + hipGetErrorString(le != hipSuccess ? le : se));
    return LTK_OK;
}

int ltk_attention_f16(ltk_engine* e, const void* d_q, int q_cbt, int q_cb0, const void* d_k, int k_cbt, int k_cb0, const void* d_v, int v_cbt,
                      int v_cb0, void* d_o, int o_cbt, int o_cb0, int N, int heads, int d16, int Tq, int Tk, int impl) {
    if (!e || !d_q || !d_k || !d_v || !d_o || N <= 0 || heads <= 0 || Tq <= 0 || Tk <= 0) return fail(LTK_E_INVALID, "bad arguments");
    if (d16 != 48 && d16 != 64 && d16 != 80 && d16 != 160 && d16 != 512) return fail(LTK_E_INVALID, "attention: d16 must be 48, 64, 80, 160 or 512");
    const int hcb = heads * (d16 / 16);
    if (q_cb0 < 0 || k_cb0 < 0 || v_cb0 < 0 || o_cb0 < 0 || q_cb0 + hcb > q_cbt || k_cb0 + hcb > k_cbt || v_cb0 + hcb > v_cbt || o_cb0 + hcb > o_cbt)
        return fail(LTK_E_INVALID, "attention: the heads do not fit the buffer's channel blocks");
    if (N > 65535 || heads > 65535 || (double)N * std::max(std::max(q_cbt, o_cbt), std::max(k_cbt, v_cbt)) * 16.0 * std::max(Tq, Tk) >= 2147483647.0)
        return fail(LTK_E_INVALID, "attention: tensor too large");
    if (impl < 0 || impl > 2 || (impl == 2 && !attn_lds_serves(d16, Tk))) return fail(LTK_E_INVALID, "this attention kernel does not serve the shape");
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    DevBuf vt;
    CHK(hipMalloc(&vt.p, (size_t)N * heads * attn_dv32(d16) * attn_tkp(Tk) * sizeof(f16)));
    hipStream_t s = e->compute;
    launch_v_transpose((const f16*)d_v, N, v_cbt, v_cb0, heads, d16, Tk, (f16*)vt.p, s);
    hipError_t le = hipGetLastError();
    const int rc = le == hipSuccess ? launch_attention((const f16*)d_q, q_cbt, q_cb0, Tq, (const f16*)d_k, k_cbt, k_cb0, Tk, (const f16*)vt.p, (f16*)d_o,
                                                       o_cbt, o_cb0, N, heads, d16, s, impl) : 0;
    const hipError_t se = hipStreamSynchronize(s);       // before the V^T scratch goes
    if (le != hipSuccess || se != hipSuccess) return fail(LTK_E_HIP, std::string("attention kernel: ") + hipGetErrorString(le != hipSuccess ? le : se));
    if (rc) return conv_status(rc, "attention launch failed (head dim " + std::to_string(d16) + ")");
    return LTK_OK;
}

// ------------------------------------------------------------------ Ultralight hooks
int ltk_ultralight_forward_host(ltk_engine* e, int avatar_id, const float* img6, const float* feat, int B, float* pred) {
    if (!e || !img6 || !feat || !pred || B <= 0) return fail(LTK_E_INVALID, "bad arguments");
    const std::shared_ptr<UlAvatar> ap = find_ul_avatar(e, avatar_id);
    if (!ap) return fail(LTK_E_STATE, "unknown Ultralight avatar id");
    CHK(enter_device(e->device));
    constexpr size_t P = (size_t)kUlRes * kUlRes;
    std::lock_guard<std::mutex> g(e->mu);
    const int cap = std::min(std::min(e->ul_frames, kPackMaxFrames), B);
    if (cap <= 0) return fail(LTK_E_STATE, "no Ultralight arena");
    if (e->capture && B > cap) return fail(LTK_E_INVALID, "layer capture needs B <= max_frames");
    DevBuf d_img, d_feat, d_pred;
    CHK(hipMalloc(&d_img.p, cap * 6 * P * sizeof(float)));
    CHK(hipMalloc(&d_feat.p, (size_t)cap * 16 * 1024 * sizeof(float)));
    CHK(hipMalloc(&d_pred.p, cap * 3 * P * sizeof(float)));
    for (int f0 = 0; f0 < B; f0 += cap) {
        const int nf = std::min(cap, B - f0);
        CHK(hipMemcpy(d_img.p, img6 + f0 * 6 * P, nf * 6 * P * sizeof(float), hipMemcpyHostToDevice));
        CHK(hipMemcpy(d_feat.p, feat + (size_t)f0 * 16 * 1024, (size_t)nf * 16 * 1024 * sizeof(float), hipMemcpyHostToDevice));
        MelPtrs mp;
        for (int i = 0; i < nf; ++i) mp.p[i] = (const float*)d_feat.p + (size_t)i * 16 * 1024;
        launch_upload_tables(nullptr, &mp, nullptr, nf, e->ul_tab, e->compute);
        CHK(hipGetLastError());
        UlPassArgs args;
        args.d_img6 = (const float*)d_img.p; args.d_pred_f32 = (float*)d_pred.p;
        const int rc = ul_pass(e, *ap, nf, args);
        const hipError_t se = hipStreamSynchronize(e->compute);
        if (rc) return rc;
        if (se != hipSuccess) return fail(LTK_E_HIP, std::string("ultralight forward: ") + hipGetErrorString(se));
        CHK(hipMemcpy(pred + f0 * 3 * P, d_pred.p, nf * 3 * P * sizeof(float), hipMemcpyDeviceToHost));
    }
    return LTK_OK;
}

int ltk_ultralight_time(ltk_engine* e, int avatar_id, int frames, int iters, float* ms_per_pass, double* macs_per_pass) {
    if (!e || frames <= 0 || iters <= 0 || !ms_per_pass) return fail(LTK_E_INVALID, "bad arguments");
    const std::shared_ptr<UlAvatar> ap = find_ul_avatar(e, avatar_id);
    if (!ap) return fail(LTK_E_STATE, "unknown Ultralight avatar id");
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    if (e->capture) return fail(LTK_E_STATE, "disable capture before timing");
    if (frames > e->ul_frames || frames > kPackMaxFrames) return fail(LTK_E_INVALID, "frames exceeds max_frames");
    // every frame reads the avatar's first bank crop and one zero chunk and writes its own scratch frame: the pass as
    // ltk_ultralight_infer enqueues it
    DevBuf d_feat, d_frames;
    CHK(hipMalloc(&d_feat.p, 16 * 1024 * sizeof(float)));
    CHK(hipMemset(d_feat.p, 0, 16 * 1024 * sizeof(float)));
    CHK(hipMalloc(&d_frames.p, (size_t)frames * kUlRes * kUlRes * 3));
    FacePtrs fp; MelPtrs mp; OutPtrs op;
    for (int i = 0; i < frames; ++i) { fp.p[i] = ap->d_face; mp.p[i] = (const float*)d_feat.p; op.p[i] = (uint8_t*)d_frames.p + (size_t)i * kUlRes * kUlRes * 3; }
    launch_upload_tables(&fp, &mp, &op, frames, e->ul_tab, e->compute);
    CHK(hipGetLastError());
    int rc = ul_pass(e, *ap, frames);      // eager
    if (!rc) rc = ul_pass(e, *ap, frames); // captures under knob GRAPH
    float ms = 0.f;
    if (!rc) rc = time_iters(e->compute, iters, [&]() { return ul_pass(e, *ap, frames); }, &ms);
    const hipError_t se = hipStreamSynchronize(e->compute);       // before the scratch buffers go
    if (rc) return rc;
    if (se != hipSuccess) return fail(LTK_E_HIP, std::string("ultralight pass: ") + hipGetErrorString(se));
    *ms_per_pass = ms / iters;
    if (macs_per_pass) *macs_per_pass = ul_macs_per_frame() * frames;
    return LTK_OK;
}

int ltk_dwconv3x3_f16(ltk_engine* e, const void* d_x, int N, int H, int W, int C, const float* weight, int stride, const float* scale,
                      const float* shift, int relu, void* d_y) {
    if (!e || !d_x || !weight || !d_y || N <= 0 || H <= 0 || W <= 0 || C <= 0) return fail(LTK_E_INVALID, "bad arguments");
    if (C % 16 || (stride != 1 && stride != 2)) return fail(LTK_E_INVALID, "depthwise conv: C % 16 == 0, stride 1 or 2");
    if ((long long)N * (C / 16) > 65535 || (double)N * C * H * W >= 2147483647.0) return fail(LTK_E_INVALID, "depthwise conv: tensor too large");
    CHK(enter_device(e->device));
    std::vector<float> h((size_t)C * 11);
    dw_pack(weight, scale, shift, C, C, h.data());
    DevBuf d_w;
    const int rc = upload(h.data(), h.size() * sizeof(float), &d_w);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(e->mu);
    const float* w = (const float*)d_w.p;
    launch_dwconv3x3((const f16*)d_x, N, C / 16, 0, C, H, W, stride, w, w + (size_t)C * 9, w + (size_t)C * 10, relu, (f16*)d_y, C / 16, 0, e->compute);
    const hipError_t le = hipGetLastError();
    const hipError_t se = hipStreamSynchronize(e->compute);
    if (le != hipSuccess || se != hipSuccess) return fail(LTK_E_HIP, std::string("depthwise conv kernel: ") + hipGetErrorString(le != hipSuccess ? le : se));
    return LTK_OK;
}

int ltk_ul_gconv_f16(ltk_engine* e, const void* d_x, int N, int H, int W, int Cin, const float* weight, int n_sets, const int32_t* set,
                     int Cout, int k, int stride, int pad, const float* scale, const float* shift, const void* d_res, int relu, void* d_y,
                     const ltk_conv_opts* opts, ltk_conv_report* rep) {
    // what the host alone can refuse comes first (also with no engine): the shape, the views, the set indices
    if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || n_sets <= 0) return fail(LTK_E_INVALID, "bad arguments");
    if (opts && (opts->act || opts->ups || opts->force_pxw || opts->force_nbt || opts->force_ksplit || opts->family))
        return fail(LTK_E_INVALID, "ul_gconv: only the channel views of the options apply");
    UlGconvIO io;
    io.N = N; io.H = H; io.W = W; io.Cin = Cin; io.Cout = Cout; io.k = k; io.stride = stride; io.pad = pad; io.relu = relu ? 1 : 0;
    io.x_ld = opts && opts->x_ld ? opts->x_ld : Cin; io.x_coff = opts ? opts->x_coff : 0;
    io.y_ld = opts && opts->y_ld ? opts->y_ld : Cout; io.y_coff = opts ? opts->y_coff : 0;
    io.res_ld = opts && opts->res_ld ? opts->res_ld : Cout; io.res_coff = opts ? opts->res_coff : 0;
    io.x = (const f16*)d_x; io.y = (f16*)d_y; io.res = (const f16*)d_res;
    UlGconvGeom geo;
    std::string err;
    if (ul_gconv_geom(io, &geo, &err)) return fail(LTK_E_INVALID, err);
    if (!set) return fail(LTK_E_INVALID, "bad arguments");
    for (int n = 0; n < N; ++n)
        if (set[n] < 0 || set[n] >= n_sets) return fail(LTK_E_INVALID, "ul_gconv: image " + std::to_string(n) + " names a weight set outside [0, n_sets)");
    if (rep) {
        memset(rep, 0, sizeof(*rep));
        snprintf(rep->kernel, sizeof(rep->kernel), "%s", ul_gconv_kernel_name());
        rep->PXW = geo.tile_px; rep->NBT = geo.tile_co; rep->T = geo.ksteps; rep->S = stride; rep->grid = geo.blocks;
        rep->items = geo.grid_x * 65536 + geo.grid_y; rep->NB = geo.grid_z;
    }
    if (!e || !d_x || !weight || !d_y) return fail(LTK_E_INVALID, "bad arguments");
    CHK(enter_device(e->device));
    // one record per weight set, as an avatar's (op 0), and the per-image table
    const size_t wh = ul_gconv_pack(nullptr, Cin, Cout, k, nullptr), wsz = (size_t)Cout * Cin * k * k;
    std::vector<f16> packed(wh * n_sets);
    std::vector<float> ss((size_t)2 * Cout * n_sets);
    for (int i = 0; i < n_sets; ++i) {
        ul_gconv_pack(weight + i * wsz, Cin, Cout, k, packed.data() + i * wh);
        for (int c = 0; c < Cout; ++c) {
            ss[((size_t)2 * i) * Cout + c] = scale ? scale[(size_t)i * Cout + c] : 1.f;
            ss[((size_t)2 * i + 1) * Cout + c] = shift ? shift[(size_t)i * Cout + c] : 0.f;
        }
    }
    DevBuf d_w, d_ss, d_rec, d_tab;
    int rc = upload(packed.data(), packed.size() * sizeof(f16), &d_w);
    if (!rc) rc = upload(ss.data(), ss.size() * sizeof(float), &d_ss);
    if (rc) return rc;
    std::vector<UlGroupW> recs(n_sets);
    memset(recs.data(), 0, recs.size() * sizeof(UlGroupW));
    for (int i = 0; i < n_sets; ++i) {
        recs[i].op[0].w = (const f16*)d_w.p + i * wh;
        recs[i].op[0].scale = (const float*)d_ss.p + ((size_t)2 * i) * Cout;
        recs[i].op[0].shift = (const float*)d_ss.p + ((size_t)2 * i + 1) * Cout;
    }
    rc = upload(recs.data(), recs.size() * sizeof(UlGroupW), &d_rec);
    if (rc) return rc;
    CHK(hipMalloc(&d_tab.p, sizeof(UlGroupTab)));
    UlGroupTab tab;
    memset(&tab, 0, sizeof(tab));
    for (int n = 0; n < N; ++n) tab.w[n] = (const UlGroupW*)d_rec.p + set[n];
    std::lock_guard<std::mutex> g(e->mu);
    hipStream_t s = e->compute;
    launch_upload_group_table(&tab, N, (UlGroupTab*)d_tab.p, s);
    hipError_t le = hipGetLastError();
    const int lrc = le == hipSuccess ? launch_ul_gconv((const UlGroupTab*)d_tab.p, 0, io, s, &err) : 0;
    const hipError_t se = hipStreamSynchronize(s);          // before the operands go
    if (lrc) return conv_status(lrc, err);
    if (le != hipSuccess || se != hipSuccess) return fail(LTK_E_HIP, std::string("ul_gconv kernel: ") + hipGetErrorString(le != hipSuccess ? le : se));
    return LTK_OK;
}

namespace {

// the planner's answer for a hook call: 0 with *rep the plan, or -1 with rep->reason (and *err) the refusal
int ul_ir_hook_plan(ltk::UlIrIO* io, int N, int H, int W, int Cin, int mid, int Cout, int stride, int has_res, bool tap, const ltk_conv_opts* opts,
                    ltk_ul_ir_report* rep, std::string* err) {
    using namespace ltk;
    io->N = N; io->H = H; io->W = W; io->Cin = Cin; io->mid = mid; io->Cout = Cout; io->stride = stride; io->has_res = has_res ? 1 : 0;
    io->x_ld = opts && opts->x_ld ? opts->x_ld : Cin; io->x_coff = opts ? opts->x_coff : 0;
    io->y_ld = opts && opts->y_ld ? opts->y_ld : Cout; io->y_coff = opts ? opts->y_coff : 0;
    io->res_ld = opts && opts->res_ld ? opts->res_ld : Cout; io->res_coff = opts ? opts->res_coff : 0;
    UlIrPlan pl;
    int rc;
    if (opts && (opts->act || opts->ups || opts->force_pxw || opts->force_nbt || opts->force_ksplit || opts->family)) {
        *err = "ul_ir: only the channel views of the options apply";
        memset(&pl, 0, sizeof(pl));
        rc = -1;
    } else {
        rc = ul_ir_plan(*io, tap, &pl, err);
    }
    if (rep) {
        memset(rep, 0, sizeof(*rep));
        if (rc) {
            snprintf(rep->reason, sizeof(rep->reason), "%s", err->c_str());
        } else {
            snprintf(rep->kernel, sizeof(rep->kernel), "%s", pl.kernel);
            rep->accepted = 1;
            rep->Ho = pl.Ho; rep->Wo = pl.Wo; rep->TH = pl.TH; rep->TW = pl.TW; rep->MC = pl.MC; rep->chunks = pl.chunks;
            rep->hidden_px = pl.hidden_px; rep->lds_bytes = pl.lds_bytes; rep->lds_limit = pl.lds_limit;
            rep->grid_x = pl.grid_x; rep->grid_y = pl.grid_y; rep->grid_z = pl.grid_z; rep->blocks = pl.blocks; rep->threads = pl.threads;
        }
    }
    return rc;
}

}  // namespace

int ltk_debug_ul_ir_plan(int N, int H, int W, int Cin, int mid, int Cout, int stride, int has_res, int tap, const ltk_conv_opts* opts,
                         ltk_ul_ir_report* rep) {
    if (!rep) return fail(LTK_E_INVALID, "bad arguments");
    ltk::UlIrIO io;
    std::string err;
    if (ul_ir_hook_plan(&io, N, H, W, Cin, mid, Cout, stride, has_res, tap != 0, opts, rep, &err)) (void)fail(LTK_E_INVALID, err);
    return LTK_OK;
}

int ltk_ul_ir_f16(ltk_engine* e, const void* d_x, int N, int H, int W, int Cin, int mid, int Cout, int stride, const float* w1,
                  const float* wd, const float* w2, const float* scale1, const float* shift1, const float* scale_d, const float* shift_d,
                  const float* scale2, const float* shift2, const void* d_res, void* d_y, const ltk_conv_opts* opts, void* d_e1, void* d_e2,
                  ltk_ul_ir_report* rep) {
    // the planner first, on the host alone (also with no engine): what it refuses is refused before anything is allocated or launched
    UlIrIO io;
    std::string err;
    if (ul_ir_hook_plan(&io, N, H, W, Cin, mid, Cout, stride, d_res != nullptr, d_e1 || d_e2, opts, rep, &err)) return fail(LTK_E_INVALID, err);
    if ((d_e1 == nullptr) != (d_e2 == nullptr)) return fail(LTK_E_INVALID, "ul_ir: both tap buffers or neither");
    if (!e || !d_x || !w1 || !wd || !w2 || !d_y) return fail(LTK_E_INVALID, "bad arguments");
    CHK(enter_device(e->device));
    size_t off[4];
    std::vector<uint8_t> img(ul_ir_pack(nullptr, nullptr, nullptr, Cin, mid, Cout, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, off));
    ul_ir_pack(w1, wd, w2, Cin, mid, Cout, scale1, shift1, scale_d, shift_d, scale2, shift2, img.data(), off);
    DevBuf d_w;
    const int rc = upload(img.data(), img.size(), &d_w);
    if (rc) return rc;
    io.x = (const f16*)d_x; io.y = (f16*)d_y; io.res = (const f16*)d_res; io.e1 = (f16*)d_e1; io.e2 = (f16*)d_e2;
    std::lock_guard<std::mutex> g(e->mu);
    hipStream_t s = e->compute;
    const int lrc = launch_ul_ir(ul_ir_weights((const uint8_t*)d_w.p, off), io, s, nullptr, &err);
    const hipError_t se = hipStreamSynchronize(s);          // before the operands go
    if (lrc) return conv_status(lrc, err);
    if (se != hipSuccess) return fail(LTK_E_HIP, std::string("ul_ir kernel: ") + hipGetErrorString(se));
    return LTK_OK;
}

int ltk_upsample2x_cat_f16(ltk_engine* e, const void* d_x, int N, int h, int w, int C_up, const void* d_skip, int Hs, int Ws, int C_skip,
                           void* d_y) {
    if (!e || !d_x || !d_skip || !d_y || N <= 0 || h <= 0 || w <= 0 || C_up <= 0 || C_skip <= 0) return fail(LTK_E_INVALID, "bad arguments");
    if (C_up % 16 || C_skip % 16) return fail(LTK_E_INVALID, "upsample + concat: channel counts must be multiples of 16");
    if (Hs != 2 * h || Ws != 2 * w) return fail(LTK_E_INVALID, "upsample + concat: the skip tensor must be 2h x 2w");
    const int CT = C_up + C_skip;
    if ((long long)N * (C_up / 16) > 65535 || (double)N * CT * Hs * Ws >= 2147483647.0) return fail(LTK_E_INVALID, "upsample + concat: tensor too large");
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    hipStream_t s = e->compute;
    launch_upsample2x((const f16*)d_x, N, C_up / 16, 0, C_up, h, w, (f16*)d_y, CT / 16, 0, s);
    hipError_t le = hipGetLastError();
    // the skip half: image n's C_skip x Hs x Ws halfs behind its upsampled channels
    const size_t row = (size_t)C_skip * Hs * Ws * sizeof(f16), pitch = (size_t)CT * Hs * Ws * sizeof(f16);
    if (le == hipSuccess)
        le = hipMemcpy2DAsync((char*)d_y + (size_t)C_up * Hs * Ws * sizeof(f16), pitch, d_skip, row, row, (size_t)N, hipMemcpyDeviceToDevice, s);
    const hipError_t se = hipStreamSynchronize(s);
    if (le != hipSuccess || se != hipSuccess) return fail(LTK_E_HIP, std::string("upsample + concat: ") + hipGetErrorString(le != hipSuccess ? le : se));
    return LTK_OK;
}

namespace {

// the channel views of a face-parser hook: channels -> channel blocks, LTK_OK or the refusal
struct ParseViews { int x_cbt, x_cb0, y_cbt, y_cb0, r_cbt, r_cb0; };
int parse_views(const ltk_conv_opts* o, int Cx, int Cy, ParseViews* v, const std::string& who = "face parser op") {
    if (o && (o->act || o->ups || o->force_pxw || o->force_nbt || o->force_ksplit || o->family))
        return fail(LTK_E_INVALID, who + ": only the channel views of the options apply");
    if (Cx <= 0 || Cx % 16) return fail(LTK_E_INVALID, who + ": C % 16 == 0");
    const int x_ld = o && o->x_ld ? o->x_ld : Cx, y_ld = o && o->y_ld ? o->y_ld : Cy, r_ld = o && o->res_ld ? o->res_ld : Cy;
    const int x_coff = o ? o->x_coff : 0, y_coff = o ? o->y_coff : 0, r_coff = o ? o->res_coff : 0;
    if ((x_ld | x_coff | y_ld | y_coff | r_ld | r_coff) & 15) return fail(LTK_E_INVALID, who + ": channel views are multiples of 16 channels");
    *v = ParseViews{x_ld / 16, x_coff / 16, y_ld / 16, y_coff / 16, r_ld / 16, r_coff / 16};
    return LTK_OK;
}

// what every one of these hooks does behind its launch: the launcher's refusal, the launch error, the stream's
int parse_finish(ltk_engine* e, int lrc, const std::string& err, const char* what) {
    const hipError_t le = hipGetLastError();
    const hipError_t se = hipStreamSynchronize(e->compute);          // before the operands go
    if (lrc) return conv_status(lrc, err);
    if (le != hipSuccess || se != hipSuccess) return fail(LTK_E_HIP, std::string(what) + ": " + hipGetErrorString(le != hipSuccess ? le : se));
    return LTK_OK;
}

}  // namespace

int ltk_parse_stem_f16(ltk_engine* e, const void* d_rgb, int N, int H, int W, const float* weight, const float* scale, const float* shift,
                       void* d_y, const ltk_conv_opts* opts) {
    if (!e || !d_rgb || !weight || !d_y) return fail(LTK_E_INVALID, "bad arguments");
    ParseViews v;
    { const int rc = parse_views(opts, 16, kStemCout, &v); if (rc) return rc; }
    CHK(enter_device(e->device));
    std::vector<f16> wq(kStemWHalfs);
    parse_stem_pack(weight, wq.data());
    std::vector<float> ss(2 * kStemCout);
    for (int c = 0; c < kStemCout; ++c) { ss[c] = scale ? scale[c] : 1.f; ss[kStemCout + c] = shift ? shift[c] : 0.f; }
    DevBuf d_w, d_ss;
    int rc = upload(wq.data(), wq.size() * sizeof(f16), &d_w);
    if (!rc) rc = upload(ss.data(), ss.size() * sizeof(float), &d_ss);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(e->mu);
    std::string err;
    const int lrc = launch_parse_stem((const uint8_t*)d_rgb, N, H, W, (const f16*)d_w.p, (const float*)d_ss.p, (const float*)d_ss.p + kStemCout,
                                      (f16*)d_y, v.y_cbt, v.y_cb0, e->compute, &err);
    return parse_finish(e, lrc, err, "parse stem kernel");
}

int ltk_maxpool3x3s2_f16(ltk_engine* e, const void* d_x, int N, int H, int W, int C, void* d_y, const ltk_conv_opts* opts) {
    if (!e || !d_x || !d_y) return fail(LTK_E_INVALID, "bad arguments");
    ParseViews v;
    { const int rc = parse_views(opts, C, C, &v); if (rc) return rc; }
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    std::string err;
    const int lrc = launch_maxpool3x3s2((const f16*)d_x, N, v.x_cbt, v.x_cb0, C, H, W, (f16*)d_y, v.y_cbt, v.y_cb0, e->compute, &err);
    return parse_finish(e, lrc, err, "maxpool kernel");
}

int ltk_global_avgpool_f16(ltk_engine* e, const void* d_x, int N, int P, int C, void* d_y, const ltk_conv_opts* opts) {
    if (!e || !d_x || !d_y) return fail(LTK_E_INVALID, "bad arguments");
    ParseViews v;
    { const int rc = parse_views(opts, C, C, &v); if (rc) return rc; }
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    std::string err;
    const int lrc = launch_gap((const f16*)d_x, N, v.x_cbt, v.x_cb0, C, P, (f16*)d_y, v.y_cbt, v.y_cb0, e->compute, &err);
    return parse_finish(e, lrc, err, "global average pool kernel");
}

int ltk_chan_gate_f16(ltk_engine* e, const void* d_x, int N, int P, int C, const void* d_a, const void* d_b, const void* d_r, int plus1,
                      void* d_y, const ltk_conv_opts* opts) {
    if (!e || !d_x || !d_a || !d_y) return fail(LTK_E_INVALID, "bad arguments");
    ParseViews v;
    { const int rc = parse_views(opts, C, C, &v); if (rc) return rc; }
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    std::string err;
    const int lrc = launch_chan_gate((const f16*)d_x, N, v.x_cbt, v.x_cb0, C, P, (const f16*)d_a, (const f16*)d_b, (const f16*)d_r, v.r_cbt, v.r_cb0,
                                     plus1, (f16*)d_y, v.y_cbt, v.y_cb0, e->compute, &err);
    return parse_finish(e, lrc, err, "channel gate kernel");
}

int ltk_seg_argmax_f16(ltk_engine* e, const void* d_x, int N, int h, int w, void* d_labels) {
    if (!e || !d_x || !d_labels) return fail(LTK_E_INVALID, "bad arguments");
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    std::string err;
    const int lrc = launch_seg_argmax((const f16*)d_x, N, h, w, (uint8_t*)d_labels, e->compute, &err);
    return parse_finish(e, lrc, err, "seg argmax kernel");
}

int ltk_debug_face_parse_program(int size, ltk_fp_op_info* ops, int max_ops, int* n_ops) {
    if (!ops || !n_ops || max_ops <= 0) return fail(LTK_E_INVALID, "bad arguments");
    const std::vector<FpOp> prog = fp_program(size);
    if (prog.empty()) return fail(LTK_E_INVALID, "face parser: size must be a multiple of 32 in [64, 512]");
    if ((int)prog.size() > max_ops) return fail(LTK_E_INVALID, "face parser: the program has " + std::to_string(prog.size()) + " ops");
    for (size_t i = 0; i < prog.size(); ++i) {
        const FpOp& p = prog[i];
        ltk_fp_op_info& o = ops[i];
        memset(&o, 0, sizeof(o));
        snprintf(o.name, sizeof(o.name), "%s", p.name.c_str());
        o.type = p.type; o.cin = p.cin; o.cout = p.cout; o.k = p.k; o.stride = p.stride; o.pad = p.pad; o.relu = p.relu; o.ups = p.ups;
        o.has_res = p.has_res; o.plus1 = p.plus1; o.H = p.H; o.W = p.W; o.Ho = p.Ho; o.Wo = p.Wo;
    }
    *n_ops = (int)prog.size();
    return LTK_OK;
}

int ltk_debug_face_parse_plan(int size, int max_images, ltk_fp_bind* ops, int max_ops, int* n_ops, unsigned long long* buf_bytes,
                              int max_bufs, int* n_bufs, int* image_buf, int* label_buf) {
    if (!ops || !n_ops || !buf_bytes || !n_bufs || !image_buf || !label_buf || max_ops <= 0 || max_bufs <= 0) return fail(LTK_E_INVALID, "bad arguments");
    FpPlan pl;
    std::string err;
    if (fp_plan(size, max_images, &pl, &err)) return fail(LTK_E_INVALID, err);
    if ((int)pl.ops.size() > max_ops) return fail(LTK_E_INVALID, "face parser: the program has " + std::to_string(pl.ops.size()) + " ops");
    if ((int)pl.buf_bytes.size() > max_bufs) return fail(LTK_E_INVALID, "face parser: the program has " + std::to_string(pl.buf_bytes.size()) + " buffers");
    auto view = [](const FpView& v) { return ltk_fp_view{v.buf, v.ld, v.coff, v.C, v.H, v.W}; };
    for (size_t i = 0; i < pl.ops.size(); ++i) {
        ltk_fp_bind& o = ops[i];
        memset(&o, 0, sizeof(o));
        snprintf(o.name, sizeof(o.name), "%s", pl.ops[i].name.c_str());
        const FpBind& b = pl.bind[i];
        o.x = view(b.x); o.y = view(b.y); o.r = view(b.r); o.a = view(b.a); o.b = view(b.b);
    }
    for (size_t i = 0; i < pl.buf_bytes.size(); ++i) buf_bytes[i] = (unsigned long long)pl.buf_bytes[i];
    *n_ops = (int)pl.ops.size(); *n_bufs = (int)pl.buf_bytes.size();
    *image_buf = pl.image_buf; *label_buf = pl.label_buf;
    return LTK_OK;
}

// ---- the face detector's own ops (s3fd_kernels.h) and its launch list (facedet.h)
int ltk_s3fd_stem_f16(ltk_engine* e, const void* d_bgr, int N, int H, int W, const float* weight, const float* bias, void* d_y,
                      const ltk_conv_opts* opts) {
    if (!e || !d_bgr || !weight || !d_y) return fail(LTK_E_INVALID, "bad arguments");
    ParseViews v;
    { const int rc = parse_views(opts, 16, kFdStemCout, &v, "face detector op"); if (rc) return rc; }
    CHK(enter_device(e->device));
    std::vector<f16> wq(kFdStemWHalfs);
    s3fd_stem_pack(weight, wq.data());
    std::vector<float> bs(kFdStemCout);
    for (int c = 0; c < kFdStemCout; ++c) bs[c] = bias ? bias[c] : 0.f;
    DevBuf d_w, d_b;
    int rc = upload(wq.data(), wq.size() * sizeof(f16), &d_w);
    if (!rc) rc = upload(bs.data(), bs.size() * sizeof(float), &d_b);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(e->mu);
    std::string err;
    const int lrc = launch_s3fd_stem((const uint8_t*)d_bgr, N, H, W, (const f16*)d_w.p, (const float*)d_b.p, (f16*)d_y, v.y_cbt, v.y_cb0, e->compute, &err);
    return parse_finish(e, lrc, err, "s3fd stem kernel");
}

int ltk_maxpool2x2s2_f16(ltk_engine* e, const void* d_x, int N, int H, int W, int C, void* d_y, const ltk_conv_opts* opts) {
    if (!e || !d_x || !d_y) return fail(LTK_E_INVALID, "bad arguments");
    ParseViews v;
    { const int rc = parse_views(opts, C, C, &v, "face detector op"); if (rc) return rc; }
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    std::string err;
    const int lrc = launch_maxpool2x2s2((const f16*)d_x, N, v.x_cbt, v.x_cb0, C, H, W, (f16*)d_y, v.y_cbt, v.y_cb0, e->compute, &err);
    return parse_finish(e, lrc, err, "maxpool 2x2 kernel");
}

int ltk_l2norm_f16(ltk_engine* e, const void* d_x, int N, int P, int C, const float* weight, void* d_y, const ltk_conv_opts* opts) {
    if (!e || !d_x || !weight || !d_y) return fail(LTK_E_INVALID, "bad arguments");
    ParseViews v;
    { const int rc = parse_views(opts, C, C, &v, "face detector op"); if (rc) return rc; }
    CHK(enter_device(e->device));
    DevBuf d_w;
    { const int rc = upload(weight, (size_t)C * sizeof(float), &d_w); if (rc) return rc; }
    std::lock_guard<std::mutex> g(e->mu);
    std::string err;
    const int lrc = launch_l2norm((const f16*)d_x, N, v.x_cbt, v.x_cb0, C, P, (const float*)d_w.p, (f16*)d_y, v.y_cbt, v.y_cb0, e->compute, &err);
    return parse_finish(e, lrc, err, "l2norm kernel");
}

int ltk_s3fd_detect_f16(ltk_engine* e, const void* d_x, int N, int H, int W, int maxout, int level, float thresh, void* d_recs, int cap,
                        void* d_counts, const ltk_conv_opts* opts) {
    if (!e || !d_x || !d_recs || !d_counts) return fail(LTK_E_INVALID, "bad arguments");
    ParseViews v;
    { const int rc = parse_views(opts, 16, 16, &v, "face detector op"); if (rc) return rc; }
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    std::string err;
    const int lrc = launch_s3fd_detect((const f16*)d_x, N, v.x_cbt, v.x_cb0, H, W, maxout, level, thresh, nullptr, (uint32_t*)d_recs, cap, (uint32_t*)d_counts,
                                       e->compute, &err);
    return parse_finish(e, lrc, err, "s3fd detect kernel");
}

int ltk_debug_face_detect_program(int H, int W, ltk_fd_op_info* ops, int max_ops, int* n_ops) {
    if (!ops || !n_ops || max_ops <= 0) return fail(LTK_E_INVALID, "bad arguments");
    const std::vector<FdOp> prog = fd_program(H, W);
    if (prog.empty()) return fail(LTK_E_INVALID, "face detector: H and W must be in [32, 16384]");
    if ((int)prog.size() > max_ops) return fail(LTK_E_INVALID, "face detector: the program has " + std::to_string(prog.size()) + " ops");
    for (size_t i = 0; i < prog.size(); ++i) {
        const FdOp& p = prog[i];
        ltk_fd_op_info& o = ops[i];
        memset(&o, 0, sizeof(o));
        snprintf(o.name, sizeof(o.name), "%s", p.name.c_str());
        o.type = p.type; o.cin = p.cin; o.cout = p.cout; o.k = p.k; o.stride = p.stride; o.pad = p.pad; o.relu = p.relu; o.maxout = p.maxout;
        o.level = p.level; o.H = p.H; o.W = p.W; o.Ho = p.Ho; o.Wo = p.Wo;
    }
    *n_ops = (int)prog.size();
    return LTK_OK;
}

int ltk_debug_face_detect_plan(int H, int W, int max_images, ltk_fd_bind* ops, int max_ops, int* n_ops, unsigned long long* buf_bytes,
                               int max_bufs, int* n_bufs, int* image_buf, unsigned long long* total_bytes) {
    if (!ops || !n_ops || !buf_bytes || !n_bufs || !image_buf || !total_bytes || max_ops <= 0 || max_bufs <= 0) return fail(LTK_E_INVALID, "bad arguments");
    FdPlan pl;
    std::string err;
    if (fd_plan(H, W, max_images, &pl, &err)) return fail(LTK_E_INVALID, err);
    if ((int)pl.ops.size() > max_ops) return fail(LTK_E_INVALID, "face detector: the program has " + std::to_string(pl.ops.size()) + " ops");
    if ((int)pl.buf_bytes.size() > max_bufs) return fail(LTK_E_INVALID, "face detector: the program has " + std::to_string(pl.buf_bytes.size()) + " buffers");
    auto view = [](const FdView& v) { return ltk_fp_view{v.buf, v.ld, v.coff, v.C, v.H, v.W}; };
    for (size_t i = 0; i < pl.ops.size(); ++i) {
        ltk_fd_bind& o = ops[i];
        memset(&o, 0, sizeof(o));
        snprintf(o.name, sizeof(o.name), "%s", pl.ops[i].name.c_str());
        o.x = view(pl.bind[i].x); o.y = view(pl.bind[i].y);
    }
    for (size_t i = 0; i < pl.buf_bytes.size(); ++i) buf_bytes[i] = (unsigned long long)pl.buf_bytes[i];
    *n_ops = (int)pl.ops.size(); *n_bufs = (int)pl.buf_bytes.size();
    *image_buf = pl.image_buf; *total_bytes = (unsigned long long)pl.total_bytes;
    return LTK_OK;
}

int ltk_face_parse_debug_get(ltk_engine* e, const char* op_name, int images, float* out_f32, size_t n_floats) {
    if (!e || !op_name || !out_f32 || images <= 0) return fail(LTK_E_INVALID, "bad arguments");
    if (!e->face_parse) return fail(LTK_E_STATE, "ltk_face_parse_load has not been called");
    if (!strcmp(op_name, "labels")) return fail(LTK_E_INVALID, "face parser: labels are bytes, not an fp16 tensor: they come from ltk_face_parse");
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    if (images > e->face_parse_last)
        return fail(LTK_E_INVALID, "face parser: the last run held " + std::to_string(e->face_parse_last) + " images");
    int cout = 0;
    for (const FpOp& p : fp_program(e->face_parse_size)) if (p.name == op_name) cout = p.cout;
    int C, ld, coff, H, W;
    f16* t = mt_named(e->face_parse, op_name, &C, &ld, &coff, &H, &W);
    if (!t || !cout) return fail(LTK_E_STATE, std::string("no face parser tensor named ") + op_name);
    const size_t cnt = (size_t)images * cout * H * W;
    if (cnt != n_floats) return fail(LTK_E_INVALID, "size mismatch: tensor has " + std::to_string(cnt) + " floats for these images");
    return read_cb16(e, t, images, cout, ld, coff, H, W, out_f32);          // the real channels of the view
}

int ltk_face_detect_debug_get(ltk_engine* e, const char* op_name, int images, float* out_f32, size_t n_floats) {
    if (!e || !op_name || !out_f32 || images <= 0) return fail(LTK_E_INVALID, "bad arguments");
    if (!e->face_det_w) return fail(LTK_E_STATE, "ltk_face_detect_load has not been called");
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->face_det_last) return fail(LTK_E_STATE, "face detector: no program has run");
    if (images > e->face_det_last_n)
        return fail(LTK_E_INVALID, "face detector: the last run held " + std::to_string(e->face_det_last_n) + " images");
    int C, ld, coff, H, W;
    f16* t = mt_named(e->face_det_last, op_name, &C, &ld, &coff, &H, &W);
    if (!t) return fail(LTK_E_STATE, std::string("no face detector tensor named ") + op_name);
    const size_t cnt = (size_t)images * C * H * W;
    if (cnt != n_floats) return fail(LTK_E_INVALID, "size mismatch: tensor has " + std::to_string(cnt) + " floats for these images");
    // a tapped map, a norm and a head have buffers of their own: they are read as the (replayed) run left them.  The trunk's other
    // ops write two buffers in turn (fd_plan), so what such a launch wrote is gone by the end of a run: the program runs again,
    // eagerly, on the frames the last call left in its image buffer, up to and including this launch - the same kernels with the
    // same arguments on the same bytes.  The detect launches stand behind every tensor: the records are not touched.
    if (mt_named_writers(e->face_det_last, op_name) == 1) return read_cb16(e, t, images, C, ld, coff, H, W, out_f32);
    int k = -1;
    for (int i = 0; i < mt_op_count(e->face_det_last) && k < 0; ++i)
        if (!strcmp(mt_op_name(e->face_det_last, i, nullptr), op_name)) k = i;
    if (k < 0) return fail(LTK_E_STATE, std::string("no face detector launch named ") + op_name);
    const int prc = mt_run_head(e->face_det_last, e->face_det_last_n, e->d_partial, e->partial_cap, e->compute, k + 1);
    if (prc) return conv_status(prc, std::string("face detector: ") + mt_graph_error(e->face_det_last));
    return read_cb16(e, t, images, C, ld, coff, H, W, out_f32);
}

int ltk_debug_face_detect_time(ltk_engine* e, int images, int iters, float* ms_per_pass, float* ms_per_op, int n_ops) {
    if (!e || images <= 0 || iters <= 0 || !ms_per_pass) return fail(LTK_E_INVALID, "bad arguments");
    if (!e->face_det_w) return fail(LTK_E_STATE, "ltk_face_detect_load has not been called");
    if (images > e->face_det_images) return fail(LTK_E_INVALID, "images exceeds max_images");
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    MtGraph* prog = e->face_det_last;
    if (!prog) return fail(LTK_E_STATE, "face detector: no program has run");
    if (ms_per_op && n_ops != mt_op_count(prog)) return fail(LTK_E_INVALID, "n_ops != the program's launches");
    auto pass = [&]() -> int {
        const int prc = run_program(e, prog, images);
        return prc ? conv_status(prc, std::string("face detector: ") + mt_graph_error(prog)) : 0;
    };
    int rc = pass();
    if (!rc) rc = pass();
    float ms = 0.f;
    if (!rc) rc = time_iters(e->compute, iters, pass, &ms);
    if (rc) return rc;
    e->face_det_last_n = images;
    *ms_per_pass = ms / iters;
    if (ms_per_op) {
        auto run = [&](std::vector<hipEvent_t>* evs) -> int {
            const int prc = mt_run_timed(prog, images, e->d_partial, e->partial_cap, e->compute, evs);
            return prc ? conv_status(prc, std::string("face detector: ") + mt_graph_error(prog)) : 0;
        };
        std::vector<float> per((size_t)n_ops);
        rc = time_intervals(n_ops, iters, run, per.data());
        if (rc) return rc;
        memcpy(ms_per_op, per.data(), per.size() * sizeof(float));
    }
    return LTK_OK;
}

int ltk_debug_face_parse_time(ltk_engine* e, int images, int iters, float* ms_per_pass, float* ms_per_op, int n_ops) {
    if (!e || images <= 0 || iters <= 0 || !ms_per_pass) return fail(LTK_E_INVALID, "bad arguments");
    if (!e->face_parse) return fail(LTK_E_STATE, "ltk_face_parse_load has not been called");
    if (images > e->face_parse_images) return fail(LTK_E_INVALID, "images exceeds max_images");
    if (ms_per_op && n_ops != mt_op_count(e->face_parse)) return fail(LTK_E_INVALID, "n_ops != the program's launches");
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    // as ltk_face_parse enqueues the program: eagerly the first time an image count is seen, then captured, then replayed
    auto pass = [&]() -> int {
        const int prc = run_program(e, e->face_parse, images);
        return prc ? conv_status(prc, std::string("face parser: ") + mt_graph_error(e->face_parse)) : 0;
    };
    int rc = pass();
    if (!rc) rc = pass();
    float ms = 0.f;
    if (!rc) rc = time_iters(e->compute, iters, pass, &ms);
    if (rc) return rc;
    e->face_parse_last = images;
    *ms_per_pass = ms / iters;
    if (ms_per_op) {
        auto run = [&](std::vector<hipEvent_t>* evs) -> int {
            const int prc = mt_run_timed(e->face_parse, images, e->d_partial, e->partial_cap, e->compute, evs);
            return prc ? conv_status(prc, std::string("face parser: ") + mt_graph_error(e->face_parse)) : 0;
        };
        std::vector<float> per((size_t)n_ops);
        rc = time_intervals(n_ops, iters, run, per.data());
        if (rc) return rc;
        memcpy(ms_per_op, per.data(), per.size() * sizeof(float));
    }
    return LTK_OK;
}

int ltk_f32_to_e4m3(const float* in, size_t n, uint8_t* out) {
    if (!in || !out) return fail(LTK_E_INVALID, "bad arguments");
    for (size_t i = 0; i < n; ++i) out[i] = f32_to_e4m3(in[i]);
    return LTK_OK;
}

int ltk_conv2d_fp8(ltk_engine* e, const void* d_x, int N, int H, int W, int Cin, const float* weight, int Cout,
                   const float* scale, const float* shift, float act_scale, const void* d_res, int act, void* d_y, int iters,
                   float* ms_avg) {
    return conv2d_hook(e, d_x, N, H, W, Cin, weight, Cout, 3, 3, 1, 1, 1, 1, false, 0, scale, shift, conv_fp8_quant(Cin), act_scale, d_res, 0, act,
                       d_y, iters, ms_avg);
}

int ltk_conv2d_fp8_ex(ltk_engine* e, const void* d_x, int N, int H, int W, int Cin, const float* weight, int Cout, const float* scale,
                      const float* shift, float act_scale, int quant, const void* d_res, void* d_y, const ltk_conv_opts* opts, ltk_conv_report* rep) {
    if (!e || !d_x || !weight || !d_y || quant < 0 || quant > 2 || !(act_scale > 0.f)) return fail(LTK_E_INVALID, "bad arguments");
    ConvHookCall c;
    const int rc = conv_hook_plan(N, H, W, Cin, Cout, 3, 3, 1, 1, 1, 1, 0, 0, d_res != nullptr, 0, quant ? quant : conv_fp8_quant(Cin), opts, rep, &c);
    if (rc) return rc;
    CHK(enter_device(e->device));
    return conv_hook_launch(e, c, d_x, weight, Cin, Cout, 3, 3, 1, 1, 1, 1, 0, 0, scale, shift, act_scale, 0, d_res, d_y, rep);
}

int ltk_debug_conv3_fp8_variants(char* buf, int cap) {
    const std::string names = conv3_fp8_variant_names();
    if (!buf || cap <= (int)names.size()) return fail(LTK_E_INVALID, "buffer too small: " + std::to_string(names.size() + 1) + " bytes needed");
    memcpy(buf, names.c_str(), names.size() + 1);
    return LTK_OK;
}

int ltk_musetalk_forward_host(ltk_engine* e, const float* latents, const float* feat, int B, float* unet_out, float* image,
                              uint8_t* frames) {
    if (!e || !latents || !feat || B <= 0) return fail(LTK_E_INVALID, "bad arguments");
    if (!e->mt) return fail(LTK_E_STATE, "ltk_musetalk_load has not been called");
    if (B > e->mt_max_frames) return fail(LTK_E_INVALID, "B exceeds max_frames");
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    hipStream_t s = e->compute;
    CHK(hipMemcpyAsync(e->d_mt_lat, latents, (size_t)B * 8 * 1024 * sizeof(float), hipMemcpyHostToDevice, s));
    CHK(hipMemcpyAsync(e->d_mt_feat, feat, (size_t)B * 50 * 384 * sizeof(float), hipMemcpyHostToDevice, s));
    int cbt;
    f16* lat = mt_latent_in(e->mt, &cbt);
    launch_nchw_to_cb16(e->d_mt_lat, B, 8, 1024, lat, cbt, 0, s);
    DevBuf d_img, d_frames;
    if (image) CHK(hipMalloc(&d_img.p, (size_t)B * 3 * 65536 * sizeof(float)));
    if (frames) CHK(hipMalloc(&d_frames.p, (size_t)B * 65536 * 3));
    OutList64 op;
    for (int i = 0; i < 64; ++i) op.p[i] = (frames && i < B) ? (uint8_t*)d_frames.p + (size_t)i * 65536 * 3 : nullptr;
    int rc = mt_run_locked(e, e->d_mt_feat, nullptr, B, &op, (float*)d_img.p);
    if (!rc && hipStreamSynchronize(s) != hipSuccess) rc = fail(LTK_E_HIP, "stream sync failed");
    if (!rc && unet_out) {
        int C, ld, coff, H, W;
        f16* t = mt_named(e->mt, "conv_out", &C, &ld, &coff, &H, &W);
        rc = read_cb16(e, t, B, 4, ld, coff, H, W, unet_out);          // the 4 real channels of the block
    }
    if (!rc && image) CHK(hipMemcpy(image, d_img.p, (size_t)B * 3 * 65536 * sizeof(float), hipMemcpyDeviceToHost));
    if (!rc && frames) CHK(hipMemcpy(frames, d_frames.p, (size_t)B * 65536 * 3, hipMemcpyDeviceToHost));
    return rc;
}

int ltk_musetalk_debug_get(ltk_engine* e, const char* name, int frames, float* out, size_t n_floats) {
    if (!e || !name || !out || frames <= 0) return fail(LTK_E_INVALID, "bad arguments");
    if (!e->mt) return fail(LTK_E_STATE, "ltk_musetalk_load has not been called");
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    return read_named(e, e->mt, "MuseTalk", name, frames, " for these frames", out, n_floats);
}

int ltk_musetalk_op_count(ltk_engine* e) { return (e && e->mt) ? mt_op_count(e->mt) : 0; }

int ltk_musetalk_op_name(ltk_engine* e, int op, char* buf, int buf_len, int* type) {
    if (!e || !e->mt || !buf || buf_len <= 0) return fail(LTK_E_INVALID, "bad arguments");
    return copy_op_name(e->mt, op, buf, buf_len, type);
}

int ltk_musetalk_time_ops(ltk_engine* e, int frames, int iters, float* ms_per_op, int n_ops) {
    if (!e || frames <= 0 || iters <= 0 || !ms_per_op) return fail(LTK_E_INVALID, "bad arguments");
    if (!e->mt) return fail(LTK_E_STATE, "ltk_musetalk_load has not been called");
    if (frames > e->mt_max_frames) return fail(LTK_E_INVALID, "frames exceeds max_frames");
    if (n_ops != mt_op_count(e->mt)) return fail(LTK_E_INVALID, "n_ops != ltk_musetalk_op_count");
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    auto run = [&](std::vector<hipEvent_t>* evs) -> int {
        const int prc = evs ? mt_run_timed(e->mt, frames, e->d_partial, e->partial_cap, e->compute, evs)
                            : mt_run(e->mt, frames, e->d_partial, e->partial_cap, e->compute);
        return prc ? fail(LTK_E_INVALID, std::string("musetalk: ") + mt_graph_error(e->mt)) : 0;
    };
    std::vector<float> ms((size_t)n_ops);
    int rc = run(nullptr);                                               // warm
    if (!rc) rc = time_intervals(n_ops, iters, run, ms.data());
    if (rc) return rc;
    if (mt_gn_error(e->mt)) return fail(LTK_E_HIP, std::string("musetalk: ") + mt_graph_error(e->mt));
    memcpy(ms_per_op, ms.data(), ms.size() * sizeof(float));
    return LTK_OK;
}

int ltk_musetalk_time(ltk_engine* e, int frames, int iters, float* ms_per_pass, double* macs_per_pass) {
    if (!e || frames <= 0 || iters <= 0 || !ms_per_pass) return fail(LTK_E_INVALID, "bad arguments");
    if (!e->mt) return fail(LTK_E_STATE, "ltk_musetalk_load has not been called");
    if (frames > e->mt_max_frames) return fail(LTK_E_INVALID, "frames exceeds max_frames");
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    // as ltk_musetalk_infer enqueues the program: eagerly the first time a frame count is seen, then captured, then replayed
    auto pass = [&]() -> int { return run_program(e, e->mt, frames) ? fail(LTK_E_INVALID, std::string("musetalk: ") + mt_graph_error(e->mt)) : 0; };
    int rc = pass();
    if (!rc) rc = pass();
    float ms = 0.f;
    if (!rc) rc = time_iters(e->compute, iters, pass, &ms);
    if (rc) return rc;
    if (mt_gn_error(e->mt)) return fail(LTK_E_HIP, std::string("musetalk: ") + mt_graph_error(e->mt));
    *ms_per_pass = ms / iters;
    if (macs_per_pass) *macs_per_pass = mt_macs_per_frame(e->mt) * frames;
    return LTK_OK;
}

int ltk_whisper_debug_get(ltk_engine* e, const char* name, float* out, size_t n_floats) {
    if (!e || !name || !out) return fail(LTK_E_INVALID, "bad arguments");
    if (!e->whisper) return fail(LTK_E_STATE, "ltk_whisper_load has not been called");
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    return read_named(e, e->whisper, "Whisper", name, 1, "", out, n_floats);
}

int ltk_whisper_debug_get_clip(ltk_engine* e, const char* name, int clip, float* out, size_t n_floats) {
    if (!e || !name || !out || clip < 0) return fail(LTK_E_INVALID, "bad arguments");
    if (!e->whisper) return fail(LTK_E_STATE, "ltk_whisper_load has not been called");
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->whisper_b || !e->whisper_b_nf) return fail(LTK_E_STATE, "no batched Whisper run yet");
    if (clip >= e->whisper_b_nf) return fail(LTK_E_INVALID, "the last batched run carried " + std::to_string(e->whisper_b_nf) + " clips");
    int C, ld, coff, H, W;
    f16* t = mt_named(e->whisper_b, name, &C, &ld, &coff, &H, &W);
    if (!t) return fail(LTK_E_STATE, std::string("no Whisper tensor named ") + name);
    const size_t cnt = (size_t)C * H * W;
    if (cnt != n_floats) return fail(LTK_E_INVALID, "size mismatch: tensor has " + std::to_string(cnt) + " floats per clip");
    return read_cb16(e, t + (size_t)clip * ld * H * W, 1, C, ld, coff, H, W, out);
}

int ltk_whisper_batch_info(ltk_engine* e, int* capacity, int* built, size_t* activation_bytes) {
    if (!e) return fail(LTK_E_INVALID, "bad arguments");
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->whisper) return fail(LTK_E_STATE, "ltk_whisper_load has not been called");
    if (capacity) *capacity = kWhisperBatchClips;
    if (built) *built = e->whisper_b ? 1 : 0;
    if (activation_bytes) *activation_bytes = e->whisper_b ? mt_activation_bytes(e->whisper_b) : 0;
    return LTK_OK;
}

int ltk_debug_whisper_batch_plan(int nreq, int* run_of, int* slot_of, int* run_batched, int* n_runs) {
    if (nreq <= 0 || !run_of || !slot_of || !run_batched || !n_runs) return fail(LTK_E_INVALID, "bad arguments");
    const std::vector<WhisperRun> runs = whisper_batch_plan(nreq, kWhisperBatchClips);
    for (size_t i = 0; i < runs.size(); ++i) {
        run_batched[i] = runs[i].batched ? 1 : 0;
        for (int j = 0; j < runs[i].count; ++j) { run_of[runs[i].first + j] = (int)i; slot_of[runs[i].first + j] = j; }
    }
    *n_runs = (int)runs.size();
    return LTK_OK;
}

// ---------------------------------------------------------------- HuBERT: the program's tensors and ops, and its kernels on their own
int ltk_hubert_debug_get(ltk_engine* e, const char* name, float* out, size_t n_floats) {
    if (!e || !name || !out) return fail(LTK_E_INVALID, "bad arguments");
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->hubert_w) return fail(LTK_E_STATE, "ltk_hubert_load has not been called");
    if (!e->hubert_last) return fail(LTK_E_STATE, "no HuBERT program has run yet");
    CHK(hipStreamSynchronize(e->compute));
    if (std::string(name) == "input_values") {                 // the normalised waveform of the clip, fp32 [n_samples]
        size_t n = 0;
        for (auto& p : e->hubert_progs) if (p.g == e->hubert_last) n = (size_t)p.n_samples;
        if (n != n_floats) return fail(LTK_E_INVALID, "size mismatch: the clip has " + std::to_string(n) + " samples");
        CHK(hipMemcpy(out, mt_hubert_pcm_in(e->hubert_last), n * sizeof(float), hipMemcpyDeviceToHost));
        return LTK_OK;
    }
    return read_named(e, e->hubert_last, "HuBERT", name, 1, "", out, n_floats);
}

int ltk_hubert_op_count(ltk_engine* e) {
    if (!e) return 0;
    std::lock_guard<std::mutex> g(e->mu);
    return e->hubert_w ? mt_op_count(e->hubert_w) : 0;
}

int ltk_hubert_op_name(ltk_engine* e, int op, char* buf, int buf_len, int* type) {
    if (!e || !buf || buf_len <= 0) return fail(LTK_E_INVALID, "bad arguments");
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->hubert_w) return fail(LTK_E_STATE, "ltk_hubert_load has not been called");
    return copy_op_name(e->hubert_w, op, buf, buf_len, type);
}

int ltk_hubert_info(ltk_engine* e, int* layers, int* programs, size_t* activation_bytes) {
    if (!e) return fail(LTK_E_INVALID, "bad arguments");
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->hubert_w) return fail(LTK_E_STATE, "ltk_hubert_load has not been called");
    if (layers) *layers = mt_hubert_layers(e->hubert_w);
    if (programs) *programs = (int)e->hubert_progs.size();
    if (activation_bytes) *activation_bytes = e->hubert_last ? mt_activation_bytes(e->hubert_last) : 0;
    return LTK_OK;
}

int ltk_hubert_debug_get_clip(ltk_engine* e, const char* name, int clip, float* out, size_t n_floats) {
    if (!e || !name || !out || clip < 0) return fail(LTK_E_INVALID, "bad arguments");
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->hubert_w) return fail(LTK_E_STATE, "ltk_hubert_load has not been called");
    if (!e->hubert_blast) return fail(LTK_E_STATE, "no batched HuBERT run yet");
    if (clip >= e->hubert_blast_nf) return fail(LTK_E_INVALID, "the last batched run carried " + std::to_string(e->hubert_blast_nf) + " clips");
    CHK(hipStreamSynchronize(e->compute));
    if (std::string(name) == "input_values") {
        size_t n = 0;
        for (auto& p : e->hubert_bprogs) if (p.g == e->hubert_blast) n = (size_t)p.n_samples;
        if (n != n_floats) return fail(LTK_E_INVALID, "size mismatch: the clip has " + std::to_string(n) + " samples");
        CHK(hipMemcpy(out, mt_hubert_pcm_in(e->hubert_blast) + (size_t)clip * n, n * sizeof(float), hipMemcpyDeviceToHost));
        return LTK_OK;
    }
    int C, ld, coff, H, W;
    f16* t = mt_named(e->hubert_blast, name, &C, &ld, &coff, &H, &W);
    if (!t) return fail(LTK_E_STATE, std::string("no HuBERT tensor named ") + name);
    const size_t cnt = (size_t)C * H * W;
    if (cnt != n_floats) return fail(LTK_E_INVALID, "size mismatch: tensor has " + std::to_string(cnt) + " floats per clip");
    return read_cb16(e, t + (size_t)clip * ld * H * W, 1, C, ld, coff, H, W, out);
}

int ltk_hubert_batch_info(ltk_engine* e, int* capacity, int* programs, size_t* activation_bytes) {
    if (!e) return fail(LTK_E_INVALID, "bad arguments");
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->hubert_w) return fail(LTK_E_STATE, "ltk_hubert_load has not been called");
    if (capacity) *capacity = kHubertBatchClips;
    if (programs) *programs = (int)e->hubert_bprogs.size();
    if (activation_bytes) {
        *activation_bytes = 0;
        for (auto& p : e->hubert_bprogs)
            if (p.g == e->hubert_blast) *activation_bytes = hubert_clip_activation_bytes(p.n_samples, mt_hubert_layers(e->hubert_w)) * kHubertBatchClips;
    }
    return LTK_OK;
}

int ltk_debug_hubert_batch_plan(const int* n_samples, int nreq, int layers, int* run_of, int* slot_of, int* run_batched, int* n_runs,
                                size_t* clip_bytes) {
    if (!n_samples || nreq <= 0 || layers <= 0 || !run_of || !slot_of || !run_batched || !n_runs) return fail(LTK_E_INVALID, "bad arguments");
    const std::vector<HubertRun> runs = hubert_batch_plan(n_samples, nreq, layers);
    for (size_t i = 0; i < runs.size(); ++i) {
        run_batched[i] = runs[i].batched ? 1 : 0;
        for (size_t j = 0; j < runs[i].req.size(); ++j) { run_of[runs[i].req[j]] = (int)i; slot_of[runs[i].req[j]] = (int)j; }
    }
    *n_runs = (int)runs.size();
    if (clip_bytes)
        for (int r = 0; r < nreq; ++r) clip_bytes[r] = hubert_clip_activation_bytes(n_samples[r], layers);
    return LTK_OK;
}

int ltk_hubert_stats(ltk_engine* e, const float* pcm, long long n, float* mean_var) {
    if (!e || !pcm || !mean_var || n <= 0) return fail(LTK_E_INVALID, "bad arguments");
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    DevBuf x, st;
    const int rc = upload(pcm, (size_t)n * sizeof(float), &x);
    if (rc) return rc;
    CHK(hipMalloc(&st.p, 2 * sizeof(float)));
    launch_hubert_stats((const float*)x.p, n, (float*)st.p, e->compute);
    CHK(hipGetLastError());
    CHK(hipStreamSynchronize(e->compute));
    CHK(hipMemcpy(mean_var, st.p, 2 * sizeof(float), hipMemcpyDeviceToHost));
    return LTK_OK;
}

namespace {

// host fp32 [T][C] -> a CB16 device tensor (back: read_cb16, host fp32 [C][T])
int hb_up(ltk_engine* e, const float* host, int T, int C, DevBuf* stage, DevBuf* cb) {
    const int rc = upload(host, (size_t)T * C * sizeof(float), stage);
    if (rc) return rc;
    CHK(hipMalloc(&cb->p, (size_t)T * C * sizeof(f16)));
    launch_tokens_to_cb16((const float*)stage->p, 1, T, C, nullptr, (f16*)cb->p, C / 16, 0, e->compute);
    return LTK_OK;
}

}  // namespace

int ltk_hubert_layer0_host(ltk_engine* e, const float* x, int n, const float* w, const float* bias, const float* gamma, const float* beta,
                           float* out) {
    if (!e || !x || !w || !bias || !gamma || !beta || !out || n < 10) return fail(LTK_E_INVALID, "bad arguments");
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    const int L0 = (n - 10) / 5 + 1;
    DevBuf dx, dw, db, dg, de, dy;
    int rc = upload(x, (size_t)n * sizeof(float), &dx);
    if (!rc) rc = upload(w, 5120 * sizeof(float), &dw);
    if (!rc) rc = upload(bias, 512 * sizeof(float), &db);
    if (!rc) rc = upload(gamma, 512 * sizeof(float), &dg);
    if (!rc) rc = upload(beta, 512 * sizeof(float), &de);
    if (rc) return rc;
    CHK(hipMalloc(&dy.p, (size_t)L0 * 512 * sizeof(f16)));
    launch_hubert_layer0((const float*)dx.p, n, (const float*)dw.p, (const float*)db.p, (const float*)dg.p, (const float*)de.p, 1e-5f,
                         (f16*)dy.p, e->compute);
    return read_cb16(e, (const f16*)dy.p, 1, 512, 512, 0, L0, 1, out);
}

int ltk_hubert_ln_gelu_host(ltk_engine* e, const float* x, int T, const float* gamma, const float* beta, float* out) {
    if (!e || !x || !gamma || !beta || !out || T <= 0) return fail(LTK_E_INVALID, "bad arguments");
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    DevBuf st, dx, dg, de, dy;
    int rc = hb_up(e, x, T, 512, &st, &dx);
    if (!rc) rc = upload(gamma, 512 * sizeof(float), &dg);
    if (!rc) rc = upload(beta, 512 * sizeof(float), &de);
    if (rc) return rc;
    CHK(hipMalloc(&dy.p, (size_t)T * 512 * sizeof(f16)));
    launch_ln_gelu512((const f16*)dx.p, 0, T, 1e-5f, (const float*)dg.p, (const float*)de.p, (f16*)dy.p, 0, e->compute);
    return read_cb16(e, (const f16*)dy.p, 1, 512, 512, 0, T, 1, out);
}

int ltk_hubert_posconv_host(ltk_engine* e, const float* x, int T, const float* w, const float* bias, float* out) {
    if (!e || !x || !w || !bias || !out || T <= 0) return fail(LTK_E_INVALID, "bad arguments");
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    DevBuf st, dx, dw, db, dy;
    int rc = hb_up(e, x, T, 1024, &st, &dx);
    if (!rc) rc = upload(bias, 1024 * sizeof(float), &db);
    if (!rc) {
        std::vector<f16> packed(kPosConvPackHalfs);
        hubert_posconv_pack(w, packed.data());
        rc = upload(packed.data(), packed.size() * sizeof(f16), &dw);
    }
    if (rc) return rc;
    CHK(hipMalloc(&dy.p, (size_t)T * 1024 * sizeof(f16)));
    launch_hubert_posconv((const f16*)dx.p, 0, T, (const f16*)dw.p, (const float*)db.p, (f16*)dy.p, 0, e->compute);
    return read_cb16(e, (const f16*)dy.p, 1, 1024, 1024, 0, T, 1, out);
}

int ltk_hubert_chunks_host(ltk_engine* e, const float* feat, int T, int batch, int first_row, int row_step, int rows, float* out) {
    if (!e || !feat || !out || T <= 0 || batch <= 0 || rows <= 0) return fail(LTK_E_INVALID, "bad arguments");
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    DevBuf st, dx, dy;
    const int rc = hb_up(e, feat, T, 1024, &st, &dx);
    if (rc) return rc;
    const size_t cnt = (size_t)batch * rows * 1024;
    CHK(hipMalloc(&dy.p, cnt * sizeof(float)));
    launch_hubert_chunks((const f16*)dx.p, 0, T, batch, first_row, row_step, rows, (float*)dy.p, e->compute);
    CHK(hipGetLastError());
    CHK(hipStreamSynchronize(e->compute));
    CHK(hipMemcpy(out, dy.p, cnt * sizeof(float), hipMemcpyDeviceToHost));
    return LTK_OK;
}

}  // extern "C"

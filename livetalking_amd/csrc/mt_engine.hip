// MuseTalk (U-Net + VAE decoder), Whisper and HuBERT audio features and the VAE encoder: their entry points and run_program.
#include "engine_internal.h"
#include "facedet.h"
#include "faceparse.h"
#include "s3fd_kernels.h"

#include <algorithm>

extern "C" {

// ================================================================================ MuseTalk
int ltk_musetalk_set_fp8(ltk_engine* e, int enable, float act_scale) {
    if (!e) return fail(LTK_E_INVALID, "bad arguments");
    std::lock_guard<std::mutex> g(e->mu);
    if (e->mt) return fail(LTK_E_STATE, "ltk_musetalk_set_fp8 must precede ltk_musetalk_load");
    e->mt_fp8 = enable ? 1 : 0;
    e->mt_fp8_ascale = act_scale > 0.f ? act_scale : 8.f;
    return LTK_OK;
}

int ltk_musetalk_info(ltk_engine* e, double* macs_per_frame, double* macs_fp8_per_frame) {
    if (!e) return fail(LTK_E_INVALID, "bad arguments");
    if (!e->mt) return fail(LTK_E_STATE, "ltk_musetalk_load has not been called");
    if (macs_per_frame) *macs_per_frame = mt_macs_per_frame(e->mt);
    if (macs_fp8_per_frame) *macs_fp8_per_frame = mt_macs_fp8_per_frame(e->mt);
    return LTK_OK;
}

int ltk_musetalk_load(ltk_engine* e, const ltk_named_tensor* unet_sd, int n_unet, const ltk_named_tensor* vae_sd, int n_vae,
                      int max_frames) {
    if (!e || !unet_sd || !vae_sd || n_unet <= 0 || n_vae <= 0) return fail(LTK_E_INVALID, "bad arguments");
    if (max_frames < 1 || max_frames > 64) return fail(LTK_E_INVALID, "max_frames must be in [1, 64] for MuseTalk");
    std::lock_guard<std::mutex> g(e->mu);
    if (e->mt) return fail(LTK_E_STATE, "a MuseTalk model is already loaded in this engine");
    CHK(enter_device(e->device));
    MtGraph* mg = mt_graph_new();
    mt_set_fp8(mg, e->mt_fp8, e->mt_fp8_ascale);
    const int rc = mt_build(mg, unet_sd, n_unet, vae_sd, n_vae, max_frames);
    if (rc) {
        const std::string msg = mt_graph_error(mg);
        mt_graph_delete(mg);
        return fail(rc == -4 ? LTK_E_NOMEM : LTK_E_INVALID, "musetalk: " + msg);
    }
    // avatars/musetalk/models/unet.py:12-27 PositionalEncoding(d_model=384), first 50 positions
    std::vector<float> pe(50 * 384);
    for (int pos = 0; pos < 50; ++pos)
        for (int i = 0; i < 384; i += 2) {
            const float div = expf((float)i * (-logf(10000.0f) / 384.0f));
            pe[pos * 384 + i] = sinf((float)pos * div);
            pe[pos * 384 + i + 1] = cosf((float)pos * div);
        }
    const int arc = [&]() -> int {
        CHK(hipMalloc((void**)&e->d_pe, pe.size() * sizeof(float)));
        CHK(hipMemcpy(e->d_pe, pe.data(), pe.size() * sizeof(float), hipMemcpyHostToDevice));
        CHK(hipMalloc((void**)&e->d_mt_feat, (size_t)max_frames * 50 * 384 * sizeof(float)));
        CHK(hipMalloc((void**)&e->d_mt_lat, (size_t)max_frames * 8 * 1024 * sizeof(float)));
        return LTK_OK;
    }();
    if (arc) {                                       // a failed load leaves nothing behind and can be retried
        if (e->d_pe) { (void)hipFree(e->d_pe); e->d_pe = nullptr; }
        if (e->d_mt_feat) { (void)hipFree(e->d_mt_feat); e->d_mt_feat = nullptr; }
        if (e->d_mt_lat) { (void)hipFree(e->d_mt_lat); e->d_mt_lat = nullptr; }
        mt_graph_delete(mg);
        return arc;
    }
    if (e->hw_mt.alloc(mt_op_count(mg))) {
        (void)hipFree(e->d_pe); (void)hipFree(e->d_mt_feat); (void)hipFree(e->d_mt_lat);
        e->d_pe = nullptr; e->d_mt_feat = nullptr; e->d_mt_lat = nullptr;
        mt_graph_delete(mg);
        return fail(LTK_E_NOMEM, "health table allocation failed");
    }
    e->mt = mg;
    e->mt_max_frames = max_frames;
    return LTK_OK;
}

int ltk_musetalk_avatar_register(ltk_engine* e, const float* latents, const uint8_t* full_bank, const int32_t* face_boxes,
                                 const int32_t* crop_boxes, const uint8_t* masks, const int64_t* mask_offsets, int n, int H,
                                 int W, int* avatar_id) {
    if (!e || !latents || !full_bank || !face_boxes || !crop_boxes || !masks || !mask_offsets || !avatar_id || n <= 0 || H <= 0 || W <= 0)
        return fail(LTK_E_INVALID, "bad arguments");
    for (int i = 0; i < n; ++i) {
        const int32_t* f = face_boxes + 4 * i;   // (x1,y1,x2,y2), musetalk_avatar.py:157
        const int32_t* c = crop_boxes + 4 * i;   // (x_s,y_s,x_e,y_e), myutil.py:7
        if (c[0] < 0 || c[1] < 0 || c[2] > W || c[3] > H || c[2] <= c[0] || c[3] <= c[1])
            return fail(LTK_E_INVALID, "crop box outside the frame (the reference's slicing is undefined there)");
        if (f[0] < c[0] || f[1] < c[1] || f[2] > c[2] || f[3] > c[3] || f[2] <= f[0] || f[3] <= f[1])
            return fail(LTK_E_INVALID, "face box must lie inside its crop box");
        if (mask_offsets[i + 1] - mask_offsets[i] != (int64_t)(c[3] - c[1]) * (c[2] - c[0]) * 3)
            return fail(LTK_E_INVALID, "mask size does not match its crop box");
    }
    CHK(enter_device(e->device));
    auto ap = std::make_shared<MtAvatar>();
    MtAvatar& a = *ap;
    a.device = e->device;
    a.n = n; a.H = H; a.W = W;
    a.face_box.assign(face_boxes, face_boxes + 4 * (size_t)n);
    a.crop_box.assign(crop_boxes, crop_boxes + 4 * (size_t)n);
    a.mask_off.assign(mask_offsets, mask_offsets + n + 1);
    const size_t lb = (size_t)n * 8 * 1024 * sizeof(float), ub = (size_t)n * H * W * 3, mb = (size_t)mask_offsets[n];
    CHK(hipMalloc((void**)&a.d_latents, lb));
    CHK(hipMalloc((void**)&a.d_full, ub));
    CHK(hipMalloc((void**)&a.d_masks, mb));
    CHK(hipMemcpy(a.d_latents, latents, lb, hipMemcpyHostToDevice));
    CHK(hipMemcpy(a.d_full, full_bank, ub, hipMemcpyHostToDevice));
    CHK(hipMemcpy(a.d_masks, masks, mb, hipMemcpyHostToDevice));
    std::lock_guard<std::mutex> g(e->pool_mu);
    const int id = e->next_avatar++;
    e->mt_avatars[id] = ap;
    *avatar_id = id;
    return LTK_OK;
}

}  // extern "C"

// under e->mu: while the guard lives, the runs of `g` are a watched call's (ltk_health_watch): scanned into `w`'s records, which the
// program indexes by its op list (a program with another op count than the table is left alone)
namespace {
struct MtWatched {
    MtGraph* g = nullptr;
    MtWatched(MtGraph* g_, HealthWatch& w, bool on) {
        if (on && g_ && w.d && mt_op_count(g_) == w.n) { g = g_; mt_set_health(g, w.d, w.observed.data()); }
    }
    MtWatched(const MtWatched&) = delete;
    MtWatched& operator=(const MtWatched&) = delete;
    ~MtWatched() { if (g) mt_set_health(g, nullptr, nullptr); }
};
}  // namespace

// One run of a device program (the U-Net + VAE decoder pass, the Whisper encoder) on the compute stream, under e->mu.  Every op
// of a program reads and writes the program's own persistent buffers with launch arguments that depend on the frame count only,
// so the whole launch list (436 launches for a MuseTalk pass, ~60 for a Whisper step) is captured as ONE hipGraph the second time a
// (program, frame count) is seen and replayed from then on (knob GRAPH, as for the Wav2Lip pass: the first, eager run also sets
// every kernel's dynamic-LDS attribute, which a capture must not do).  The kernels that carry per-call pointers - latent / token
// gather in front, uint8 frame writer behind - stay outside the graph.  What this buys is the host side: one launch per pass
// instead of hundreds, on a host that also runs the sessions' Python.
int ltk::run_program(ltk_engine* e, MtGraph* prog, int nf) {
    hipStream_t s = e->compute;
    auto enq = [&]() -> int { return mt_run(prog, nf, e->d_partial, e->partial_cap, s); };
    if (mt_health_on(prog)) return enq();       // a watched call (ltk_health_watch): eagerly, scans between the ops, the graph cache untouched
    return knob(K_GRAPH) ? e->prog_graphs.run(e, {(const void*)prog, nf}, s, "program", nf, enq) : enq();
}

// latents already gathered into the graph's latent tensor; d_feat = fp32 [nf][50][384] on the device
int ltk::mt_run_locked(ltk_engine* e, const float* d_feat, const PtrList64* feat_ptrs, int nf, const OutList64* outs, float* d_image_f32) {
    hipStream_t s = e->compute;
    int cbt;
    f16* ctx = mt_ctx_in(e->mt, &cbt);
    if (feat_ptrs) launch_tokens_gather_to_cb16(*feat_ptrs, nf, 50, 384, e->d_pe, ctx, cbt, s);
    else launch_tokens_to_cb16(d_feat, nf, 50, 384, e->d_pe, ctx, cbt, 0, s);
    const int rc = run_program(e, e->mt, nf);
    if (rc) return conv_status(rc, std::string("musetalk: ") + mt_graph_error(e->mt));
    if (outs || d_image_f32) {
        OutList64 none;
        for (int i = 0; i < 64; ++i) none.p[i] = nullptr;
        f16* img = mt_vae_out(e->mt, &cbt);
        launch_vae_post(img, cbt, nf, 65536, outs ? *outs : none, d_image_f32, s);
    }
    CHK(hipGetLastError());
    return 0;
}

extern "C" {

int ltk_musetalk_infer(ltk_engine* e, const ltk_mt_req* reqs, int nreq, void* stream) {
    if (!e || !reqs || nreq <= 0) return fail(LTK_E_INVALID, "bad arguments");
    if (!e->mt) return fail(LTK_E_STATE, "ltk_musetalk_load has not been called");
    CHK(enter_device(e->device));
    std::vector<const float*> lptr, fptr;
    std::vector<uint8_t*> optr;
    std::vector<std::shared_ptr<MtAvatar>> hold;      // the banks stay alive until this call has synchronised
    for (int r = 0; r < nreq; ++r) {
        hold.push_back(find_mt_avatar(e, reqs[r].avatar));
        if (!hold.back()) return fail(LTK_E_STATE, "unknown MuseTalk avatar id");
        if (reqs[r].batch <= 0 || reqs[r].index < 0 || !reqs[r].d_feat || !reqs[r].d_pred) return fail(LTK_E_INVALID, "bad request");
        const MtAvatar& a = *hold.back();
        for (int i = 0; i < reqs[r].batch; ++i) {
            const int idx = mirror_index(a.n, reqs[r].index + i);   // musetalk_avatar.py:137-139
            lptr.push_back(a.d_latents + (size_t)idx * 8 * 1024);
            fptr.push_back((const float*)reqs[r].d_feat + (size_t)i * 50 * 384);
            optr.push_back((uint8_t*)reqs[r].d_pred + (size_t)i * 65536 * 3);
        }
    }
    const int total = (int)lptr.size();
    int rc = infer_call(e, stream, [&]() -> int {
        int rc = 0;
        const MtWatched watch(e->mt, e->hw_mt, e->hw_mt.begin());
        for (int f0 = 0; f0 < total && !rc; f0 += e->mt_max_frames) {
            const int nf = std::min(e->mt_max_frames, total - f0);
            PtrList64 lp, fp;
            OutList64 op;
            for (int i = 0; i < 64; ++i) { lp.p[i] = nullptr; fp.p[i] = nullptr; op.p[i] = nullptr; }
            for (int i = 0; i < nf; ++i) { lp.p[i] = lptr[f0 + i]; fp.p[i] = fptr[f0 + i]; op.p[i] = optr[f0 + i]; }
            int cbt;
            f16* lat = mt_latent_in(e->mt, &cbt);
            launch_gather_latents(lp, nf, 8, 1024, lat, cbt, e->compute);
            rc = mt_run_locked(e, nullptr, &fp, nf, &op, nullptr);
        }
        return rc;
    });
    if (!rc && mt_gn_error(e->mt)) rc = fail(LTK_E_HIP, std::string("musetalk: ") + mt_graph_error(e->mt));
    return rc;
}

// ================================================================================ Whisper audio features
int ltk_whisper_load(ltk_engine* e, const ltk_named_tensor* encoder_sd, int n) {
    if (!e || !encoder_sd || n <= 0) return fail(LTK_E_INVALID, "bad arguments");
    std::lock_guard<std::mutex> g(e->mu);
    if (e->whisper) return fail(LTK_E_STATE, "a Whisper encoder is already loaded in this engine");
    CHK(enter_device(e->device));
    MtGraph* wg = mt_graph_new();
    if (mt_build_whisper_graph(wg, encoder_sd, n)) {
        const std::string msg = mt_graph_error(wg);
        mt_graph_delete(wg);
        return fail(LTK_E_INVALID, "whisper: " + msg);
    }
    std::vector<float> basis;
    std::vector<int32_t> lohi;
    build_mel_basis(&basis, &lohi, 201, 0.0, 8000.0);     // WhisperFeatureExtractor.mel_filters (slaney, 80 x 201)
    CHK(hipMalloc((void**)&e->d_wbasis, basis.size() * sizeof(float)));
    CHK(hipMemcpy(e->d_wbasis, basis.data(), basis.size() * sizeof(float), hipMemcpyHostToDevice));
    CHK(hipMalloc((void**)&e->d_wlogspec, (size_t)80 * 3000 * sizeof(float)));
    CHK(hipMalloc((void**)&e->d_wpcm, (size_t)480000 * sizeof(float)));
    CHK(hipMalloc((void**)&e->d_wgmax, 16));
    if (e->hw_whisper.alloc(mt_op_count(wg))) {       // nothing half-loaded stays behind
        (void)hipFree(e->d_wbasis); (void)hipFree(e->d_wlogspec); (void)hipFree(e->d_wpcm); (void)hipFree(e->d_wgmax);
        e->d_wbasis = nullptr; e->d_wlogspec = nullptr; e->d_wpcm = nullptr; e->d_wgmax = nullptr;
        mt_graph_delete(wg);
        return fail(LTK_E_NOMEM, "health table allocation failed");
    }
    e->whisper = wg;
    return LTK_OK;
}

}  // extern "C"

namespace {

// under e->mu: one clip through the single-clip program (upload, log-mel, encoder, chunk gather), enqueued on the compute stream
// (`watched`: the engine call is one of a headroom watch's, ltk_health_watch)
int whisper_step_locked(ltk_engine* e, const float* pcm, int n_samples, int batch, int first_row, int row_step, int rows, void* d_out, bool watched) {
    hipStream_t s = e->compute;
    const MtWatched watch(e->whisper, e->hw_whisper, watched);
    CHK(hipMemcpyAsync(e->d_wpcm, pcm, (size_t)n_samples * sizeof(float), hipMemcpyHostToDevice, s));
    int cbt, cb0;
    f16* mel = mt_latent_in(e->whisper, &cbt);
    launch_whisper_logmel(e->d_wpcm, n_samples, e->d_wbasis, e->d_wlogspec, e->d_wgmax, mel, s);
    int rc = run_program(e, e->whisper, 1);
    if (rc) rc = fail(LTK_E_INVALID, std::string("whisper: ") + mt_graph_error(e->whisper));
    if (!rc) {
        WhisperStates st;
        for (int i = 0; i < 5; ++i) { st.p[i] = mt_whisper_state(e->whisper, i, &cbt, &cb0); st.cb0[i] = cb0; }
        launch_whisper_chunks(st, 1500, batch, first_row, row_step, rows, (float*)d_out, s);
        if (hipGetLastError() != hipSuccess) rc = fail(LTK_E_HIP, "whisper kernels failed to launch");
    }
    return rc;
}

// under e->mu, on the first batched run: the 16-clip program over the loaded encoder's weights and its staging.  All or nothing: a
// failed build leaves the engine as it was (the single-clip path keeps working) and is tried again by the next batched run.
int whisper_batch_build(ltk_engine* e) {
    if (e->whisper_b) return LTK_OK;
    MtGraph* g = mt_graph_new();
    const int brc = mt_build_whisper_batch_graph(g, e->whisper, kWhisperBatchClips);
    float *pcm = nullptr, *logspec = nullptr;
    int* gmax = nullptr;
    const bool ok = !brc && hipMalloc((void**)&pcm, (size_t)kWhisperBatchClips * 480000 * sizeof(float)) == hipSuccess &&
                    hipMalloc((void**)&logspec, (size_t)kWhisperBatchClips * 80 * 3000 * sizeof(float)) == hipSuccess &&
                    hipMalloc((void**)&gmax, (size_t)kWhisperBatchClips * sizeof(int)) == hipSuccess;
    if (!ok) {
        const int rc = brc == -1 ? fail(LTK_E_INVALID, std::string("whisper: ") + mt_graph_error(g))
                                 : fail(LTK_E_NOMEM, "whisper: the batched program's buffers could not be allocated");
        (void)hipGetLastError();
        if (pcm) (void)hipFree(pcm);
        if (logspec) (void)hipFree(logspec);
        if (gmax) (void)hipFree(gmax);
        mt_graph_delete(g);
        return rc;
    }
    e->whisper_b = g; e->d_wbpcm = pcm; e->d_wblogspec = logspec; e->d_wbgmax = gmax;
    return LTK_OK;
}

// under e->mu: requests reqs[0..nf) as the nf images of one run of the batched program
int whisper_batch_run_locked(ltk_engine* e, const ltk_whisper_req* reqs, int nf, bool watched) {
    int rc = whisper_batch_build(e);
    if (rc) return rc;
    const MtWatched watch(e->whisper_b, e->hw_whisper, watched);      // the single-clip program's table: one op list
    hipStream_t s = e->compute;
    // every clip by a pageable copy of its own, as the single step's: the runtime has read the caller's samples when the call returns,
    // so no host staging block of ours can be refilled under a copy of the call in flight in front (the device block is stream-ordered)
    WhisperClipTab ct = {};
    for (int i = 0; i < nf; ++i) {
        ct.n_samples[i] = reqs[i].n_samples; ct.pcm_off[i] = i * 480000;
        CHK(hipMemcpyAsync(e->d_wbpcm + (size_t)ct.pcm_off[i], reqs[i].pcm, (size_t)reqs[i].n_samples * sizeof(float), hipMemcpyHostToDevice, s));
    }
    int cbt, cb0;
    f16* mel = mt_latent_in(e->whisper_b, &cbt);
    launch_whisper_logmel_batch(e->d_wbpcm, ct, nf, e->d_wbasis, e->d_wblogspec, e->d_wbgmax, mel, (size_t)cbt * 3000 * 16, s);
    rc = run_program(e, e->whisper_b, nf);
    if (rc) return fail(LTK_E_INVALID, std::string("whisper: ") + mt_graph_error(e->whisper_b));
    e->whisper_b_nf = nf;
    WhisperStatesN st;
    for (int i = 0; i < 5; ++i) {
        st.p[i] = mt_whisper_state(e->whisper_b, i, &cbt, &cb0);
        st.cb0[i] = cb0; st.img_halfs[i] = (size_t)cbt * 1500 * 16;
    }
    WhisperChunkTab tab;
    tab.n = nf; tab.total = 0;
    for (int i = 0; i < nf; ++i) {
        tab.r[i] = {(float*)reqs[i].d_out, i, reqs[i].batch, reqs[i].first_row, reqs[i].row_step, reqs[i].rows, tab.total};
        tab.total += reqs[i].batch * reqs[i].rows * 5 * 48;
    }
    for (int i = nf; i < kWhisperBatchClips; ++i) tab.r[i] = {nullptr, 0, 0, 0, 0, 0, tab.total};
    launch_whisper_chunks_batch(st, tab, 1500, s);
    if (hipGetLastError() != hipSuccess) return fail(LTK_E_HIP, "whisper kernels failed to launch");
    return LTK_OK;
}

}  // namespace

extern "C" {

int ltk_whisper_step(ltk_engine* e, const float* pcm, int n_samples, int batch, int first_row, int row_step, int rows, void* d_out,
                     void* stream) {
    if (!e || !pcm || !d_out || n_samples <= 0 || n_samples > 479000 || batch <= 0 || rows <= 0 || rows > 64)
        return fail(LTK_E_INVALID, "bad arguments");
    if (!e->whisper) return fail(LTK_E_STATE, "ltk_whisper_load has not been called");
    CHK(enter_device(e->device));
    return infer_call(e, stream, [&]() -> int {
        return whisper_step_locked(e, pcm, n_samples, batch, first_row, row_step, rows, d_out, e->hw_whisper.begin());
    });
}

// N concurrent live steps in one call.  whisper_batch_plan cuts the call into runs of at most kWhisperBatchClips in request order; a
// run of more than one uploads its clips into one device block, takes every clip's log-mel features with its own maximum word in one
// launch pair, forwards them as the images of ONE run of the batched program (captured per clip count as every program, run_program)
// and gathers every request's chunks from its own image in one launch.  A run of one request takes ltk_whisper_step's path.
int ltk_whisper_step_batch(ltk_engine* e, const ltk_whisper_req* reqs, int nreq) {
    if (!reqs || nreq <= 0) return fail(LTK_E_INVALID, "bad arguments");
    const std::vector<WhisperRun> runs = whisper_batch_plan(nreq, kWhisperBatchClips);
    for (int r = 0; r < nreq; ++r)          // every request before the first launch: a refused call has touched nothing
        if (!reqs[r].pcm || !reqs[r].d_out || reqs[r].n_samples <= 0 || reqs[r].n_samples > 479000 || reqs[r].batch <= 0 || reqs[r].rows <= 0 ||
            reqs[r].rows > 64)
            return fail(LTK_E_INVALID, "bad request " + std::to_string(r) + " (0 < n_samples <= 479000, batch positive, 0 < rows <= 64)");
    for (const WhisperRun& run : runs) {    // the work items of a run's one gather launch are counted in an int
        long long items = 0;
        for (int i = 0; i < run.count; ++i) {
            items += (long long)reqs[run.first + i].batch * reqs[run.first + i].rows * 240;
            if (items > 0x7fffffffll) return fail(LTK_E_INVALID, "bad request " + std::to_string(run.first + i) + " (batch too large)");
        }
    }
    if (!e) return fail(LTK_E_INVALID, "bad arguments");
    if (!e->whisper) return fail(LTK_E_STATE, "ltk_whisper_load has not been called");
    if (nreq == 1)
        return ltk_whisper_step(e, reqs[0].pcm, reqs[0].n_samples, reqs[0].batch, reqs[0].first_row, reqs[0].row_step, reqs[0].rows, reqs[0].d_out,
                                nullptr);
    CHK(enter_device(e->device));
    return infer_call(e, nullptr, [&]() -> int {
        const bool watched = e->hw_whisper.begin();
        for (const WhisperRun& run : runs) {
            const ltk_whisper_req* q = reqs + run.first;
            const int rc = run.batched ? whisper_batch_run_locked(e, q, run.count, watched)
                                       : whisper_step_locked(e, q->pcm, q->n_samples, q->batch, q->first_row, q->row_step, q->rows, q->d_out, watched);
            if (rc) return rc;
        }
        return LTK_OK;
    });
}

}  // extern "C"

// ================================================================================ HuBERT-large audio features (Ultralight)
// under e->mu: a program that leaves a cache takes its captured graphs with it (a graph holds its buffers' addresses, and the next
// program may land on the same ones); the stream is drained first.  The HuBERT and the face detector caches drop through here.
void ltk::drop_program_graphs(ltk_engine* e, const MtGraph* old) {
    (void)hipStreamSynchronize(e->compute);
    for (auto it = e->prog_graphs.graphs.begin(); it != e->prog_graphs.graphs.end();) {
        if (it->first.first != (const void*)old) { ++it; continue; }
        if (it->second.exec) (void)hipGraphExecDestroy(it->second.exec);
        it = e->prog_graphs.graphs.erase(it);
    }
}

// The program for clips of n_samples, built on first use over the engine's packed weights; at most kHubertPrograms are kept.  A dropped
// program takes its captured graph with it (the graph holds its buffers' addresses, and the next program may land on the same one).
namespace {
// `cache` = e->hubert_progs (single clips, `frames` 1) or e->hubert_bprogs (batched runs, kHubertBatchClips)
MtGraph* hubert_cached_program(ltk_engine* e, std::vector<ltk_engine::HubertProg>& cache, size_t cap, int n_samples, int frames, int* rc) {
    *rc = LTK_OK;
    for (auto& p : cache)
        if (p.n_samples == n_samples) { p.stamp = ++e->hubert_clock; return p.g; }
    if (cache.size() >= cap) {
        size_t v = 0;
        for (size_t i = 1; i < cache.size(); ++i)
            if (cache[i].stamp < cache[v].stamp) v = i;
        MtGraph* old = cache[v].g;
        drop_program_graphs(e, old);
        if (e->hubert_last == old) e->hubert_last = nullptr;
        if (e->hubert_blast == old) { e->hubert_blast = nullptr; e->hubert_blast_nf = 0; }
        mt_graph_delete(old);
        cache.erase(cache.begin() + v);
    }
    MtGraph* g = mt_graph_new();
    const int brc = mt_build_hubert_program(g, e->hubert_w, n_samples, frames);
    if (brc) {
        *rc = fail(brc == -4 ? LTK_E_NOMEM : LTK_E_INVALID, std::string("hubert: ") + mt_graph_error(g));
        mt_graph_delete(g);
        return nullptr;
    }
    ltk_engine::HubertProg p;
    p.g = g; p.n_samples = n_samples; p.stamp = ++e->hubert_clock;
    cache.push_back(p);
    return g;
}
}  // namespace

MtGraph* ltk::hubert_program(ltk_engine* e, int n_samples, int* rc) {
    return hubert_cached_program(e, e->hubert_progs, kHubertPrograms, n_samples, 1, rc);
}

// The face detector's program for H x W frames, built on first use over the engine's packed weights; at most kFaceDetPrograms are kept.
// A dropped program takes its captured graphs with it, as a HuBERT program does.
MtGraph* ltk::face_det_program(ltk_engine* e, int H, int W, int* rc) {
    *rc = LTK_OK;
    auto& cache = e->face_det_progs;
    for (auto& p : cache)
        if (p.H == H && p.W == W) { p.stamp = ++e->face_det_clock; return p.g; }
    {   // a size the plan refuses must not cost a cached program
        FdPlan pl;
        std::string err;
        if (fd_plan(H, W, e->face_det_images, &pl, &err)) { *rc = fail(LTK_E_INVALID, err); return nullptr; }
    }
    if (cache.size() >= kFaceDetPrograms) {
        size_t v = 0;
        for (size_t i = 1; i < cache.size(); ++i)
            if (cache[i].stamp < cache[v].stamp) v = i;
        MtGraph* old = cache[v].g;
        drop_program_graphs(e, old);
        if (e->face_det_last == old) { e->face_det_last = nullptr; e->face_det_last_n = 0; }
        mt_graph_delete(old);
        cache.erase(cache.begin() + v);
    }
    MtGraph* g = mt_graph_new();
    const int brc = mt_build_face_detect_graph(g, e->face_det_w, nullptr, 0, H, W, e->face_det_images, true);
    if (brc) {
        *rc = fail(brc == -4 ? LTK_E_NOMEM : LTK_E_INVALID, std::string("face detector: ") + mt_graph_error(g));
        mt_graph_delete(g);
        (void)hipGetLastError();
        return nullptr;
    }
    // mt_graph_alloc clears the new buffers with fills on the null stream, which the compute stream does not wait for: a large
    // program's fill could still be running when the first call writes the threshold word and the frames
    (void)hipDeviceSynchronize();
    ltk_engine::FaceDetProg p;
    p.g = g; p.H = H; p.W = W; p.stamp = ++e->face_det_clock;
    cache.push_back(p);
    return g;
}

void ltk::face_det_unload(ltk_engine* e) {
    for (auto& p : e->face_det_progs) mt_graph_delete(p.g);
    e->face_det_progs.clear();
    e->face_det_last = nullptr; e->face_det_last_n = 0;
    if (e->face_det_w) { mt_graph_delete(e->face_det_w); e->face_det_w = nullptr; }
    e->hw_facedet.release();
}

void ltk::hubert_unload(ltk_engine* e) {
    for (auto& p : e->hubert_progs) mt_graph_delete(p.g);
    e->hubert_progs.clear();
    e->hubert_last = nullptr;
    for (auto& p : e->hubert_bprogs) mt_graph_delete(p.g);
    e->hubert_bprogs.clear();
    e->hubert_blast = nullptr; e->hubert_blast_nf = 0;
    if (e->d_hbpcm) { (void)hipFree(e->d_hbpcm); e->d_hbpcm = nullptr; e->hbpcm_cap = 0; }
    if (e->d_hbstats) { (void)hipFree(e->d_hbstats); e->d_hbstats = nullptr; }
    if (e->hubert_w) { mt_graph_delete(e->hubert_w); e->hubert_w = nullptr; }
    if (e->d_hpcm) { (void)hipFree(e->d_hpcm); e->d_hpcm = nullptr; e->hpcm_cap = 0; }
    if (e->d_hstats) { (void)hipFree(e->d_hstats); e->d_hstats = nullptr; }
    e->hw_hubert.release();
    if (e->d_hrows) { (void)hipFree(e->d_hrows); e->d_hrows = nullptr; e->hrows_cap = 0; }
}

namespace {

constexpr int kHubertKernel = 400, kHubertStride = 320, kHubertClip = 320 * 1000;      // audio2feature.py:21-23

// under e->mu: the utterance on the device and its statistics (Wav2Vec2FeatureExtractor normalises over the whole input)
int hubert_upload(ltk_engine* e, const float* pcm, long long n, hipStream_t s) {
    if ((size_t)n > e->hpcm_cap) {
        CHK(hipStreamSynchronize(s));
        if (e->d_hpcm) (void)hipFree(e->d_hpcm);
        e->d_hpcm = nullptr; e->hpcm_cap = 0;
        const size_t cap = std::max((size_t)n, (size_t)kHubertClip + 80);
        CHK(hipMalloc((void**)&e->d_hpcm, cap * sizeof(float)));
        e->hpcm_cap = cap;
    }
    CHK(hipMemcpyAsync(e->d_hpcm, pcm, (size_t)n * sizeof(float), hipMemcpyHostToDevice, s));
    launch_hubert_stats_n(e->d_hpcm, n, 1, e->d_hstats, e->d_hstats + 2, s);
    return LTK_OK;
}

// under e->mu: one forward of samples [off, off + len) of the uploaded utterance; *prog = the program that holds the result
// (`watched`: the engine call is one of a headroom watch's; every program of the model scans into the model's one table)
int hubert_forward(ltk_engine* e, long long off, int len, MtGraph** prog, bool watched) {
    int rc;
    MtGraph* g = hubert_program(e, len, &rc);
    if (!g) return rc;
    const MtWatched watch(g, e->hw_hubert, watched);
    launch_hubert_normalise_n(e->d_hpcm + off, len, 1, e->d_hstats, e->d_hstats + 2, mt_hubert_pcm_in(g), e->compute);
    rc = run_program(e, g, 1);
    if (rc) return conv_status(rc, std::string("hubert: ") + mt_graph_error(g));
    e->hubert_last = g;
    *prog = g;
    return LTK_OK;
}

}  // namespace

extern "C" {

int ltk_hubert_load(ltk_engine* e, const ltk_named_tensor* sd, int n) {
    if (!e || !sd || n <= 0) return fail(LTK_E_INVALID, "bad arguments");
    std::lock_guard<std::mutex> g(e->mu);
    if (e->hubert_w) return fail(LTK_E_STATE, "a HuBERT model is already loaded in this engine");
    CHK(enter_device(e->device));
    MtGraph* wg = mt_graph_new();
    if (mt_build_hubert_weights(wg, sd, n)) {
        const std::string msg = mt_graph_error(wg);
        mt_graph_delete(wg);
        return fail(LTK_E_INVALID, "hubert: " + msg);
    }
    if (!e->d_hstats && hipMalloc((void**)&e->d_hstats, 3 * sizeof(float)) != hipSuccess) {
        mt_graph_delete(wg);
        return fail(LTK_E_NOMEM, "hubert: hipMalloc failed");
    }
    if (e->hw_hubert.alloc(mt_op_count(wg))) {
        mt_graph_delete(wg);
        return fail(LTK_E_NOMEM, "hubert: health table allocation failed");
    }
    e->hubert_w = wg;
    return LTK_OK;
}

int ltk_hubert_features(ltk_engine* e, const float* pcm, long long n_samples, float* out_host, int cap_rows, int* rows) {
    if (!e || !pcm || !out_host || !rows || cap_rows <= 0) return fail(LTK_E_INVALID, "bad arguments");
    if (n_samples < kHubertKernel || n_samples > 0x7fffffffll) return fail(LTK_E_INVALID, "n_samples must be at least 400");
    const int expected = (int)((n_samples - (kHubertKernel - kHubertStride)) / kHubertStride);
    if (cap_rows < expected) return fail(LTK_E_INVALID, "out_host holds " + std::to_string(cap_rows) + " rows, " + std::to_string(expected) + " are needed");
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->hubert_w) return fail(LTK_E_STATE, "ltk_hubert_load has not been called");
    hipStream_t s = e->compute;
    // every return below leaves nothing queued that still reads pcm or writes out_host
    auto drained = [&](int code) { (void)hipStreamSynchronize(s); return code; };
    int rc = hubert_upload(e, pcm, n_samples, s);
    if (rc) return drained(rc);
    // audio2feature.py:24-47: clips of 320 000 samples, each forwarded with the 80 samples behind it; then the tail if it has a kernel's length
    const bool watched = e->hw_hubert.begin();
    std::vector<std::pair<long long, int>> clips;
    const long long n_iter = n_samples / kHubertClip;
    for (long long i = 0; i < n_iter; ++i)
        clips.push_back({i * kHubertClip, (int)std::min<long long>(kHubertClip - kHubertStride + kHubertKernel, n_samples - i * kHubertClip)});
    if (n_samples - n_iter * kHubertClip >= kHubertKernel) clips.push_back({n_iter * kHubertClip, (int)(n_samples - n_iter * kHubertClip)});
    long long total = 0;
    for (auto& c : clips) {
        MtGraph* prog = nullptr;
        rc = hubert_forward(e, c.first, c.second, &prog, watched);
        if (rc) break;
        const int T = mt_hubert_rows(prog);
        const int take = (int)std::max<long long>(0, std::min<long long>(T, expected - total));
        if (take > 0) {
            if ((size_t)T > e->hrows_cap) {
                (void)hipStreamSynchronize(s);
                if (e->d_hrows) (void)hipFree(e->d_hrows);
                e->d_hrows = nullptr; e->hrows_cap = 0;
                if (hipMalloc((void**)&e->d_hrows, (size_t)T * 1024 * sizeof(float)) != hipSuccess) { rc = fail(LTK_E_NOMEM, "hubert: hipMalloc failed"); break; }
                e->hrows_cap = (size_t)T;
            }
            int cbt, cb0;
            const f16* h = mt_hubert_out(prog, &cbt, &cb0);
            launch_hubert_chunks(h, cb0, T, 1, 0, 0, take, e->d_hrows, s);
            if (hipMemcpyAsync(out_host + (size_t)total * 1024, e->d_hrows, (size_t)take * 1024 * sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess) {
                rc = fail(LTK_E_HIP, "hubert: copy of the rows to the host failed"); break;
            }
        }
        // d_hrows and a same-length program's buffers are reused by the next clip
        if (hipStreamSynchronize(s) != hipSuccess) { rc = fail(LTK_E_HIP, "hubert: hipStreamSynchronize failed"); break; }
        total += T;
    }
    if (rc) { (void)hipStreamSynchronize(s); return rc; }
    if (hipGetLastError() != hipSuccess) return fail(LTK_E_HIP, "hubert kernels failed to launch");
    if (std::llabs(total - expected) > 1)
        return fail(LTK_E_INVALID, "hubert: " + std::to_string(total) + " rows for " + std::to_string(expected) + " expected");
    for (long long r = total; r < expected; ++r) memset(out_host + (size_t)r * 1024, 0, 1024 * sizeof(float));      // F.pad with zero rows
    *rows = expected;
    return LTK_OK;
}

int ltk_hubert_step(ltk_engine* e, const float* pcm, int n_samples, int batch, int first_row, int row_step, int rows, void* d_out) {
    if (!e || !pcm || !d_out || n_samples < kHubertKernel || n_samples >= kHubertClip || batch <= 0 || rows <= 0)
        return fail(LTK_E_INVALID, "bad arguments (400 <= n_samples < 320000, batch and rows positive)");
    CHK(enter_device(e->device));
    return infer_call(e, nullptr, [&]() -> int {
        if (!e->hubert_w) return fail(LTK_E_STATE, "ltk_hubert_load has not been called");
        hipStream_t s = e->compute;
        int rc = hubert_upload(e, pcm, n_samples, s);
        if (rc) return rc;
        MtGraph* prog = nullptr;
        rc = hubert_forward(e, 0, n_samples, &prog, e->hw_hubert.begin());
        if (rc) return rc;
        int cbt, cb0;
        const f16* h = mt_hubert_out(prog, &cbt, &cb0);
        launch_hubert_chunks(h, cb0, mt_hubert_rows(prog), batch, first_row, row_step, rows, (float*)d_out, s);
        if (hipGetLastError() != hipSuccess) return fail(LTK_E_HIP, "hubert kernels failed to launch");
        return LTK_OK;
    });
}

// N concurrent live steps in one call.  hubert_batch_plan cuts the call; a batched run uploads its clips into [nf][n] staging, takes
// each clip's statistics in a block of its own, and forwards them as the nf images of ONE program run (captured per (program, nf)
// as every program, run_program), so that the 0.63 GB of weights stream once for all of them; every request then gathers its own
// chunks from its own image.  Runs of one request, and lengths past the budget, take ltk_hubert_step's path one by one.
int ltk_hubert_step_batch(ltk_engine* e, const ltk_hubert_req* reqs, int nreq) {
    if (!reqs || nreq <= 0) return fail(LTK_E_INVALID, "bad arguments");
    for (int r = 0; r < nreq; ++r)          // every request before the first launch: a refused call has touched nothing
        if (!reqs[r].pcm || !reqs[r].d_out || reqs[r].n_samples < kHubertKernel || reqs[r].n_samples >= kHubertClip || reqs[r].batch <= 0 ||
            reqs[r].rows <= 0)
            return fail(LTK_E_INVALID, "bad request " + std::to_string(r) + " (400 <= n_samples < 320000, batch and rows positive)");
    if (!e) return fail(LTK_E_INVALID, "bad arguments");
    if (nreq == 1)
        return ltk_hubert_step(e, reqs[0].pcm, reqs[0].n_samples, reqs[0].batch, reqs[0].first_row, reqs[0].row_step, reqs[0].rows, reqs[0].d_out);
    CHK(enter_device(e->device));
    return infer_call(e, nullptr, [&]() -> int {
        if (!e->hubert_w) return fail(LTK_E_STATE, "ltk_hubert_load has not been called");
        hipStream_t s = e->compute;
        const bool watched = e->hw_hubert.begin();
        std::vector<int> ns(nreq);
        for (int r = 0; r < nreq; ++r) ns[r] = reqs[r].n_samples;
        int cbt, cb0;
        for (const HubertRun& run : hubert_batch_plan(ns.data(), nreq, mt_hubert_layers(e->hubert_w))) {
            const int n = run.n_samples;
            if (!run.batched) {
                const ltk_hubert_req& q = reqs[run.req[0]];
                int rc = hubert_upload(e, q.pcm, n, s);
                if (rc) return rc;
                MtGraph* prog = nullptr;
                rc = hubert_forward(e, 0, n, &prog, watched);
                if (rc) return rc;
                const f16* h = mt_hubert_out(prog, &cbt, &cb0);
                launch_hubert_chunks(h, cb0, mt_hubert_rows(prog), q.batch, q.first_row, q.row_step, q.rows, (float*)q.d_out, s);
                continue;
            }
            const int nf = (int)run.req.size();
            if ((size_t)nf * n > e->hbpcm_cap) {
                CHK(hipStreamSynchronize(s));
                if (e->d_hbpcm) (void)hipFree(e->d_hbpcm);
                e->d_hbpcm = nullptr; e->hbpcm_cap = 0;
                const size_t cap = (size_t)kHubertBatchClips * n;
                CHK(hipMalloc((void**)&e->d_hbpcm, cap * sizeof(float)));
                e->hbpcm_cap = cap;
            }
            if (!e->d_hbstats) CHK(hipMalloc((void**)&e->d_hbstats, (size_t)kHubertBatchClips * 3 * sizeof(float)));
            for (int i = 0; i < nf; ++i)
                CHK(hipMemcpyAsync(e->d_hbpcm + (size_t)i * n, reqs[run.req[i]].pcm, (size_t)n * sizeof(float), hipMemcpyHostToDevice, s));
            launch_hubert_stats_n(e->d_hbpcm, n, nf, e->d_hbstats, e->d_hbstats + 2 * kHubertBatchClips, s);
            int rc;
            MtGraph* g = hubert_cached_program(e, e->hubert_bprogs, kHubertBatchPrograms, n, kHubertBatchClips, &rc);
            if (!g) return rc;
            launch_hubert_normalise_n(e->d_hbpcm, n, nf, e->d_hbstats, e->d_hbstats + 2 * kHubertBatchClips, mt_hubert_pcm_in(g), s);
            const MtWatched watch(g, e->hw_hubert, watched);
            rc = run_program(e, g, nf);
            if (rc) return conv_status(rc, std::string("hubert: ") + mt_graph_error(g));
            e->hubert_blast = g; e->hubert_blast_nf = nf;
            const f16* h = mt_hubert_out(g, &cbt, &cb0);
            for (int i = 0; i < nf; ++i) {
                const ltk_hubert_req& q = reqs[run.req[i]];
                launch_hubert_chunks_img(h, i, cbt, cb0, mt_hubert_rows(g), q.batch, q.first_row, q.row_step, q.rows, (float*)q.d_out, s);
            }
        }
        if (hipGetLastError() != hipSuccess) return fail(LTK_E_HIP, "hubert kernels failed to launch");
        return LTK_OK;
    });
}

// ================================================================================ VAE encoder (avatar preparation)
int ltk_vae_encoder_load(ltk_engine* e, const ltk_named_tensor* vae_sd, int n, int max_faces) {
    if (!e || !vae_sd || n <= 0 || max_faces < 1 || max_faces > 32) return fail(LTK_E_INVALID, "bad arguments (max_faces in [1,32])");
    std::lock_guard<std::mutex> g(e->mu);
    if (e->vae_enc) return fail(LTK_E_STATE, "a VAE encoder is already loaded in this engine");
    CHK(enter_device(e->device));
    MtGraph* vg = mt_graph_new();
    if (mt_build_vae_encoder_graph(vg, vae_sd, n, 2 * max_faces)) {
        const std::string msg = mt_graph_error(vg);
        mt_graph_delete(vg);
        return fail(LTK_E_INVALID, "vae encoder: " + msg);
    }
    e->vae_enc = vg;
    e->vae_enc_faces = max_faces;
    return LTK_OK;
}

int ltk_vae_encode_faces(ltk_engine* e, const uint8_t* faces_bgr, int nfaces, const float* noise, float* latents_out) {
    if (!e || !faces_bgr || !latents_out || nfaces <= 0) return fail(LTK_E_INVALID, "bad arguments");
    if (!e->vae_enc) return fail(LTK_E_STATE, "ltk_vae_encoder_load has not been called");
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    hipStream_t s = e->compute;
    uint8_t* d_faces = nullptr;
    float *d_noise = nullptr, *d_out = nullptr;
    const int cap = e->vae_enc_faces;
    CHK(hipMalloc((void**)&d_faces, (size_t)cap * 65536 * 3));
    CHK(hipMalloc((void**)&d_out, (size_t)cap * 8 * 1024 * sizeof(float)));
    if (noise) CHK(hipMalloc((void**)&d_noise, (size_t)cap * 2 * 4 * 1024 * sizeof(float)));
    int rc = 0;
    for (int f0 = 0; f0 < nfaces && !rc; f0 += cap) {
        const int nf = std::min(cap, nfaces - f0);
        CHK(hipMemcpyAsync(d_faces, faces_bgr + (size_t)f0 * 65536 * 3, (size_t)nf * 65536 * 3, hipMemcpyHostToDevice, s));
        if (noise) CHK(hipMemcpyAsync(d_noise, noise + (size_t)f0 * 2 * 4 * 1024, (size_t)nf * 2 * 4 * 1024 * sizeof(float), hipMemcpyHostToDevice, s));
        int cbt;
        launch_vae_pre(d_faces, nf, mt_latent_in(e->vae_enc, &cbt), s);
        rc = mt_run(e->vae_enc, 2 * nf, e->d_partial, e->partial_cap, s);
        if (rc) { rc = fail(LTK_E_INVALID, std::string("vae encoder: ") + mt_graph_error(e->vae_enc)); break; }
        launch_vae_latents(mt_unet_out(e->vae_enc, &cbt), nf, noise ? d_noise : nullptr, 0.18215f, d_out, s);
        CHK(hipMemcpyAsync(latents_out + (size_t)f0 * 8 * 1024, d_out, (size_t)nf * 8 * 1024 * sizeof(float), hipMemcpyDeviceToHost, s));
        CHK(hipStreamSynchronize(s));
        if (mt_gn_error(e->vae_enc)) { rc = fail(LTK_E_HIP, std::string("vae encoder: ") + mt_graph_error(e->vae_enc)); break; }
    }
    (void)hipFree(d_faces); (void)hipFree(d_out);
    if (d_noise) (void)hipFree(d_noise);
    return rc;
}

// ================================================================================ face parser (avatar preparation: blend masks)
int ltk_face_parse_load(ltk_engine* e, const ltk_named_tensor* sd, int n, int size, int max_images) {
    if (!e || !sd || n <= 0) return fail(LTK_E_INVALID, "bad arguments");
    if (size < 64 || size > 512 || size % 32) return fail(LTK_E_INVALID, "face parser: size must be a multiple of 32 in [64, 512]");
    if (max_images < 1 || max_images > kFpMaxImages) return fail(LTK_E_INVALID, "face parser: max_images must be in [1, 8]");
    std::lock_guard<std::mutex> g(e->mu);
    if (e->face_parse) return fail(LTK_E_STATE, "a face parser is already loaded in this engine");
    CHK(enter_device(e->device));
    MtGraph* fg = mt_graph_new();
    const int rc = mt_build_face_parse_graph(fg, sd, n, size, max_images);
    if (rc) {
        const std::string msg = mt_graph_error(fg);
        mt_graph_delete(fg);
        (void)hipGetLastError();
        return fail(rc == -4 ? LTK_E_NOMEM : LTK_E_INVALID, "face parser: " + msg);
    }
    if (e->hw_faceparse.alloc(mt_op_count(fg))) {       // nothing half-loaded stays behind
        mt_graph_delete(fg);
        return fail(LTK_E_NOMEM, "face parser: health table allocation failed");
    }
    e->face_parse = fg;
    e->face_parse_size = size;
    e->face_parse_images = max_images;
    e->face_parse_last = 0;
    return LTK_OK;
}

int ltk_face_parse(ltk_engine* e, const uint8_t* rgb_host, int n, uint8_t* labels_host) {
    if (!e || !rgb_host || !labels_host || n <= 0) return fail(LTK_E_INVALID, "bad arguments");
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->face_parse) return fail(LTK_E_STATE, "ltk_face_parse_load has not been called");
    hipStream_t s = e->compute;
    const size_t S = (size_t)e->face_parse_size, img = S * S * 3, lab = S * S;
    const int cap = e->face_parse_images;
    const MtWatched watch(e->face_parse, e->hw_faceparse, e->hw_faceparse.begin());      // one engine call = one watched call, whatever its chunks
    int rc = LTK_OK;
    for (int i0 = 0; i0 < n && !rc; i0 += cap) {
        const int nf = std::min(cap, n - i0);
        hipError_t he = hipMemcpyAsync(mt_face_parse_image_in(e->face_parse), rgb_host + (size_t)i0 * img, (size_t)nf * img, hipMemcpyHostToDevice, s);
        if (he != hipSuccess) { rc = fail(LTK_E_HIP, std::string("face parser: upload: ") + hipGetErrorString(he)); break; }
        const int prc = run_program(e, e->face_parse, nf);
        if (prc) { rc = conv_status(prc, std::string("face parser: ") + mt_graph_error(e->face_parse)); break; }
        e->face_parse_last = nf;
        he = hipMemcpyAsync(labels_host + (size_t)i0 * lab, mt_face_parse_labels(e->face_parse), (size_t)nf * lab, hipMemcpyDeviceToHost, s);
        if (he == hipSuccess) he = hipStreamSynchronize(s);       // the one wait of the chunk: the next one refills the image buffer
        if (he != hipSuccess) rc = fail(LTK_E_HIP, std::string("face parser: ") + hipGetErrorString(he));
    }
    if (rc) {                                            // nothing of the call still reads rgb_host or writes labels_host when it returns
        const std::string msg = g_err;
        (void)hipStreamSynchronize(s);
        (void)hipGetLastError();
        return fail(rc, msg);
    }
    return LTK_OK;
}

// ================================================================================ face detector (avatar preparation: face boxes)
int ltk_face_detect_load(ltk_engine* e, const ltk_named_tensor* sd, int n, int max_images) {
    if (!e || !sd || n <= 0) return fail(LTK_E_INVALID, "bad arguments");
    if (max_images < 1 || max_images > kFdMaxImages) return fail(LTK_E_INVALID, "face detector: max_images must be in [1, 16]");
    std::lock_guard<std::mutex> g(e->mu);
    if (e->face_det_w) return fail(LTK_E_STATE, "a face detector is already loaded in this engine");
    CHK(enter_device(e->device));
    MtGraph* wg = mt_graph_new();
    const int rc = mt_build_face_detect_graph(wg, nullptr, sd, n, 32, 32, 1, false);
    if (rc) {
        const std::string msg = mt_graph_error(wg);
        mt_graph_delete(wg);
        (void)hipGetLastError();
        return fail(rc == -4 ? LTK_E_NOMEM : LTK_E_INVALID, "face detector: " + msg);
    }
    if (e->hw_facedet.alloc(mt_op_count(wg))) {        // nothing half-loaded stays behind
        mt_graph_delete(wg);
        return fail(LTK_E_NOMEM, "face detector: health table allocation failed");
    }
    e->face_det_w = wg;
    e->face_det_images = max_images;
    return LTK_OK;
}

int ltk_face_detect(ltk_engine* e, const uint8_t* bgr_host, int n, int H, int W, float thresh, uint32_t* cand_out, int cap, int* counts_out) {
    if (!e || !bgr_host || !cand_out || !counts_out || n <= 0) return fail(LTK_E_INVALID, "bad arguments");
    if (!(thresh >= 0.f && thresh < 1.f)) return fail(LTK_E_INVALID, "face detector: thresh must be in [0, 1)");
    if (cap < 1 || cap > kFdDevCap) return fail(LTK_E_INVALID, "face detector: cap must be in [1, " + std::to_string(kFdDevCap) + "]");
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->face_det_w) return fail(LTK_E_STATE, "ltk_face_detect_load has not been called");
    int rc = LTK_OK;
    MtGraph* prog = face_det_program(e, H, W, &rc);
    if (!prog) return rc;
    hipStream_t s = e->compute;
    const size_t img = (size_t)H * W * 3, rec = (size_t)kFdDevCap * kFdRecWords;
    const int chunk = e->face_det_images;
    const MtWatched watch(prog, e->hw_facedet, e->hw_facedet.begin());           // one engine call = one watched call, whatever its chunks
    // the threshold lives on the device (a captured detect launch reads it there): it is written when a program first runs and when a
    // call brings another value, not per chunk
    if (!mt_face_detect_thresh_is(prog, thresh)) {
        const hipError_t te = hipMemcpyAsync(mt_face_detect_records(prog) + kFdThreshAt, &thresh, sizeof(float), hipMemcpyHostToDevice, s);
        const hipError_t ts = te == hipSuccess ? hipStreamSynchronize(s) : te;       // `thresh` is this call's argument
        if (ts != hipSuccess) return fail(LTK_E_HIP, std::string("face detector: threshold: ") + hipGetErrorString(ts));
        mt_face_detect_set_thresh(prog, thresh);
    }
    std::vector<uint32_t> back(kFdHeadBytes / 4 + (size_t)chunk * rec);
    struct Rec { uint32_t w[kFdRecWords]; };
    for (int i0 = 0; i0 < n && !rc; i0 += chunk) {
        const int nf = std::min(chunk, n - i0);
        // one upload (the frames); the images' counters go back to zero by a fill on the device
        hipError_t he = hipMemsetAsync(mt_face_detect_records(prog), 0, kFdThreshAt, s);
        if (he == hipSuccess) he = hipMemcpyAsync(mt_face_detect_image_in(prog), bgr_host + (size_t)i0 * img, (size_t)nf * img, hipMemcpyHostToDevice, s);
        if (he != hipSuccess) { rc = fail(LTK_E_HIP, std::string("face detector: upload: ") + hipGetErrorString(he)); break; }
        const int prc = run_program(e, prog, nf);
        if (prc) { rc = conv_status(prc, std::string("face detector: ") + mt_graph_error(prog)); break; }
        e->face_det_last = prog; e->face_det_last_n = nf;
        he = hipMemcpyAsync(back.data(), mt_face_detect_records(prog), kFdHeadBytes + (size_t)nf * rec * 4, hipMemcpyDeviceToHost, s);
        if (he == hipSuccess) he = hipStreamSynchronize(s);       // the one wait of the chunk: the next one refills the buffers
        if (he != hipSuccess) { rc = fail(LTK_E_HIP, std::string("face detector: ") + hipGetErrorString(he)); break; }
        for (int i = 0; i < nf; ++i) {
            // arrival order is the atomics': the records of an image leave sorted by key, so the output does not depend on it
            const uint32_t count = back[i];
            const size_t held = std::min<size_t>(count, kFdDevCap);
            Rec* r = reinterpret_cast<Rec*>(back.data() + kFdHeadBytes / 4 + (size_t)i * rec);
            std::sort(r, r + held, [](const Rec& a, const Rec& b) { return a.w[0] < b.w[0]; });
            uint32_t* out = cand_out + (size_t)(i0 + i) * cap * kFdRecWords;
            const size_t keep = std::min<size_t>(held, (size_t)cap);
            memcpy(out, r, keep * sizeof(Rec));
            memset(out + keep * kFdRecWords, 0, ((size_t)cap - keep) * sizeof(Rec));
            counts_out[i0 + i] = (int)std::min<uint32_t>(count, 0x7fffffffu);      // above cap: reported as it is
        }
    }
    if (rc) {                                            // nothing of the call still reads bgr_host when it returns
        const std::string msg = g_err;
        (void)hipStreamSynchronize(s);
        (void)hipGetLastError();
        return fail(rc, msg);
    }
    return LTK_OK;
}

}  // extern "C"

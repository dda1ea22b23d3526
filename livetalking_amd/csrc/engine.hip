// libltk_hip.so: engine lifetime, avatar banks, mel step and paste-back of the C ABI (include/ltk.h).  The Wav2Lip program is
// in w2l_program.hip, its inference path in w2l_infer.hip, MuseTalk / Whisper / VAE encoder in mt_engine.hip, frame egress in
// egress.hip, the Ultralight avatar (launch program, register / infer / paste-back) in ultralight.hip, the test and measurement hooks
// in engine_debug.hip; engine_internal.h is what they share.
#include "engine_internal.h"

thread_local std::string ltk::g_err;

namespace {

// ---- Slaney mel filterbank (librosa.filters.mel semantics: htk=False, norm='slaney', float32),
// as avatars/wav2lip/audio.py:98-101 requests it (sr 16000, n_fft 800, 80 mels, 55..7600 Hz).
double hz_to_mel(double f) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = log(6.4) / 27.0;
    return f >= min_log_hz ? min_log_mel + log(f / min_log_hz) / logstep : f / f_sp;
}
double mel_to_hz(double m) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = log(6.4) / 27.0;
    return m >= min_log_mel ? min_log_hz * exp(logstep * (m - min_log_mel)) : f_sp * m;
}
}  // namespace

void ltk::build_mel_basis(std::vector<float>* basis, std::vector<int32_t>* lohi, int n_bins, double f_lo, double f_hi) {
    const int n_mels = 80;
    const double sr = 16000.0;
    std::vector<double> mel_f(n_mels + 2);
    const double m0 = hz_to_mel(f_lo), m1 = hz_to_mel(f_hi);
    for (int i = 0; i < n_mels + 2; ++i) mel_f[i] = mel_to_hz(m0 + (m1 - m0) * i / (n_mels + 1));
    basis->assign((size_t)n_mels * n_bins, 0.f);
    lohi->assign(2 * n_mels, 0);
    for (int i = 0; i < n_mels; ++i) {
        const double enorm = 2.0 / (mel_f[i + 2] - mel_f[i]);
        int lo = n_bins, hi = 0;
        for (int k = 0; k < n_bins; ++k) {
            const double f = (sr / 2) * k / (n_bins - 1);
            const double lower = -(mel_f[i] - f) / (mel_f[i + 1] - mel_f[i]);
            const double upper = (mel_f[i + 2] - f) / (mel_f[i + 2] - mel_f[i + 1]);
            const double w = fmax(0.0, lower < upper ? lower : upper) * enorm;
            const float wf = (float)w;
            (*basis)[(size_t)i * n_bins + k] = wf;
            if (wf != 0.f) { if (k < lo) lo = k; if (k + 1 > hi) hi = k + 1; }
        }
        if (lo > hi) lo = hi = 0;
        (*lohi)[2 * i] = lo; (*lohi)[2 * i + 1] = hi;
    }
}

// ================================================================================ C ABI
extern "C" {

const char* ltk_last_error(void) { return g_err.c_str(); }
const char* ltk_version(void) { return "ltk_hip 0.1 (gfx950)"; }

int ltk_engine_create(int device, ltk_engine** out) {
    if (!out) return fail(LTK_E_INVALID, "out is null");
    // a knob that no longer exists would be ignored in silence: say so, once per process
    static std::once_flag stale_env;
    if (getenv("LTK_SAT_CHECK"))
        std::call_once(stale_env, [] {
            fprintf(stderr, "ltk: LTK_SAT_CHECK is set, but that knob has been removed and scans nothing: use LTK_HEALTH_WATCH=N "
                            "(ltk_health_watch) or scripts/checkpoint_health.py instead\n");
        });
    int ndev = 0;
    CHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(LTK_E_INVALID, "no such HIP device");
    CHK(hipSetDevice(device));
    std::unique_ptr<ltk_engine> e(new ltk_engine());
    e->device = device;
    CHK(hipStreamCreateWithFlags(&e->compute, hipStreamNonBlocking));
    CHK(hipStreamCreateWithFlags(&e->aux, hipStreamNonBlocking));
    CHK(hipStreamCreateWithFlags(&e->aux2, hipStreamNonBlocking));
    e->graphs.side = e->aux2;
    CHK(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
    CHK(hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming));
    e->partial_cap = (size_t)128 << 20;
    e->partial_aux_cap = (size_t)16 << 20;
    e->partial_pf_cap = (size_t)64 << 20;
    CHK(hipMalloc((void**)&e->d_partial, e->partial_cap));
    CHK(hipMalloc((void**)&e->d_partial_aux, e->partial_aux_cap));
    CHK(hipMalloc((void**)&e->d_partial_pf, e->partial_pf_cap));
    std::vector<float> basis;
    std::vector<int32_t> lohi;
    build_mel_basis(&basis, &lohi);
    CHK(hipMalloc((void**)&e->d_basis, basis.size() * sizeof(float)));
    CHK(hipMemcpy(e->d_basis, basis.data(), basis.size() * sizeof(float), hipMemcpyHostToDevice));
    CHK(hipMalloc((void**)&e->d_lohi, lohi.size() * sizeof(int32_t)));
    CHK(hipMemcpy(e->d_lohi, lohi.data(), lohi.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    *out = e.release();
    return LTK_OK;
}

void ltk_engine_destroy(ltk_engine* e) {
    if (!e) return;
    if (e->tm_calls)
        fprintf(stderr, "ltk: ltk_wav2lip_infer host time per call over %lu calls: prepare %.1f us, upload + pass launch %.1f us, prefetch join / serial launch %.1f us, wait for the device %.1f us, wait for the previous pass (deferred calls) %.1f us\n",
                e->tm_calls, e->tm_prep / e->tm_calls, e->tm_launch / e->tm_calls, e->tm_pf / e->tm_calls, e->tm_wait / e->tm_calls, e->tm_prev / e->tm_calls);
    (void)hipSetDevice(e->device);
    (void)hipDeviceSynchronize();
    (void)drain_pending(e);              // knob DEFER: the banks a pass in flight held go with its record
    e->defer.clear([](hipEvent_t& ev) { if (ev) (void)hipEventDestroy(ev); });
    wav2lip_unload(e);
    if (e->d_basis) (void)hipFree(e->d_basis);
    if (e->d_lohi) (void)hipFree(e->d_lohi);
    e->avatars.clear();
    e->mt_avatars.clear();
    e->prog_graphs.drop();
    ul_unload(e);
    if (e->mt) mt_graph_delete(e->mt);
    if (e->whisper_b) mt_graph_delete(e->whisper_b);      // holds copies of e->whisper's weight handles and frees none of them
    if (e->whisper) mt_graph_delete(e->whisper);
    if (e->d_wbpcm) (void)hipFree(e->d_wbpcm);
    if (e->d_wblogspec) (void)hipFree(e->d_wblogspec);
    if (e->d_wbgmax) (void)hipFree(e->d_wbgmax);
    hubert_unload(e);
    if (e->vae_enc) mt_graph_delete(e->vae_enc);
    if (e->face_parse) mt_graph_delete(e->face_parse);
    face_det_unload(e);
    if (e->d_wbasis) (void)hipFree(e->d_wbasis);
    if (e->d_wlogspec) (void)hipFree(e->d_wlogspec);
    if (e->d_wpcm) (void)hipFree(e->d_wpcm);
    if (e->d_wgmax) (void)hipFree(e->d_wgmax);
    if (e->d_pe) (void)hipFree(e->d_pe);
    if (e->d_mt_feat) (void)hipFree(e->d_mt_feat);
    if (e->d_mt_lat) (void)hipFree(e->d_mt_lat);
    for (Scratch& s : e->scratch_free) (void)hipFree(s.d);
    for (hipStream_t s : e->stream_free) (void)hipStreamDestroy(s);
    if (e->d_partial) (void)hipFree(e->d_partial);
    if (e->d_partial_aux) (void)hipFree(e->d_partial_aux);
    if (e->d_partial_pf) (void)hipFree(e->d_partial_pf);
    if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
    if (e->ev_join) (void)hipEventDestroy(e->ev_join);
    if (e->aux2) (void)hipStreamDestroy(e->aux2);
    if (e->aux) (void)hipStreamDestroy(e->aux);
    if (e->compute) (void)hipStreamDestroy(e->compute);
    delete e;
}

int ltk_engine_sync(ltk_engine* e) {
    if (!e) return fail(LTK_E_INVALID, "engine is null");
    CHK(enter_device(e->device));
    const hipError_t se = hipDeviceSynchronize();
    const int drc = drain_pending(e);     // knob DEFER: the window is empty afterwards; a pass that failed on the device is reported here
    if (se != hipSuccess) return fail(LTK_E_HIP, std::string("hipDeviceSynchronize(): ") + hipGetErrorString(se));
    return drc;
}

int ltk_avatar_register(ltk_engine* e, const uint8_t* face_bank, const uint8_t* full_bank,
                        const int32_t* coords, int n, int H, int W, int* avatar_id) {
    if (!e || !face_bank || !full_bank || !coords || !avatar_id || n <= 0 || H <= 0 || W <= 0)
        return fail(LTK_E_INVALID, "bad arguments");
    for (int i = 0; i < n; ++i) {
        const int32_t* c = coords + 4 * i;  // (y1,y2,x1,x2), wav2lip_avatar.py:144
        if (c[0] < 0 || c[2] < 0 || c[1] > H || c[3] > W || c[1] <= c[0] || c[3] <= c[2])
            return fail(LTK_E_INVALID, "coords box outside the frame");
    }
    CHK(enter_device(e->device));
    auto ap = std::make_shared<Avatar>();
    Avatar& a = *ap;
    a.device = e->device;
    a.n = n; a.H = H; a.W = W;
    a.coords.assign(coords, coords + 4 * (size_t)n);
    const size_t fb = (size_t)n * 256 * 256 * 3, ub = (size_t)n * H * W * 3;
    CHK(hipMalloc((void**)&a.d_face, fb));
    CHK(hipMalloc((void**)&a.d_full, ub));
    CHK(hipMemcpy(a.d_face, face_bank, fb, hipMemcpyHostToDevice));
    CHK(hipMemcpy(a.d_full, full_bank, ub, hipMemcpyHostToDevice));
    std::lock_guard<std::mutex> g(e->pool_mu);
    const int id = e->next_avatar++;
    e->avatars[id] = ap;
    *avatar_id = id;
    return LTK_OK;
}

int ltk_avatar_release(ltk_engine* e, int avatar_id) {
    if (!e) return fail(LTK_E_INVALID, "engine is null");
    // knob DEFER: a pass in flight keeps the banks it reads through its record; the release waits for it, so that - as without the
    // knob - the bank's memory is free when the last holder lets go and nothing enqueued still names the id
    if (e->defer.newest()) { (void)hipSetDevice(e->device); (void)drain_pending(e); }
    {   // prefetch slots keyed by this avatar: their data will never be asked for again, and their hold on the bank goes once the
        // prefetch that reads it has finished (ids are never reused, so a stale key could not match anyway)
        std::lock_guard<std::mutex> ge(e->mu);
        for (ltk_engine::PfSlot& sl : e->pfs)
            if (sl.avatar == avatar_id && (sl.valid || sl.hold)) {
                if (sl.filled && sl.ev_done) (void)hipEventSynchronize(sl.ev_done);
                sl.valid = false;
                sl.hold.reset();
            }
        ul_drop_graphs(e, avatar_id);        // the captured passes of an Ultralight avatar hold its weights' addresses
    }
    std::lock_guard<std::mutex> g(e->pool_mu);
    auto it = e->avatars.find(avatar_id);
    if (it != e->avatars.end()) { e->avatars.erase(it); return LTK_OK; }      // buffers go with the last call that still uses them
    auto mt = e->mt_avatars.find(avatar_id);                                       // ids of both kinds come from one counter
    if (mt != e->mt_avatars.end()) { e->mt_avatars.erase(mt); return LTK_OK; }
    auto ul = e->ul_avatars.find(avatar_id);
    if (ul != e->ul_avatars.end()) { e->ul_avatars.erase(ul); return LTK_OK; }
    return fail(LTK_E_STATE, "unknown avatar id");
}

int ltk_mel_step(ltk_engine* e, const float* pcm, int n_samples, const int32_t* win_start, int n_win,
                 void* d_out, void* stream) {
    if (!e || !pcm || !win_start || !d_out || n_samples <= 0 || n_win <= 0 || n_win > 1024)
        return fail(LTK_E_INVALID, "bad arguments");
    const int n_cols_total = 1 + n_samples / 200;  // librosa.stft(center=True)
    int cmin = 1 << 30, cmax = -1;
    for (int i = 0; i < n_win; ++i) {
        if (win_start[i] < 0 || win_start[i] + 16 > n_cols_total) return fail(LTK_E_INVALID, "mel window outside the spectrogram");
        if (win_start[i] < cmin) cmin = win_start[i];
        if (win_start[i] + 15 > cmax) cmax = win_start[i] + 15;
    }
    CHK(enter_device(e->device));
    const size_t pcm_bytes = (size_t)n_samples * sizeof(float);
    const size_t ws_off = (pcm_bytes + 255) / 256 * 256;
    ScratchLease sc(e, ws_off + (size_t)n_win * sizeof(int32_t));
    if (!sc.s.d) return fail(LTK_E_NOMEM, "scratch allocation failed");
    StreamLease sl(e, stream);
    CHK(hipMemcpyAsync(sc.s.d, pcm, pcm_bytes, hipMemcpyHostToDevice, sl.s));
    CHK(hipMemcpyAsync((char*)sc.s.d + ws_off, win_start, (size_t)n_win * sizeof(int32_t), hipMemcpyHostToDevice, sl.s));
    launch_mel((const float*)sc.s.d, n_samples, (const int32_t*)((char*)sc.s.d + ws_off), n_win, cmin, cmax - cmin + 1,
               e->d_basis, e->d_lohi, (float*)d_out, sl.s);
    CHK(hipGetLastError());
    CHK(hipStreamSynchronize(sl.s));
    return LTK_OK;
}

int ltk_paste_back(ltk_engine* e, int avatar_id, int idx, const void* d_pred, void* out, int out_is_device, void* stream) {
    if (!e || !d_pred || !out) return fail(LTK_E_INVALID, "bad arguments");
    const std::shared_ptr<Avatar> ap = find_avatar(e, avatar_id);
    if (!ap) return fail(LTK_E_STATE, "unknown avatar id");
    const Avatar& a = *ap;
    if (idx < 0 || idx >= a.n) return fail(LTK_E_INVALID, "frame index outside the bank");
    CHK(enter_device(e->device));
    const int32_t* c = a.coords.data() + 4 * (size_t)idx;
    const size_t bytes = (size_t)a.H * a.W * 3;
    StreamLease sl(e, stream);
    CHK(order_behind_pending(e, sl.s, d_pred, (size_t)256 * 256 * 3));      // knob DEFER: the pass that writes the frame may be in flight
    const uint8_t* full = a.d_full + (size_t)idx * bytes;
    if (out_is_device) {
        launch_paste(full, a.H, a.W, (const uint8_t*)d_pred, c[0], c[1], c[2], c[3], (uint8_t*)out, sl.s);
        CHK(hipGetLastError());
        CHK(hipStreamSynchronize(sl.s));
        return LTK_OK;
    }
    ScratchLease sc(e, bytes);
    if (!sc.s.d) return fail(LTK_E_NOMEM, "scratch allocation failed");
    launch_paste(full, a.H, a.W, (const uint8_t*)d_pred, c[0], c[1], c[2], c[3], (uint8_t*)sc.s.d, sl.s);
    CHK(hipGetLastError());
    CHK(hipMemcpyAsync(out, sc.s.d, bytes, hipMemcpyDeviceToHost, sl.s));
    CHK(hipStreamSynchronize(sl.s));
    return LTK_OK;
}

int ltk_paste_back_batch(ltk_engine* e, int avatar_id, const int32_t* idx, const void* d_pred, int n, void* out, void* stream) {
    if (!e || !idx || !d_pred || !out || n <= 0) return fail(LTK_E_INVALID, "bad arguments");
    const std::shared_ptr<Avatar> ap = find_avatar(e, avatar_id);
    if (!ap) return fail(LTK_E_STATE, "unknown avatar id");
    const Avatar& a = *ap;
    for (int i = 0; i < n; ++i)
        if (idx[i] < 0 || idx[i] >= a.n) return fail(LTK_E_INVALID, "frame index outside the bank");
    CHK(enter_device(e->device));
    const size_t bytes = (size_t)a.H * a.W * 3;
    StreamLease sl(e, stream);
    ScratchLease sc(e, bytes * n);
    if (!sc.s.d) return fail(LTK_E_NOMEM, "scratch allocation failed");
    CHK(order_behind_pending(e, sl.s, d_pred, (size_t)n * 256 * 256 * 3));  // knob DEFER: the pass that writes the frames may be in flight
    for (int i0 = 0; i0 < n; i0 += kPasteBatch) {          // one launch per 16 frames
        const int m = std::min(kPasteBatch, n - i0);
        PasteBatch pb;
        for (int i = 0; i < m; ++i) {
            const int32_t* c = a.coords.data() + 4 * (size_t)idx[i0 + i];
            pb.full[i] = a.d_full + (size_t)idx[i0 + i] * bytes;
            pb.y1[i] = c[0]; pb.y2[i] = c[1]; pb.x1[i] = c[2]; pb.x2[i] = c[3];
        }
        launch_paste_batch(pb, m, a.H, a.W, (const uint8_t*)d_pred + (size_t)i0 * 256 * 256 * 3, (uint8_t*)sc.s.d + (size_t)i0 * bytes, bytes, sl.s);
    }
    // an error past this point must not hand the scratch back to the pool while earlier launches may still be writing it
    hipError_t pe = hipGetLastError();
    if (pe == hipSuccess) pe = hipMemcpyAsync(out, sc.s.d, bytes * n, hipMemcpyDeviceToHost, sl.s);
    const hipError_t se = hipStreamSynchronize(sl.s);
    if (pe != hipSuccess || se != hipSuccess) return fail(LTK_E_HIP, std::string("paste_back_batch: ") + hipGetErrorString(pe != hipSuccess ? pe : se));
    return LTK_OK;
}

int ltk_paste_blend(ltk_engine* e, int avatar_id, int idx, const void* d_pred, void* out, int out_is_device, void* stream) {
    if (!e || !d_pred || !out) return fail(LTK_E_INVALID, "bad arguments");
    const std::shared_ptr<MtAvatar> hold = find_mt_avatar(e, avatar_id);
    if (!hold) return fail(LTK_E_STATE, "unknown MuseTalk avatar id");
    const MtAvatar& a = *hold;
    if (idx < 0 || idx >= a.n) return fail(LTK_E_INVALID, "frame index outside the bank");
    const int H = a.H, W = a.W;
    const uint8_t* full = a.d_full + (size_t)idx * H * W * 3;
    const uint8_t* mask = a.d_masks + a.mask_off[idx];
    const int32_t* fb = a.face_box.data() + 4 * (size_t)idx;
    const int32_t* cb = a.crop_box.data() + 4 * (size_t)idx;
    CHK(enter_device(e->device));
    const size_t bytes = (size_t)H * W * 3;
    StreamLease sl(e, stream);
    if (out_is_device) {
        launch_paste_blend(full, H, W, (const uint8_t*)d_pred, fb[0], fb[1], fb[2], fb[3], cb[0], cb[1], cb[2], cb[3], mask, (uint8_t*)out, sl.s);
        CHK(hipGetLastError());
        CHK(hipStreamSynchronize(sl.s));
        return LTK_OK;
    }
    ScratchLease sc(e, bytes);
    if (!sc.s.d) return fail(LTK_E_NOMEM, "scratch allocation failed");
    launch_paste_blend(full, H, W, (const uint8_t*)d_pred, fb[0], fb[1], fb[2], fb[3], cb[0], cb[1], cb[2], cb[3], mask, (uint8_t*)sc.s.d, sl.s);
    CHK(hipGetLastError());
    CHK(hipMemcpyAsync(out, sc.s.d, bytes, hipMemcpyDeviceToHost, sl.s));
    CHK(hipStreamSynchronize(sl.s));
    return LTK_OK;
}

}  // extern "C"

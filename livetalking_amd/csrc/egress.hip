#include "engine_internal.h"

// ------------------------------------------------------------------ frame egress (base_avatar.py:384-453)
struct ltk_egress {
    int H = 0, W = 0;
    std::mutex mu;                     // one frame at a time per session (the reference's process thread is serial)
    uint8_t* d_cache[2] = {nullptr, nullptr};   // [0] _last_silent_frame, [1] _last_speaking_frame
    bool have[2] = {false, false};
    uint8_t* d_frame = nullptr;        // composite / uploaded frame
    uint8_t* d_out = nullptr;          // converted frame before the D2H copy
    uint8_t* d_wm = nullptr;
    int wm_x = 0, wm_y = 0, wm_w = 0, wm_h = 0, wm_b = 0, wm_g = 0, wm_r = 0;
};

extern "C" {

int ltk_egress_open(ltk_engine* e, int H, int W, ltk_egress** out) {
    if (!e || !out || H <= 0 || W <= 0) return fail(LTK_E_INVALID, "bad arguments");
    CHK(enter_device(e->device));
    ltk_egress* s = new ltk_egress();
    s->H = H; s->W = W;
    const size_t bytes = (size_t)H * W * 3;
    if (hipMalloc((void**)&s->d_cache[0], bytes) != hipSuccess || hipMalloc((void**)&s->d_cache[1], bytes) != hipSuccess ||
        hipMalloc((void**)&s->d_frame, bytes) != hipSuccess || hipMalloc((void**)&s->d_out, bytes) != hipSuccess) {
        (void)hipFree(s->d_cache[0]); (void)hipFree(s->d_cache[1]); (void)hipFree(s->d_frame); (void)hipFree(s->d_out);
        delete s;
        return fail(LTK_E_NOMEM, "egress session buffers");
    }
    *out = s;
    return LTK_OK;
}

int ltk_egress_close(ltk_engine* e, ltk_egress* s) {
    if (!e || !s) return fail(LTK_E_INVALID, "bad arguments");
    CHK(enter_device(e->device));
    {
        std::lock_guard<std::mutex> g(s->mu);
        (void)hipFree(s->d_cache[0]); (void)hipFree(s->d_cache[1]); (void)hipFree(s->d_frame); (void)hipFree(s->d_out); (void)hipFree(s->d_wm);
    }
    delete s;
    return LTK_OK;
}

int ltk_egress_watermark(ltk_engine* e, ltk_egress* s, const uint8_t* mask, int x, int y, int w, int h, int b, int g, int r) {
    if (!e || !s) return fail(LTK_E_INVALID, "bad arguments");
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> gd(s->mu);
    (void)hipFree(s->d_wm);
    s->d_wm = nullptr;
    s->wm_w = s->wm_h = 0;
    if (!mask) return LTK_OK;
    if (w <= 0 || h <= 0) return fail(LTK_E_INVALID, "empty watermark rectangle");
    CHK(hipMalloc((void**)&s->d_wm, (size_t)w * h));
    CHK(hipMemcpy(s->d_wm, mask, (size_t)w * h, hipMemcpyHostToDevice));
    s->wm_x = x; s->wm_y = y; s->wm_w = w; s->wm_h = h; s->wm_b = b; s->wm_g = g; s->wm_r = r;
    return LTK_OK;
}

int ltk_egress_frame(ltk_engine* e, ltk_egress* s, const ltk_egress_req* q, uint8_t* h_out, void* stream) {
    if (!e || !s || !q || !h_out) return fail(LTK_E_INVALID, "bad arguments");
    const int H = s->H, W = s->W;
    const size_t bytes = (size_t)H * W * 3;
    if (q->format != LTK_FMT_BGR24 && q->format != LTK_FMT_I420) return fail(LTK_E_INVALID, "unknown output format");
    if (q->format == LTK_FMT_I420 && ((H | W) & 1)) return fail(LTK_E_INVALID, "I420 needs even frame dimensions");
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> gs(s->mu);
    StreamLease sl(e, stream);
    const uint8_t* src = nullptr;
    std::shared_ptr<Avatar> hold_w;           // keep the bank alive until the stream has been synchronised below
    std::shared_ptr<MtAvatar> hold_m;
    std::shared_ptr<UlAvatar> hold_u;
    if (q->source == LTK_SRC_HOST) {
        if (!q->h_frame) return fail(LTK_E_INVALID, "LTK_SRC_HOST without h_frame");
        CHK(hipMemcpyAsync(s->d_frame, q->h_frame, bytes, hipMemcpyHostToDevice, sl.s));
        src = s->d_frame;
    } else if (q->source == LTK_SRC_WAV2LIP) {
        if (!(hold_w = find_avatar(e, q->avatar))) return fail(LTK_E_STATE, "unknown avatar id");
        const Avatar& a = *hold_w;
        if (q->idx < 0 || q->idx >= a.n) return fail(LTK_E_INVALID, "frame index outside the bank");
        if (a.H != H || a.W != W) return fail(LTK_E_INVALID, "avatar frame size differs from the egress session");
        const uint8_t* full = a.d_full + (size_t)q->idx * bytes;
        if (q->d_pred) {
            const int32_t* c = a.coords.data() + 4 * (size_t)q->idx;
            CHK(order_behind_pending(e, sl.s, q->d_pred, (size_t)256 * 256 * 3));     // knob DEFER: the pass that writes the frame may be in flight
            launch_paste(full, H, W, (const uint8_t*)q->d_pred, c[0], c[1], c[2], c[3], s->d_frame, sl.s);
            src = s->d_frame;
        } else {
            src = full;                               // base_avatar.py:417: the cached frame itself
        }
    } else if (q->source == LTK_SRC_MUSETALK) {
        if (!(hold_m = find_mt_avatar(e, q->avatar))) return fail(LTK_E_STATE, "unknown MuseTalk avatar id");
        const MtAvatar& a = *hold_m;
        if (q->idx < 0 || q->idx >= a.n) return fail(LTK_E_INVALID, "frame index outside the bank");
        if (a.H != H || a.W != W) return fail(LTK_E_INVALID, "avatar frame size differs from the egress session");
        const uint8_t* full = a.d_full + (size_t)q->idx * bytes;
        const uint8_t* mask = a.d_masks + a.mask_off[q->idx];
        const int32_t* fb = a.face_box.data() + 4 * (size_t)q->idx;
        const int32_t* cb = a.crop_box.data() + 4 * (size_t)q->idx;
        if (q->d_pred) {
            launch_paste_blend(full, H, W, (const uint8_t*)q->d_pred, fb[0], fb[1], fb[2], fb[3], cb[0], cb[1], cb[2], cb[3], mask,
                               s->d_frame, sl.s);
            src = s->d_frame;
        } else {
            src = full;
        }
    } else if (q->source == LTK_SRC_ULTRALIGHT) {
        if (!(hold_u = find_ul_avatar(e, q->avatar))) return fail(LTK_E_STATE, "unknown Ultralight avatar id");
        const UlAvatar& a = *hold_u;
        if (q->idx < 0 || q->idx >= a.n) return fail(LTK_E_INVALID, "frame index outside the bank");
        if (a.H != H || a.W != W) return fail(LTK_E_INVALID, "avatar frame size differs from the egress session");
        const uint8_t* full = a.d_full + (size_t)q->idx * bytes;
        if (q->d_pred) {
            const int32_t* c = a.boxes.data() + 4 * (size_t)q->idx;      // (x1, y1, x2, y2)
            launch_ul_paste(full, H, W, a.d_face + (size_t)q->idx * kUlFace * kUlFace * 3, (const uint8_t*)q->d_pred, c[0], c[1], c[2], c[3],
                            s->d_frame, sl.s);
            src = s->d_frame;
        } else {
            src = full;
        }
    } else {
        return fail(LTK_E_INVALID, "unknown frame source");
    }
    const int me = q->speaking ? 1 : 0, other = me ^ 1;
    const bool blend = q->alpha >= 0.0 && q->alpha < 1.0 && s->have[other];
    // cv2.addWeighted(other, 1 - alpha, frame, alpha, 0): the weights are Python doubles there, OpenCV's 8-bit kernel
    // computes in float32
    const float w_src = (float)q->alpha, w_prev = (float)(1.0 - q->alpha);
    launch_egress(src, blend ? s->d_cache[other] : nullptr, w_prev, w_src, q->keep ? s->d_cache[me] : nullptr, s->d_wm, s->wm_x,
                  s->wm_y, s->wm_w, s->wm_h, s->wm_b, s->wm_g, s->wm_r, s->d_out, H, W, q->format == LTK_FMT_I420, q->chroma, sl.s);
    CHK(hipGetLastError());
    if (q->keep) s->have[me] = true;
    const size_t out_bytes = q->format == LTK_FMT_I420 ? bytes / 2 : bytes;
    CHK(hipMemcpyAsync(h_out, s->d_out, out_bytes, hipMemcpyDeviceToHost, sl.s));
    CHK(hipStreamSynchronize(sl.s));
    return LTK_OK;
}

int ltk_egress_batch(ltk_engine* e, ltk_egress* s, int source, int avatar, const int32_t* idx, const void* d_pred, int n, int format,
                     int chroma, uint8_t* h_out, void* stream) {
    if (!e || !s || !idx || !d_pred || !h_out || n <= 0) return fail(LTK_E_INVALID, "bad arguments");
    const int H = s->H, W = s->W;
    const size_t bytes = (size_t)H * W * 3;
    if (format != LTK_FMT_BGR24 && format != LTK_FMT_I420) return fail(LTK_E_INVALID, "unknown output format");
    if (format == LTK_FMT_I420 && ((H | W) & 1)) return fail(LTK_E_INVALID, "I420 needs even frame dimensions");
    if (source != LTK_SRC_WAV2LIP && source != LTK_SRC_MUSETALK && source != LTK_SRC_ULTRALIGHT)
        return fail(LTK_E_INVALID, "batch egress: Wav2Lip, MuseTalk or Ultralight frames only");
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> gs(s->mu);
    std::shared_ptr<Avatar> hold_w;           // keep the bank alive until the stream has been synchronised below
    std::shared_ptr<MtAvatar> hold_m;
    std::shared_ptr<UlAvatar> hold_u;
    int bank_n, bank_h, bank_w;
    if (source == LTK_SRC_WAV2LIP) {
        if (!(hold_w = find_avatar(e, avatar))) return fail(LTK_E_STATE, "unknown avatar id");
        bank_n = hold_w->n; bank_h = hold_w->H; bank_w = hold_w->W;
    } else if (source == LTK_SRC_MUSETALK) {
        if (!(hold_m = find_mt_avatar(e, avatar))) return fail(LTK_E_STATE, "unknown MuseTalk avatar id");
        bank_n = hold_m->n; bank_h = hold_m->H; bank_w = hold_m->W;
    } else {
        if (!(hold_u = find_ul_avatar(e, avatar))) return fail(LTK_E_STATE, "unknown Ultralight avatar id");
        bank_n = hold_u->n; bank_h = hold_u->H; bank_w = hold_u->W;
    }
    if (bank_h != H || bank_w != W) return fail(LTK_E_INVALID, "avatar frame size differs from the egress session");
    for (int i = 0; i < n; ++i)
        if (idx[i] < 0 || idx[i] >= bank_n) return fail(LTK_E_INVALID, "frame index outside the bank");
    const size_t out_bytes = format == LTK_FMT_I420 ? bytes / 2 : bytes;
    StreamLease sl(e, stream);
    ScratchLease sc(e, (bytes + out_bytes) * n);           // [n composites][n converted frames]
    if (!sc.s.d) return fail(LTK_E_NOMEM, "scratch allocation failed");
    uint8_t* const comp = (uint8_t*)sc.s.d;
    uint8_t* const conv = comp + bytes * n;
    if (hold_w) {                                          // composites: one launch per 16 frames
        const Avatar& a = *hold_w;
        const hipError_t oe = order_behind_pending(e, sl.s, d_pred, (size_t)n * 256 * 256 * 3);      // knob DEFER: the frames' pass may be in flight
        if (oe != hipSuccess) return fail(LTK_E_HIP, std::string("egress_batch: ") + hipGetErrorString(oe));
        for (int i0 = 0; i0 < n; i0 += kPasteBatch) {
            const int m = std::min(kPasteBatch, n - i0);
            PasteBatch pb;
            for (int i = 0; i < m; ++i) {
                const int32_t* c = a.coords.data() + 4 * (size_t)idx[i0 + i];
                pb.full[i] = a.d_full + (size_t)idx[i0 + i] * bytes;
                pb.y1[i] = c[0]; pb.y2[i] = c[1]; pb.x1[i] = c[2]; pb.x2[i] = c[3];
            }
            launch_paste_batch(pb, m, H, W, (const uint8_t*)d_pred + (size_t)i0 * 256 * 256 * 3, comp + bytes * i0, bytes, sl.s);
        }
    } else if (hold_u) {
        for (int i0 = 0; i0 < n; i0 += kPasteBatch) {
            const int m = std::min(kPasteBatch, n - i0);
            UlPasteBatch pb;
            ul_fill_paste_batch(*hold_u, idx + i0, m, &pb);
            launch_ul_paste_batch(pb, m, H, W, (const uint8_t*)d_pred + (size_t)i0 * kUlRes * kUlRes * 3, comp + bytes * i0, bytes, sl.s);
        }
    } else {
        const MtAvatar& a = *hold_m;
        for (int i = 0; i < n; ++i) {
            const int32_t* fb = a.face_box.data() + 4 * (size_t)idx[i];
            const int32_t* cb = a.crop_box.data() + 4 * (size_t)idx[i];
            launch_paste_blend(a.d_full + (size_t)idx[i] * bytes, H, W, (const uint8_t*)d_pred + (size_t)i * 256 * 256 * 3, fb[0], fb[1], fb[2], fb[3],
                               cb[0], cb[1], cb[2], cb[3], a.d_masks + a.mask_off[idx[i]], comp + bytes * i, sl.s);
        }
    }
    // watermark + format conversion of all n composites in one launch
    launch_egress_batch(comp, bytes, n, s->d_wm, s->wm_x, s->wm_y, s->wm_w, s->wm_h, s->wm_b, s->wm_g, s->wm_r, conv, out_bytes, H, W,
                        format == LTK_FMT_I420, chroma, sl.s);
    // an error past this point must not hand the scratch back to the pool while earlier launches may still be writing it
    hipError_t pe = hipGetLastError();
    if (pe == hipSuccess) pe = hipMemcpyAsync(h_out, conv, out_bytes * n, hipMemcpyDeviceToHost, sl.s);
    const hipError_t se = hipStreamSynchronize(sl.s);
    if (pe != hipSuccess || se != hipSuccess) return fail(LTK_E_HIP, std::string("egress_batch: ") + hipGetErrorString(pe != hipSuccess ? pe : se));
    return LTK_OK;
}

}  // extern "C"

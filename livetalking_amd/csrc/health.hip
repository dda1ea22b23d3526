// The headroom watch's entry points (include/ltk.h: ltk_health_watch / _report / _scan).  The tables live beside their programs
// (engine_internal.h HealthWatch); the watched calls themselves are in w2l_infer.hip, mt_engine.hip and ultralight.hip.
#include "engine_internal.h"

namespace {

// a magnitude code (the value's bits without the sign) as the value
float decode_code(unsigned code, int q8) {
    if (q8) {                                   // e4m3fn: bias 7, 3 mantissa bits
        const int ex = (int)(code >> 3) & 15, m = (int)code & 7;
        return ex ? ldexpf(1.f + (float)m / 8.f, ex - 7) : ldexpf((float)m, -9);
    }
    const int ex = (int)(code >> 10) & 31, m = (int)code & 1023;      // fp16: bias 15, 10 mantissa bits
    return ex ? ldexpf(1.f + (float)m / 1024.f, ex - 15) : ldexpf((float)m, -24);
}

void fill_op(ltk_health_op* o, const char* name, int type, int observed, int q8, const HealthRec& r) {
    memset(o, 0, sizeof(*o));
    snprintf(o->name, sizeof(o->name), "%s", name);
    o->type = type; o->observed = observed; o->q8 = q8;
    o->elements = r.elements; o->at_limit = r.at_limit; o->near_limit = r.near_limit; o->nonfinite = r.nonfinite;
    o->max_abs = decode_code(r.max_code, q8);
    o->limit = q8 ? 448.f : 65504.f;
}

bool known_program(int program) { return (program >= LTK_HEALTH_WAV2LIP && program <= LTK_HEALTH_HUBERT) || program == LTK_HEALTH_FACEPARSE || program == LTK_HEALTH_FACEDET; }

// one row of a program's listing: the op's name and type, whether it writes e4m3, and its record in the table
struct Row { std::string name; int type, q8, rec; };

// under e->mu: the table of `program` (null with *rc set) and, when `rows` is asked for, its listing.  `hold` keeps an Ultralight
// avatar alive for the caller's use of its table.
HealthWatch* find_watch(ltk_engine* e, int program, int avatar_id, std::shared_ptr<UlAvatar>* hold, std::vector<Row>* rows, int* rc) {
    auto mt_rows = [&](MtGraph* g) {
        if (!rows) return;
        for (int i = 0; i < mt_op_count(g); ++i) {
            int type = 0;
            const char* nm = mt_op_name(g, i, &type);
            rows->push_back(Row{nm ? nm : "", type, mt_op_out_q8(g, i), i});
        }
    };
    *rc = LTK_OK;
    switch (program) {
        case LTK_HEALTH_WAV2LIP:
            if (!e->loaded) { *rc = fail(LTK_E_STATE, "ltk_wav2lip_load has not been called"); return nullptr; }
            if (rows)
                for (size_t i = 0; i < e->layers.size(); ++i) rows->push_back(Row{e->layers[i].name, 0, 0, (int)i});
            return &e->hw_w2l;
        case LTK_HEALTH_MUSETALK:
            if (!e->mt) { *rc = fail(LTK_E_STATE, "ltk_musetalk_load has not been called"); return nullptr; }
            mt_rows(e->mt);
            return &e->hw_mt;
        case LTK_HEALTH_WHISPER:
            if (!e->whisper) { *rc = fail(LTK_E_STATE, "ltk_whisper_load has not been called"); return nullptr; }
            mt_rows(e->whisper);
            return &e->hw_whisper;
        case LTK_HEALTH_HUBERT:
            if (!e->hubert_w) { *rc = fail(LTK_E_STATE, "ltk_hubert_load has not been called"); return nullptr; }
            mt_rows(e->hubert_w);
            return &e->hw_hubert;
        case LTK_HEALTH_FACEPARSE:
            if (!e->face_parse) { *rc = fail(LTK_E_STATE, "ltk_face_parse_load has not been called"); return nullptr; }
            mt_rows(e->face_parse);
            return &e->hw_faceparse;
        case LTK_HEALTH_FACEDET:
            if (!e->face_det_w) { *rc = fail(LTK_E_STATE, "ltk_face_detect_load has not been called"); return nullptr; }
            mt_rows(e->face_det_w);
            return &e->hw_facedet;
        case LTK_HEALTH_ULTRALIGHT: {
            *hold = find_ul_avatar(e, avatar_id);
            if (!*hold || !(*hold)->health) { *rc = fail(LTK_E_STATE, "unknown Ultralight avatar id"); return nullptr; }
            if (rows) {
                std::vector<std::string> names;
                std::vector<int> types, arch;
                ul_health_listing(&names, &types, &arch);
                for (size_t i = 0; i < names.size(); ++i) rows->push_back(Row{names[i], types[i], 0, arch[i]});
            }
            return (*hold)->health.get();
        }
    }
    *rc = fail(LTK_E_INVALID, "unknown program");
    return nullptr;
}

}  // namespace

extern "C" {

int ltk_health_watch(ltk_engine* e, int program, int avatar_id, int calls) {
    if (!e) return fail(LTK_E_INVALID, "engine is null");
    if (!known_program(program)) return fail(LTK_E_INVALID, "unknown program");
    if (calls < 0) return fail(LTK_E_INVALID, "calls must not be negative");
    CHK(enter_device(e->device));
    // armed under the enqueue lock: a call sees the watch whole or not at all
    std::lock_guard<std::mutex> g(e->mu);
    std::shared_ptr<UlAvatar> hold;
    int rc;
    HealthWatch* w = find_watch(e, program, avatar_id, &hold, nullptr, &rc);
    if (!w) return rc;
    if (!w->d) return fail(LTK_E_STATE, "the program has no health table");
    if (calls == 0) { w->left = 0; return LTK_OK; }          // disarmed; what was counted stays readable
    // the records back to zero behind whatever an earlier watched call still has on the streams (its scans on the audio stream are
    // joined into the compute stream by the pass itself)
    CHK(hipMemsetAsync(w->d, 0, (size_t)w->n * sizeof(HealthRec), e->compute));
    std::fill(w->observed.begin(), w->observed.end(), 0);
    w->seen = 0;
    w->left = calls;
    return LTK_OK;
}

int ltk_health_report(ltk_engine* e, int program, int avatar_id, ltk_health_op* ops, int cap, int* n_ops, int* calls_seen, int* calls_left) {
    if (!e || !ops || !n_ops || cap <= 0) return fail(LTK_E_INVALID, "bad arguments");
    if (!known_program(program)) return fail(LTK_E_INVALID, "unknown program");
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    std::shared_ptr<UlAvatar> hold;
    std::vector<Row> rows;
    int rc;
    HealthWatch* w = find_watch(e, program, avatar_id, &hold, &rows, &rc);
    if (!w) return rc;
    *n_ops = (int)rows.size();
    if (cap < (int)rows.size()) return fail(LTK_E_INVALID, "the report has " + std::to_string(rows.size()) + " ops, the buffer holds " + std::to_string(cap));
    std::vector<HealthRec> h((size_t)w->n);
    if (w->n) {
        CHK(hipDeviceSynchronize());
        CHK(hipMemcpy(h.data(), w->d, h.size() * sizeof(HealthRec), hipMemcpyDeviceToHost));
    }
    const HealthRec none = {};
    for (size_t i = 0; i < rows.size(); ++i) {
        const Row& r = rows[i];
        const bool have = r.rec >= 0 && r.rec < w->n;
        fill_op(&ops[i], r.name.c_str(), r.type, have ? (int)w->observed[(size_t)r.rec] : 0, r.q8, have ? h[(size_t)r.rec] : none);
    }
    if (calls_seen) *calls_seen = w->seen;
    if (calls_left) *calls_left = w->left;
    return LTK_OK;
}

int ltk_musetalk_debug_get_q8(ltk_engine* e, const char* op, int frames, uint8_t* out, size_t n_bytes) {
    if (!e || !op || !out || frames <= 0) return fail(LTK_E_INVALID, "bad arguments");
    CHK(enter_device(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->mt) return fail(LTK_E_STATE, "ltk_musetalk_load has not been called");
    if (frames > e->mt_max_frames) return fail(LTK_E_INVALID, "frames exceeds max_frames");
    int C, ld, coff, P, q8;
    const void* d = mt_op_out(e->mt, op, &C, &ld, &coff, &P, &q8);
    if (!d || !q8) return fail(LTK_E_INVALID, std::string("no e4m3 output tensor of an op named ") + op);
    if (n_bytes != (size_t)frames * C * P) return fail(LTK_E_INVALID, "out holds " + std::to_string(n_bytes) + " bytes, the tensor has " + std::to_string((size_t)frames * C * P));
    CHK(hipDeviceSynchronize());
    // the whole buffer [frames][ld / 32][P][32] to the host, then the view's channels one by one
    std::vector<uint8_t> h((size_t)frames * ld * P);
    CHK(hipMemcpy(h.data(), d, h.size(), hipMemcpyDeviceToHost));
    for (int n = 0; n < frames; ++n)
        for (int c = 0; c < C; ++c) {
            const int cc = coff + c;
            const uint8_t* src = h.data() + (((size_t)n * (ld / 32) + cc / 32) * P) * 32 + cc % 32;
            uint8_t* dst = out + ((size_t)n * C + c) * P;
            for (int p = 0; p < P; ++p) dst[p] = src[(size_t)p * 32];
        }
    return LTK_OK;
}

int ltk_health_scan(ltk_engine* e, const void* d_x, int N, int cbt, int cb0, int CB, long long P, int q8, ltk_health_op* rec) {
    if (!e || !d_x || !rec) return fail(LTK_E_INVALID, "bad arguments");
    if (N <= 0 || cbt <= 0 || cb0 < 0 || CB <= 0 || P <= 0 || (q8 != 0 && q8 != 1)) return fail(LTK_E_INVALID, "bad view");
    if ((long long)cb0 + CB > cbt) return fail(LTK_E_INVALID, "the view's channel blocks lie outside the tensor");
    if ((long long)N * cbt > (1ll << 40) / P) return fail(LTK_E_INVALID, "tensor too large");
    CHK(enter_device(e->device));
    StreamLease sl(e, nullptr);
    if (!sl.s) return fail(LTK_E_HIP, "no stream");
    DevBuf d;
    CHK(hipMalloc(&d.p, sizeof(HealthRec)));
    CHK(hipMemsetAsync(d.p, 0, sizeof(HealthRec), sl.s));
    launch_health_scan(d_x, N, cbt, cb0, CB, P, q8, (HealthRec*)d.p, sl.s);
    CHK(hipGetLastError());
    HealthRec h;
    CHK(hipMemcpyAsync(&h, d.p, sizeof(h), hipMemcpyDeviceToHost, sl.s));
    CHK(hipStreamSynchronize(sl.s));
    fill_op(rec, "", 0, 1, q8, h);
    return LTK_OK;
}

}  // extern "C"

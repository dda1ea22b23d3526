// The Wav2Lip inference path: one pass, its captured graphs, the prefetch slots, the face cache, ltk_wav2lip_infer.
#include "engine_internal.h"

// geometry of a face-cache record against the concat buffers (misc_kernels.h FeatGeom): level k = face_encoder_blocks.k's output
static FeatGeom feat_geom(ltk_engine* e) {
    FeatGeom g;
    unsigned off = 0;
    for (int k = 0; k < 8; ++k) {
        const int cat = B_CAT0 + (7 - k), hw = kFeatHW[k] * kFeatHW[k];
        g.cat[k] = e->buf[cat] + (size_t)(kDecCh[7 - k] / 16) * hw * 16;     // channel blocks [dec_ch/16, +feat_ch/16) of a frame
        g.cat_stride[k] = (unsigned)e->buf_halfs[cat];
        g.off[k] = off;
        off += (unsigned)((size_t)kFeatCh[k] * hw * sizeof(f16) / 16);
    }
    g.off[8] = off;
    return g;
}

// One pass over frames [0, nf) of the arena on `s`; the per-frame pointer tables are already in e->d_tab.
// bank_faces: the faces table holds uint8 bank crops (else `d_face6`: float32 NCHW test input); have_outs: the outs table holds
// the uint8 frame destinations; d_pred_f32 (test hook): float32 NCHW sigmoid output.
// `cached` (knob FACE_CACHE): the faces table holds the frames' skip-cache records instead of their bank crops; the face encoder
// does not run, one copy launch puts its eight outputs where it would have written them.
// Knob PREFETCH (see tune.h): `par` = the concat-buffer set this call's decoder works in; `have_feats` = the face encoder's
// outputs for this call's frames are already there (the previous call prefetched them): the pass starts at the audio encoder /
// decoder.
static int enqueue_pass(ltk_engine* e, int nf, hipStream_t s, bool bank_faces, const float* d_face6, bool fused, bool have_outs,
                        float* d_pred_f32, bool cached = false, int par = 0, bool have_feats = false) {
    const FacePtrs* d_faces = &e->d_tab->faces;
    const OutPtrs* d_outs = &e->d_tab->outs;
    const bool pack_fused = bank_faces && e->c7;     // the first layer reads the bank crops itself
    if (cached) launch_feat_copy(d_faces, nf, feat_geom(e), 0, s);
    else if (have_feats) {}
    else if (bank_faces) { if (!pack_fused) launch_pack_faces(d_faces, nf, e->buf[B_X0], s); }
    else launch_pack_face6_nchw(d_face6, nf, e->buf[B_X0], s);
    if (!(e->a0 && (knob(K_AUDIO0) & 1))) launch_pack_mel(&e->d_tab->mels, nf, e->buf[B_MEL], s);     // (audio0_kernel reads the windows itself)
    const int rc = run_convs(e, nf, s, fused ? d_outs : nullptr, nullptr, (pack_fused && !cached && !have_feats) ? d_faces : nullptr,
                             (cached || have_feats) ? 2 : 0, par);
    if (rc) return rc;
    if (!fused) {
        launch_head(e->buf[B_OUT32], 32, nf, e->d_head, e->d_head + 96, have_outs ? d_outs : nullptr, d_pred_f32, s);
        CHK(hipGetLastError());
    }
    return 0;
}

// key of e->graphs: the whole pass, the cached pass, the pipelined variants (decoder only, per slot) and the prefetched face
// encoder (per slot) of a frame count are different launch sequences
static int pass_graph_key(int nf, bool cached, bool have_feats, bool prefetch, int slot) {
    return nf | (cached ? (1 << 20) : 0) | (have_feats ? (1 << 21) : 0) | (prefetch ? (1 << 22) : 0) | (slot << 24);
}

// enqueue_pass, replayed from a captured hipGraph where the pass has no per-call arguments: the product configuration (bank crops
// in, fused head out) on the engine's own streams.  A frame count runs eagerly the first time it is seen (which also sets every
// kernel's dynamic-LDS attribute) and is captured the second time; a dependent launch costs ~3.1 us on a stream and ~2.0 us inside a
// graph (profiles/r03_ubench_launch_chain.txt), and the host issues one launch instead of ~70.  The audio-encoder branch on the aux
// stream becomes a branch of the graph (its fork / join events are captured as dependencies).
int ltk::launch_pass(ltk_engine* e, int nf, hipStream_t s, bool bank_faces, const float* d_face6, bool have_outs, float* d_pred_f32, bool cached, int par,
                     bool have_feats) {
    // the float32 NCHW output (test hook) and layer capture need the 32-channel map in memory: unfused
    const bool fused = have_outs && !d_pred_f32 && !e->capture && knob(K_HEAD_FUSED);
    // knob GRAPH: 0 never, non-zero (default 1) every eligible pass.  Measured (profiles/r04_vs_r03_same_job.txt, r04_graph_auto_ab.txt): the replay of a
    // 16-frame pass is ~5-15 us (0.5-1 %) slower on the device than the same launches issued one by one (equal from 64 frames on), the host side is
    // one launch instead of ~70: a single session's step is 0..1.8 % faster end to end depending on the box's host (three interleaved pairs on the
    // last box: 1.3836 / 1.3904 / 1.3956 ms eager, 1.3619 / 1.3699 / 1.3596 ms replayed), and a host serving hundreds of sessions sustains 512 instead
    // of 448 of them (profiles/r04_delivered_graph_ab.txt).
    // (a watched call, ltk_health_watch, runs these launches eagerly with its scans between them and leaves the graph cache alone)
    const bool graphable = knob(K_GRAPH) && bank_faces && fused && e->c7 && s == e->compute && !e->w2l_scan;
    if (!graphable) {
        const bool product = bank_faces && fused && e->c7 && s == e->compute;
        if ((par || have_feats) && !product) return fail(LTK_E_STATE, "pipelined pass outside the product configuration");
        return enqueue_pass(e, nf, s, bank_faces, d_face6, fused, have_outs, d_pred_f32, cached && bank_faces, par, have_feats);
    }
    return e->graphs.run(e, pass_graph_key(nf, cached, have_feats, false, par), s, "pass", nf,
                         [&]() -> int { return enqueue_pass(e, nf, s, bank_faces, d_face6, fused, have_outs, d_pred_f32, cached, par, have_feats); });
}

// Knob PREFETCH.  A whole-pass call works in set 0; the prefetched encoder has temporaries, split-K scratch and a pointer table of its
// own and writes prefetch slots only, so nothing but a slot's own users has to wait for it (PfSlot::ev_done / ev_read).
// The face encoder of `nf` frames (bank crops in e->d_tab_next, uploaded on aux2 by the caller) into slot `slot`, on the third stream,
// its own graph per (frame count, slot).  Ordering: behind the previous prefetch (stream order) and behind the pass that last worked in
// the slot (ev_read); whoever then works in the slot waits for ev_done.
int ltk::launch_prefetch(ltk_engine* e, int nf, int slot) {
    hipStream_t s = e->aux2;
    ltk_engine::PfSlot& sl = e->pfs[slot];
    if (sl.read) CHK(hipStreamWaitEvent(s, sl.ev_read, 0));
    auto enq = [&]() -> int { return run_convs(e, nf, s, nullptr, nullptr, &e->d_tab_next->faces, 1, slot, true); };
    const int rc = knob(K_GRAPH) ? e->graphs.run(e, pass_graph_key(nf, false, false, true, slot), s, "prefetch", nf, enq) : enq();
    // whatever reached the stream (also part of a failed eager sequence) is ordered in front of the slot's next user
    CHK(hipEventRecord(sl.ev_done, s));
    sl.filled = true;
    return rc;
}

// Knob FACE_CACHE: the face encoder's outputs of every bank frame of `a`, computed by the SAME kernels a 16-frame pass runs (the
// bank is walked in chunks of 16 frames - the last chunk overlaps its predecessor so that every launch has 16 frames - hence a
// 16-frame call renders byte for byte what it renders with the knob off; other call sizes may pick other split factors for the
// small-map encoder layers, as two different call sizes do among themselves: <= 1 LSB, exact under LTK_SPLITK=0).  Under e->mu, on
// the compute stream (stream order keeps the arena and the pointer table consistent with the calls around it).
static int build_face_cache(ltk_engine* e, Avatar& a) {
    const FeatGeom g = feat_geom(e);
    const size_t rec = (size_t)g.off[8] * 16;
    if (!a.d_feat) {
        // 4.15 MB per bank frame: a long avatar is gigabytes; the budget (knob FACE_CACHE_MAX_MB, per avatar) refuses instead of
        // taking the HBM from under the arenas of later loads
        const size_t budget = (size_t)std::max(0, knob(K_FACE_CACHE_MAX_MB)) << 20;
        if (rec * a.n > budget)
            return fail(LTK_E_NOMEM, "face cache of this avatar needs " + std::to_string((rec * a.n) >> 20) + " MB, over LTK_FACE_CACHE_MAX_MB = " +
                                         std::to_string(knob(K_FACE_CACHE_MAX_MB)));
        if (hipMalloc((void**)&a.d_feat, rec * a.n) != hipSuccess) { (void)hipGetLastError(); return fail(LTK_E_NOMEM, "face-cache allocation failed"); }
        a.feat_rec_bytes = rec;
        a.feat_bytes.store(rec * a.n, std::memory_order_release);
    }
    const int chunk = std::min(std::min(16, a.n), std::min(e->micro_batch, kPackMaxFrames));
    const bool pack_fused = e->c7;
    for (int f0 = 0; f0 < a.n; f0 += chunk) {
        const int first = std::min(f0, a.n - chunk);
        FacePtrs fp;
        for (int i = 0; i < chunk; ++i) fp.p[i] = a.d_face + (size_t)(first + i) * 256 * 256 * 3;
        launch_upload_tables(&fp, nullptr, nullptr, chunk, e->d_tab, e->compute);
        if (!pack_fused) launch_pack_faces(&e->d_tab->faces, chunk, e->buf[B_X0], e->compute);
        const int rc = run_convs(e, chunk, e->compute, nullptr, nullptr, pack_fused ? &e->d_tab->faces : nullptr, 1);
        if (rc) return rc;
        for (int i = 0; i < chunk; ++i) fp.p[i] = a.d_feat + (size_t)(first + i) * rec;
        launch_upload_tables(&fp, nullptr, nullptr, chunk, e->d_tab, e->compute);
        launch_feat_copy(&e->d_tab->faces, chunk, g, 1, e->compute);
        CHK(hipGetLastError());
    }
    a.feat_epoch = knob_epoch();
    return 0;
}

extern "C" {

int ltk_avatar_face_cache_bytes(ltk_engine* e, int avatar_id, size_t* bytes) {
    if (!e || !bytes) return fail(LTK_E_INVALID, "bad arguments");
    const std::shared_ptr<Avatar> ap = find_avatar(e, avatar_id);
    if (!ap) return fail(LTK_E_STATE, "unknown avatar id");
    *bytes = ap->feat_bytes.load(std::memory_order_acquire);
    return LTK_OK;
}

}  // extern "C"

// ltk_wav2lip_infer (dc == nullptr) and ltk_wav2lip_infer_deferred.  A call that fails before it enqueues anything still drains the
// window: after an error return nothing is in flight (include/ltk.h).
static int w2l_infer_checked(ltk_engine* e, const ltk_w2l_req* reqs, int nreq, void* stream, DeferCall* dc);
static int w2l_infer(ltk_engine* e, const ltk_w2l_req* reqs, int nreq, void* stream, DeferCall* dc) {
    if (!e) return fail(LTK_E_INVALID, "bad arguments");
    // a knob changed since the pass in flight was enqueued (tests, tuners): plans and graphs are rebuilt behind a drained engine
    if (e->defer_epoch.load(std::memory_order_relaxed) != knob_epoch() && e->defer.newest()) {
        CHK(enter_device(e->device));
        const int drc = drain_pending(e);
        if (drc) return drc;
    }
    const int rc = w2l_infer_checked(e, reqs, nreq, stream, dc);
    if (rc && e->defer.newest()) {
        const std::string msg = g_err;
        (void)hipSetDevice(e->device);
        (void)drain_pending(e);
        return fail(rc, msg);
    }
    return rc;
}

static int w2l_infer_checked(ltk_engine* e, const ltk_w2l_req* reqs, int nreq, void* stream, DeferCall* dc) {
    if (!e || !reqs || nreq <= 0) return fail(LTK_E_INVALID, "bad arguments");
    if (!e->loaded) return fail(LTK_E_STATE, "ltk_wav2lip_load has not been called");
    static const bool timing = getenv("LTK_INFER_TIMING") != nullptr;
    const auto tp0 = std::chrono::steady_clock::now();
    auto tp1 = tp0, tp2 = tp0, tp3 = tp0;
    CHK(enter_device(e->device));
    // resolve every frame's bank crop and mel window up front
    const bool want_cache = knob(K_FACE_CACHE) != 0;
    std::vector<int> fidx;                            // knob FACE_CACHE: (request, bank frame) of every frame
    std::vector<const uint8_t*> fptr;
    std::vector<const float*> mptr;
    std::vector<uint8_t*> optr;
    std::vector<std::shared_ptr<Avatar>> hold;        // the banks stay alive until this call has synchronised
    for (int r = 0; r < nreq; ++r) {
        hold.push_back(find_avatar(e, reqs[r].avatar));
        if (!hold.back()) return fail(LTK_E_STATE, "unknown avatar id");
        if (reqs[r].batch <= 0 || reqs[r].index < 0 || !reqs[r].d_mel || !reqs[r].d_pred) return fail(LTK_E_INVALID, "bad request");
        const Avatar& a = *hold.back();
        for (int i = 0; i < reqs[r].batch; ++i) {
            const int idx = mirror_index(a.n, reqs[r].index + i);  // wav2lip_avatar.py:121-124
            fptr.push_back(a.d_face + (size_t)idx * 256 * 256 * 3);
            if (want_cache) { fidx.push_back(r); fidx.push_back(idx); }
            mptr.push_back((const float*)reqs[r].d_mel + (size_t)i * 80 * 16);
            optr.push_back((uint8_t*)reqs[r].d_pred + (size_t)i * 65536 * 3);
        }
    }
    const int total = (int)fptr.size();
    if (total > e->max_frames) return fail(LTK_E_INVALID, "more frames than max_frames given to ltk_wav2lip_load");
    // (infer_call: one arena, one table, so calls are serialised for the enqueue; scheduler.py keeps two calls in flight)
    const int rc = infer_call(e, stream, [&]() -> int {
        int rc = 0;
        const int mbs = std::min(e->micro_batch, kPackMaxFrames);
        // knob FACE_CACHE: every avatar of the call gets its skip cache on first use (and again after a knob change); the call then
        // runs without the face encoder.  The mode needs the product configuration (fused head, no layer capture).
        const bool cached = want_cache && !e->capture && knob(K_HEAD_FUSED);
        // ltk_health_watch: a watched call takes the whole-pass route (the prefetched encoder's frames are byte-identical), eagerly, with
        // a scan behind every layer; it is not deferred, and it neither reads nor writes the prefetch slots and session records, so the
        // calls behind the window meet them as the calls of a fresh session do
        const bool watched = e->hw_w2l.begin();
        if (cached) {
            for (auto& ap : hold)
                if (!rc && (!ap->d_feat || ap->feat_epoch != knob_epoch())) rc = build_face_cache(e, *ap);
            if (!rc)
                for (int i = 0; i < total; ++i) fptr[i] = hold[fidx[2 * i]]->d_feat + (size_t)fidx[2 * i + 1] * hold[fidx[2 * i]]->feat_rec_bytes;
        } else if (!want_cache) {
            // the mode was switched off: give the records back (earlier cached calls may still read them on the compute stream)
            for (auto& ap : hold)
                if (ap->d_feat) {
                    CHK(hipStreamSynchronize(e->compute));
                    (void)hipFree(ap->d_feat);
                    ap->d_feat = nullptr;
                    ap->feat_bytes.store(0, std::memory_order_release);
                }
        }
        // knob PREFETCH: a single-request call of <= 32 frames finds the face-encoder outputs of its frames in the slot a previous call of
        // its session prefetched them into (key: avatar, first bank index, frame count), and - when it continues a session's sequence
        // (it was a hit, or it starts where a recent solo call of the same avatar and size ended) - prefetches the next call's in turn
        const bool solo = !watched && nreq == 1 && !cached && knob(K_PREFETCH) && e->alt_frames > 0 && total <= std::min(e->alt_frames, mbs) &&
                          !e->capture && knob(K_HEAD_FUSED) && e->c7;
        // knob DEFER: a solo call that was asked to may return with its pass in flight
        const bool defer = solo && dc && dc->want && knob(K_DEFER) != 0;
        const int first = reqs[0].index;
        int slot = 0;
        if (solo)
            for (int k = 1; k <= ltk_engine::kPfSlots && !slot; ++k) {
                const ltk_engine::PfSlot& sl = e->pfs[k];
                if (sl.valid && sl.avatar == reqs[0].avatar && sl.first == first && sl.nf == total && sl.epoch == knob_epoch()) slot = k;
            }
        const bool hit = slot > 0;
        ltk_engine::SoloSeq* seq_rec = nullptr;
        if (solo)
            for (ltk_engine::SoloSeq& q : e->solo_seq)
                if (q.avatar == reqs[0].avatar && q.next == first && q.nf == total) { seq_rec = &q; break; }
        const bool prefetch = solo && (hit || seq_rec != nullptr);
        const int par = slot;
        if (solo) { if (hit) ++e->pf_hits; else ++e->pf_misses; }
        if (hit) {                              // the slot's data must have landed; the slot is consumed by this call
            CHK(hipStreamWaitEvent(e->compute, e->pfs[slot].ev_done, 0));
            e->pfs[slot].valid = false;
            e->pfs[slot].stamp = ++e->pf_clock;
        }
        if (timing) tp1 = std::chrono::steady_clock::now();
        e->w2l_scan = watched ? &e->hw_w2l : nullptr;
        for (int f0 = 0; f0 < total && !rc; f0 += mbs) {
            const int nf = std::min(mbs, total - f0);
            FacePtrs fp; MelPtrs mp; OutPtrs op;
            for (int i = 0; i < nf; ++i) { fp.p[i] = fptr[f0 + i]; mp.p[i] = mptr[f0 + i]; op.p[i] = optr[f0 + i]; }
            launch_upload_tables(hit ? nullptr : &fp, &mp, &op, nf, e->d_tab, e->compute);       // a hit does not read its own bank crops
            if (hipGetLastError() != hipSuccess) rc = fail(LTK_E_HIP, "pointer table upload failed");
            else rc = launch_pass(e, nf, e->compute, true, nullptr, true, nullptr, cached, par, hit);
        }
        e->w2l_scan = nullptr;
        if (hit) {                              // the next prefetch into this slot starts behind this pass
            if (hipEventRecord(e->pfs[slot].ev_read, e->compute) != hipSuccess) { if (!rc) rc = fail(LTK_E_HIP, "hipEventRecord failed"); }
            else e->pfs[slot].read = true;
        }
        if (timing) tp2 = std::chrono::steady_clock::now();
        if (!rc && prefetch) {
            // behind the pass (its launch costs the host ~40 us, this one ~15 us: the branch reaches the GPU ~55 us into the pass, beside the
            // audio encoder): the next call's face encoder, on the third stream, into a free slot other than this call's.
            // Victim: a slot nobody is waiting for - consumed, never used, or filled for a call that did not come within kPfStale seconds
            // (a session that jumped or left).  A slot another session still waits for is NOT taken: round-robin sessions are the worst
            // case of plain LRU (the oldest slot belongs to the session that calls next), so with more interleaved sessions than free
            // slots the surplus sessions simply run whole passes instead of evicting each other.
            constexpr double kPfStale = 1.5;
            const double now = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
            PfSlotView view[ltk_engine::kPfSlots + 1];
            const unsigned long long in_flight = e->defer.slots_in_use();
            for (int k = 1; k <= ltk_engine::kPfSlots; ++k) {
                const ltk_engine::PfSlot& sl = e->pfs[k];
                view[k].valid = sl.valid;
                view[k].age = now - sl.filled_at;
                view[k].stamp = sl.stamp;
                // ... and among the free ones the MOST recently used: a lone session then alternates between two slots (five graphs: captured
                // within its first six calls) instead of walking all sixteen (33 graphs, each launch variant run eagerly once and captured
                // once: the first ~35 calls of a session - all of a 20-step benchmark run - paid for captures, 4.5 % on its timed line)
                // (... whose last reader is done: with calls of several sessions in flight the most recently consumed slot may still be read by
                // another session's pass, and a prefetch into it would wait for that pass instead of running beside it)
                // (knob DEFER: the pass the previous call left in flight works in its slot whether or not the query already says so - the
                // lone session's walk over three slots, and with it the set of captured graphs, does not depend on host timing;
                // defer_window.h choose_prefetch_slot is the rule, checked on the CPU)
                view[k].reader_running = k != slot && !(sl.valid && view[k].age < kPfStale) &&
                                         (((in_flight >> k) & 1) || (sl.read && hipEventQuery(sl.ev_read) != hipSuccess));
            }
            (void)hipGetLastError();          // hipEventQuery's hipErrorNotReady is not an error
            const int victim = choose_prefetch_slot(view, ltk_engine::kPfSlots, slot, kPfStale);
            if (victim) {
            ltk_engine::PfSlot& sl = e->pfs[victim];
            sl.valid = false;
            FacePtrs nx;
            const Avatar& a = *hold[0];
            for (int i = 0; i < total; ++i) nx.p[i] = a.d_face + (size_t)mirror_index(a.n, first + total + i) * 256 * 256 * 3;
            sl.hold = hold[0];                  // (a previous prefetch into this slot is behind us on aux2: its bank may go now)
            // (knob DEFER: the host runs one pass ahead of the device, so this encoder starts as soon as its slot's last reader - two passes
            // back - is done, beside the pass in flight; gating it on that pass's end instead measured 7-17 us per step slower,
            // profiles/defer_ab.txt)
            launch_upload_tables(&nx, nullptr, nullptr, total, e->d_tab_next, e->aux2);
            // a prefetch that cannot be launched does not fail the call: this call's pass is already enqueued and complete without it (returning
            // an error here would hand the caller an error while the pass still writes its frames); the session's next call misses and runs whole
            if (launch_prefetch(e, total, victim) == 0) {
                ++e->pf_issued;
                sl.valid = true; sl.avatar = reqs[0].avatar; sl.first = first + total; sl.nf = total; sl.epoch = knob_epoch();
                sl.stamp = ++e->pf_clock;
                sl.filled_at = now;
            } else {
                (void)hipGetLastError();
                if (!e->pf_fail_logged.exchange(true))
                    fprintf(stderr, "ltk: prefetch of %d frames could not be launched (%s); such calls run whole passes\n", total, g_err.c_str());
            }
            }
        }
        if (!rc && solo) {                      // where this session's next call will start
            if (!seq_rec) {
                seq_rec = &e->solo_seq[0];
                for (ltk_engine::SoloSeq& q : e->solo_seq) if (q.stamp < seq_rec->stamp) seq_rec = &q;
            }
            seq_rec->avatar = reqs[0].avatar; seq_rec->next = first + total; seq_rec->nf = total; seq_rec->stamp = ++e->pf_clock;
        }
        if (timing) tp3 = std::chrono::steady_clock::now();
        if (!rc && defer) {
            dc->ok = true;
            dc->slot = slot;
            for (auto& ap : hold) dc->hold.push_back(ap);
            dc->ranges.push_back({(const unsigned char*)reqs[0].d_pred, (size_t)total * 65536 * 3});
            e->defer_epoch.store(knob_epoch(), std::memory_order_relaxed);
        }
        return rc;
    }, dc);
    if (timing) {
        const auto tp4 = std::chrono::steady_clock::now();
        auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
        std::lock_guard<std::mutex> g(e->pool_mu);
        const double prev = dc ? dc->wait_prev_us : 0.0;
        e->tm_prep += us(tp0, tp1); e->tm_launch += us(tp1, tp2); e->tm_pf += us(tp2, tp3); e->tm_wait += us(tp3, tp4) - prev; e->tm_prev += prev; ++e->tm_calls;
    }
    return rc;
}

extern "C" {

int ltk_wav2lip_infer(ltk_engine* e, const ltk_w2l_req* reqs, int nreq, void* stream) { return w2l_infer(e, reqs, nreq, stream, nullptr); }

int ltk_wav2lip_infer_deferred(ltk_engine* e, const ltk_w2l_req* reqs, int nreq, void* stream, int flags, int* deferred) {
    if (deferred) *deferred = 0;
    if (flags & ~LTK_DEFER_SYNC) return fail(LTK_E_INVALID, "unknown flags");
    DeferCall dc;
    dc.want = !(flags & LTK_DEFER_SYNC);
    const int rc = w2l_infer(e, reqs, nreq, stream, &dc);
    if (!rc && deferred) *deferred = dc.deferred ? 1 : 0;
    return rc;
}

int ltk_wav2lip_order_stream(ltk_engine* e, const void* d_pred, size_t bytes, void* stream) {
    if (!e || !d_pred || !bytes) return fail(LTK_E_INVALID, "bad arguments");
    if (e->defer.writers_of(d_pred, bytes).empty()) return LTK_OK;      // the frames are complete: nothing to wait for
    CHK(enter_device(e->device));
    CHK(order_behind_pending(e, (hipStream_t)stream, d_pred, bytes));
    return LTK_OK;
}

int ltk_wav2lip_defer_stats(ltk_engine* e, unsigned long long* deferred, unsigned long long* max_outstanding, unsigned long long* outstanding) {
    if (!e) return fail(LTK_E_INVALID, "engine is null");
    const DeferStats st = e->defer.stats();
    if (deferred) *deferred = st.deferred;
    if (max_outstanding) *max_outstanding = st.max_outstanding;
    if (outstanding) *outstanding = st.outstanding;
    return LTK_OK;
}

}  // extern "C"

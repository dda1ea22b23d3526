/*
 * libltk_hip.so - MI355X (gfx950) native lip-sync render hot path.
 *
 * C ABI: plain pointers and sizes, no torch types.  Every function returns 0 on
 * success or a negative LTK_E_* code; ltk_last_error() returns a thread-local
 * message.  All entry points are thread-safe (the reference calls
 * inference_batch / paste_back_frame / run_step from three threads per session,
 * avatars/base_avatar.py:475-481).  Device pointers and streams come from the
 * host runtime (PyTorch-ROCm: tensor.data_ptr(), torch.cuda.current_stream()
 * .cuda_stream) or are owned by the engine; `stream` is a hipStream_t passed as
 * void* (NULL = the engine's own stream).
 *
 * Each entry point names the reference interface it replaces
 * (paths relative to the upstream LiveTalking checkout).
 */
#ifndef LTK_H
#define LTK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LTK_OK 0
#define LTK_E_INVALID (-1)   /* bad argument / shape / missing tensor */
#define LTK_E_HIP (-2)       /* a HIP runtime call failed */
#define LTK_E_STATE (-3)     /* call order (model not loaded, avatar unknown, ...) */
#define LTK_E_NOMEM (-4)

typedef struct ltk_engine ltk_engine;

/* One named fp32 host tensor of a PyTorch state_dict (row-major, torch layout). */
typedef struct ltk_named_tensor {
    const char* name;
    const float* data;
    int ndim;
    const int64_t* shape;
} ltk_named_tensor;

/* One session's request inside a cross-session batch: `batch` consecutive
 * frames starting at running frame index `index` (ping-pong `mirror_index`
 * over the avatar's bank, utils/image.py:26-32), mel windows at d_mel. */
typedef struct ltk_w2l_req {
    int avatar;            /* id returned by ltk_avatar_register */
    int index;             /* BaseAvatar.inference's running `index` (base_avatar.py:328,366) */
    int batch;             /* frames in this request (opt.batch_size) */
    const void* d_mel;     /* device, float32 [batch][80][16] (what ltk_mel_step wrote) */
    void* d_pred;          /* device, uint8 [batch][256][256][3] BGR: this request's frames */
} ltk_w2l_req;

const char* ltk_last_error(void);
const char* ltk_version(void);

/* utils/device.py:4-10 initialize_device + per-process model ownership
 * (app.py:62,140-151): one engine per GPU. */
int ltk_engine_create(int device, ltk_engine** out);
void ltk_engine_destroy(ltk_engine* e);
int ltk_engine_sync(ltk_engine* e);

/* avatars/wav2lip_avatar.py:59-70 load_model: takes checkpoint["state_dict"]
 * (380 fp32 tensors, names as in avatars/wav2lip/models/wav2lip_v2.py with any
 * "module." prefix already stripped), folds eval-mode BatchNorm
 * (conv.py:7-10,36-39) into per-channel scale/shift, repacks the conv kernels
 * to fp16 MFMA tiles and sizes the activation arena for `max_frames` frames
 * per launch (the sum of all requests of one ltk_wav2lip_infer call). */
int ltk_wav2lip_load(ltk_engine* e, const ltk_named_tensor* sd, int n, int max_frames);

/* avatars/wav2lip_avatar.py:72-88 load_avatar: uploads one avatar bank.
 * face_bank  uint8 [n][256][256][3] BGR (face_imgs/), full_bank uint8
 * [n][H][W][3] BGR (full_imgs/), coords int32 [n][4] = (y1,y2,x1,x2)
 * (coords.pkl, avatars/wav2lip/genavatar.py:130).  Host pointers. */
int ltk_avatar_register(ltk_engine* e, const uint8_t* face_bank, const uint8_t* full_bank,
                        const int32_t* coords, int n, int H, int W, int* avatar_id);
/* Drops a bank registered by ltk_avatar_register, ltk_musetalk_avatar_register or ltk_ultralight_avatar_register (ids of all kinds come
 * from one counter).
 * Safe while other threads render from it: every call holds a reference to its bank until it returns, the device buffers are
 * freed when the last of them does. */
int ltk_avatar_release(ltk_engine* e, int avatar_id);

/* avatars/audio_features/mel.py:43-63 (MelASR.run_step feature part) +
 * avatars/wav2lip/audio.py:45-51 melspectrogram: `n_samples` PCM samples (the
 * concatenated l + 2B + r 20-ms chunks, host float32) -> `n_win` windows of
 * (80,16) float32 written to d_out [n_win][80][16]; window i starts at STFT
 * column win_start[i] (mel.py:56).  hop 200 / n_fft 800 / 80 mels
 * (avatars/wav2lip/hparams.py:33-73). */
int ltk_mel_step(ltk_engine* e, const float* pcm, int n_samples, const int32_t* win_start,
                 int n_win, void* d_out, void* stream);

/* avatars/wav2lip_avatar.py:116-139 LipReal.inference_batch for `nreq`
 * sessions at once: bank gather + lower-half mask + 6-channel pack, the 55
 * conv/convT layers of Wav2Lip.forward (wav2lip_v2.py:123-163), sigmoid*255 and
 * the uint8 truncation paste_back_frame applies (wav2lip_avatar.py:138,145).
 * Each request's frames land in its own d_pred.  Returns when they are ready;
 * an error return likewise leaves none of the call's launches in flight (the
 * caller may free d_pred / d_mel at once), and a face-encoder prefetch for the
 * session's NEXT call (knob PREFETCH) that cannot be launched is not an error. */
int ltk_wav2lip_infer(ltk_engine* e, const ltk_w2l_req* reqs, int nreq, void* stream);

/* The same call with a deferred wait (knob DEFER, default on; LTK_DEFER=0 makes it ltk_wav2lip_infer): for a lone session issuing
 * its calls back to back.  The reference's inference thread only queues the handles it gets (avatars/base_avatar.py:366-376);
 * whoever reads the frames does so through this library or on a stream, so the call need not wait for its OWN pass.
 *
 * Contract.  A deferred call returns when its pass is enqueued and every pass issued before it is complete: when a call
 * returns, at most one pass - its own - is outstanding, frames complete in issue order, and in steady state a call still takes one
 * period (what the caller measures as its inference rate stays true).  d_mel and d_pred of a call must stay allocated until the
 * NEXT call on this engine (deferred or not) or ltk_engine_sync has returned.
 *   stream      as `stream` of ltk_wav2lip_infer: where d_mel was produced; 0 = none, the inputs are ready.
 *   flags       LTK_DEFER_SYNC: behave as ltk_wav2lip_infer for this call.
 *   deferred    (may be NULL) set to 1 when the call returned with its pass in flight, to 0 when the frames are ready (knob off,
 *               LTK_DEFER_SYNC, a call that does not qualify): a caller wraps or orders its frames only in the first case.
 * No stream is made to wait at the call: such a wait sits in one of the process's few hardware queues for the length of the
 * pass, and for a caller that issues calls back to back it cost more than the deferral gains (45 us of a 1.2-ms step).  Readers
 * use ltk_wav2lip_order_stream: the wait is issued when the frames are read.
 * Who may read a frame when: ltk_paste_back / ltk_paste_back_batch / ltk_egress_frame / ltk_egress_batch order themselves behind
 * the pass that writes the d_pred they are given (GPU-side); any other reader first calls
 * ltk_wav2lip_order_stream(e, d_pred, bytes, stream) - `stream` (0 = the default stream) then waits, on the GPU, for the pass in
 * flight that writes [d_pred, d_pred + bytes), if there is one; no host wait - or ltk_engine_sync, or passes LTK_DEFER_SYNC.
 * Only a call that qualifies for knob PREFETCH defers - one request, product configuration, no face cache, one arena pass; every
 * other call (and every ltk_wav2lip_infer call) runs behind the pass in flight and returns when its own frames are ready, which
 * implies the earlier ones.  ltk_avatar_release, ltk_engine_sync / _destroy, a knob change and the debug / timing entries wait
 * for the pass in flight (host side); the avatar banks it reads are held by the pass, not by the call.
 * Errors.  On an error return nothing is in flight - neither of this call nor of the pass before it - and the frames of BOTH
 * calls are invalid when the error is a device failure (LTK_E_HIP); after a refused request (bad arguments, unknown avatar) the
 * earlier call's frames are complete and valid.  A device failure of pass N is reported by the call that waits for it - call
 * N+1, or whichever entry drains the engine first - and its text says so.
 * ltk_wav2lip_defer_stats: calls that returned with their pass outstanding, the most passes outstanding at such a return (1 with
 * one caller thread), passes outstanding now. */
#define LTK_DEFER_SYNC 2
int ltk_wav2lip_infer_deferred(ltk_engine* e, const ltk_w2l_req* reqs, int nreq, void* stream, int flags, int* deferred);
int ltk_wav2lip_order_stream(ltk_engine* e, const void* d_pred, size_t bytes, void* stream);
int ltk_wav2lip_defer_stats(ltk_engine* e, unsigned long long* deferred, unsigned long long* max_outstanding, unsigned long long* outstanding);

/* avatars/wav2lip_avatar.py:141-147 LipReal.paste_back_frame: bilinear-resize
 * (cv2.resize INTER_LINEAR semantics) the 256x256 prediction to the frame's box
 * and paste it into a copy of full_bank[idx].  d_pred: device uint8
 * [256][256][3].  out: uint8 [H][W][3]; out_is_device selects a device buffer
 * or a (pinned or pageable) host buffer. */
int ltk_paste_back(ltk_engine* e, int avatar_id, int idx, const void* d_pred, void* out,
                   int out_is_device, void* stream);

/* The same composite for the `n` frames of one inference_batch result at once (the process thread of
 * avatars/base_avatar.py:383-467 calls paste_back_frame once per frame, in order, for the items inference_batch returned):
 * d_pred = n contiguous device uint8 [256][256][3] predictions, idx[i] = bank frame of prediction i, out = HOST uint8
 * [n][H][W][3] - pinned memory moves at the PCIe rate.  n composites on the device, ONE device-to-host copy, one
 * synchronisation (per frame: ltk_paste_back costs a 2.76 MB pageable copy and a stream synchronisation each). */
int ltk_paste_back_batch(ltk_engine* e, int avatar_id, const int32_t* idx, const void* d_pred, int n, void* out, void* stream);

/* =========================== MuseTalk path (avatars/musetalk_avatar.py) =========================== */

/* avatars/musetalk_avatar.py:57-67 load_model + avatars/musetalk/utils/utils.py:16-37 load_all_model: the
 * conditional U-Net (diffusers UNet2DConditionModel state_dict, MuseTalk-1.5 config) and the AutoencoderKL
 * decoder of sd-vae (state_dict keys "post_quant_conv.*", "decoder.*"), both fp32 host tensors under their
 * diffusers names.  The timestep-0 embedding, attention scale, VAE scaling factor and the sinusoidal
 * PositionalEncoding (avatars/musetalk/models/unet.py:12-27) are folded / precomputed here; arenas are sized
 * for `max_frames` frames per launch. */
int ltk_musetalk_load(ltk_engine* e, const ltk_named_tensor* unet_sd, int n_unet, const ltk_named_tensor* vae_sd,
                      int n_vae, int max_frames);

/* avatars/musetalk_avatar.py:69-91 load_avatar.  latents: fp32 [n][8][32][32] (input_latent_list_cycle,
 * latents.pt); full_bank uint8 [n][H][W][3] BGR; face_boxes int32 [n][4] = (x1,y1,x2,y2) (coords.pkl,
 * musetalk_avatar.py:157); crop_boxes int32 [n][4] = (x_s,y_s,x_e,y_e) (mask_coords.pkl); masks: the n blend
 * masks (mask/<i>.png, uint8 [h_i][w_i][3] with h_i = y_e-y_s, w_i = x_e-x_s) concatenated, mask i starting at
 * byte mask_offsets[i] (n+1 offsets).  Boxes must lie inside the frame.  Host pointers. */
int ltk_musetalk_avatar_register(ltk_engine* e, const float* latents, const uint8_t* full_bank, const int32_t* face_boxes,
                                 const int32_t* crop_boxes, const uint8_t* masks, const int64_t* mask_offsets, int n,
                                 int H, int W, int* avatar_id);

/* BASELINE configs[4] "fp8 conv path": before ltk_musetalk_load, ask for the ResnetBlock2D 3x3 convolutions of the U-Net
 * and the VAE decoder (the GroupNorm -> SiLU -> conv pairs) to run on OCP e4m3 operands: the GroupNorm kernel writes
 * saturate(y * act_scale) as fp8, weights are quantised per output channel (224 / max|w|), accumulation stays fp32 and
 * the residual stream fp16.  act_scale <= 0 selects the default 8 (e4m3 then covers |y| <= 56 with 2^-12 resolution
 * near zero).  Everything else (attention, linears, up/down-samplers, conv_in/out) stays fp16. */
int ltk_musetalk_set_fp8(ltk_engine* e, int enable, float act_scale);
/* conv / linear MACs per frame of the loaded U-Net + VAE decoder, and the part of them on fp8 operands */
int ltk_musetalk_info(ltk_engine* e, double* macs_per_frame, double* macs_fp8_per_frame);

typedef struct ltk_mt_req {
    int avatar;            /* id returned by ltk_musetalk_avatar_register */
    int index;             /* running frame index (mirror_index over the latent bank) */
    int batch;
    const void* d_feat;    /* device, float32 [batch][50][384]: the whisper chunks of WhisperASR (before PE) */
    void* d_pred;          /* device, uint8 [batch][256][256][3] BGR */
} ltk_mt_req;

/* avatars/musetalk_avatar.py:130-152 MuseReal.inference_batch for `nreq` sessions at once: latent gather,
 * positional encoding, U-Net (timestep 0), vae.decode_latents incl. the uint8 rounding and RGB->BGR flip. */
int ltk_musetalk_infer(ltk_engine* e, const ltk_mt_req* reqs, int nreq, void* stream);

/* avatars/musetalk_avatar.py:154-164 paste_back_frame + avatars/musetalk/myutil.py:4-25 get_image_blending:
 * resize the 256x256 prediction to the face box, paste into the crop region and cv2.blendLinear it with the
 * cached frame under the avatar's mask.  out: uint8 [H][W][3] (device or host, as ltk_paste_back). */
int ltk_paste_blend(ltk_engine* e, int avatar_id, int idx, const void* d_pred, void* out, int out_is_device, void* stream);

/* =========================== Ultralight path (avatars/ultralight_avatar.py) =========================== */

/* avatars/ultralight_avatar.py:63-81 load_avatar.  The model is per avatar (`ultralight.pth`, :69-70), so the state_dict travels with
 * the bank: sd = the 484 tensors of avatars/ultralight/unet.py Model(6, 'hubert') under their names, fp32 host (the
 * num_batches_tracked counters may be left out).  Eval-mode BatchNorm is folded into per-channel scale / shift, the 1x1 / dense
 * kernels are repacked to fp16 MFMA tiles, the depthwise kernels stay fp32.  face_bank uint8 [n][168][168][3] BGR (face_imgs/),
 * full_bank uint8 [n][H][W][3] BGR (full_imgs/), coords int32 [n][4] = (x1,y1,x2,y2) (coords.pkl, :176).  Host pointers.
 * max_frames (1..256) sizes the engine's Ultralight activation arena (frames per launch; it grows to the largest value asked for,
 * longer requests run as several launches).  The id comes from the counter ltk_avatar_register uses; ltk_avatar_release frees the
 * avatar.  A missing tensor, a wrong shape or a box outside the frame returns LTK_E_INVALID with a message. */
int ltk_ultralight_avatar_register(ltk_engine* e, const ltk_named_tensor* sd, int n_tensors, const uint8_t* face_bank,
                                   const uint8_t* full_bank, const int32_t* coords, int n, int H, int W, int max_frames, int* avatar_id);

typedef struct ltk_ul_req {
    int avatar;            /* id returned by ltk_ultralight_avatar_register */
    int index;             /* running frame index (mirror_index over the face bank) */
    int batch;
    const void* d_feat;    /* device, float32 [batch][16][32][32]: the (16, 1024) HuBERT chunks of HubertASR, reshaped (:164) */
    void* d_pred;          /* device, uint8 [batch][160][160][3] BGR */
} ltk_ul_req;

/* avatars/ultralight_avatar.py:143-171 LightReal.inference_batch for `nreq` sessions at once: bank gather, the [4:164, 4:164] crop,
 * the zeroed rectangle (5, 5, 150, 145) of the masked copy and the 6-channel pack (fused into the first kernel's loads),
 * Model.forward (unet.py:198-215), and trunc(sigmoid * 255) as paste_back_frame's astype(uint8) applies it (:170,181).  Requests may
 * name different avatars (each runs its own weights).  Return contract as ltk_wav2lip_infer: returns when the frames are ready,
 * an error return leaves none of the call's launches in flight.  A frame count's pass runs eagerly the first time, is captured
 * the second time and replayed afterwards (knob GRAPH, counted by ltk_program_graph_count). */
int ltk_ultralight_infer(ltk_engine* e, const ltk_ul_req* reqs, int nreq, void* stream);

/* What an ltk_ultralight_infer_merged call launched.  The arrays hold the first LTK_UL_MERGE_MAX_PASSES passes; n_passes, grouped
 * and frames count all of them. */
#define LTK_UL_MERGE_MAX_PASSES 64
#define LTK_UL_PATH_PER_AVATAR 0 /* one avatar's program (the kernels and captured graph of ltk_ultralight_infer) */
#define LTK_UL_PATH_GROUPED 1    /* the grouped program: every frame takes its own avatar's weights through a per-frame table */
typedef struct ltk_ul_merge_report {
    int n_passes;                          /* launch sequences the call ran */
    int n_avatars;                         /* distinct avatars among its requests */
    int grouped;                           /* passes on the grouped path */
    int frames;                            /* frames over all passes */
    int path[LTK_UL_MERGE_MAX_PASSES];     /* per pass: LTK_UL_PATH_* */
    int nf[LTK_UL_MERGE_MAX_PASSES];       /* per pass: frames (<= the arena's) */
    int avatar[LTK_UL_MERGE_MAX_PASSES];   /* per pass: its avatar, -1 on the grouped path */
} ltk_ul_merge_report;

/* ltk_ultralight_infer for the sessions of one scheduler tick, with the requests' passes MERGED: where ltk_ultralight_infer runs one
 * launch sequence (86 launches) per request, this call runs one per pass of the plan below, each over up to the arena's frames.
 * Same requests, same results per request (every request's frames land in its own d_pred, in its own order) and the same return
 * contract: it returns when the frames are ready, an error return leaves nothing in flight.  EVERY request is validated before the
 * first launch (LTK_E_INVALID names the request; an unknown avatar is LTK_E_STATE), so a caller that batched several sessions can
 * re-issue them one by one and only the offender fails again.  The avatars are held until the call has synchronised.
 * mode 0, the rule: requests of ONE avatar -> per-avatar passes over the union of their frames; of several avatars -> grouped passes
 * over all frames in request order under knob UL_GROUPED (default off, profiles/ultralight_merge.txt), else each avatar's requests
 * merged, avatars in order of first appearance.  mode 1 forces the per-avatar form, mode 2 the grouped form.  Frames keep request
 * order inside a pass; a request is a contiguous span and is split only where a pass is full.  A call of one request runs exactly
 * what ltk_ultralight_infer runs for it (same launches, same captured graph).  In a per-avatar pass every conv keeps, per frame, the
 * split-K factor of the ltk_ultralight_infer pass that would have carried the frame, so a request's frames are byte-identical to its
 * own call's whatever shares the pass (a few convs then take more than one launch where the requests' sizes differ; such a pass is
 * captured per avatar and run lengths of those sizes).  A grouped pass is captured per frame count under a
 * key of its own, holds no avatar's address and survives ltk_avatar_release.  rep (or NULL): what was launched. */
int ltk_ultralight_infer_merged(ltk_engine* e, const ltk_ul_req* reqs, int nreq, int mode, void* stream, ltk_ul_merge_report* rep);

/* The Ultralight arena: frames per pass (0: no avatar registered yet), its bytes, the bytes one frame takes, and whether the grouped
 * path is part of this build.  Any pointer may be NULL. */
int ltk_ultralight_info(ltk_engine* e, int* arena_frames, size_t* arena_bytes, size_t* bytes_per_frame, int* grouped);

/* avatars/ultralight_avatar.py:173-184 LightReal.paste_back_frame: the 168x168 bank face with the prediction written at
 * [4:164, 4:164], bilinear-resized (cv2.resize INTER_LINEAR semantics) to the frame's box and pasted into a copy of full_bank[idx].
 * d_pred: device uint8 [160][160][3].  out: uint8 [H][W][3], device or host as ltk_paste_back. */
int ltk_ultralight_paste_back(ltk_engine* e, int avatar_id, int idx, const void* d_pred, void* out, int out_is_device, void* stream);

/* The twin of ltk_paste_back_batch for avatars/ultralight_avatar.py:173-184: the composites of the `n` frames of one
 * LightReal.inference_batch result at once (the process thread of avatars/base_avatar.py:383-467 asks for them one by one, in
 * order).  d_pred = n contiguous device uint8 [160][160][3] predictions, idx[i] = bank frame of prediction i, out = HOST uint8
 * [n][H][W][3] (pinned memory moves at the PCIe rate).  One launch per 16 frames, ONE device-to-host copy, one synchronisation.
 * n <= 0, a NULL pointer or an idx[i] outside the bank: LTK_E_INVALID; an unknown avatar id: LTK_E_STATE. */
int ltk_ultralight_paste_back_batch(ltk_engine* e, int avatar_id, const int32_t* idx, const void* d_pred, int n, void* out, void* stream);

/* ---- frame egress: the steps between paste_back_frame and the encoder ------------
 * Reference: avatars/base_avatar.py:384-453 process_frames (silent path :407-428, transition blend :419-426 and
 * :436-445, watermark :449), server/webrtc.py:190-193 (VideoFrame.from_ndarray(bgr24), converted to yuv420p by the
 * encoder's swscale), streamout/rtmp.py:81-83.
 *
 * One egress session per render session: it owns the two cached frames of the transition effect
 * (_last_silent_frame / _last_speaking_frame) and the watermark. */
typedef struct ltk_egress ltk_egress;
int ltk_egress_open(ltk_engine* e, int H, int W, ltk_egress** out);
int ltk_egress_close(ltk_engine* e, ltk_egress* s);
/* Watermark as a coverage bitmap: cv2.putText(..., thickness 1, LINE_8) sets every covered pixel to the colour, so
 * the host rasterises the text once (cv2.putText on a zero image) and hands the non-zero rectangle over.
 * mask host uint8 [h][w] (non-zero = covered) placed at (x, y); NULL removes the watermark. */
int ltk_egress_watermark(ltk_engine* e, ltk_egress* s, const uint8_t* mask, int x, int y, int w, int h, int b, int g, int r);

#define LTK_FMT_BGR24 0
#define LTK_FMT_I420 1      /* Y [H][W], U [H/2][W/2], V [H/2][W/2]; H and W even; BT.601 limited range, swscale's integer matrix */
#define LTK_SRC_WAV2LIP 0   /* composite = ltk_paste_back(avatar, idx, d_pred); d_pred NULL = the cached full frame (silent) */
#define LTK_SRC_MUSETALK 1  /* composite = ltk_paste_blend(avatar, idx, d_pred); d_pred NULL = the cached full frame */
#define LTK_SRC_HOST 2      /* frame = h_frame, host uint8 [H][W][3] (custom action video, base_avatar.py:411-414) */
#define LTK_SRC_ULTRALIGHT 3 /* composite = ltk_ultralight_paste_back(avatar, idx, d_pred), d_pred device uint8 [160][160][3];
                              * d_pred NULL = the cached full frame */
typedef struct ltk_egress_req {
    int source;             /* LTK_SRC_* */
    int avatar, idx;        /* bank frame (ignored for LTK_SRC_HOST) */
    const void* d_pred;     /* device uint8 [256][256][3] ([160][160][3] for LTK_SRC_ULTRALIGHT) or NULL */
    const uint8_t* h_frame; /* LTK_SRC_HOST only */
    int speaking;           /* which cache this frame refreshes: 1 = _last_speaking_frame, 0 = _last_silent_frame */
    double alpha;           /* transition weight of THIS frame: out = addWeighted(other-state cache, 1-alpha, frame, alpha);
                             * < 0 or >= 1 (or no cached frame of the other state yet): no blend */
    int keep;               /* non-zero: store the (blended, un-watermarked) frame as this state's cache, as the reference
                             * does while enable_transition is on */
    int format;             /* LTK_FMT_* */
    int chroma;             /* I420 chroma: 1 = 2x2 mean, 0 = top-left pixel of each quad */
} ltk_egress_req;
/* h_out: host uint8, H*W*3 bytes (BGR24) or H*W*3/2 bytes (I420); returns after the copy completed. */
int ltk_egress_frame(ltk_engine* e, ltk_egress* s, const ltk_egress_req* req, uint8_t* h_out, void* stream);

/* The speaking frames of ONE inference_batch result at once, for sessions without the transition effect (the reference's
 * default, base_avatar.py:384 enable_transition = False): n composites (ltk_paste_back / ltk_paste_blend /
 * ltk_ultralight_paste_back of prediction i onto bank frame idx[i]), watermark and format conversion on the device, ONE
 * device-to-host copy into `h_out` ([n][H][W][3] for LTK_FMT_BGR24, [n][H*3/2][W] for LTK_FMT_I420; pinned memory moves at the PCIe rate) and one
 * synchronisation.  With I420 a 25-fps 720p session costs 35 MB/s of PCIe instead of 69: the link, not the GPU, bounds
 * how many sessions a GPU can serve (bench.py `delivered`).  source: LTK_SRC_WAV2LIP, LTK_SRC_MUSETALK or
 * LTK_SRC_ULTRALIGHT; d_pred: n contiguous device uint8 predictions, [256][256][3] each ([160][160][3] for
 * LTK_SRC_ULTRALIGHT).  The session's transition caches are neither read nor written. */
int ltk_egress_batch(ltk_engine* e, ltk_egress* s, int source, int avatar, const int32_t* idx, const void* d_pred, int n, int format,
                     int chroma, uint8_t* h_out, void* stream);

/* avatars/musetalk/whisper/audio2feature.py:15-23 Audio2Feature.__init__: the Whisper-tiny ENCODER
 * (transformers WhisperModel(...).encoder.state_dict(): conv1, conv2, embed_positions, layers.{0..3}.*, layer_norm),
 * fp32 host tensors.  The WhisperFeatureExtractor constants (n_fft 400, hop 160, 80 slaney mels, 30-s padding) are
 * built in. */
int ltk_whisper_load(ltk_engine* e, const ltk_named_tensor* encoder_sd, int n);

/* avatars/audio_features/whisper.py:58-76 WhisperASR.run_step feature part: audio2feat
 * (audio2feature.py:106-117: log-mel of the zero-padded 30-s window -> encoder with all 5 hidden states) and
 * _feature2chunks (whisper.py:35-56, base_asr.py:91-133): frame i takes encoder rows
 * [first_row + i*row_step, first_row + i*row_step + rows), index-clamped, each row = its 5 hidden states.
 * pcm: host float32 [n_samples] (the concatenated l + 2B + r chunks).  d_out: device float32
 * [batch][rows*5][384] (= the (50,384) whisper chunks at rows 10, first_row 2*(l/2), row_step 2). */
int ltk_whisper_step(ltk_engine* e, const float* pcm, int n_samples, int batch, int first_row, int row_step, int rows,
                     void* d_out, void* stream);

/* The live steps of nreq concurrent MuseTalk sessions in one call (scheduler.py kind "whisper").  Every request is what
 * ltk_whisper_step takes.  Requests are forwarded in runs of at most 16 in request order, every run of more than one as the images of
 * ONE run of a 16-clip encoder program over the loaded encoder's packed weights: one log-mel launch pair, one ~60-launch program
 * (replayed from a captured graph from its second sight of a clip count) and one chunk gather for all of them.  No clip's spectral
 * maximum, attention or chunk clamp sees another clip, and a clip's log-mel features are the single step's bit for bit.  The 16-clip
 * program and its staging are built on the first batched run (ltk_whisper_batch_info reports their size); a run of one request runs
 * as ltk_whisper_step does, and nreq == 1 IS ltk_whisper_step.  All requests are validated before the first launch (LTK_E_INVALID
 * names the request; LTK_E_STATE without a loaded encoder); returns when every d_out is complete; an error return leaves nothing in
 * flight. */
typedef struct ltk_whisper_req {
    const float* pcm; int n_samples;              /* host, 0 < n_samples <= 479000 */
    int batch, first_row, row_step, rows;         /* as ltk_whisper_step; 0 < rows <= 64 */
    void* d_out;                                  /* device float32 [batch][rows*5][384] */
} ltk_whisper_req;
int ltk_whisper_step_batch(ltk_engine* e, const ltk_whisper_req* reqs, int nreq);

/* =========================== HuBERT-large audio features (Ultralight, avatars/ultralight/audio2feature.py) =========================== */

/* audio2feature.py:9-11: transformers HubertModel in the configuration of facebook/hubert-large-ls960-ft (feat_extract_norm "layer",
 * conv_bias, do_stable_layer_norm, feat_proj_layer_norm; 7 conv layers of 512 channels, hidden 1024, 16 heads, FFN 4096, positional conv
 * k 128 in 16 groups).  sd = HubertModel.state_dict() names, fp32 host tensors, with ONE difference: the positional conv arrives with
 * its weight norm folded, as "encoder.pos_conv_embed.conv.weight" [1024][64][128] (Engine.load_hubert folds it).  The depth is the
 * number of "encoder.layers.N" present; "masked_spec_embed" is ignored.  A missing tensor or a wrong shape returns LTK_E_INVALID with
 * a message, a second load LTK_E_STATE.  The weights are packed once (0.63 GB of fp16 at 24 layers); every clip length gets a
 * program of its own over them on first use, at most 3 are kept. */
int ltk_hubert_load(ltk_engine* e, const ltk_named_tensor* sd, int n);

/* audio2feature.py:15-54 get_hubert_from_16k_speech: pcm host float32 [n_samples] at 16 kHz, normalised over the whole input
 * ((x - mean) / sqrt(var + 1e-7), Wav2Vec2FeatureExtractor), forwarded in clips of 320 000 samples (each with the 80 samples behind
 * it) and a tail of at least 400 samples, concatenated, then padded with zero rows or trimmed to expected = (n_samples - 80) / 320
 * rows.  out_host: float32 [cap_rows][1024], cap_rows >= expected; *rows = expected.  LTK_E_INVALID if the model returned a row count
 * more than one off the expected one. */
int ltk_hubert_features(ltk_engine* e, const float* pcm, long long n_samples, float* out_host, int cap_rows, int* rows);

/* avatars/audio_features/hubert.py:24-49 HubertASR.run_step feature part: one forward of the step's l + 2B + r chunks (400 <= n_samples
 * < 320 000) and feature2chunks (base_asr.py:91-156): frame i takes rows [first_row + i*row_step, first_row + i*row_step + rows),
 * index-clamped.  d_out: device float32 [batch][rows][1024] (= the (16,1024) chunks ltk_ultralight_infer takes at rows 16,
 * first_row 2*(l/2) - 8, row_step 2).  Returns when d_out is complete. */
int ltk_hubert_step(ltk_engine* e, const float* pcm, int n_samples, int batch, int first_row, int row_step, int rows, void* d_out);

/* The live steps of nreq concurrent sessions in one call (scheduler.py kind "hubert").  Every request is what ltk_hubert_step takes.
 * Requests of one length are forwarded together, up to 16 clips per program run, so that the weights stream once for all of them;
 * no clip's statistics, padding, attention or chunk clamp sees another clip.  Batched programs (16 clips of one length) live in a
 * cache of their own, at most 2, least recently used dropped, and are built only while their activations at 16 clips stay under
 * 2 GiB; a request alone at its length, or of a longer length, runs as ltk_hubert_step does, and nreq == 1 IS ltk_hubert_step.
 * All requests are validated before the first launch (LTK_E_INVALID names the request); returns when every d_out is complete; an
 * error return leaves nothing in flight. */
typedef struct ltk_hubert_req {
    const float* pcm; int n_samples;              /* host, 400 <= n_samples < 320000 */
    int batch, first_row, row_step, rows;         /* feature2chunks of this request */
    void* d_out;                                  /* device float32 [batch][rows][1024] */
} ltk_hubert_req;
int ltk_hubert_step_batch(ltk_engine* e, const ltk_hubert_req* reqs, int nreq);

/* Avatar preparation: avatars/musetalk/models/vae.py:84-94,110-122 get_latents_for_unet, as
 * avatars/musetalk/genavatar.py:116-128 calls it.  vae_sd: the AutoencoderKL state_dict keys "encoder.*" and
 * "quant_conv.*" (fp32 host).  faces_bgr: host uint8 [nfaces][256][256][3] (the LANCZOS-resized crops);
 * latents_out: host fp32 [nfaces][8][32][32] = cat(masked, reference) latents * scaling_factor.
 * noise: host fp32 [nfaces][2][4][32][32] standard-normal draws for latent_dist.sample() (the reference draws them
 * from torch's global RNG), or NULL for the distribution mean. */
int ltk_vae_encoder_load(ltk_engine* e, const ltk_named_tensor* vae_sd, int n, int max_faces);
int ltk_vae_encode_faces(ltk_engine* e, const uint8_t* faces_bgr, int nfaces, const float* noise, float* latents_out);

/* Avatar preparation, blend masks: the BiSeNet face parser (avatars/musetalk/utils/face_parsing/model.py BiSeNet.forward()[0],
 * resnet.py; face_parsing/__init__.py:72-90: ToTensor + Normalize, the net, argmax) as one replayed device program over the 41 launches
 * of ltk_debug_face_parse_program, wired as ltk_debug_face_parse_plan lists.
 * ltk_face_parse_load: sd = BiSeNet(n_classes=19).state_dict() (fp32 host); read are the keys of the network's main output - the
 * conv_out16.* / conv_out32.* heads and the num_batches_tracked counters are ignored when present; a missing key is LTK_E_INVALID and
 * the message names it.  Eval-mode BatchNorm is folded into each conv's fp32 scale / shift.  size: the square image size, a multiple
 * of 32 in [64, 512] (the reference uses 512); max_images in [1, 8]: images per run of the program.  LTK_E_STATE on a second load.
 * ltk_face_parse: rgb_host uint8 [n][size][size][3] (RGB, as PIL hands it over) -> labels_host uint8 [n][size][size], classes 0..18.
 * n may exceed max_images: the images go through in chunks of max_images (the last one short), each uploaded, run and copied back with
 * one synchronisation.  LTK_E_STATE before a load; a refused call has launched nothing.
 * ltk_face_parse_debug_get (test hook): the output of the launch named op_name as the last run left it, `images` <= the images of that
 * run, as float32 [images][cout][Ho][Wo], real channels only; "labels" is refused (bytes: they come from ltk_face_parse). */
int ltk_face_parse_load(ltk_engine* e, const ltk_named_tensor* sd, int n, int size, int max_images);
int ltk_face_parse(ltk_engine* e, const uint8_t* rgb_host, int n, uint8_t* labels_host);
int ltk_face_parse_debug_get(ltk_engine* e, const char* op_name, int images, float* out_f32, size_t n_floats);

/* Avatar preparation, face boxes: the S3FD face detector (avatars/wav2lip/face_detection/detection/sfd/net_s3fd.py s3fd.forward, then
 * what detect.py batch_detect does per level: softmax, threshold, bbox.py batch_decode) as one replayed device program over the 39
 * launches of ltk_debug_face_detect_program, wired as ltk_debug_face_detect_plan lists.  genavatar.py and MuseTalk's preprocessing.py
 * take their face box from it (through api.py get_detections_for_batch; livetalking_amd/face_detect.py has the host side).
 * ltk_face_detect_load: sd = s3fd().state_dict() (fp32 host); a missing key is LTK_E_INVALID and the message names it.  max_images in
 * [1, 16] (the reference's face_det_batch_size): images per run of a program.  LTK_E_STATE on a second load.
 * ltk_face_detect: bgr_host uint8 [n][H][W][3] as cv2.imread gives the frames (the channel reversal of api.py:65 and the mean
 * subtraction of detect.py:59 happen on the device).  The program for (H, W) is built on first use over the loaded weights and captured
 * once per image count; the engine keeps the 2 most recently used.  H, W >= 32 and the program's buffers below 8 GiB, else
 * LTK_E_INVALID with the figure.  n may exceed max_images: the images go through in chunks of max_images (the last one short), each
 * uploaded (one copy: the frames), run and copied back with one synchronisation.  thresh in [0, 1) (the reference: 0.05).  Output per image i: counts_out[i] =
 * the positions whose score is above thresh, and in cand_out[i][cap][6] (32-bit words) the first min(counts_out[i], cap) of them in
 * ascending key order, zeros behind: word 0 the key = level << 28 | h << 14 | w, words 1..5 the floats x1, y1, x2, y2, score.  The
 * output does not depend on the order the device found them in.  counts_out[i] > cap is reported as it is (the list is then cut);
 * cap in [1, 4096], the device's own list length: beyond 4096 candidates the kept ones are an arbitrary subset.  Every image gets its
 * OWN positions (batch_detect decodes a position for every image of the batch when any image passes there; greedy NMS followed by the
 * 0.5 filter makes those extra rows irrelevant, see face_detect.py).  LTK_E_STATE before a load; a refused call has launched nothing.
 * ltk_face_detect_debug_get (test hook): the output of the launch named op_name as the last run left it, `images` <= the images of that
 * run, as float32 [images][cout][Ho][Wo] (a merged head: 16 channels); the detect launches have no tensor.  The trunk's launches share
 * two buffers, so for those the hook runs the program again up to the named launch, on the frames that run left on the device, and reads
 * then; a tapped map, a norm and a head have buffers of their own and are read as the run left them. */
int ltk_face_detect_load(ltk_engine* e, const ltk_named_tensor* sd, int n, int max_images);
int ltk_face_detect(ltk_engine* e, const uint8_t* bgr_host, int n, int H, int W, float thresh, uint32_t* cand_out, int cap, int* counts_out);
int ltk_face_detect_debug_get(ltk_engine* e, const char* op_name, int images, float* out_f32, size_t n_floats);

/* =========================== fp16 headroom watch: the first calls on a real checkpoint =========================== */

/* The conv epilogues clamp to the fp16 range (fmed3f(t, -65504, 65504); +-448 on the e4m3 tensors of the fp8 path) and nothing reports
 * it: a network whose activations reach the limit is no longer computing the reference's fp32 numbers, the fp16 parity tolerance does
 * not hold from there on, and the checkpoint renders wrong frames silently.
 * A watch is armed for the next `calls` inference calls of ONE program and disarms itself after them.  A watched call issues exactly the compute launches it would issue unwatched - same routes, tiles,
 * split-K factors, fused head, fused inverted residuals - launch by launch instead of from a captured graph (the graph cache is neither
 * read nor written, no knob changes, no graph is dropped), with one scan launch behind every op whose output is in memory, on that
 * op's stream: its frames and features are byte-identical to the unwatched call's.  One engine call counts as one call, whatever its
 * nreq; arming and counting happen under the engine's enqueue lock.  Unarmed, no call launches anything it did not launch before.
 * Reference: the reference runs these networks in fp32 on the CPU and under fp16 autocast on CUDA (avatars/wav2lip_avatar.py:51-70,
 * avatars/musetalk_avatar.py:57-66, avatars/ultralight_avatar.py:63-81); it has no such check.
 *
 * Programs and their op listings (the report's index): LTK_HEALTH_WAV2LIP the layers of ltk_wav2lip_layer_name (type 0);
 * LTK_HEALTH_MUSETALK ltk_musetalk_op_name (U-Net + VAE decoder); LTK_HEALTH_WHISPER the Whisper encoder's ops (types as
 * ltk_musetalk_op_name; the 16-clip program of ltk_whisper_step_batch counts into the same table); LTK_HEALTH_HUBERT
 * ltk_hubert_op_name (every clip length's program and the batched programs count into one table); LTK_HEALTH_ULTRALIGHT one
 * avatar's ltk_ultralight_op_name as knob UL_FUSE_IR stands when the report is read; LTK_HEALTH_FACEPARSE the 41 launches of
 * ltk_debug_face_parse_program with its types (a watched ltk_face_parse call counts once whatever its chunks; `labels` writes bytes and
 * stays unobserved).
 * What a watch does not see (observed = 0, counters zero): an output that never reaches memory on the route the call took - the
 * 32-channel map inside the fused Wav2Lip head (output_block.0), the hidden tensors of a fused Ultralight inverted residual (the block
 * is listed once, with its project conv's output), the byte-writing heads; an op the call did not run (the face encoder under knob
 * FACE_CACHE); Ultralight passes on the grouped path.  Float32 outputs (features, sigmoid hooks) are not scanned.
 * A watched ltk_wav2lip_infer call takes the whole-pass route (the prefetched encoder's frames are byte-identical), is not deferred -
 * its counters are complete when it returns - and leaves the prefetch slots and session records alone: the calls behind the window
 * find prefetching as the first calls of a session do. */
enum { LTK_HEALTH_WAV2LIP = 0, LTK_HEALTH_MUSETALK = 1, LTK_HEALTH_ULTRALIGHT = 2, LTK_HEALTH_WHISPER = 3, LTK_HEALTH_HUBERT = 4,
       /* 5 stays unassigned: callers written against the five codes above treat it as the first unknown program */
       LTK_HEALTH_FACEPARSE = 6,
       /* the 39 launches of ltk_debug_face_detect_program with its types; every frame size's program counts into one table, a watched
        * ltk_face_detect call counts once whatever its chunks, the detect launches write records and stay unobserved */
       LTK_HEALTH_FACEDET = 7 };

typedef struct ltk_health_op {
    char name[64];
    int type;                      /* the listing's op type */
    int observed;                  /* 0: output never in memory on this route */
    int q8;                        /* 0: fp16, 1: e4m3 */
    unsigned long long elements, at_limit, near_limit, nonfinite;
    float max_abs, limit;          /* limit: 65504 or 448 */
} ltk_health_op;

/* elements: values scanned; at_limit: |v| exactly at the type's limit (what a clamp leaves behind); near_limit: finite values in the
 * top binade (fp16 |v| >= 32768, e4m3 |v| >= 256), the at_limit ones included; nonfinite: inf / NaN; max_abs: the largest finite |v|.
 *
 * ltk_health_watch: arms the next `calls` calls of `program` and zeroes its counters; calls = 0 disarms (what was counted stays
 * readable).  avatar_id is read for LTK_HEALTH_ULTRALIGHT only.  LTK_E_STATE when the program is not loaded (the avatar unknown),
 * LTK_E_INVALID for an unknown program or negative calls.
 * ltk_health_report: waits for the device, then the listing with the counters accumulated over the watched calls since the watch was
 * armed; *n_ops = ops in the listing (also set when cap is too small: LTK_E_INVALID), calls_seen / calls_left (may be NULL) = watched
 * calls so far / still to come.
 * ltk_health_scan: the scan kernel on its own (unit tests): one tensor view, d_x device fp16 [N][cbt][P][16] (q8 = 0) or e4m3
 * [N][cbt][P][32] (q8 = 1), channel blocks [cb0, cb0 + CB); *rec = its record (name empty).  Returns when it is complete. */
int ltk_health_watch(ltk_engine* e, int program, int avatar_id, int calls);
int ltk_health_report(ltk_engine* e, int program, int avatar_id, ltk_health_op* ops, int cap, int* n_ops, int* calls_seen, int* calls_left);
int ltk_health_scan(ltk_engine* e, const void* d_x, int N, int cbt, int cb0, int CB, long long P, int q8, ltk_health_op* rec);

/* ---- test / measurement hooks (not on the production call path) ---- */

/* named tensor of the last Whisper step as [C][T] float32: "input_features", "hidden_states.0".."hidden_states.4",
 * or an op name ("conv1", "layers.0.self_attn.out_proj", ...) */
int ltk_whisper_debug_get(ltk_engine* e, const char* name, float* out, size_t n_floats);
/* ... of clip `clip` of the batched run (ltk_whisper_step_batch) that ran last, under the same names: [C][T] float32 */
int ltk_whisper_debug_get_clip(ltk_engine* e, const char* name, int clip, float* out, size_t n_floats);
/* clips per batched program run, 1 once the batched program is built (0 before the first batched run), and its activation bytes at full
 * capacity (0 until built); any may be NULL */
int ltk_whisper_batch_info(ltk_engine* e, int* capacity, int* built, size_t* activation_bytes);
/* How ltk_whisper_step_batch cuts a call of nreq requests, on the host alone (no engine, no GPU): run_of[r] / slot_of[r] = the run that
 * carries request r and its place in it, run_batched[i] = 1 if run i is one batched program run (0: the single-clip path), runs in
 * execution order, *n_runs of them (all arrays hold nreq entries) */
int ltk_debug_whisper_batch_plan(int nreq, int* run_of, int* slot_of, int* run_batched, int* n_runs);

/* named tensor of the HuBERT program that ran last as [C][T] float32: an op name (ltk_hubert_op_name; an attention's output is
 * "<op>.attn"), or "input_values": the normalised waveform fp32 [n_samples] of that clip */
int ltk_hubert_debug_get(ltk_engine* e, const char* name, float* out, size_t n_floats);
/* ... of clip `clip` of the batched run (ltk_hubert_step_batch) that ran last: [C][T] float32, or "input_values" */
int ltk_hubert_debug_get_clip(ltk_engine* e, const char* name, int clip, float* out, size_t n_floats);
/* clips per batched program run, batched programs currently kept, activation bytes of the one that ran last at full capacity (any may
 * be NULL) */
int ltk_hubert_batch_info(ltk_engine* e, int* capacity, int* programs, size_t* activation_bytes);
/* How ltk_hubert_step_batch cuts a call of nreq requests of n_samples[r] for a model of `layers` encoder layers, on the host alone (no
 * engine, no GPU): run_of[r] / slot_of[r] = the run that carries request r and its place in it, run_batched[i] = 1 if run i is one
 * batched program run (0: the single-clip path), runs in execution order, *n_runs of them (all arrays hold nreq entries);
 * clip_bytes[r] (may be NULL) = activation bytes of one clip of that length. */
int ltk_debug_hubert_batch_plan(const int* n_samples, int nreq, int layers, int* run_of, int* slot_of, int* run_batched, int* n_runs,
                                size_t* clip_bytes);
/* ops of a HuBERT program in execution order; type as ltk_musetalk_op_name, and 7 conv layer 0 + LayerNorm + GELU, 8 LayerNorm +
 * GELU, 9 positional conv */
int ltk_hubert_op_count(ltk_engine* e);
int ltk_hubert_op_name(ltk_engine* e, int op, char* buf, int buf_len, int* type);
/* encoder layers of the loaded model, programs currently kept, activation bytes of the program that ran last (any may be NULL) */
int ltk_hubert_info(ltk_engine* e, int* layers, int* programs, size_t* activation_bytes);
/* The HuBERT kernels on their own (unit tests; host in, host out; token-major inputs [T][C] are rounded to fp16 on the way in, outputs
 * come back channel-major [C][T]).  stats: mean_var[0] = mean, [1] = population variance of pcm.  layer0: x fp32 [n] (read as is), w
 * [512][10] -> [512][(n-10)/5+1].  ln_gelu: LayerNorm(512, eps 1e-5) + GELU.  posconv: x [T][1024], w [1024][64][128] ->
 * x + GELU(conv)[:T].  chunks: feat [T][1024] -> out [batch][rows][1024]. */
int ltk_hubert_stats(ltk_engine* e, const float* pcm, long long n, float* mean_var);
int ltk_hubert_layer0_host(ltk_engine* e, const float* x, int n, const float* w, const float* bias, const float* gamma, const float* beta,
                           float* out);
int ltk_hubert_ln_gelu_host(ltk_engine* e, const float* x, int T, const float* gamma, const float* beta, float* out);
int ltk_hubert_posconv_host(ltk_engine* e, const float* x, int T, const float* w, const float* bias, float* out);
int ltk_hubert_chunks_host(ltk_engine* e, const float* feat, int T, int batch, int first_row, int row_step, int rows, float* out);

/* U-Net + VAE decoder on explicit inputs: latents host fp32 [B][8][32][32], feat host fp32 [B][50][384] (before
 * the positional encoding).  Outputs (any may be NULL): unet_out fp32 [B][4][32][32], image fp32 [B][3][256][256]
 * (AutoencoderKL.decode sample, RGB), frames uint8 [B][256][256][3] BGR. */
int ltk_musetalk_forward_host(ltk_engine* e, const float* latents, const float* feat, int B, float* unet_out, float* image,
                              uint8_t* frames);
/* fp8 conv path: the e4m3 output tensor of op `op` (ltk_musetalk_op_name; the GroupNorm + SiLU ops in front of the ResnetBlock2D convs)
 * as the last pass left it, raw codes, uint8 [frames][C][H * W]; n_bytes must be exactly that.  Such tensors share buffers: an op's
 * codes are intact only until a later op writes the same buffer (the last e4m3 op of the program always is).  LTK_E_INVALID when the op
 * does not exist or writes fp16. */
int ltk_musetalk_debug_get_q8(ltk_engine* e, const char* op, int frames, uint8_t* out, size_t n_bytes);
/* copy a named intermediate of the last MuseTalk forward as NCHW float32 (first `frames` frames) */
int ltk_musetalk_debug_get(ltk_engine* e, const char* name, int frames, float* out, size_t n_floats);
/* average milliseconds of one U-Net + VAE pass over `frames` frames, and its conv/linear MACs */
int ltk_musetalk_time(ltk_engine* e, int frames, int iters, float* ms_per_pass, double* macs_per_pass);
/* Per-op view of the MuseTalk launch program (profiling): op names in execution order (diffusers module paths), type 0 conv /
 * linear, 1 GroupNorm, 2 LayerNorm, 3 attention, 4 GEGLU, 5 add-pos; time of every op inside a whole pass (HIP events between
 * consecutive ops on the compute stream). */
int ltk_musetalk_op_count(ltk_engine* e);
int ltk_musetalk_op_name(ltk_engine* e, int op, char* buf, int buf_len, int* type);
int ltk_musetalk_time_ops(ltk_engine* e, int frames, int iters, float* ms_per_op, int n_ops);


/* Run Wav2Lip.forward on explicit inputs: mel host float32 [B][80][16], face6
 * host float32 [B][6][256][256] in [0,1] (as wav2lip_avatar.py:133-134 builds
 * them); pred host float32 [B][3][256][256] = sigmoid output (before *255). */
int ltk_wav2lip_forward_host(ltk_engine* e, const float* mel, const float* face6, int B, float* pred);

/* Model.forward of an Ultralight avatar on explicit inputs (avatars/ultralight_avatar.py:85-90 warm_up, tests): img6 host float32
 * [B][6][160][160] in [0,1] (reference crop then masked crop, BGR, as :156-161 builds them), feat host float32 [B][16][32][32];
 * pred host float32 [B][3][160][160] = the sigmoid output (before * 255).  With ltk_debug_capture on, every launch's output is kept
 * under its state_dict prefix for ltk_debug_get ("inc.inconv.0.conv.0", "down1.maxpool_conv.0.double_conv.1.conv.6", "audio_model.conv3",
 * "up1.up", "outc.conv", ...): a conv's tap is the tensor after its BatchNorm, ReLU and residual add. */
int ltk_ultralight_forward_host(ltk_engine* e, int avatar_id, const float* img6, const float* feat, int B, float* pred);
/* the launches of an Ultralight avatar's program in execution order: the tap name of each (as ltk_ultralight_forward_host lists them,
 * and "audio_feat", the packed feature chunk) and its type: 0 dense conv (as ltk_musetalk_op_name), 10 depthwise conv, 11 upsample,
 * 12 input conv, 13 feature pack, 14 head, 15 a fused inverted residual.  The list follows knob UL_FUSE_IR as it stands (environment
 * LTK_UL_FUSE_IR or ltk_debug_set_knob; default 0: 86 ops): with the knob on, an inverted residual that ul_ir_kernel takes is listed
 * ONCE, as type 15 under its project conv's name "<block>.conv.6" (60 ops); its "<block>.conv.0" / ".conv.3" tensors do not exist in
 * such a pass and ltk_debug_get reports them as absent. */
int ltk_ultralight_op_count(ltk_engine* e, int avatar_id);
int ltk_ultralight_op_name(ltk_engine* e, int avatar_id, int op, char* buf, int buf_len, int* type);
/* The same listing with its geometry, on the host alone (no engine, no GPU): the architecture is one for every avatar.  fuse 0 / 1: the
 * listing with knob UL_FUSE_IR off / on; -1: as the knob stands.  Per launch: name and type as above; the input, output and residual
 * views - arena buffer index (-1: none; the input conv, the feature pack and the head read or write the caller's tables), channel pitch
 * `ld` and first channel `coff` of the view - and the maps H x W -> Ho x Wo; C / Creal: channels written in the layout / of the
 * reference's tensor; cin: layout channels read; k, stride, pad, relu.  A fused inverted residual (type 15) has its expand conv's input
 * view, map and cin, its depthwise conv's k / stride / pad and its project conv's everything else.  buf_halfs[b]: fp16 elements per frame
 * of arena buffer b (ltk_ultralight_info's bytes per frame = 2 * their sum).  LTK_E_INVALID when an array is NULL or too small (96 ops
 * and 12 buffers are enough). */
typedef struct ltk_ul_op_info {
    char name[64];
    int type;
    int in_buf, in_ld, in_coff, H, W;
    int out_buf, out_ld, out_coff, Ho, Wo;
    int res_buf, res_ld, res_coff;
    int C, Creal, cin, k, stride, pad, relu;
} ltk_ul_op_info;
int ltk_debug_ultralight_program(int fuse, ltk_ul_op_info* ops, int max_ops, int* n_ops, uint64_t* buf_halfs, int max_bufs, int* n_bufs);
/* average milliseconds of one pass of `frames` frames as ltk_ultralight_infer enqueues it (replayed graph under knob GRAPH), on
 * dummy inputs, and the MACs (dense + depthwise + head) it executes */
int ltk_ultralight_time(ltk_engine* e, int avatar_id, int frames, int iters, float* ms_per_pass, double* macs_per_pass);

/* Standalone depthwise 3x3 conv (nn.Conv2d(C, C, 3, stride, 1, groups=C, bias=False), avatars/ultralight/unet.py:19-25) used by kernel
 * unit tests: x device fp16 [N][C/16][H][W][16], weight host fp32 [C][1][3][3], scale / shift host fp32 [C] (NULL = 1 / 0), stride 1
 * or 2, zero padding 1; y device fp16 [N][C/16][Ho][Wo][16] = act(conv * scale + shift), Ho = (H - 1) / stride + 1. */
int ltk_dwconv3x3_f16(ltk_engine* e, const void* d_x, int N, int H, int W, int C, const float* weight, int stride, const float* scale,
                      const float* shift, int relu, void* d_y);
/* Standalone Up.forward head (unet.py:79-85): y[:, :C_up] = nn.Upsample(scale_factor=2, bilinear, align_corners=True)(x),
 * y[:, C_up:] = skip.  x device fp16 [N][C_up/16][h][w][16], skip [N][C_skip/16][Hs][Ws][16], y [N][(C_up+C_skip)/16][2h][2w][16];
 * LTK_E_INVALID unless Hs == 2h and Ws == 2w (the reference pads; the network never needs it at 160 x 160). */
int ltk_upsample2x_cat_f16(ltk_engine* e, const void* d_x, int N, int h, int w, int C_up, const void* d_skip, int Hs, int Ws, int C_skip,
                           void* d_y);

/* The call plan of ltk_ultralight_infer_merged on the host alone (no engine, no GPU): requests (avatar[r], batch[r]), the arena's
 * frames `cap`, the mode, whether the grouped path is available, and knob UL_GROUPED (0 / 1; -1: the process's knob).  Out: per pass
 * its path, avatar (-1 grouped) and frames; per span (in pass order) its pass, request, first frame of the request, frame count and
 * first frame in the pass.  LTK_E_INVALID: bad arguments, mode 2 without the grouped path, or arrays too small. */
int ltk_debug_ul_merge_plan(const int* avatar, const int* batch, int nreq, int cap, int mode, int grouped_available, int grouped_knob,
                            int* pass_path, int* pass_avatar, int* pass_nf, int max_passes, int* n_passes,
                            int* span_pass, int* span_req, int* span_first, int* span_count, int* span_at, int max_spans, int* n_spans);

/* After a forward with capture enabled, copy one layer's activation
 * (state_dict prefix, e.g. "face_encoder_blocks.1.0") as NCHW float32. */
int ltk_debug_capture(ltk_engine* e, int enable);
int ltk_debug_get(ltk_engine* e, const char* layer, float* out, size_t n_floats);

/* Tuning / A-B knobs (livetalking_amd/csrc/tune.h).  Every knob is read from the environment once per process; this call
 * changes one in-process (sweep scripts, tests).  `name` with or without the LTK_ prefix.  Process-wide, not per engine:
 * knobs that shape a plan (weight pack order) only affect plans created afterwards. */
int ltk_debug_set_knob(const char* name, int value);

/* Device-free consistency check of the engine's measured per-layer tile table (csrc/w2l_program.hip kTileTable, knob TILE_TABLE):
 * every entry must name an existing layer, a frame-count bucket and a tile / split conv3 has an instantiation for.  Returns
 * the number of bad entries (0 = consistent) and writes their descriptions into `msg` (NUL-terminated, at most `cap` bytes). */
int ltk_debug_tile_table_check(char* msg, int cap);

/* The device side of one ltk_wav2lip_infer pass, exactly as that call enqueues it (mel pack, conv stack with the bank gather
 * and the output head fused, replayed from the captured hipGraph under knob GRAPH), on dummy inputs, timed with HIP events
 * on the engine's compute stream: used by bench.py for `roofline.achieved`.  Returns average milliseconds per pass over
 * `iters` passes of `frames` frames, and the number of conv/convT MACs one pass executes (27,788,599,296 x frames for
 * wav2lip256). */
int ltk_wav2lip_time_convs(ltk_engine* e, int frames, int iters, float* ms_per_pass, double* macs_per_pass);

/* Number of frame counts whose pass currently runs from a captured hipGraph (knob GRAPH; a frame count is captured the
 * second time ltk_wav2lip_infer sees it).  Tests and bench.py use it to prove that the graph path is the one that ran. */
int ltk_wav2lip_graph_count(ltk_engine* e);

/* Opt-in deployment mode, knob FACE_CACHE (environment LTK_FACE_CACHE=1 or ltk_debug_set_knob): the Wav2Lip face encoder reads
 * the bank frame only (avatars/wav2lip/models/wav2lip_v2.py:132-140: `feats` come from the masked + reference crop, the audio
 * enters at the decoder), so its eight skip tensors are computed once per avatar - on the avatar's first ltk_wav2lip_infer call,
 * 4.15 MB of fp16 per bank frame, resident in HBM - and a pass copies them into the decoder's concat buffers instead of running
 * conv7 + 20 encoder layers.  Frames are byte-identical to the mode off for 16-frame calls (the cache is built by 16-frame
 * launches), within 1 LSB for other call sizes, byte-identical for every size under LTK_SPLITK=0.  bench.py never times this
 * mode on its headline line (cached outputs are skipped work there); it reports it on its own also[] entry.  One avatar's cache
 * is limited to LTK_FACE_CACHE_MAX_MB (default 16384; a call for a longer avatar fails with LTK_E_NOMEM, nothing allocated); the
 * first call of an avatar after the mode was switched off frees its records.  The getter may be polled from any thread.
 * Returns the bytes of skip cache the avatar currently holds (0 = none built). */
int ltk_avatar_face_cache_bytes(ltk_engine* e, int avatar_id, size_t* bytes);

/* Knob PREFETCH (default on; LTK_PREFETCH=0 switches it off): software pipelining ACROSS the calls of one session.  The face
 * encoder reads the bank frame only (wav2lip_v2.py:132-140) and a session walks its bank in order (base_avatar.py:366-376:
 * inference_batch(index, ...), index advancing by one per frame), so when a single-request call of <= 32 frames continues
 * the previous one (same avatar, index = previous index + batch) the engine runs, beside that call's audio encoder + decoder and
 * on a third stream, the face encoder of the frames the NEXT call will ask for, into the other set of concat buffers; the next
 * call then starts at the decoder.  Every layer still runs once per frame and step and the frames are byte-identical to the
 * knob off (same kernels, same launch shapes).  The prefetch is its own hipGraph on the engine's third stream, replayed right behind
 * the call's own graph.  A call that does not continue the sequence (another session, a jump of the
 * index, a multi-request call) runs the whole pass and the unused prefetch is dropped.  Counters since engine creation:
 * single-request calls that found their encoder outputs prefetched / that did not / prefetches issued. */
int ltk_wav2lip_prefetch_stats(ltk_engine* e, unsigned long long* hits, unsigned long long* misses, unsigned long long* issued);

/* Device-free: the prefetch-slot walk of a lone session's first `calls` back-to-back calls (csrc/defer_window.h, the rule
 * ltk_wav2lip_infer runs), with `outstanding` = 0 (synchronous calls: two slots) or 1 (deferred calls: the slot of the pass in
 * flight is skipped, three slots) and the index jumping in front of call `jump_at` (-1: never).  Returns the last call
 * (0-based) that runs a launch variant for the first or second time - eagerly, then captured (knob GRAPH); every later call
 * replays - or -1 for bad arguments; *slots_used = slots the walk touched.  Tests derive from it when
 * ltk_wav2lip_graph_count must have stopped growing. */
int ltk_debug_solo_walk(int outstanding, int calls, int jump_at, int* slots_used);

/* Number of (program, frame count) pairs of the MuseTalk side - the U-Net + VAE decoder pass behind ltk_musetalk_infer, the
 * Whisper encoder behind ltk_whisper_step - that currently run from a captured hipGraph (knob GRAPH; captured the second time
 * a frame count is seen). */
int ltk_program_graph_count(ltk_engine* e);

/* Per-layer view of the same pass (tuning / profiling): layer names in execution order (state_dict prefixes), the time
 * of every layer inside a whole pass on one stream (HIP events between consecutive launches, so a layer sees the cache
 * state its predecessor left, not the hot loop of an isolated microbenchmark), and the engine's per-layer tile table:
 * bucket 0..4 = launches of <= 16 / 32 / 64 / 128 / more frames; pxw in {0,1,2,4}, nbt in {0,1,2}, ksplit >= 0; 0 = rule. */
int ltk_wav2lip_layer_count(ltk_engine* e);
int ltk_wav2lip_layer_name(ltk_engine* e, int layer, char* buf, int buf_len);
int ltk_wav2lip_set_layer_tile(ltk_engine* e, int layer, int bucket, int pxw, int nbt, int ksplit);
int ltk_wav2lip_time_layers(ltk_engine* e, int frames, int iters, float* ms_per_layer, int n_layers);

/* Generic standalone fp16 conv used by kernel unit tests and per-layer timing.  Activations are in the engine's
 * channel-blocked layout: x device fp16 [N][Cin/16][H][W][16] ([N][H][W][8] when Cin <= 8), res / y device fp16
 * [N][Cout/16][Ho][Wo][16]; weight host fp32 torch layout ([Cout][Cin][kh][kw], or [Cin][Cout][kh][kw] when
 * transposed), scale/shift host fp32 [Cout] (NULL = 1 / 0).  livetalking_amd/layout.py converts from NCHW. */
int ltk_conv2d_f16(ltk_engine* e, const void* d_x, int N, int H, int W, int Cin,
                   const float* weight, int Cout, int kh, int kw, int sh, int sw, int ph, int pw,
                   int transposed, int out_pad, const float* scale, const float* shift,
                   const void* d_res, int relu, void* d_y, int iters, float* ms_avg);

/* The same fp16 conv with the caller saying WHAT runs and the hook reporting what ran (kernel unit tests).  `opts`:
 *   x_ld, x_coff / y_ld, y_coff / res_ld, res_coff : the tensor is channels [coff, coff + C) of a channel-blocked buffer of `ld` channels
 *                  (multiples of 16); ld = 0: contiguous, as ltk_conv2d_f16
 *   act          : 0 none, 1 ReLU, 2 GELU (erf), 3 SiLU (`relu` != 0 is shorthand for 1)
 *   ups          : 0; 1 = d_x is the H/2 x W/2 source map, read through a nearest 2x upsample; 2 = the same as the four-phase plan
 *                  (2x2 taps per output phase on the source map); H, W are the upsampled size in both
 *   force_pxw, force_nbt, force_ksplit : the per-layer tile table's fields, handed to the launch as the programs hand theirs (0 = rule).
 *                  A forced tile conv3 has no instantiation for is refused (LTK_E_INVALID), never replaced
 *   family       : 0 the conv kernels; 1 rowgemm (1x1 map, 1x1 conv, <= 32 frames), 2 rowconv (3x3 pad 1, stride 1 / 2, output map
 *                  <= 8 x 8), 3 rowconvT (ConvTranspose2d k3 s2 p1 op1, source map <= 8 x 8), their plans built from the torch-layout
 *                  weight as the Wav2Lip program builds them
 * `rep` (may be NULL): family as asked; conv3: kernel = the instantiation's name as ltk_debug_conv3_variants spells it, its template
 * arguments G, NBT, PXW, NC8, T, S, the effective split factor, the work items and the grid; rowgemm / rowconv / rowconvT: kernel and
 * the instantiation's FT / UB.  The first-generation kernel (csrc/conv_mfma.hip, every family-0 layer conv3 does not take): kernel =
 * "conv_mfma_kernel<NC8,NBT,TT9,MAXA>" as ltk_debug_conv1_variants spells it (TT9 true / false), NC8, NBT (the effective one, after the
 * rule that keeps a launch at 512 blocks), T = the taps per chunk (padded to even at NC8 = 1), S = the column stride, items = grid = the
 * blocks, and the tile: l2w / l2h = log2 of its width / height in output pixels, NB = its images, s2half = the column-parity pitch of the
 * patch rows (0: plain rows), phases = sub-pixel phases of the launch (4 for the transposed conv), lds = its dynamic LDS bytes, args_hash =
 * 31 bits of an FNV-1a hash over the kernel's scalar arguments (everything but the pointers); 0 for every other kernel. */
typedef struct ltk_conv_opts {
    int x_ld, x_coff, y_ld, y_coff, res_ld, res_coff;
    int act, ups;
    int force_pxw, force_nbt, force_ksplit;
    int family;
} ltk_conv_opts;
typedef struct ltk_conv_report {
    char kernel[64];
    int family, G, NBT, PXW, NC8, T, S, ksplit, items, grid, FT, UB;
    int l2w, l2h, NB, s2half, phases, lds, args_hash;
} ltk_conv_report;
int ltk_conv2d_f16_ex(ltk_engine* e, const void* d_x, int N, int H, int W, int Cin,
                      const float* weight, int Cout, int kh, int kw, int sh, int sw, int ph, int pw,
                      int transposed, int out_pad, const float* scale, const float* shift,
                      const void* d_res, int relu, void* d_y, const ltk_conv_opts* opts, ltk_conv_report* rep);

/* What ltk_conv2d_f16_ex decides about the same call before it allocates or enqueues anything, on the host alone (no engine, no GPU):
 * the option and view checks, the plan's route (conv_route), the launch plan (conv3_plan_launch with the split-K scratch taken as
 * unbounded, or the first-generation kernel's conv1_plan_launch), the row families' shape checks.  `has_res`: a residual would be passed.  `rep` as above.  Refusals that only a launcher
 * makes (more rows or frames than a row kernel is built for) are not seen here. */
int ltk_debug_conv_plan(int N, int H, int W, int Cin, int Cout, int kh, int kw, int sh, int sw, int ph, int pw,
                        int transposed, int out_pad, int has_res, int relu, const ltk_conv_opts* opts, ltk_conv_report* rep);

/* The grouped dense conv of the Ultralight program on its own (ul_gconv_kernel; the twin of ltk_conv2d_f16_ex for kernel unit tests):
 * y = clamp(relu?(conv(x, weight[set[n]]) * scale[set[n]] + shift[set[n]] + res)) for image n.  weight host fp32 [n_sets][Cout][Cin]
 * [k][k] (rounded to fp16), scale / shift host fp32 [n_sets][Cout] (NULL = 1 / 0), set host int32 [N] in [0, n_sets).  k = 1 (stride 1,
 * pad 0) or k = 3 with stride 2 and pad 1 or 3; Cin and Cout multiples of 16; N <= 256.  opts (or NULL): the channel views of x, y
 * and res as ltk_conv2d_f16_ex takes them (act, ups and the force_* fields must be 0).  rep (or NULL): kernel = "ul_gconv_kernel",
 * PXW = pixels and NBT = output channels of a block's tile, T = k-steps, grid = blocks, items = grid x * 65536 + grid y, NB = grid z.
 * Everything else: LTK_E_INVALID. */
int ltk_ul_gconv_f16(ltk_engine* e, const void* d_x, int N, int H, int W, int Cin, const float* weight, int n_sets, const int32_t* set,
                     int Cout, int k, int stride, int pad, const float* scale, const float* shift, const void* d_res, int relu, void* d_y,
                     const ltk_conv_opts* opts, ltk_conv_report* rep);

/* One inverted residual of the Ultralight program in one launch (ul_ir_kernel, csrc/ul_ir.hip; knob UL_FUSE_IR puts it into the
 * program): e1 = f16_sat(relu(w1 . x * scale1 + shift1)) [mid channels], e2 = f16_sat(relu(dw3x3(e1; stride, zero padding of the
 * hidden map) * scale_d + shift_d)), y = f16_sat(w2 . e2 * scale2 + shift2 + res); the hidden tensors stay in LDS.
 *
 * ltk_debug_ul_ir_plan: what the planner decides about a block, on the host alone (no engine, no GPU).  N <= 256 images, any H, W >= 1,
 * Cin, mid and Cout multiples of 16, stride 1 or 2 (Ho = (H - 1) / stride + 1), has_res only with Cin == Cout and stride 1, Cout / 16 one
 * of 1, 2, 3, 4, 8, 16 (the accumulators the kernel is built for), opts (or NULL): the channel views of x, y and res as ltk_conv2d_f16_ex
 * takes them (every other field must be 0); tap: the instantiation that also stores e1 / e2.  Returns LTK_OK with rep->accepted = 1 and
 * the plan, or LTK_OK with rep->accepted = 0 and rep->reason (also ltk_last_error) where the planner refuses. */
typedef struct ltk_ul_ir_report {
    char kernel[64];            /* "ul_ir_kernel<JT,tap>" */
    char reason[160];           /* why the planner refused; "" when accepted */
    int accepted;
    int Ho, Wo;
    int TH, TW;                 /* a block's tile of output pixels */
    int MC, chunks;             /* hidden channels per chunk, chunks */
    int hidden_px;              /* hidden pixels a block expands per chunk (tile + halo) */
    int lds_bytes, lds_limit;
    int grid_x, grid_y, grid_z, blocks, threads;
} ltk_ul_ir_report;
int ltk_debug_ul_ir_plan(int N, int H, int W, int Cin, int mid, int Cout, int stride, int has_res, int tap, const ltk_conv_opts* opts,
                         ltk_ul_ir_report* rep);

/* The op on its own (the twin of ltk_ul_gconv_f16).  d_x device fp16 [N][x_ld/16][H][W][16]; w1 [mid][Cin], wd [mid][3][3], w2 [Cout][mid]
 * host fp32 torch layout (w1, w2 rounded to fp16, wd stays fp32); scale / shift pairs host fp32 (NULL = 1 / 0); d_res (or NULL) and d_y
 * device fp16 at the output's geometry.  d_e1 / d_e2 (both or neither): device fp16 tap buffers [N][mid/16][H][W][16] and
 * [N][mid/16][Ho][Wo][16]; with them the tap instantiation also stores the hidden tensors, every element by the block that owns it.
 * rep (or NULL): the planner's report.  What the planner refuses: LTK_E_INVALID with its text, nothing launched. */
int ltk_ul_ir_f16(ltk_engine* e, const void* d_x, int N, int H, int W, int Cin, int mid, int Cout, int stride, const float* w1,
                  const float* wd, const float* w2, const float* scale1, const float* shift1, const float* scale_d, const float* shift_d,
                  const float* scale2, const float* shift2, const void* d_res, void* d_y, const ltk_conv_opts* opts, void* d_e1, void* d_e2,
                  ltk_ul_ir_report* rep);

/* Standalone ops of the BiSeNet face parser (avatars/musetalk/utils/face_parsing/model.py, resnet.py; csrc/parse_kernels.h), used by
 * kernel unit tests.  Tensors are device fp16 [N][C/16][H][W][16]; `opts` (may be NULL) carries channel views only - x_ld / x_coff,
 * y_ld / y_coff, res_ld / res_coff in channels, multiples of 16, 0 = the op's own channel count - as for ltk_ul_gconv_f16.
 * LTK_E_INVALID for what an op does not take (named in ltk_last_error), nothing launched.
 *   ltk_parse_stem_f16     : cp.resnet.conv1 + bn1 + ReLU on the image itself: rgb device uint8 [N][H][W][3], H and W even; each tap is
 *                            f16((v / 255 - mean_c) / std_c) with mean (0.485, 0.456, 0.406), std (0.229, 0.224, 0.225) inside the image
 *                            and 0 outside it (the padding of the NORMALISED tensor); weight host fp32 [64][3][7][7] (rounded to fp16),
 *                            scale / shift host fp32 [64] (NULL = 1 / 0); y = relu(conv * scale + shift), 64 channels on H/2 x W/2.
 *   ltk_maxpool3x3s2_f16   : nn.MaxPool2d(3, 2, 1), padding -inf; y on ((H - 1) / 2 + 1) x ((W - 1) / 2 + 1).  Exact.
 *   ltk_global_avgpool_f16 : mean over the P <= 4096 pixels of each channel, y [N][C/16][1][16]; fp32 sums in one fixed tree, so a
 *                            channel's bytes depend on its own P values only.
 *   ltk_chan_gate_f16      : y = x * (sigmoid(a) [+ 1 if plus1]) [+ b] [+ r]; a and b (may be NULL) dense device fp16 [N][C/16][1][16],
 *                            r (may be NULL) a map like x (view: res_ld / res_coff); fp32, one rounding.
 *   ltk_seg_argmax_f16     : x [N][2][h][w][16] logits, classes 0..18; labels device uint8 [N][8h][8w] = argmax over the 19 classes of
 *                            the bilinear x8 upsample (align_corners=True), fp32 interpolation, the lowest class wins a tie. */
int ltk_parse_stem_f16(ltk_engine* e, const void* d_rgb, int N, int H, int W, const float* weight, const float* scale, const float* shift,
                       void* d_y, const ltk_conv_opts* opts);
int ltk_maxpool3x3s2_f16(ltk_engine* e, const void* d_x, int N, int H, int W, int C, void* d_y, const ltk_conv_opts* opts);
int ltk_global_avgpool_f16(ltk_engine* e, const void* d_x, int N, int P, int C, void* d_y, const ltk_conv_opts* opts);
int ltk_chan_gate_f16(ltk_engine* e, const void* d_x, int N, int P, int C, const void* d_a, const void* d_b, const void* d_r, int plus1,
                      void* d_y, const ltk_conv_opts* opts);
int ltk_seg_argmax_f16(ltk_engine* e, const void* d_x, int N, int h, int w, void* d_labels);

/* The launch list of the face parser's main output (BiSeNet.forward()[0] + argmax) at one square image size, on the host alone (no
 * engine, no GPU; the program of ltk_face_parse_load runs it): per launch its name - the module's, a conv's output standing behind its BatchNorm, ReLU and
 * residual add -, type (0 the library's conv, 10 stem, 11 max pool, 12 global average pool, 13 channel gate, 14 labels), real channels
 * in and out, k / stride / pad, relu, ups (the conv reads its input through a nearest x2 upsample; H x W is then the upsampled map),
 * has_res (a residual, or the gate's added map), plus1 (the gate's feat * atten + feat form), the map read H x W (the stem: the image)
 * and written Ho x Wo (labels: the image).  41 launches.  LTK_E_INVALID: size not a multiple of 32 in [64, 512], or max_ops too small. */
typedef struct ltk_fp_op_info {
    char name[64];
    int type, cin, cout, k, stride, pad, relu, ups, has_res, plus1;
    int H, W, Ho, Wo;
} ltk_fp_op_info;
int ltk_debug_face_parse_program(int size, ltk_fp_op_info* ops, int max_ops, int* n_ops);

/* Where every launch of that list reads and writes at (size, max_images), on the host alone: the binding table the device program of
 * ltk_face_parse_load is built from (csrc/faceparse.h fp_plan).  A view = channels [coff, coff + C) of buffer `buf`, which holds `ld`
 * channels, on an H x W map; buf = -1: the op has no such operand.  x, y: input and output (a conv behind a nearest x2 upsample: x is the
 * stored map, half the op's H x W); r: a conv's residual or the map a gate adds; a, b: a gate's pre-sigmoid attention and the per-channel
 * value it adds, dense 1 x 1 maps.  fp16 buffers are channel-blocked (C, ld, coff multiples of 16; conv_out.conv_out writes 32 layout
 * channels, 19 real); *image_buf is uint8 [max_images][size][size][3] (C = ld = 3), *label_buf uint8 [max_images][size][size]
 * (C = ld = 1).  buf_bytes[i]: bytes of buffer i at max_images; *n_bufs of them.  ffm.convblk reads ONE 256-channel buffer whose halves
 * cp.resnet.layer2.1.conv2 and cp.conv_head16 write.  LTK_E_INVALID: size as above, max_images outside [1, 8], max_ops / max_bufs too
 * small. */
typedef struct ltk_fp_view { int buf, ld, coff, C, H, W; } ltk_fp_view;
typedef struct ltk_fp_bind {
    char name[64];
    ltk_fp_view x, y, r, a, b;
} ltk_fp_bind;
int ltk_debug_face_parse_plan(int size, int max_images, ltk_fp_bind* ops, int max_ops, int* n_ops, unsigned long long* buf_bytes,
                              int max_bufs, int* n_bufs, int* image_buf, int* label_buf);
/* Measurement hook (scripts/face_parse_time.py; not on the production call path), the twin of ltk_musetalk_time / _time_ops for the
 * program of ltk_face_parse_load: *ms_per_pass = milliseconds of one device pass of `images` <= max_images images, replayed as
 * ltk_face_parse replays it, without upload or copy-back, over `iters` runs; ms_per_op (or NULL; n_ops = 41): per-launch times from
 * events between eager launches.  Whatever the last ltk_face_parse left in the program's buffers is the input.  LTK_E_STATE before a
 * load; a run the program refuses: its code and text as ltk_face_parse reports them. */
int ltk_debug_face_parse_time(ltk_engine* e, int images, int iters, float* ms_per_pass, float* ms_per_op, int n_ops);

/* Standalone ops of the S3FD face detector (avatars/wav2lip/face_detection/detection/sfd/net_s3fd.py, detect.py, bbox.py;
 * csrc/s3fd_kernels.h), used by kernel unit tests.  Tensors are device fp16 [N][C/16][H][W][16]; `opts` (may be NULL) carries channel
 * views only, as for the face parser's ops.  LTK_E_INVALID for what an op does not take (named in ltk_last_error), nothing launched.
 *   ltk_s3fd_stem_f16    : conv1_1 + ReLU (net_s3fd.py:71) on the frame itself: bgr device uint8 [N][H][W][3] as cv2.imread gives it, any
 *                          H, W >= 1.  The input transform of api.py:65 and detect.py:59 is fused: the network's channel c is byte 2 - c
 *                          of the pixel minus (104, 117, 123)[c] (the means in the order the reference applies them to the REVERSED
 *                          image); 0 outside the image (the padding of the mean-subtracted tensor).  weight host fp32 [64][3][3][3]
 *                          (rounded to fp16), bias host fp32 [64] (NULL = 0); y = relu(conv + bias), 64 channels on H x W.
 *   ltk_maxpool2x2s2_f16 : F.max_pool2d(x, 2, 2), floor mode: y on (H / 2) x (W / 2), an odd last row / column is dropped.  Exact.
 *   ltk_l2norm_f16       : L2Norm (net_s3fd.py:16-19) over the C channels of each of P pixels: y = x / (sqrt(sum x^2) + 1e-10) * weight[c],
 *                          the sum in fp32 in ascending channel order, one fp16 rounding; weight host fp32 [C].
 *   ltk_s3fd_detect_f16  : detect.py:71-89 + bbox.py:111-129 for level `level` (stride 2^(level+2)) of a merged head map x [N][1][H][W][16]
 *                          (conf at channels 0..1 - 0..3 with maxout: conf = [max(c0, c1, c2), c3] -, loc at 4..7): where the fp32
 *                          two-way softmax score > thresh, one record {uint32 key = level << 28 | h << 14 | w, float x1, y1, x2, y2,
 *                          score} is appended to d_recs [N][cap][6 words] through the counter d_counts[n] (uint32 [N], NOT reset by the
 *                          call; it keeps counting past cap, records beyond cap are dropped).  Arrival order is arbitrary. */
int ltk_s3fd_stem_f16(ltk_engine* e, const void* d_bgr, int N, int H, int W, const float* weight, const float* bias, void* d_y,
                      const ltk_conv_opts* opts);
int ltk_maxpool2x2s2_f16(ltk_engine* e, const void* d_x, int N, int H, int W, int C, void* d_y, const ltk_conv_opts* opts);
int ltk_l2norm_f16(ltk_engine* e, const void* d_x, int N, int P, int C, const float* weight, void* d_y, const ltk_conv_opts* opts);
int ltk_s3fd_detect_f16(ltk_engine* e, const void* d_x, int N, int H, int W, int maxout, int level, float thresh, void* d_recs, int cap,
                        void* d_counts, const ltk_conv_opts* opts);

/* The launch list of the S3FD face detector at one frame size, on the host alone (no engine, no GPU; csrc/facedet.h fd_program): per
 * launch its name, type (0 the library's conv, 20 stem, 21 max pool 2x2, 22 L2Norm, 23 detect), channels in and out, k / stride / pad,
 * relu, maxout and level (heads and detects; -1 elsewhere), the map read H x W (the stem: the frame) and written Ho x Wo.  A level's conf
 * and loc convs are ONE conv "<source>_mbox" of 16 output channels (conf at 0..1 - 0..3 at level 0 -, loc at 4..7, the rest zero).
 * 39 launches.  Level 3 is the fc7 map, (H/32 + 4) x (W/32 + 4), read with stride 32, as in the reference.
 * LTK_E_INVALID: H or W outside [32, 16384], or max_ops too small. */
typedef struct ltk_fd_op_info {
    char name[64];
    int type, cin, cout, k, stride, pad, relu, maxout, level;
    int H, W, Ho, Wo;
} ltk_fd_op_info;
int ltk_debug_face_detect_program(int H, int W, ltk_fd_op_info* ops, int max_ops, int* n_ops);

/* Where every launch of that list reads (x) and writes (y) at (H, W, max_images), on the host alone (csrc/facedet.h fd_plan); views as
 * in ltk_debug_face_parse_plan.  The two trunk buffers are written in turn; tapped maps, norms and heads have buffers of their own; a
 * detect op has no y: it appends to the record buffer, the last of the table (per image 4096 records of 24 bytes and a share of the
 * 256-byte head).  *image_buf is uint8 [max_images][H][W][3].  buf_bytes[i]: bytes of buffer i at
 * max_images, *total_bytes their sum.  LTK_E_INVALID: sizes as above, max_images outside [1, 16], total_bytes at or above 8 GiB (the
 * text names the figure), max_ops / max_bufs too small. */
typedef struct ltk_fd_bind {
    char name[64];
    ltk_fp_view x, y;
} ltk_fd_bind;
int ltk_debug_face_detect_plan(int H, int W, int max_images, ltk_fd_bind* ops, int max_ops, int* n_ops, unsigned long long* buf_bytes,
                               int max_bufs, int* n_bufs, int* image_buf, unsigned long long* total_bytes);

/* Measurement hook (scripts/face_detect_time.py; not on the production call path), the twin of ltk_debug_face_parse_time for the
 * program of the frame size the last ltk_face_detect ran: *ms_per_pass = milliseconds of one device pass of `images` <= max_images
 * images, replayed as ltk_face_detect replays it, without upload or copy-back, over `iters` runs; ms_per_op (or NULL; n_ops = 39):
 * per-launch times from events between eager launches.  Whatever that call left in the program's buffers is the input (the counters
 * are not reset: the lists fill up and the detect launches go on counting).  LTK_E_STATE before a load or a first call. */
int ltk_debug_face_detect_time(ltk_engine* e, int images, int iters, float* ms_per_pass, float* ms_per_op, int n_ops);

/* Names of every fp16 conv3 instantiation the launch path can pick, one per line, NUL-terminated, into buf[cap]; no GPU needed.
 * Returns LTK_E_INVALID when cap is too small. */
int ltk_debug_conv3_variants(char* buf, int cap);

/* ... and of every instantiation of the first-generation kernel its picker can return (csrc/conv_mfma.hip: the table pick_kernel is
 * made of), the same way. */
int ltk_debug_conv1_variants(char* buf, int cap);

/* The special-case kernels at the head of the Wav2Lip program (csrc/conv7_mfma.hip) on their own, for kernel unit tests: the op's plan
 * from torch-layout fp32 weights and the folded scale / shift (host fp32, one per output channel), its existing launch on the compute
 * stream, synchronised.  All ops end in ReLU.
 *   CONV7_BANK    Conv2d(6, 16, 7, 1, 3) with the input pack fused: frame i is frame_ptrs[i], device uint8 [256][256][3]; the operand is
 *                 fp16(fp32(byte) * fp32(1 / 255)) = {b, g, r with rows >= 128 zero, b, g, r, 0, 0}; y = 16 channels at 256 x 256
 *   CONV7_PACKED  the same layer from d_x = fp16 [N][256][256][8], the packed operand itself
 *   AUDIO0        Conv2d(1, 32, 3, 1, 1): frame i is frame_ptrs[i], device fp32 [80][16], rounded to fp16; y = 32 channels at 80 x 16
 *   AUDIO3        Conv2d(32, 64, 3, (3, 1), 1): d_x = CB16 of 32 channels at 80 x 16; y = 64 channels at 27 x 16
 *   CONVS2D       Conv2d(Cin, Cout, 3, 2, 1), Cin 16 or 32, Cout % 32 == 0: d_x = CB16 of Cin channels at H x W (H even, W % 64 == 0);
 *                 y = Cout channels at H/2 x W/2
 * frame_ptrs: HOST array of N device pointers (BANK, AUDIO0; any order, repeats allowed - the hook uploads it as the launch's FacePtrs /
 * MelPtrs table, as the bank gather does); d_x: the other ops' input.  H, W, Cin, Cout: CONVS2D only.  `opts`: y (and x of AUDIO3 /
 * CONVS2D) are channels [coff, coff + C) of a channel-blocked buffer of `ld` channels; ld = 0: contiguous.  What the launchers and plans
 * refuse - more than 256 frames, a view that is no multiple of 16 channels, odd H, W % 64 != 0, another Cin - comes back as
 * LTK_E_INVALID with their message. */
enum { LTK_W2L_CONV7_BANK = 0, LTK_W2L_CONV7_PACKED = 1, LTK_W2L_AUDIO0 = 2, LTK_W2L_AUDIO3 = 3, LTK_W2L_CONVS2D = 4 };

/* Standalone GroupNorm (+ SiLU) over a channel-blocked fp16 tensor, for kernel unit tests and timing (diffusers GroupNorm as the MuseTalk U-Net / VAE
 * use it; `avatars/musetalk/models/unet.py:36-46`, `vae.py:96-108` call sites).  x, y: device fp16 [N][C/16][P][16]; gamma / beta host fp32 [C];
 * impl: 0 = what the MuseTalk program would pick for this shape, 1 = gn_stats + gn_apply (two launches, three tensor passes), 2 = gn_group_kernel
 * (one block per (image, group)), 3 = gn_coop_kernel (one tensor pass, blocks exchange partial sums); an impl that does not serve the shape is refused.
 * out_fp8 != 0: y is e4m3 [N][C/32][P][32] = min(max(result * out_scale, -448), 448) (the operand format of the fp8 conv path).
 * iters > 0: additionally timed over `iters` back-to-back runs. */
int ltk_groupnorm_f16(ltk_engine* e, const void* d_x, int N, int C, int P, int groups, float eps, const float* gamma, const float* beta,
                      int silu, int impl, int out_fp8, float out_scale, void* d_y, int iters, float* ms_avg);

/* The same GroupNorm on channel VIEWS, reporting what ran (kernel unit tests; one body with ltk_groupnorm_f16).  `opts`: x / y are channels
 * [coff, coff + C) of a channel-blocked buffer of `ld` channels - multiples of 16, for an e4m3 y of 32; ld = 0: contiguous.  `rep` (may be
 * NULL): impl as resolved; kernel = the instantiation, "gn_stats_kernel+gn_apply_kernel<false|true>", "gn_group_kernel<KMAX,NT,false|true>"
 * (from gn_group_variant, the rule the launch itself switches on) or "gn_coop_kernel<false|true>"; segs (two-pass: pixel segments of the
 * statistics), members (gn_coop: blocks per set), grid (blocks of the launch that writes y).  x and y must not overlap (both hooks refuse it:
 * the kernels read a group's shift from x while other blocks store y). */
typedef struct ltk_norm_opts {
    int x_ld, x_coff, y_ld, y_coff;
} ltk_norm_opts;
typedef struct ltk_norm_report {
    char kernel[64];
    int impl, segs, members, grid;
} ltk_norm_report;
int ltk_groupnorm_f16_ex(ltk_engine* e, const void* d_x, int N, int C, int P, int groups, float eps, const float* gamma, const float* beta,
                         int silu, int impl, int out_fp8, float out_scale, void* d_y, const ltk_norm_opts* opts, ltk_norm_report* rep);

/* (the LTK_W2L_* ops above) */
int ltk_w2l_head_f16(ltk_engine* e, int op, const void* const* frame_ptrs, const void* d_x, int N, int H, int W, int Cin, int Cout,
                     const float* weight, const float* scale, const float* shift, void* d_y, const ltk_norm_opts* opts);

/* The pointwise and layout kernels of csrc/nn_kernels.hip on their own (kernel unit tests): the existing launch, on the compute stream,
 * synchronised.  N images of P pixels / tokens and C channels; `opts` as above (views of 16-channel blocks; x_* unused where x is fp32).
 *   LAYERNORM      x, y fp16 CB16; v0 = gamma[C], v1 = beta[C] (host fp32), eps; C % 16 == 0
 *   GEGLU          x fp16 CB16 of 2 C channels (a = [0, C), gate = [C, 2 C)), y of C; C % 16 == 0
 *   ACT_GELU/SILU  x, y fp16 CB16; C % 16 == 0
 *   ADD_POS        in place on y (d_x unused): y += v0[P][C] (host fp32); any C, the view spans ceil(C / 16) blocks
 *   NCHW_TO_CB16   x device fp32 [N][C][P] -> y; padding channels of the last block zero
 *   TOKENS_TO_CB16 x device fp32 [N][P][C] (+ v0[P][C] host fp32 when not NULL) -> y
 *   VAE_POST       x fp16 CB16 (channels 0..2 = RGB in [-1, 1]), C = 3, N <= 64 -> y uint8 [N][P][3] BGR (y_* unused; P * 3 % 4 == 0 when N > 1)
 * v0 / v1 are ignored by the ops that take none. */
enum { LTK_PW_LAYERNORM = 0, LTK_PW_GEGLU = 1, LTK_PW_ACT_GELU = 2, LTK_PW_ACT_SILU = 3, LTK_PW_ADD_POS = 4, LTK_PW_NCHW_TO_CB16 = 5,
       LTK_PW_TOKENS_TO_CB16 = 6, LTK_PW_VAE_POST = 7 };
int ltk_pointwise_f16(ltk_engine* e, int op, const void* d_x, void* d_y, int N, int C, int P, float eps, const float* v0, const float* v1,
                      const ltk_norm_opts* opts);

/* Standalone attention O = softmax(Q K^T) V per (image, head) over channel-blocked fp16 tensors, for kernel unit tests: v_transpose_kernel into a
 * scratch V^T of the hook's own, then the attention kernel, on the compute stream, synchronised.  q / o: device fp16 [N][cbt][Tq][16], k / v:
 * [N][cbt][Tk][16]; every tensor has its own cbt (channel blocks in its buffer) and cb0 (first block of head 0), head h at blocks
 * [cb0 + h * d16 / 16, + d16 / 16): views into a stacked q|k|v buffer and an output in the middle of a wider one.  d16 in {48, 64, 80, 160, 512};
 * the 1 / sqrt(d) scale is the caller's, as in the programs (folded into q).  impl: 0 = what a program would launch under the current
 * knobs, 1 = the per-wave kernel (attn_kernel; attn_wide_kernel at d16 = 512) even where the LDS form serves the shape, 2 = attn_lds_kernel
 * (d16 48 / 80, Tk a multiple of 64 and >= 128); an impl that does not serve the shape is refused. */
int ltk_attention_f16(ltk_engine* e, const void* d_q, int q_cbt, int q_cb0, const void* d_k, int k_cbt, int k_cb0, const void* d_v, int v_cbt,
                      int v_cb0, void* d_o, int o_cbt, int o_cb0, int N, int heads, int d16, int Tq, int Tk, int impl);

/* host-side fp32 -> OCP e4m3fn conversion of the weight packer (round to nearest even, saturating at +-448); no GPU needed */
int ltk_f32_to_e4m3(const float* in, size_t n, uint8_t* out);

/* fp8-operand 3x3 stride-1 pad-1 conv used by kernel unit tests and per-layer timing: x device e4m3 bytes
 * [N][Cin/32][H][W][32] holding round(x * act_scale), weight host fp32 [Cout][Cin][3][3] (quantised per output channel
 * by the engine), y = act((conv(x, w)) * scale + shift + res) as fp16 [N][Cout/16][H][W][16]; act: 0 none, 1 ReLU,
 * 2 GELU, 3 SiLU. */
int ltk_conv2d_fp8(ltk_engine* e, const void* d_x, int N, int H, int W, int Cin, const float* weight, int Cout,
                   const float* scale, const float* shift, float act_scale, const void* d_res, int act, void* d_y, int iters,
                   float* ms_avg);

/* The same fp8 conv with the caller saying WHAT runs and the hook reporting what ran (kernel unit tests; one body with
 * ltk_conv2d_f16_ex).  quant: 0 = the program's rule (MX from 512 input channels on, Cin % 64 == 0), 1 = the e4m3 MFMA, 2 = the MX-scaled
 * MFMA (Cin % 64 == 0).  `opts` as for ltk_conv2d_f16_ex with family 0 and ups 0; x_ld / x_coff count fp8 channels, in multiples of
 * 32 (one 32-byte block per pixel), y_* and res_* fp16 channels in multiples of 16.  `rep` (may be NULL): kernel = the instantiation as
 * ltk_debug_conv3_fp8_variants spells it, conv3_kernel<1,NBT,PXW,NC8,9,1,Q> with Q = 1 (e4m3) or 2 (MX); NC8 counts 16-byte planes
 * of 16 fp8 channels; the other fields as above. */
int ltk_conv2d_fp8_ex(ltk_engine* e, const void* d_x, int N, int H, int W, int Cin, const float* weight, int Cout,
                      const float* scale, const float* shift, float act_scale, int quant, const void* d_res, void* d_y,
                      const ltk_conv_opts* opts, ltk_conv_report* rep);

/* What ltk_conv2d_fp8_ex decides before it allocates or enqueues anything, on the host alone (no engine, no GPU), as
 * ltk_debug_conv_plan does for the fp16 hook.  The layer geometry is an argument here so that what the fp8 route refuses (anything
 * but 3x3 stride 1 pad 1, Cin % 32, MX with Cin % 64) can be seen refused. */
int ltk_debug_conv_fp8_plan(int N, int H, int W, int Cin, int Cout, int kh, int kw, int sh, int sw, int ph, int pw,
                            int transposed, int out_pad, int quant, int has_res, const ltk_conv_opts* opts, ltk_conv_report* rep);

/* Names of every fp8 conv3 instantiation the launch path can pick (e4m3 and MX), one per line, as ltk_debug_conv3_variants. */
int ltk_debug_conv3_fp8_variants(char* buf, int cap);

#ifdef __cplusplus
}
#endif
#endif /* LTK_H */

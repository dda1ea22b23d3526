// What the engine's sources share (engine.hip, w2l_program.hip, w2l_infer.hip, mt_engine.hip, egress.hip, engine_debug.hip): the
// engine's state, its error and RAII helpers, and the few functions that cross sources.  Not installed, not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ltk.h"
#include "conv_mfma.h"
#include "defer_window.h"
#include "dw_kernels.h"
#include "hubert_kernels.h"
#include "misc_kernels.h"
#include "musetalk.h"
#include "nn_kernels.h"
#include "state_dict.h"
#include "tune.h"

namespace ltk {

// The last error text of the calling host thread (ltk_last_error): ONE thread_local string, defined in engine.hip, whichever
// source sets it
extern thread_local std::string g_err;
inline int fail(int code, const std::string& msg) { g_err = msg; return code; }
// the plan / launch functions' -1 (refused) and -2 (HIP error), with their text, as the ABI's codes
inline int conv_status(int rc, const std::string& err) { return fail(rc == -2 ? LTK_E_HIP : LTK_E_INVALID, err); }

// Entry of every call that launches: select the engine's GPU, and drop whatever error an EARLIER runtime call left behind on this
// host thread (ours after a reported failure, or another library's) - hipGetLastError() after a launch must speak about that launch
inline hipError_t enter_device(int device) {
    (void)hipGetLastError();
    return hipSetDevice(device);
}

#define CHK(expr)                                                                        \
    do {                                                                                 \
        hipError_t _e = (expr);                                                          \
        if (_e != hipSuccess) return fail(LTK_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

const int kDecCh[8] = {512, 512, 512, 512, 384, 256, 128, 64};
const int kFeatCh[8] = {16, 32, 64, 128, 256, 512, 512, 512};
const int kFeatHW[8] = {256, 128, 64, 32, 16, 8, 4, 1};
constexpr int kPrefetchMaxFrames = 32;     // knob PREFETCH: calls of at most this many frames are pipelined across calls
enum BufId { B_MEL = 0, B_AT0, B_AT1, B_X0, B_T0, B_T1, B_OUT32, B_CAT0, B_COUNT = B_CAT0 + 8 };

struct Layer {
    std::string name;
    ConvPlan plan;
    RowGemmPlan rg;                 // set for the layers whose input and output maps are one pixel per frame (rowgemm.hip)
    int rg_y_ld = 0;               // output row pitch of that GEMM (the 1x1-expand layer writes k*k*Cout contiguous channels)
    bool rowconv = false;          // `rg` is a rowconv plan instead: 3x3 conv on a map of <= 8 x 8 output pixels (rowgemm.hip)
    int rc_stride = 1, rc_stride_w = 0;
    RowGemmPlan rgT[4];            // ConvTranspose2d(k3,s2,p1,op1) on a source map of <= 8 x 8 pixels: one plan per output phase (rowconvT_launch)
    int cin_real = 0;
    int in_buf = 0, in_ld = 0, in_coff = 0, H = 0, W = 0;
    int out_buf = 0, out_ld = 0, out_coff = 0, Ho = 0, Wo = 0;
    bool residual = false;
    bool res_folded = false;   // the identity branch lives in the centre tap of the packed weights
    bool audio = false;   // audio-encoder layer (independent of the face encoder until decoder block 0)
    int special = 0;      // 3: audio_encoder.3, which has a kernel of its own (audio3_kernel, knob AUDIO0 bit 1)
    ConvS2dPlan* s2d = nullptr;   // face_encoder_blocks.1.0 / 2.0: the shallow stride-2 layers on convs2d_kernel (conv7_mfma.hip, knob CONV_S2D)
    bool face_enc = false;   // face-encoder layer: depends on the bank frame only (knob FACE_CACHE)
    double macs = 0;  // per frame
    // measured tile / split choice per frame-count bucket (<= 16, 32, 64, 128, 256+ frames per launch); 0 = conv3's rule
    struct Tile { signed char pxw = 0, nbt = 0, ks = 0; } tile[5];
};

// Avatar banks are shared_ptr-owned: an entry point keeps its avatar alive for the duration of the call, so a concurrent
// ltk_avatar_release only drops the table's reference and the device buffers go when the last call using them returns
// (every entry point synchronises its stream before it returns).  The destructor also frees a half-built bank when a
// register call fails part-way.
struct Avatar {
    uint8_t* d_face = nullptr;
    uint8_t* d_full = nullptr;
    std::vector<int32_t> coords;
    int n = 0, H = 0, W = 0;
    int device = 0;
    // knob FACE_CACHE: the face encoder's skip tensors of every bank frame (records of feat_rec_bytes, misc_kernels.h FeatGeom),
    // built on first use under the engine's enqueue lock; feat_epoch = knob_epoch() it was built under
    // (d_feat / feat_rec_bytes / feat_epoch are touched under the engine's enqueue lock only; feat_bytes is what the statistics
    // getter reads from other threads)
    uint8_t* d_feat = nullptr;
    size_t feat_rec_bytes = 0;
    unsigned feat_epoch = 0;
    std::atomic<size_t> feat_bytes{0};
    Avatar() = default;
    Avatar(const Avatar&) = delete;
    Avatar& operator=(const Avatar&) = delete;
    ~Avatar() {
        (void)hipSetDevice(device);
        if (d_face) (void)hipFree(d_face);
        if (d_full) (void)hipFree(d_full);
        if (d_feat) (void)hipFree(d_feat);
    }
};

struct Scratch {
    void* d = nullptr;
    size_t cap = 0;
};

// MuseTalk avatar bank (musetalk_avatar.py:69-91)
struct MtAvatar {
    float* d_latents = nullptr;      // [n][8][32][32]
    uint8_t* d_full = nullptr;       // [n][H][W][3]
    uint8_t* d_masks = nullptr;      // concatenated
    std::vector<int64_t> mask_off;
    std::vector<int32_t> face_box, crop_box;
    int n = 0, H = 0, W = 0;
    int device = 0;
    MtAvatar() = default;
    MtAvatar(const MtAvatar&) = delete;
    MtAvatar& operator=(const MtAvatar&) = delete;
    ~MtAvatar() {
        (void)hipSetDevice(device);
        if (d_latents) (void)hipFree(d_latents);
        if (d_full) (void)hipFree(d_full);
        if (d_masks) (void)hipFree(d_masks);
    }
};

// Ultralight avatar (avatars/ultralight_avatar.py:63-81): the model is per avatar, so the launch program (ultralight.hip) lives with
// the bank.  boxes = coords.pkl as (x1, y1, x2, y2).
struct UlProgram;                                     // ultralight.hip: the avatar's operands, one record per op of the architecture
struct UlGroupTab;                                    // ul_gconv.h
struct HealthWatch;                                   // below
struct UlAvatar {
    std::unique_ptr<UlProgram> prog;
    std::unique_ptr<HealthWatch> health;  // the avatar's headroom watch, one record per op of the architecture table; under the engine's enqueue lock
    uint8_t* d_face = nullptr;       // [n][168][168][3]
    uint8_t* d_full = nullptr;       // [n][H][W][3]
    std::vector<int32_t> boxes;
    int n = 0, H = 0, W = 0;
    int device = 0;
    int id = 0;
    UlAvatar();                      // ultralight.hip, where UlProgram is complete
    UlAvatar(const UlAvatar&) = delete;
    UlAvatar& operator=(const UlAvatar&) = delete;
    ~UlAvatar();                     // selects the device, frees the banks, then the program's operands
};
constexpr int kUlBufs = 12;           // activation buffers of the Ultralight program (ultralight.hip UlBuf)

// ---------------------------------------------------------------- headroom watch (ltk_health_watch, include/ltk.h)
// One table of op records (misc_kernels.h HealthRec) beside a launch program, indexed by the program's own op listing, owned by whoever
// owns the program (the engine; an Ultralight avatar).  Armed for the next `left` engine calls of the program; a watched call runs its
// usual launches eagerly with one launch_health_scan behind every op whose output is in memory.  Everything here is touched under the
// engine's enqueue lock (ltk_engine::mu) only.
struct HealthWatch {
    HealthRec* d = nullptr;               // [n] records; the scan kernel is their only writer, arming zeroes them
    int n = 0;
    int left = 0, seen = 0;               // calls still to watch / watched since the watch was armed
    std::vector<unsigned char> observed;  // [n] a scan was launched for the op since the watch was armed
    HealthWatch() = default;
    HealthWatch(const HealthWatch&) = delete;
    HealthWatch& operator=(const HealthWatch&) = delete;
    ~HealthWatch() { release(); }         // (the owner has selected the device)
    int alloc(int n_ops) {
        release();
        if (n_ops <= 0) return 0;
        if (hipMalloc((void**)&d, (size_t)n_ops * sizeof(HealthRec)) != hipSuccess) { d = nullptr; (void)hipGetLastError(); return -1; }
        if (hipMemset(d, 0, (size_t)n_ops * sizeof(HealthRec)) != hipSuccess) { release(); return -1; }
        n = n_ops;
        observed.assign((size_t)n_ops, 0);
        return 0;
    }
    void release() {
        if (d) (void)hipFree(d);
        d = nullptr; n = 0; left = 0; seen = 0; observed.clear();
    }
    // the engine call being enqueued: is it watched?  Counts it.
    bool begin() {
        if (!d || left <= 0) return false;
        --left; ++seen;
        return true;
    }
    // op `i` of the watched call wrote the view: one scan launch behind it on its stream
    void scan(int i, const void* x, int N, int cbt, int cb0, int CB, long long P, int q8, hipStream_t s) {
        if (!d || i < 0 || i >= n) return;
        launch_health_scan(x, N, cbt, cb0, CB, P, q8, d + i, s);
        observed[(size_t)i] = 1;
    }
};

// RAII HIP event: error returns between create and destroy do not leak it
struct Ev {
    hipEvent_t e = nullptr;
    hipError_t create() { return hipEventCreateWithFlags(&e, hipEventDisableTiming); }
    ~Ev() { if (e) (void)hipEventDestroy(e); }
};

// ---------------------------------------------------------------- captured launch sequences (knob GRAPH)
constexpr size_t kMaxPassGraphs = 64;
struct PassGraph {
    hipGraphExec_t exec = nullptr;
    int seen = 0;                     // sightings before the capture; -1: a capture failed, the key runs eagerly for good
    unsigned long stamp = 0;          // LRU clock (ltk_engine::graph_clock, one counter for both caches) of the last use
    hipStream_t stream = nullptr;     // where it was last launched: synchronised before the graph is destroyed
};

// "Run eagerly on first sight, capture on the second, replay after, evict the least recently used at kMaxPassGraphs": a launch
// sequence without per-call arguments (`enq` issues it on `s`, returns 0 or its error), keyed by whatever shapes it.  The eager first
// run also sets every kernel's dynamic-LDS attribute, which a capture must not do.  Under e->mu.  run() returns 0, enq's error, or
// LTK_E_HIP (= -2, also what a program's mt_run returns for a runtime failure) with the text set.  What happens when something fails:
//  - the stream cannot enter capture mode, or the captured graph cannot be instantiated: the sticky error is cleared, the key never
//    captures again (seen = -1) and the launches are issued eagerly: the call still produces its frames;
//  - `enq` fails inside a capture: the capture is ended (the stream must leave capture mode; with a forked and never joined
//    side stream EndCapture reports an unjoined capture, logged once per key), the sticky error cleared so that the next call's
//    own checks do not report this one, the graph destroyed, seen = -1, enq's error returned.  Nothing reached the stream;
//  - an evicted entry goes back to seen = 1 (captured again at its next sighting).  Before a graph is destroyed the compute
//    stream and the stream it was last launched on are synchronised: it may still be running for the previous call.
template <class Key>
struct GraphCache {
    std::map<Key, PassGraph> graphs;
    unsigned epoch = 0;               // knob_epoch() the graphs were captured under
    hipStream_t side = nullptr;       // graphs of this cache also run beside the compute stream, on this one (the prefetch stream)
    int live() const {
        int n = 0;
        for (auto& kv : graphs) n += kv.second.exec ? 1 : 0;
        return n;
    }
    void drop() {
        if (side) (void)hipStreamSynchronize(side);      // a prefetch graph may still be running on the third stream
        for (auto& kv : graphs)
            if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
        graphs.clear();
    }
    template <class Enq>
    int run(ltk_engine* e, const Key& k, hipStream_t s, const char* what, int nf, Enq enq);
};

}  // namespace ltk

using namespace ltk;      // as every engine source does

struct ltk_engine {
    int device = 0;
    hipStream_t compute = nullptr;
    hipStream_t aux = nullptr;            // audio encoder runs beside the face encoder (wav2lip_v2.py:132 vs :136-140)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    float* d_partial = nullptr;           // conv3 split-K scratch of the compute stream
    float* d_partial_aux = nullptr;       // ... of the aux stream
    float* d_partial_pf = nullptr;        // ... of the prefetch stream (aux2, knob PREFETCH)
    size_t partial_cap = 0, partial_aux_cap = 0, partial_pf_cap = 0;
    // headroom watches (ltk_health_watch), allocated when their program is loaded: Wav2Lip by layer; the MuseTalk, Whisper, HuBERT and
    // face-parser programs by op (the batched Whisper program and every HuBERT program share their model's table).  w2l_scan: set while a watched
    // Wav2Lip call is being enqueued, run_convs scans every layer it launches into it.
    HealthWatch hw_w2l, hw_mt, hw_whisper, hw_hubert, hw_faceparse, hw_facedet;
    HealthWatch* w2l_scan = nullptr;
    // Lock rule.  `mu` owns the enqueue order on compute / aux / aux2 and everything a pass works with: the loaded programs (layers,
    // mt, whisper, vae_enc, their settings), the arena and pointer tables, the prefetch slots / solo_seq / pf_* counters, both graph
    // caches, capture / taps, and an Avatar's d_feat / feat_rec_bytes / feat_epoch; it may be held across HIP calls that wait.
    // `pool_mu` owns the avatar tables + next_avatar, the scratch / stream pools and the tm_* sums.  It is a leaf: never held while
    // `mu` or an egress session's lock is taken (both may be held when it is taken), never held across a HIP call that waits.
    // (Known exception: ltk_avatar_release erases the table's reference under `pool_mu`; when no call holds the bank, its hipFree
    // runs there.)  An egress session's lock (ltk_egress::mu) owns that session's buffers; `mu` is never held when it is taken (the
    // egress entries take `mu` briefly under it, order_behind_pending).
    std::mutex mu;
    std::mutex pool_mu;
    // wav2lip
    bool loaded = false;
    int max_frames = 0;
    int micro_batch = 0;
    std::vector<Layer> layers;
    f16* buf[B_COUNT] = {nullptr};
    // knob PREFETCH: kPfSlots (16 x 0.13 GB at 32 frames) further instances of the eight concat buffers ("slots" 1..kPfSlots; set 0 = buf, where a call that runs
    // the whole network works), sized for alt_frames frames, each holding the prefetched face-encoder outputs of ONE upcoming call,
    // keyed by (avatar, first bank index, frame count): interleaved solo calls of several paced sessions each find their own slot
    // (round 5 kept one engine-wide slot, which only a lone session's calls ever hit).  pf_tmp: the prefetched encoder's own
    // temporaries (prefetches are serialised on aux2).  A call's decoder works in the set its skip tensors were written to.
    struct PfSlot {
        f16* cat[B_COUNT] = {nullptr};
        bool valid = false;               // holds the outputs for (avatar, first, nf) computed under `epoch`
        int avatar = -1, first = -1, nf = 0;
        unsigned epoch = 0;
        unsigned long stamp = 0;          // LRU clock of the last fill / use
        double filled_at = 0;             // host time of the last fill (seconds): a valid slot nobody came for is reclaimed after kPfStale
        hipEvent_t ev_done = nullptr;     // the prefetch into this slot has finished (recorded on aux2)
        hipEvent_t ev_read = nullptr;     // the last pass that worked in this slot has finished (recorded on compute)
        bool filled = false, read = false;
        std::shared_ptr<Avatar> hold;     // the bank a prefetch into this slot reads
    };
    static constexpr int kPfSlots = 16;
    PfSlot pfs[kPfSlots + 1];             // [0] unused
    f16* pf_tmp[B_COUNT] = {nullptr};
    int alt_frames = 0;
    hipStream_t aux2 = nullptr;
    unsigned long pf_clock = 0;
    DevTables* d_tab_next = nullptr;  // faces table of the prefetched frames
    // recent solo calls, per session position: a call that starts where one of them ended (same avatar, same size) continues a session
    struct SoloSeq { int avatar = -1, next = -1, nf = 0; unsigned long stamp = 0; };
    SoloSeq solo_seq[2 * kPfSlots];
    unsigned long pf_hits = 0, pf_misses = 0, pf_issued = 0;
    std::atomic<bool> pf_fail_logged{false};       // a prefetch that could not be launched is reported once (the call itself succeeds)
    // LTK_INFER_TIMING=1 (measurement): host time of ltk_wav2lip_infer by phase, printed when the engine is destroyed
    double tm_prep = 0, tm_launch = 0, tm_pf = 0, tm_wait = 0, tm_prev = 0;      // tm_prev: a deferred call's wait for the pass before it
    // knob DEFER (defer_window.h): the Wav2Lip passes that are enqueued and not yet known to be complete.  Its own (leaf) lock.
    DeferWindow<hipEvent_t> defer;
    std::atomic<unsigned> defer_epoch{0};     // knob_epoch() the newest deferred pass was enqueued under
    unsigned long tm_calls = 0;
    size_t buf_halfs[B_COUNT] = {0};  // per frame
    float* d_head = nullptr;          // 96 weights + 3 bias
    Conv7Plan* c7 = nullptr;          // first layer (7x7, 6 -> 16) with the input pack fused: conv7_mfma.hip
    Audio0Plan* a0 = nullptr;         // audio_encoder.0 (3x3, 1 -> 32) with the mel pack fused (VALU): conv7_mfma.hip, knob AUDIO0 bit 0
    Audio3Plan* a3 = nullptr;         // audio_encoder.3 (3x3 stride (3,1), 32 -> 64), MFMA operands straight from global memory: conv7_mfma.hip, knob AUDIO0 bit 1
    double macs_per_frame = 0;
    DevTables* d_tab = nullptr;       // per-frame pointer tables of the pass being enqueued (misc_kernels.h), filled on the compute stream
    // captured passes (knob GRAPH): one executable graph per launch sequence of the product configuration (bank crops in, fused head
    // out; key: w2l_infer.hip pass_graph_key), prefetch graphs (on aux2) included
    GraphCache<int> graphs;
    unsigned long graph_clock = 0;    // LRU clock of both graph caches
    // captured MuseTalk / Whisper programs (run_program): the static launch list of a program over its persistent buffers, one
    // executable graph per (program, frame count); the kernels that carry per-call pointers stay outside the graph
    GraphCache<std::pair<const void*, int>> prog_graphs;
    // debug capture
    bool capture = false;
    std::map<std::string, std::vector<float>> taps;
    std::map<std::string, std::vector<int>> tap_shape;
    // avatars
    std::map<int, std::shared_ptr<Avatar>> avatars;
    int next_avatar = 1;
    // mel
    float* d_basis = nullptr;
    int32_t* d_lohi = nullptr;
    // musetalk
    MtGraph* mt = nullptr;
    int mt_max_frames = 0;
    int mt_fp8 = 0;                    // ltk_musetalk_set_fp8
    float mt_fp8_ascale = 8.f;
    MtGraph* vae_enc = nullptr;           // AutoencoderKL encoder graph (avatar preparation), 2 images per face
    int vae_enc_faces = 0;
    MtGraph* face_parse = nullptr;        // BiSeNet face parser (avatar preparation: blend masks), face_parse_size^2 images, face_parse_images per run
    int face_parse_size = 0, face_parse_images = 0;
    int face_parse_last = 0;              // images of the run that ran last (debug read-back)
    // S3FD face detector (avatar preparation: face boxes): the packed weights once (face_det_w, never run), and one program per frame
    // size over them (MtGraph::share), built on first use; at most kFaceDetPrograms are kept, the least recently used is dropped
    MtGraph* face_det_w = nullptr;
    struct FaceDetProg { MtGraph* g = nullptr; int H = 0, W = 0; unsigned long stamp = 0; };
    std::vector<FaceDetProg> face_det_progs;
    unsigned long face_det_clock = 0;
    int face_det_images = 0;              // max_images of the load
    MtGraph* face_det_last = nullptr;     // the program that ran last and the images of that run (debug read-back)
    int face_det_last_n = 0;
    MtGraph* whisper = nullptr;           // Whisper-tiny encoder graph (Audio2Feature)
    float* d_wbasis = nullptr;            // slaney mel basis [80][201] (n_fft 400, 0..8000 Hz)
    float* d_wlogspec = nullptr;          // [80][3000]
    float* d_wpcm = nullptr;              // staging, 30 s
    int* d_wgmax = nullptr;
    // ltk_whisper_step_batch: the encoder for kWhisperBatchClips clips over `whisper`'s packed weights, built with its staging on the
    // first batched run (an engine that serves one session never pays for it) and freed with the engine
    MtGraph* whisper_b = nullptr;
    int whisper_b_nf = 0;                 // clips of the batched run that ran last (debug read-back)
    float* d_wbpcm = nullptr;             // [kWhisperBatchClips][480000] samples: clip c at c * 480000
    float* d_wblogspec = nullptr;         // [kWhisperBatchClips][80][3000]
    int* d_wbgmax = nullptr;              // [kWhisperBatchClips] maximum words
    float* d_pe = nullptr;                // PositionalEncoding table [50][384]
    float* d_mt_feat = nullptr;           // staging: fp32 [max_frames][50][384]
    float* d_mt_lat = nullptr;            // staging for the host-input hook: fp32 [max_frames][8][32][32]
    std::map<int, std::shared_ptr<MtAvatar>> mt_avatars;
    // HuBERT-large (Ultralight audio features): the packed weights once (hubert_w, never run), and one program per clip length over
    // them, at most kHubertPrograms, the least recently used dropped (a live session has one length; offline calls add the
    // 320 080-sample clip and a tail)
    MtGraph* hubert_w = nullptr;
    struct HubertProg { MtGraph* g = nullptr; int n_samples = 0; unsigned long stamp = 0; };
    std::vector<HubertProg> hubert_progs;
    MtGraph* hubert_last = nullptr;       // the program that ran last (debug read-back)
    unsigned long hubert_clock = 0;
    float* d_hpcm = nullptr;              // staging: the whole utterance, fp32
    size_t hpcm_cap = 0;                  // samples
    float* d_hstats = nullptr;            // [2] mean, variance, then [1] the residual of the stored mean (hubert_kernels.h)
    float* d_hrows = nullptr;             // staging: fp32 rows of one clip on their way to the host
    size_t hrows_cap = 0;                 // rows
    // ltk_hubert_step_batch: programs for up to kHubertBatchClips clips of one length, a cache of their own (at most
    // kHubertBatchPrograms, least recently used dropped; ltk_hubert_info does not count them), with their own staging
    std::vector<HubertProg> hubert_bprogs;
    MtGraph* hubert_blast = nullptr;      // the batched program that ran last, and how many clips it carried (debug read-back)
    int hubert_blast_nf = 0;
    float* d_hbpcm = nullptr;             // staging: fp32 [nf][n_samples] of one run
    size_t hbpcm_cap = 0;                 // samples
    float* d_hbstats = nullptr;           // [kHubertBatchClips][2] mean, variance per clip, then [kHubertBatchClips] residuals of the means
    // ultralight: per-avatar programs over ONE activation arena of ul_frames frames (grown by a register call that asks for more)
    std::map<int, std::shared_ptr<UlAvatar>> ul_avatars;
    f16* ul_buf[kUlBufs] = {nullptr};
    int ul_frames = 0;
    DevTables* ul_tab = nullptr;          // per-frame bank crop / HuBERT chunk / output pointers of the pass being enqueued
    UlGroupTab* ul_gtab = nullptr;        // per-frame weight records of a grouped pass (ul_gconv.h), uploaded like ul_tab
    size_t ul_frame_bytes = 0;            // arena bytes per frame
    // merged per-avatar passes (ul_pass with `own`): the run lengths of the frames' own-call frame counts -> the number such a pass's
    // captured graph is keyed by (kUlMaxComps of them; a pass of a composition past that runs uncaptured)
    std::map<std::vector<int>, int> ul_comps;
    // pools
    std::vector<Scratch> scratch_free;
    std::vector<hipStream_t> stream_free;
};

namespace ltk {

struct ScratchLease {
    ltk_engine* e;
    Scratch s;
    ScratchLease(ltk_engine* e_, size_t bytes) : e(e_) {
        {
            std::lock_guard<std::mutex> g(e->pool_mu);
            for (size_t i = 0; i < e->scratch_free.size(); ++i)
                if (e->scratch_free[i].cap >= bytes) {
                    s = e->scratch_free[i];
                    e->scratch_free.erase(e->scratch_free.begin() + i);
                    break;
                }
        }
        if (!s.d) {
            size_t cap = bytes < (1u << 20) ? (1u << 20) : bytes;
            if (hipMalloc(&s.d, cap) == hipSuccess) s.cap = cap; else s.d = nullptr;
        }
    }
    ~ScratchLease() {
        if (s.d) {
            std::lock_guard<std::mutex> g(e->pool_mu);
            e->scratch_free.push_back(s);
        }
    }
};

struct StreamLease {
    ltk_engine* e;
    hipStream_t s = nullptr;
    bool owned = false;
    StreamLease(ltk_engine* e_, void* user) : e(e_) {
        if (user) { s = (hipStream_t)user; return; }
        owned = true;
        {
            std::lock_guard<std::mutex> g(e->pool_mu);
            if (!e->stream_free.empty()) { s = e->stream_free.back(); e->stream_free.pop_back(); }
        }
        if (!s) (void)hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    }
    ~StreamLease() {
        if (owned && s) {
            std::lock_guard<std::mutex> g(e->pool_mu);
            e->stream_free.push_back(s);
        }
    }
};

struct DevBuf {                     // device scratch of a host-side hook: freed on every return path
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
};

inline int mirror_index(int size, int index) {  // utils/image.py:26-32
    const int turn = index / size, res = index % size;
    return (turn % 2 == 0) ? res : size - res - 1;
}

template <class Key>
template <class Enq>
int GraphCache<Key>::run(ltk_engine* e, const Key& k, hipStream_t s, const char* what, int nf, Enq enq) {
    if (epoch != knob_epoch()) {           // a knob changed (tests, tuners): the captured launch sequences are stale
        CHK(hipStreamSynchronize(e->compute));
        drop();
        epoch = knob_epoch();
    }
    PassGraph& g = graphs[k];
    g.stamp = ++e->graph_clock;
    g.stream = s;
    if (g.exec) { CHK(hipGraphLaunch(g.exec, s)); return 0; }
    if (g.seen < 0 || g.seen++ == 0) return enq();
    if ((size_t)live() >= kMaxPassGraphs) {          // the table is full: the least recently used graph goes
        PassGraph* victim = nullptr;
        for (auto& kv : graphs)
            if (kv.second.exec && (!victim || kv.second.stamp < victim->stamp)) victim = &kv.second;
        (void)hipStreamSynchronize(e->compute);
        if (victim->stream != e->compute) (void)hipStreamSynchronize(victim->stream);
        (void)hipGraphExecDestroy(victim->exec); victim->exec = nullptr; victim->seen = 1;
    }
    hipGraph_t graph = nullptr;
    if (hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed) != hipSuccess) { (void)hipGetLastError(); g.seen = -1; return enq(); }
    const int rc = enq();
    const hipError_t ce = hipStreamEndCapture(s, &graph);       // always: the stream must leave capture mode
    if (rc) {
        if (ce != hipSuccess) fprintf(stderr, "ltk: capture of the %d-frame %s aborted (%s)\n", nf, what, hipGetErrorString(ce));
        (void)hipGetLastError();
        if (graph) (void)hipGraphDestroy(graph);
        g.seen = -1;
        return rc;
    }
    hipGraphExec_t exec = nullptr;
    hipError_t ie = ce;
    if (ce == hipSuccess && graph) ie = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    if (graph) (void)hipGraphDestroy(graph);
    if (ie != hipSuccess || !exec) {
        // the sequence still runs, launch by launch; say so once per key instead of failing the call
        (void)hipGetLastError();
        g.seen = -1;
        fprintf(stderr, "ltk: hipGraph capture of the %d-frame %s failed (%s); running it as separate launches\n", nf, what, hipGetErrorString(ie));
        return enq();
    }
    g.exec = exec;
    CHK(hipGraphLaunch(exec, s));
    return 0;
}

// ---------------------------------------------------------------- knob DEFER: passes in flight behind a returned call
// Wait (host) for every pass of the window and retire its record.  The compute stream runs them in order, so the newest event covers
// all of them.  Not under e->mu (it waits).  LTK_E_HIP when a pass failed asynchronously: nothing of it is in flight any more, its
// frames are invalid.
inline int drain_pending(ltk_engine* e) {
    const auto recs = e->defer.snapshot();
    if (recs.empty()) return 0;
    const hipError_t se = hipEventSynchronize(recs.back()->ev);
    if (se != hipSuccess) (void)hipStreamSynchronize(e->compute);
    for (const auto& r : recs) e->defer.retire(r);
    if (se != hipSuccess)
        return fail(LTK_E_HIP, std::string("a deferred ltk_wav2lip_infer pass issued by an EARLIER call failed on the device (reported by the call that waited for it): ") +
                                   hipGetErrorString(se));
    return 0;
}
// A reader of [p, p + bytes) on stream `s` (paste-back, egress): `s` waits, on the GPU, for the passes of the window that write there
// (under e->mu, taken only when there is something to wait for: while another thread has a capture open on the compute stream the
// runtime refuses a wait for an event of that stream - "dependency created on uncaptured work in another stream" - and captures run
// under e->mu.  Callers hold no lock but an egress session's, which is never held when e->mu is taken elsewhere.)
inline hipError_t order_behind_pending(ltk_engine* e, hipStream_t s, const void* p, size_t bytes) {
    const auto writers = e->defer.writers_of(p, bytes);
    if (writers.empty()) return hipSuccess;
    std::lock_guard<std::mutex> g(e->mu);
    for (const auto& r : writers) {
        const hipError_t we = hipStreamWaitEvent(s, r->ev, 0);
        if (we != hipSuccess) return we;
    }
    return hipSuccess;
}

// What a call that may be deferred hands to infer_call.  `want`: the caller asked for it; `enq` sets `ok` when the call qualifies (a
// solo call under knob DEFER, w2l_infer.hip) and `slot`; hold / ranges move into the pass's record.
struct DeferCall {
    bool want = false, ok = false;
    int slot = 0;
    std::vector<std::shared_ptr<void>> hold;
    std::vector<PredRange> ranges;
    double wait_prev_us = 0;             // LTK_INFER_TIMING: host time spent waiting for the passes in front
    bool deferred = false;               // out: the call returned with its pass in flight
};

// The call protocol of an inference entry point (include/ltk.h): inputs produced on the caller's stream are waited for on the
// compute stream; `enq` enqueues under e->mu and returns 0 or its error; `done` is recorded inside the lock and the lock released
// BEFORE the wait, so the next call's launches queue up behind this one's kernels instead of behind this thread's wake-up
// (calls of several host threads are serialised for the enqueue only: stream order then keeps them apart on the GPU).  An error
// behind launches drains the compute stream: nothing of the call may still be writing the caller's buffers when it returns.
// The call then waits for `done` - or, deferred (`dc`, knob DEFER), for the passes that were in flight when it enqueued, and leaves
// its own in the window.  A synchronous call's `done` covers those passes too (one stream): it retires them.  On an error return
// nothing is in flight, neither of this call nor of the window.
template <class Enq>
int infer_call(ltk_engine* e, void* stream, Enq enq, DeferCall* dc = nullptr) {
    auto make_ev = [](hipEvent_t* ev) { return hipEventCreateWithFlags(ev, hipEventDisableTiming) == hipSuccess; };
    auto rec = e->defer.acquire(make_ev);
    if (!rec) { (void)hipGetLastError(); (void)drain_pending(e); return fail(LTK_E_HIP, "hipEventCreate failed"); }
    int rc = 0;
    bool launched = false, stream_wait_failed = false;
    std::vector<decltype(rec)> before;
    {
        std::lock_guard<std::mutex> g(e->mu);
        if (stream) {  // inputs were produced on the caller's stream
            Ev ready;
            hipError_t he = ready.create();
            if (he == hipSuccess) he = hipEventRecord(ready.e, (hipStream_t)stream);
            if (he == hipSuccess) he = hipStreamWaitEvent(e->compute, ready.e, 0);
            if (he != hipSuccess) rc = fail(LTK_E_HIP, std::string("waiting for the caller's stream: ") + hipGetErrorString(he));
        }
        if (!rc) {
            launched = true;
            rc = enq();
            if (!rc && hipEventRecord(rec->ev, e->compute) != hipSuccess) rc = fail(LTK_E_HIP, "hipEventRecord failed");
        }
        if (!rc && dc && dc->want && dc->ok) {
            rec->hold = std::move(dc->hold);
            rec->ranges = std::move(dc->ranges);
            rec->slot = dc->slot;
            before = e->defer.push(rec);
            dc->deferred = true;
            // the caller's stream sees the inputs free again behind the pass (under the lock: the runtime refuses a wait for an event of
            // the compute stream while another thread has a capture open on it, and captures run under the lock)
            if (stream && hipStreamWaitEvent((hipStream_t)stream, rec->ev, 0) != hipSuccess) stream_wait_failed = true;
        } else if (!rc) {
            before = e->defer.snapshot();
        }
    }
    if (rc) {
        const std::string msg = g_err;                 // (the drain below may set its own text: this call's error is the one reported)
        if (launched) (void)hipStreamSynchronize(e->compute);
        (void)drain_pending(e);
        e->defer.give_back(rec);
        return fail(rc, msg);
    }
    if (dc && dc->deferred) {
        if (stream_wait_failed) rc = fail(LTK_E_HIP, "hipStreamWaitEvent failed");
        if (!rc && !before.empty()) {
            const auto t0 = std::chrono::steady_clock::now();
            const hipError_t se = hipEventSynchronize(before.back()->ev);
            dc->wait_prev_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
            if (se != hipSuccess)
                rc = fail(LTK_E_HIP, std::string("the deferred pass of the PREVIOUS ltk_wav2lip_infer_deferred call failed on the device (reported by this call, which "
                                                 "waited for it; the frames of both calls are invalid): ") + hipGetErrorString(se));
        }
        if (rc) {                                       // both calls' frames are invalid, nothing stays in flight
            const std::string msg = g_err;
            (void)hipStreamSynchronize(e->compute);
            for (const auto& r : before) e->defer.retire(r);
            e->defer.retire(rec);
            dc->deferred = false;
            return fail(rc, msg);
        }
        for (const auto& r : before) e->defer.retire(r);
        e->defer.returned();
        return 0;
    }
    if (stream && hipStreamWaitEvent((hipStream_t)stream, rec->ev, 0) != hipSuccess) rc = fail(LTK_E_HIP, "hipStreamWaitEvent failed");
    if (hipEventSynchronize(rec->ev) != hipSuccess) {
        rc = fail(LTK_E_HIP, before.empty() ? "hipEventSynchronize failed"
                                            : "hipEventSynchronize failed (this call, or the deferred pass of an earlier call it ran behind: the frames of both are invalid)");
        (void)hipStreamSynchronize(e->compute);
    }
    for (const auto& r : before) e->defer.retire(r);
    e->defer.give_back(rec);
    return rc;
}

// An avatar id's bank, held for the duration of the caller's work (null: no such id).  The banks' fields are set before
// registration publishes them and never change afterwards, so they are read without a lock through the held pointer.
inline std::shared_ptr<Avatar> find_avatar(ltk_engine* e, int id) {
    std::lock_guard<std::mutex> g(e->pool_mu);
    auto it = e->avatars.find(id);
    return it == e->avatars.end() ? nullptr : it->second;
}
inline std::shared_ptr<MtAvatar> find_mt_avatar(ltk_engine* e, int id) {
    std::lock_guard<std::mutex> g(e->pool_mu);
    auto it = e->mt_avatars.find(id);
    return it == e->mt_avatars.end() ? nullptr : it->second;
}

inline std::shared_ptr<UlAvatar> find_ul_avatar(ltk_engine* e, int id) {
    std::lock_guard<std::mutex> g(e->pool_mu);
    auto it = e->ul_avatars.find(id);
    return it == e->ul_avatars.end() ? nullptr : it->second;
}
// the launch_ul_paste_batch argument of bank frames idx[0..m) (m <= kPasteBatch, every index checked by the caller)
inline void ul_fill_paste_batch(const UlAvatar& a, const int32_t* idx, int m, UlPasteBatch* pb) {
    const size_t bytes = (size_t)a.H * a.W * 3;
    for (int i = 0; i < m; ++i) {
        const int32_t* c = a.boxes.data() + 4 * (size_t)idx[i];
        pb->full[i] = a.d_full + (size_t)idx[i] * bytes;
        pb->face[i] = a.d_face + (size_t)idx[i] * kUlFace * kUlFace * 3;
        pb->x1[i] = c[0]; pb->y1[i] = c[1]; pb->x2[i] = c[2]; pb->y2[i] = c[3];
    }
}

// ---------------------------------------------------------------- what crosses the engine's sources
void build_mel_basis(std::vector<float>* basis, std::vector<int32_t>* lohi, int n_bins = 401, double f_lo = 55.0, double f_hi = 7600.0);   // engine.hip
int build_program(ltk_engine* e, const ltk_named_tensor* sd, int n);                                        // w2l_program.hip
void wav2lip_unload(ltk_engine* e);
int run_convs(ltk_engine* e, int nf, hipStream_t s, const OutPtrs* head_outs = nullptr, std::vector<hipEvent_t>* evs = nullptr,
              const FacePtrs* faces = nullptr, int part = 0, int par = 0, bool pf_enc = false);
int launch_pass(ltk_engine* e, int nf, hipStream_t s, bool bank_faces, const float* d_face6, bool have_outs, float* d_pred_f32,      // w2l_infer.hip
                bool cached = false, int par = 0, bool have_feats = false);
int launch_prefetch(ltk_engine* e, int nf, int slot);
int run_program(ltk_engine* e, MtGraph* prog, int nf);                                                      // mt_engine.hip
// ultralight.hip.  ul_pass: one pass over frames [0, nf) of the arena, the per-frame tables already in e->ul_tab, under e->mu.
// The defaults are the product configuration, which replays from e->prog_graphs.
struct UlPassArgs {
    const float* d_img6 = nullptr;          // source: null = the uint8 bank crops of the faces table; else (test hook) float32 NCHW input
    float* d_pred_f32 = nullptr;            // sink: null = the frame destinations of the outs table; else (test hook) float32 NCHW sigmoid output
    const UlGroupTab* gtab = nullptr;       // a grouped pass: every frame's operands through this table (set by ultralight.hip alone)
    // own[i] = the frame count of the pass that would carry frame i if its request came alone.  Every conv then sums a frame's channels
    // in the order that pass would (conv3's split-K factor follows a launch's frame count), so a frame's bytes do not depend on which
    // requests share its pass; nullptr or all == nf: the plain pass.
    const std::vector<int>* own = nullptr;
    // a watched call's per-avatar pass (ltk_health_watch): eagerly, every op's output scanned into the record of its index in the
    // architecture table; a grouped pass has no avatar and is never watched
    HealthWatch* health = nullptr;
};
int ul_pass(ltk_engine* e, const UlAvatar& a, int nf, UlPassArgs args = UlPassArgs());
double ul_macs_per_frame();
void ul_drop_graphs(ltk_engine* e, int avatar_id);     // under e->mu: the captured passes of a released avatar
// the listing as knob UL_FUSE_IR stands (ltk_ultralight_op_name) with, per entry, its index in the architecture table = its record in
// an avatar's HealthWatch
void ul_health_listing(std::vector<std::string>* names, std::vector<int>* types, std::vector<int>* arch_index);
// ltk_ultralight_infer_merged's call plan (ultralight.hip ul_merge_plan; seen through ltk_debug_ul_merge_plan): which frames of which
// request share a pass.  A span = frames [first, first + count) of request `req` at frames [at, at + count) of the pass.
enum { UL_PATH_PER_AVATAR = 0, UL_PATH_GROUPED = 1 };
struct UlMergeSpan { int req, first, count, at; };
struct UlMergePass {
    int path;                          // UL_PATH_*
    int avatar;                        // the pass's avatar id; -1 on the grouped path
    int nf;                            // <= cap
    std::vector<UlMergeSpan> spans;
};
// mode 0: the rule (one avatar: per-avatar passes over the union of its requests; several: grouped passes over all frames when
// `grouped_knob` and `grouped_ok`, else per avatar in order of first appearance); 1 / 2 force the per-avatar / grouped form.
// 0, or -1 with *err set.
int ul_merge_plan(const int* avatar, const int* batch, int nreq, int cap, int mode, bool grouped_ok, bool grouped_knob,
                  std::vector<UlMergePass>* out, std::string* err);
void ul_unload(ltk_engine* e);                         // engine teardown
constexpr size_t kHubertPrograms = 3;
constexpr size_t kHubertBatchPrograms = 2;
MtGraph* hubert_program(ltk_engine* e, int n_samples, int* rc);                                             // mt_engine.hip, under e->mu
void hubert_unload(ltk_engine* e);
void drop_program_graphs(ltk_engine* e, const MtGraph* old);                                                // mt_engine.hip, under e->mu
constexpr size_t kFaceDetPrograms = 2;
MtGraph* face_det_program(ltk_engine* e, int H, int W, int* rc);                                            // mt_engine.hip, under e->mu
void face_det_unload(ltk_engine* e);
int mt_run_locked(ltk_engine* e, const float* d_feat, const PtrList64* feat_ptrs, int nf, const OutList64* outs, float* d_image_f32);

}  // namespace ltk

// Tuning / A-B knobs of the engine.  Every knob is an integer read from the environment ONCE per process (first use,
// normally ltk_engine_create) and kept in a table; the launch path reads the table, never getenv.  Sweep scripts and
// tests change a knob in-process through ltk_debug_set_knob (include/ltk.h).
#pragma once

namespace ltk {

// THE knob list: X(NAME, default) makes enumerator K_NAME (below) and environment variable LTK_NAME with its default (tune.hip).
// One line per knob; the longer notes sit under the list, by name.
#define LTK_KNOBS(X) \
    X(CONV_V3, 1)              /* 1: conv3 (LDS-DMA) kernels where they apply */ \
    X(CONV_PXW, 0)             /* conv3 sweeps: force the tile width (1 / 2 / 4 = 128 / 256 / 512 pixels); 0 = rule */ \
    X(CONV3_NBT, 0)            /* conv3 sweeps: force 32-cout subtiles per block (1, 2, 4); 0 = rule */ \
    X(CONV3_NC8, 0)            /* conv3 3x3 sweeps, read when a plan is BUILT: channel planes per chunk (2 = 16 channels, 4 = 32); 0 = rule (16 channels) */ \
    X(SPLITK, 1)               /* 0: never split the channel loop (batch-size independent summation order) */ \
    X(KSPLIT, 0)               /* conv3 sweeps: force this split factor; 0 = rule */ \
    X(MICROBATCH, 0)           /* wav2lip frames per arena pass (0 = min(max_frames, 256)) */ \
    X(HEAD_FUSED, 1)           /* 1: output_block conv 80->32 + 1x1 head + sigmoid in one launch */ \
    X(TILE_TABLE, 1)           /* 1: use the engine's per-layer measured tile table where it has an entry */ \
    X(ROWGEMM, 1)              /* 1: the one-pixel-map layers of a <= 32-frame launch as skinny GEMMs (rowgemm.hip) instead of conv3 + split-K finish */ \
    X(ROWCONV, 1024)           /* 3x3 layers on the 4x4 / 8x8 maps as weight-streaming GEMMs over gathered rows (rowgemm.hip) in launches of at most this many output pixels; 0 = never */ \
    X(ABLATE, 0)               /* measurement builds only (make ABLATE=1): bit mask, see conv3_mfma.hip */ \
    X(GRAPH, 1)                /* non-zero: a Wav2Lip pass of a given frame count is captured once as a hipGraph and replayed; 0: launch by launch */ \
    X(DF_FRAMES, 0)            /* > 0: decoder blocks >= DF_BLOCK and the output conv run depth-first over sub-batches of this many frames; 0 = layer by layer */ \
    X(DF_BLOCK, 6)             /* first decoder block of the depth-first region (6: the 128^2 and 256^2 levels) */ \
    X(DF_MIN, 32)              /* depth-first only for launches of at least this many frames */ \
    X(FACE_CACHE, 0)           /* 1 (opt-in deployment mode): the face encoder's skip tensors are computed once per avatar and copied into the concat buffers */ \
    X(PREFETCH, 1)             /* 1: a session's consecutive single-request calls are software-pipelined across calls; 0: every call runs the whole pass */ \
    X(MT_FUSE, 7)              /* MuseTalk program, read at BUILD: bit 0 GEGLU epilogue, bit 1 stacked cross-attention k | v, bit 2 LayerNorm fold (needs bit 1); 0 = rounds 2-5 */ \
    X(MT_GN1, 1)               /* 1: GroupNorm of maps whose (image, group) fits one block's registers as ONE launch (gn_group_kernel) instead of gn_stats + gn_apply */ \
    X(FACE_CACHE_MAX_MB, 16384) /* largest face cache ONE avatar may take under FACE_CACHE (16384 MB = a 3 900-frame bank); longer avatars fail with LTK_E_NOMEM */ \
    X(LIN_FK, 1)               /* 1: 1x1 / linear layers with K = 320 / 384 / 512 / 640 / 1280 on >= kLinFkMinRows rows run on lin_fk_kernel; 0: conv3 1x1 */ \
    X(ATTN_LDS, 1)             /* 1: self-attention with head dims 40 / 80 over >= 128 keys shares its K / V^T tiles through LDS (attn_lds_kernel); 0: attn_kernel */ \
    X(LIN_MP, 1)               /* 1: 1x1 / linear layers with K = 2560 / 5120 on lin_mp_kernel where its grid is one round of blocks; 2 / 3: always, that many slabs; 0: conv3 / rowconv */ \
    X(GN_COOP, 1)              /* 1: GroupNorm of the maps too large for MT_GN1 in ONE tensor pass (gn_coop_kernel); 0: gn_stats + gn_apply */ \
    X(AUDIO0, 3)               /* bit 0: audio_encoder.0 as a VALU kernel reading the float32 mel windows (audio0_kernel); bit 1: audio_encoder.3 on audio3_kernel; 0: pack_mel + conv_mfma_kernel */ \
    X(CONV_S2D, 1)             /* 1: face_encoder_blocks.1.0 / 2.0 (shallow stride-2 layers) on convs2d_kernel; 0: conv_mfma_kernel (first generation) */ \
    X(DEFER, 1)                /* 1: a solo ltk_wav2lip_infer_deferred call returns with its pass in flight, once the pass before it is complete; 0: every call waits for its own */ \
    X(UL_GROUPED, 0)           /* 1: an ltk_ultralight_infer_merged call that carries several avatars runs ONE launch sequence over all its frames on the grouped kernels (per-image weights, ul_gconv.hip); 0: one merged sequence per avatar */ \
    X(UL_FUSE_IR, 0)           /* 1 (opt-in): a per-avatar Ultralight pass runs each inverted residual on a map of >= 32 x 32 pixels as ONE launch (ul_ir_kernel, hidden tile in LDS) instead of expand + depthwise + project; read at enqueue */

// Notes.
// GRAPH       the per-call pointer tables live in device memory, filled by one small launch in front of the graph.
// DF_FRAMES   producer -> consumer tensors of the depth-first region stay in the 256 MiB Infinity Cache.
// FACE_CACHE  the eight skip tensors depend on the BANK frame only (wav2lip_v2.py:132-140): 4.15 MB of fp16 per bank frame, resident in
//             HBM; a pass copies them instead of running conv7 + 20 encoder layers.
// PREFETCH    calls whose index advances by their batch size (<= 32 frames): while call N runs its audio encoder + decoder, the face
//             encoder of the frames call N+1 will ask for (bank frames index+B ..) runs beside it on a third stream into the other set
//             of concat buffers; call N+1 then starts at the decoder.  Every layer still runs once per frame and step; a call that does
//             not continue the sequence runs the whole pass (as rounds 1-4 did for every call).
// MT_FUSE     weights are packed for it.  Bit 0: GEGLU in the epilogue of ff.net.0.proj (no 8C-wide intermediate, no geglu launch);
//             bit 1: the k | v projections of the 16 cross-attentions (they read the audio context only) as ONE stacked projection +
//             ONE value-transpose launch at the head of the pass; bit 2: the transformer blocks' LayerNorms folded into the linear
//             layers around them.
// MT_GN1      the U-Net levels and the VAE's 32^2 maps (nn_kernels.hip).
// LIN_FK      conv3_mfma.hip: a wave's A rows in registers, full-K 32-cout weight slabs through LDS.
// ATTN_LDS    the four query tiles of a block share whole 64-key tiles (nn_kernels.hip); under 0 every wave reads them from L2.
// LIN_MP      conv3_mfma.hip: passes of 1280 channels, the accumulators of 2 or 3 weight slabs per block in registers
//             (conv3_lin_mp_nsl).
// GN_COOP     the VAE's 64^2 .. 256^2 maps: blocks keep their slice in registers and exchange partial sums through global memory.
// AUDIO0      conv7_mfma.hip.  Bit 0: 1 -> 32 channels on the 80 x 16 mel window, no pack_mel launch, no 8-channel padded MFMA launch;
//             bit 1: the stride-(3, 1) layer on MFMAs fed straight from global memory.
// CONV_S2D    16 -> 32 @256^2, 32 -> 64 @128^2 (conv7_mfma.hip): a wave = one output row x 32 output channels, weights in registers,
//             pixel operands straight from global memory, no LDS.
// UL_GROUPED  mode 0 of ltk_ultralight_infer_merged only (modes 1 / 2 force a form); the default follows profiles/ultralight_merge.txt.
// UL_FUSE_IR  csrc/ul_ir.hip: 13 of the 26 blocks, 60 launches per pass instead of 86; the weights are packed for it at register time whatever
//             the knob says, so it can change at run time (captured passes are keyed by knob_epoch()).  The grouped path (UL_GROUPED,
//             mode 2) ignores it.  The fused op has one summation order at every frame count: one launch over all frames of a merged pass.
//             ltk_ultralight_op_name lists a fused block once (type 15) under its project conv's name, and ltk_debug_capture taps only that
//             output: the .conv.0 / .conv.3 tensors do not exist in a fused pass.  Default 0 until a follow-up meets the rule in
//             profiles/ultralight_fuse_ir.txt.
// DEFER       engine_internal.h infer_call / defer_window.h: a lone session's host turn-around (completion wake-up, Python, the next
//             call's launches: 40-55 us of a 1.2-ms step) then runs under the pass in flight instead of between two passes.

enum Knob {
#define LTK_KNOB_ENUM(name, dflt) K_##name,
    LTK_KNOBS(LTK_KNOB_ENUM)
#undef LTK_KNOB_ENUM
    K_COUNT
};

int knob(Knob k);
// bumped by every knob_set: cached launch plans (captured graphs) are keyed by it
unsigned knob_epoch();
// hipFuncAttributeMaxDynamicSharedMemorySize = `bytes` for `func` on the CURRENT device, once per (device, function) and process
// (a launch path may run on any host thread, also inside a stream capture: the attribute is set by the first eager pass).
// Returns the hipError_t of the attribute call (0 = ok).
int ensure_dyn_lds(const void* func, int bytes);

// returns 0, or -1 when `name` (without the LTK_ prefix or with it) is not a knob
int knob_set(const char* name, int value);

}  // namespace ltk

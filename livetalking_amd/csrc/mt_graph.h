// The program layer the model builders share (musetalk.hip, whisper.hip, hubert.hip; executed by mt_graph.hip): the state-dict reader,
// tensors, ops and the graph itself.  Internal like engine_internal.h: not installed, not part of the ABI; the engine's sources see
// the opaque handle and the mt_* wrappers of musetalk.h only.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "musetalk.h"
#include "state_dict.h"

namespace ltk {

inline int up16(int c) { return (c + 15) / 16 * 16; }

struct MtTensor {
    int buf = -1;
    int C = 0;        // channels of this view (multiple of 16)
    int ld = 0;       // channels of the underlying buffer
    int coff = 0;     // first channel of the view
    int H = 1, W = 1;
    bool q8 = false;  // e4m3 bytes, [N][C/32][P][32]: C, ld, coff count real channels (multiples of 32), one byte each
    int P() const { return H * W; }
};

// (OP_FP_*: the face parser's own ops, parse_kernels.h; their listing types are faceparse.h FpOp::type, MtOp::fp_type)
enum MtOpType { OP_CONV, OP_GN, OP_LN, OP_ATTN, OP_GEGLU, OP_ADDPOS, OP_VT, OP_HB_L0, OP_LNGELU, OP_POSCONV,
                OP_FP_STEM, OP_FP_MAXPOOL, OP_FP_GAP, OP_FP_GATE, OP_FP_LABELS,
                // the face detector's own ops (s3fd_kernels.h; listing types: facedet.h FdOp::type, carried in MtOp::fp_type)
                OP_FD_STEM, OP_FD_POOL, OP_FD_L2NORM, OP_FD_DETECT };

struct MtOp {
    MtOpType type;
    std::string name;
    MtTensor x, y, r, k, v;     // r: residual; attention: x = q, k, v
    int plan = -1;
    int rplan = -1;             // index into MtGraph::rplans: the same layer as a weight-streaming GEMM over gathered rows (rowgemm.hip rowconv)
    int ksz = 1;                // its kernel size (1 or 3)
    bool unet3x3 = false;       // 3x3 stride-1 fp16 conv of the U-Net (maps of <= 32 x 32): measured per-level tile choice (mt_graph_run)
    int act = 0, ups = 0;
    int gamma = -1, beta = -1;  // indices into MtGraph::vecs
    int groups = 32, silu = 0;
    float eps = 1e-5f;
    int heads = 1, d16 = 0;
    int Tk = 0;
    // LayerNorm fold (MT_FUSE bit 2; conv3_mfma.hip K3Args::ln_*): ln_out_buf = this linear layer also writes its output's per-token
    // partial sums there; ln_in_buf = it consumes a LayerNorm'ed tensor but reads the raw one, statistics from that buffer
    int ln_out_buf = -1, ln_in_buf = -1, ln_in_tiles = 0;
    float ln_eps = 1e-5f;
    int vt_buf = -1;            // OP_ATTN: the values are already transposed in this buffer (written by the pass's OP_VT), else the shared scratch
    long long gn_slot_off = -1; // OP_GN on a map gn_coop_kernel serves: first word of this op's exchange slots in MtGraph::gn_slots
    int wvec = -1, bvec = -1;   // OP_HB_L0 / OP_POSCONV (hubert_kernels.hip): the op's own weights and bias in MtGraph::vecs
    // face parser (mt_build_face_parse_graph): OP_FP_GATE's pre-sigmoid attention `ga` and added per-channel value `gb` (dense 1 x 1 maps;
    // the added map is `r`) and its feat * atten + feat form; OP_FP_STEM: wvec = the packed weight image, gamma / beta = scale / shift
    MtTensor ga, gb;
    int plus1 = 0;
    int fp_type = -1;           // the listing type of a face-parser op (0 conv, 10 stem ... 14 labels) or face-detector op (0, 20 ... 23); -1: neither
    // face detector (mt_build_face_detect_graph): OP_FD_STEM: wvec = the packed weight image, beta = the bias; OP_FD_L2NORM: gamma = the
    // weight; OP_FD_DETECT: the level and its max-out
    int fd_level = -1, fd_maxout = 0;
    // OP_CONV, set by a builder whose outputs must not depend on the images beside an image (mt_build_face_detect_graph): every image
    // takes the split-K factor of its own one-image launch (mt_run_op_body)
    bool own_split = false;
};

// one cross-attention's share of the hoisted k | v projection (MtGraph::kv_all): its value view and where the transposed values go
struct MtVtItem { MtTensor v; int heads, d16, Tk, vt_buf; };

struct MtGraph {
    std::vector<size_t> buf_halfs;           // per frame
    std::vector<f16*> bufs;
    std::vector<ConvPlan> plans;
    std::vector<RowGemmPlan> rplans;         // small-map layers (<= 64 pixels / tokens per frame) also as rowconv plans (add_conv2)
    std::vector<float*> vecs;                // device fp32 vectors (norm affine)
    std::vector<MtOp> ops;
    std::map<std::string, MtTensor> named;
    float* gn_partial = nullptr;
    size_t gn_partial_floats = 0;
    unsigned* gn_slots = nullptr;            // gn_coop_kernel's exchange slots of every GroupNorm op it serves (reset to the sentinel at the head of a pass)
    size_t gn_slot_words = 0;
    unsigned* gn_err_host = nullptr;         // host-mapped word a block sets when its wait for its set ran out; gn_err_dev = the device's view of it
    unsigned* gn_err_dev = nullptr;
    f16* vt = nullptr;                        // transposed values scratch
    size_t vt_halfs = 0;                      // per frame
    struct KvPre { MtTensor k, v; int vt_buf; };
    std::map<std::string, KvPre> kv_pre;      // cross-attention name -> its views of the hoisted projection
    std::vector<MtVtItem> vt_items;           // OP_VT: every cross-attention's values, transposed by ONE launch at the head of the pass
    int frames = 0;
    // fp8 conv path (BASELINE configs[4]): the GroupNorm+SiLU in front of every ResnetBlock2D 3x3 conv writes e4m3
    // (x * fp8_ascale, saturating) and the conv runs on fp8 operands; everything else stays fp16
    bool fp8 = false;
    float fp8_ascale = 8.f;
    double macs = 0;                          // conv / linear MACs per frame (attention excluded)
    double macs_fp8 = 0;                      // ... of which on fp8 operands
    std::string err;
    HealthRec* health = nullptr;              // a watched call's run (mt_set_health): op i's output is scanned into health[i]
    unsigned char* health_obs = nullptr;      // ... and health_obs[i] set
    MtTensor *t_latent = nullptr, *t_ctx = nullptr, *t_unet_out = nullptr, *t_vae_out = nullptr;
    MtTensor* whisper_states = nullptr;
    // HuBERT (mt_build_hubert): one program per clip length over ONE set of packed weights.  `share` = the graph that owns them (it
    // is built once per engine and never run); a graph with `share` set looks its plans and vectors up there by name, copies the
    // handles and frees none of them.  plan_of / rplan_of / vec_of: what the owner offers.
    const MtGraph* share = nullptr;
    std::map<std::string, int> plan_of, rplan_of, vec_of;
    int hb_layers = 0, hb_samples = 0, hb_rows = 0;
    int hb_pcm_buf = -1;                      // fp32 [hb_samples]: the normalised waveform of the clip
    MtTensor* hb_out = nullptr;               // last_hidden_state
    // face parser (mt_build_face_parse_graph): the two byte buffers of the program, typed side buffers as hb_pcm_buf is
    int fp_img_buf = -1;                      // uint8 [frames][fp_size][fp_size][3]: the RGB images
    int fp_label_buf = -1;                    // uint8 [frames][fp_size][fp_size]: the labels
    int fp_size = 0;
    // face detector (mt_build_face_detect_graph): the byte buffer of the frames, and the candidate buffer all six detect ops append to:
    // [256-byte head: uint32 counters [frames] at 0, the threshold (float) at kFdThreshAt][frames][fd_cap][6 words]
    int fd_img_buf = -1;                      // uint8 [frames][fd_H][fd_W][3]: the BGR frames
    int fd_rec_buf = -1;
    int fd_H = 0, fd_W = 0, fd_cap = 0;
    float fd_thresh = __builtin_nanf("");     // what the device's threshold word holds (NaN: never written)
    bool no_rowgemm = false;                  // builder setting: add_conv plans no row-GEMM form beside conv3's (mt_build_face_parse_graph)

    MtTensor alloc(int C, int H, int W);
    MtTensor alloc_q8(int C, int H, int W);          // C % 32 == 0
    static MtTensor view(const MtTensor& b, int coff, int C);
    int add_vec(const float* host, int n, int pad_to = 0);
    // a vector the programs of one model share under `name` (host = null in a graph with `share` set)
    int add_named_vec(const std::string& name, const void* host, size_t bytes);
    // conv / linear: weight [Cout][Cin][k][k] fp32 host, bias [Cout] or null
    // `scale` (or null = 1): per-output-channel factor of the epilogue (the LayerNorm fold passes sum_ci W'[co][ci] here)
    int add_conv(const std::string& name, const float* w, const float* bias, int Cin, int Cout, int k, int stride, int pad,
                 const MtTensor& x, const MtTensor& y, const MtTensor* res, int act, int ups, const float* scale = nullptr);
    // per-token partial statistics of a C-channel tensor on an H x W map: [tokens][C / 32] float2 (LayerNorm fold)
    int alloc_ln_stats(int C, int H, int W);
    // diffusers Downsample2D(padding=0): F.pad(x, (0,1,0,1)) + Conv2d(k3, s2, p0)  (AutoencoderKL encoder)
    int add_conv_down_asym(const std::string& name, const float* w, const float* bias, int C, const MtTensor& x, const MtTensor& y);
    // rectangular kernel / stride (Conv1d over a [T][1] token map: kh x 1)
    int add_conv2(const std::string& name, const float* w, const float* bias, int Cin, int Cout, int kh, int kw, int sh, int sw,
                  int ph, int pw, const MtTensor& x, const MtTensor& y, const MtTensor* res, int act, int ups, int pad_br = 0,
                  const float* scale = nullptr);
    // add_conv2 over the packed weights of `share`: the plan handles are copied, the row-GEMM form taken where this graph's map
    // is small enough for it (the owner was built at a length that has one for every linear layer)
    int add_conv_shared(const std::string& name, int Cin, int Cout, int kh, int kw, int stride, const MtTensor& x, const MtTensor& y,
                        const MtTensor* res, int act);
    int add_gn(const std::string& name, SD& sd, const std::string& prefix, const MtTensor& x, const MtTensor& y, float eps, int silu);
    int add_ln(const std::string& name, SD& sd, const std::string& prefix, const MtTensor& x, const MtTensor& y, float eps);
    // `vt_buf` >= 0: the values were transposed into that buffer by the pass's OP_VT (hoisted cross-attention k | v, mt_build_unet)
    void add_attn(const std::string& name, const MtTensor& q, const MtTensor& k, const MtTensor& v, const MtTensor& o, int heads, int d16,
                  int vt_buf = -1);
    void add_geglu(const std::string& name, const MtTensor& x, const MtTensor& y);
};

int mt_graph_alloc(MtGraph& g, int frames);
void mt_graph_free(MtGraph& g);
// `evs` (measurement): one event in front of every op and one behind the last
int mt_graph_run(MtGraph& g, int nf, float* partial, size_t partial_cap, hipStream_t s, int op_begin, int op_end,
                 std::vector<hipEvent_t>* evs = nullptr);

}  // namespace ltk

// The device programs over MtGraph as the engine's sources see them: the opaque handle, execution (mt_graph.hip) and graph construction
// from a model's state dict (musetalk.hip: U-Net + VAE; whisper.hip; hubert.hip).  The graph itself is mt_graph.h.
#pragma once
#include <vector>
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ltk.h"
#include "conv_mfma.h"

namespace ltk {

struct MtGraph;
struct MtTensor;

MtGraph* mt_graph_new();
void mt_graph_delete(MtGraph* g);
const char* mt_graph_error(const MtGraph* g);
// after the pass's stream has been synchronised: 1 (and mt_graph_error says so) if a cooperative GroupNorm block's wait ran out during it
int mt_gn_error(MtGraph* g);
// before mt_build: run the ResnetBlock2D 3x3 convs on fp8 (e4m3) operands; act_scale = what GroupNorm+SiLU outputs are
// multiplied by before the saturating conversion (<= 0 keeps the default 8)
void mt_set_fp8(MtGraph* g, int on, float act_scale);
double mt_macs_fp8_per_frame(const MtGraph* g);
// ltk_health_watch: while `recs` is set (one record per op, misc_kernels.h HealthRec), every run scans each op's output into its
// record, one launch behind the op on its stream, and marks it in observed[op]; null (the default) launches nothing.  The engine sets
// it for a watched call's runs only and runs those outside the graph cache (run_program).
struct HealthRec;
void mt_set_health(MtGraph* g, HealthRec* recs, unsigned char* observed);
bool mt_health_on(const MtGraph* g);
// the output view of the op named `name` (null: no such op, or it has no output tensor): the buffer, and the view's geometry
const void* mt_op_out(MtGraph* g, const char* name, int* C, int* ld, int* coff, int* P, int* q8);
int mt_op_out_q8(MtGraph* g, int i);           // 1: op i writes an e4m3 tensor (fp8 conv path), 0: fp16 (or nothing)
// builds U-Net then VAE decoder; returns 0 or a negative code
int mt_build(MtGraph* g, const ltk_named_tensor* unet_sd, int n_unet, const ltk_named_tensor* vae_sd, int n_vae, int frames);
// tensors the engine feeds / reads
f16* mt_latent_in(MtGraph* g, int* cbt);       // [N][1][1024][16] (8 real channels)
f16* mt_ctx_in(MtGraph* g, int* cbt);          // [N][24][50][16]
f16* mt_unet_out(MtGraph* g, int* cbt);        // [N][1][1024][16] (4 real channels)
f16* mt_vae_out(MtGraph* g, int* cbt);         // [N][1][65536][16] (3 real channels, RGB)
int mt_run(MtGraph* g, int nf, float* partial, size_t partial_cap, hipStream_t s);
// per-op view (profiling): ops in execution order; type 0 conv/linear, 1 GroupNorm, 2 LayerNorm, 3 attention, 4 GEGLU, 5 add-pos, 6 value transpose (hoisted cross-attention values)
int mt_op_count(MtGraph* g);
const char* mt_op_name(MtGraph* g, int i, int* type);
// ops [0, op_end) only, eagerly (ltk_face_detect_debug_get: a program whose ops share buffers is run again up to the op that is read)
int mt_run_head(MtGraph* g, int nf, float* partial, size_t partial_cap, hipStream_t s, int op_end);
int mt_run_timed(MtGraph* g, int nf, float* partial, size_t partial_cap, hipStream_t s, std::vector<hipEvent_t>* evs);
// named intermediate (debug / parity): returns device pointer + geometry, or null
f16* mt_named(MtGraph* g, const char* name, int* C, int* ld, int* coff, int* H, int* W);
double mt_macs_per_frame(const MtGraph* g);
// VAE encoder graph (avatar preparation): image input = mt_latent_in() ([N][1][65536][16], RGB in [-1,1]),
// moments (mean | logvar, 8 channels at 32x32) = mt_unet_out()
int mt_build_vae_encoder_graph(MtGraph* g, const ltk_named_tensor* vae_sd, int n, int frames);
// BiSeNet face parser (avatar preparation: blend masks) at one square image size for up to max_images images per run: the launch list
// of faceparse.h fp_program over the buffers and views of fp_plan.  sd: BiSeNet.state_dict(); the unused heads and counters are not
// read.  Input: uint8 RGB [n][size][size][3] in mt_face_parse_image_in(); output: uint8 labels [n][size][size] in mt_face_parse_labels().
// 0, -1 (refused: the text in mt_graph_error) or -4 (allocation).
int mt_build_face_parse_graph(MtGraph* g, const ltk_named_tensor* sd, int n, int size, int max_images);
uint8_t* mt_face_parse_image_in(MtGraph* g);
const uint8_t* mt_face_parse_labels(MtGraph* g);
// S3FD face detector (avatar preparation: face boxes): the launch list of facedet.h fd_program over the buffers and views of fd_plan.
// The packed weights live in ONE graph that is never run (share = null, sd = s3fd().state_dict(): built at 32 x 32 with no activations
// when `allocate` is false); a program for H x W frames, up to max_images per run, is built over it (share = that graph, sd unused) and
// owns its activations and op list only - the same ops in the same order, so every program scans into the model's one health table.
// Input: uint8 BGR [n][H][W][3] in mt_face_detect_image_in(); output: mt_face_detect_records(), the candidate buffer of
// s3fd_kernels.h (head with counters and threshold, kFdDevCap records per image).  0, -1 (refused: mt_graph_error) or -4 (allocation).
int mt_build_face_detect_graph(MtGraph* g, const MtGraph* share, const ltk_named_tensor* sd, int n, int H, int W, int max_images, bool allocate);
uint8_t* mt_face_detect_image_in(MtGraph* g);
uint8_t* mt_face_detect_records(MtGraph* g);
// the threshold the program's device word holds (NaN before the first write): ltk_face_detect uploads it only when a call brings another
bool mt_face_detect_thresh_is(const MtGraph* g, float thresh);
void mt_face_detect_set_thresh(MtGraph* g, float thresh);
// launches of `g` that write the buffer of the tensor named `name` (0: no such tensor); 1 = nothing else overwrites it in a run
int mt_named_writers(MtGraph* g, const char* name);
// Whisper encoder graph (one 30-s window per run): input log-mel tensor = mt_latent_in(), 5 hidden states
int mt_build_whisper_graph(MtGraph* g, const ltk_named_tensor* encoder_sd, int n);
f16* mt_whisper_state(MtGraph* g, int i, int* cbt, int* cb0);
// Batched live steps (ltk_whisper_step_batch): the same op list over the packed weights of the loaded single-clip graph (MtGraph::share),
// with activations of its own for `frames` clips (kWhisperBatchClips, nn_kernels.h); clip c = image c of every tensor.  0, or -4 when
// the activations could not be allocated.
int mt_build_whisper_batch_graph(MtGraph* g, const MtGraph* single, int frames);
// How a call of nreq requests is cut (pure host): runs of at most `cap` in request order - every clip is the same 30-s window, so there
// is nothing to group by; a run of one request takes the single-clip path (batched = false).
struct WhisperRun { int first = 0, count = 0; bool batched = false; };
std::vector<WhisperRun> whisper_batch_plan(int nreq, int cap);
// HuBERT-large (hubert.hip): the packed weights live in ONE graph that is never run (mt_build_hubert_weights, from
// HubertModel.state_dict() with the positional conv's weight norm already folded); a program for a clip of n_samples is built
// over it and owns its activations only.  Input: the normalised fp32 waveform in mt_hubert_pcm_in(); output: last_hidden_state,
// CB16 [64][rows][16].
int hubert_rows(int n_samples);                 // rows HubertModel returns for a clip of n_samples (0: shorter than the receptive field)
int mt_build_hubert_weights(MtGraph* g, const ltk_named_tensor* sd, int n);
// a program for up to `frames` clips of n_samples each (images of one run; the waveform of clip i at i * n_samples floats of
// mt_hubert_pcm_in(), its rows in image i of every tensor)
int mt_build_hubert_program(MtGraph* g, const MtGraph* weights, int n_samples, int frames = 1);
// Batched live steps (ltk_hubert_step_batch).  Activation bytes of ONE clip of a program, from the clip length and the depth alone -
// the builder's buffer list restated, so that a call can be planned before anything is built or allocated.
size_t hubert_clip_activation_bytes(int n_samples, int layers);
constexpr int kHubertBatchClips = 16;                    // 16 x 51 = 816 rows: every linear layer of a live-length batch stays on the weight-streaming row kernel
constexpr size_t kHubertBatchBudget = (size_t)2 << 30;   // a batched program is built only if its activations at full capacity stay under this
// How a call of nreq requests is cut (pure host): requests grouped by n_samples in arrival order, every group cut into runs of at most
// kHubertBatchClips; a run of one, or a length whose program at full capacity would pass the budget, goes to the single-clip path
// (batched = false, one request per run).
struct HubertRun { int n_samples = 0; bool batched = false; std::vector<int> req; };
std::vector<HubertRun> hubert_batch_plan(const int* n_samples, int nreq, int layers);
int mt_hubert_layers(const MtGraph* g);
int mt_hubert_rows(const MtGraph* g);
float* mt_hubert_pcm_in(MtGraph* g);
f16* mt_hubert_out(MtGraph* g, int* cbt, int* cb0);
size_t mt_activation_bytes(const MtGraph* g);

}  // namespace ltk

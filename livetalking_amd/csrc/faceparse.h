// The launch list of the BiSeNet face parser's main output (avatars/musetalk/utils/face_parsing/model.py BiSeNet.forward()[0], resnet.py)
// at one square image size, as a table built on the host alone: what a program over parse_kernels.h and the conv library launches, in
// order - and fp_plan, where each of them reads and writes.  mt_build_face_parse_graph (musetalk.hip) builds the device program of
// ltk_face_parse_load from the two; ltk_debug_face_parse_program / _plan list them and the CPU suite holds the list to the float64
// restatement's op walk, every conv of it to the conv planner, and the bindings to a replay of the restatement through them.
#pragma once
#include <string>
#include <vector>

namespace ltk {

// type: 0 conv (the library's), 10 stem, 11 max pool, 12 global average pool, 13 channel gate, 14 labels (bilinear x8 + argmax)
struct FpOp {
    std::string name;      // the module's name: a conv's output stands behind its BatchNorm, ReLU and residual add
    int type = 0;
    int cin = 0, cout = 0; // real channels (19 classes: the layout pads to 32)
    int k = 1, stride = 1, pad = 0, relu = 0, ups = 0, has_res = 0, plus1 = 0;
    int H = 0, W = 0;      // the map the op reads (a conv behind a nearest x2 upsample: the upsampled size); the stem: the image
    int Ho = 0, Wo = 0;    // the map it writes (labels: the image)
};

// size: a multiple of 32 in [64, 512]; an empty vector otherwise
std::vector<FpOp> fp_program(int size);

// Where every launch of the list reads and writes: the ONE statement of the network's wiring (tests/faceparse_ref.py walk).  The device
// builder (mt_build_face_parse_graph) allocates these buffers under these ids and binds its ops to these views;
// ltk_debug_face_parse_plan lists them and the CPU suite replays the float64 restatement through them.
// A view = channels [coff, coff + C) of buffer `buf`, which holds `ld` channels, on an H x W map; buf = -1: the op has no such operand.
// fp16 tensors are channel-blocked (C, ld, coff multiples of 16: conv_out.conv_out writes 32 layout channels, 19 real); the image
// buffer (uint8 [n][S][S][3]: C = ld = 3) and the label buffer (uint8 [n][S][S]: C = ld = 1) are byte tensors.
struct FpView { int buf = -1, ld = 0, coff = 0, C = 0, H = 1, W = 1; };
struct FpBind {
    FpView x, y;
    FpView r;        // a conv's residual / the map a gate adds (cp.feat16_sum)
    FpView a, b;     // a gate's pre-sigmoid attention and the per-channel value it adds (cp.feat32_sum), both dense 1 x 1
};
struct FpPlan {
    std::vector<FpOp> ops;
    std::vector<FpBind> bind;                  // one per op
    std::vector<size_t> buf_elems;             // elements of ONE image per buffer (halfs, or bytes for the two byte buffers)
    std::vector<size_t> buf_bytes;             // bytes at max_images
    int image_buf = -1, label_buf = -1;
    int size = 0, max_images = 0;
};
constexpr int kFpMaxImages = 8;
// size as fp_program, max_images in [1, kFpMaxImages]: 0, or -1 with the refusal in *err.  Pure.
int fp_plan(int size, int max_images, FpPlan* out, std::string* err);

}  // namespace ltk

// The launch list of the BiSeNet face parser's main output (avatars/musetalk/utils/face_parsing/model.py BiSeNet.forward()[0], resnet.py)
// at one square image size, as a table built on the host alone: what a program over parse_kernels.h and the conv library launches, in
// order.  No program consumes it yet; ltk_debug_face_parse_program lists it and the CPU suite holds it to the
// float64 restatement's op walk and every conv of it to the conv planner.
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

}  // namespace ltk

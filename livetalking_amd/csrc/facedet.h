// The launch list of the S3FD face detector (avatars/wav2lip/face_detection/detection/sfd/net_s3fd.py s3fd.forward, then what
// detect.py batch_detect does per level) at one frame size, as a table built on the host alone: what a program over s3fd_kernels.h and
// the conv library launches, in order - and fd_plan, where each of them reads and writes.  ltk_debug_face_detect_program / _plan list
// them; the CPU suite holds the list to the float64 restatement's op walk (tests/s3fd_ref.py), every conv of it to the conv planner,
// and the bindings to a replay of the restatement through them.
#pragma once
#include <string>
#include <vector>

namespace ltk {

// type: 0 conv (the library's), 20 stem (conv1_1 on the frame), 21 max pool 2x2, 22 L2Norm, 23 detect (one level's candidates)
struct FdOp {
    std::string name;      // the module's name; a conv's output stands behind its ReLU.  A head is "<source>_mbox": the level's conf and
                           // loc convs as ONE conv of 16 output channels (conf at 0..1 - 0..3 at conv3_3_norm -, loc at 4..7, the rest zero)
    int type = 0;
    int cin = 0, cout = 0; // channels (a head: 16; detect: 16 in, 0 out)
    int k = 1, stride = 1, pad = 0, relu = 0;
    int maxout = 0;        // detect: conf = [max(c0, c1, c2), c3] (level 0)
    int level = -1;        // head / detect: the level index i, stride 2^(i+2)
    int H = 0, W = 0;      // the map the op reads (the stem: the frame)
    int Ho = 0, Wo = 0;    // the map it writes (detect: the map it reads)
};

// H, W >= 32 (five floor-mode pools leave at least one pixel); an empty vector otherwise.  39 launches: the stem, 18 library convs
// of the trunk, 5 pools, 3 L2Norms, 6 merged heads, 6 detects.  Level 3 is the fc7 map, (H/32 + 4) x (W/32 + 4) behind fc6's pad 3,
// read with stride 32: the reference's own behaviour.
std::vector<FdOp> fd_program(int H, int W);

// Where every launch of the list reads and writes.  A view = channels [coff, coff + C) of buffer `buf`, read as holding `ld` channels
// on an H x W map; buf = -1: the op has no such operand (a detect op appends to the record buffer, rec_buf, which is no channel-blocked tensor).
// The two trunk buffers are written in turn by the ops nothing reads later; every tapped map (conv3_3, conv4_3, conv5_3, fc7, conv6_2,
// conv7_2), every norm and every head has a buffer of its own.  The image buffer is uint8 [n][H][W][3] (C = ld = 3).
struct FdView { int buf = -1, ld = 0, coff = 0, C = 0, H = 1, W = 1; };
struct FdBind { FdView x, y; };
struct FdPlan {
    std::vector<FdOp> ops;
    std::vector<FdBind> bind;                  // one per op
    std::vector<size_t> buf_elems;             // elements of ONE image per buffer (halfs, or bytes for the image buffer)
    std::vector<size_t> buf_bytes;             // bytes at max_images
    size_t total_bytes = 0;
    int image_buf = -1;
    int rec_buf = -1;                          // the candidate buffer (s3fd_kernels.h): per image kFdDevCap records and a share of the 256-byte head
    int H = 0, W = 0, max_images = 0;
};
constexpr int kFdMaxImages = 16;               // the reference's face_det_batch_size
constexpr size_t kFdMaxBytes = (size_t)8 << 30;
// H, W as fd_program, max_images in [1, kFdMaxImages], total_bytes below 8 GiB: 0, or -1 with the refusal (and the figure) in *err.  Pure.
int fd_plan(int H, int W, int max_images, FdPlan* out, std::string* err);

}  // namespace ltk

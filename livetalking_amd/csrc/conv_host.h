// What the conv sources share on the host side and nothing else includes (conv_plan.hip, conv_mfma.hip, conv3_mfma.hip): the small
// integer helpers of the launch geometry, the HIP error macro, and the packed plan's phase metadata with the first-generation kernel's
// staging limit, which the plan builder sizes its slabs by.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "conv_mfma.h"

namespace ltk {

inline int ceil_log2(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

// __umulhi(x, magic_u16(d)) == x / d, exact for x < 2^16 (a divisor of 1 has no 32-bit magic)
inline unsigned magic_u16(int d) { return (unsigned)((0x100000000ull + (unsigned long long)d - 1) / (unsigned long long)d); }

// functions that return 0 / -1 (refused) / -2 (HIP error) with the text in `std::string* err`
#define HIPCHK(expr)                                                                  \
    do {                                                                              \
        hipError_t _e = (expr);                                                       \
        if (_e != hipSuccess) {                                                       \
            if (err) *err = std::string(#expr) + ": " + hipGetErrorString(_e);        \
            return -2;                                                                \
        }                                                                             \
    } while (0)

// One sub-pixel phase of a (transposed) convolution as the first-generation kernel reads it from device memory, behind the packed
// weights at the next 16-byte boundary (conv_plan.hip upload): a tap list over the input patch, its own weight slab and output offset
constexpr int kMaxTaps = 52;       // 7x7 = 49 (+ pairing pad)
struct PhaseMeta {
    int T, ooy, oox, w_off16;      // taps; output pixel = (oy*osy + ooy, ox*osx + oox); this phase's packed weights, in 16-byte units
    signed char dy[kMaxTaps], dx[kMaxTaps];
};

// conv_mfma.hip (first generation)
constexpr int kMaxBItems = 9;   // 16-byte weight items a thread stages per chunk
// whether the first-generation kernel has an instantiation for this plan configuration at all (conv_route)
bool conv1_has_kernel(int NC8, int NBT, bool tt9);
// conv1_launch = conv1_plan_launch (pure: checks, tile and its shrink loop, effective NBT, kernel, grid, LDS bytes, s2half, KArgs geometry,
// report; no HIP call, no device pointer dereferenced) + the enqueue.  `k1` may be null when only the verdict and the report are wanted.
struct K1Launch;
int conv1_plan_launch(const ConvPlan& p, const ConvIO& io, K1Launch* k1, std::string* err);
int conv1_launch(const ConvPlan& p, const ConvIO& io, hipStream_t stream, std::string* err);

}  // namespace ltk

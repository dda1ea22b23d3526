// Lookup in a state dict handed over the C ABI (ltk_named_tensor[]) by name and element count: the one reader of every program builder.
#pragma once
#include <math.h>

#include <string>

#include "../../include/ltk.h"

namespace ltk {

struct SD {
    const ltk_named_tensor* t;
    int n;
    std::string err;
    const float* get(const std::string& name, size_t expect) {
        for (int i = 0; i < n; ++i)
            if (name == t[i].name) {
                size_t cnt = 1;
                for (int d = 0; d < t[i].ndim; ++d) cnt *= (size_t)t[i].shape[d];
                if (cnt != expect) { err = "tensor " + name + " has " + std::to_string(cnt) + " elements, expected " + std::to_string(expect); return nullptr; }
                return t[i].data;
            }
        err = "state_dict is missing " + name;
        return nullptr;
    }
    bool has(const std::string& name) const {
        for (int i = 0; i < n; ++i) if (name == t[i].name) return true;
        return false;
    }
};

// Eval-mode BatchNorm2d behind a conv with `bias` (or null), folded into the conv's epilogue: y = (x + bias - mean) / sqrt(var + eps) * gamma
// + beta = x * scale + shift.  The packed weights of Wav2Lip and Ultralight are pinned bit for bit on this expression order.
inline void fold_bn(const float* gamma, const float* beta, const float* mean, const float* var, const float* bias, float eps, int C,
                    float* scale, float* shift) {
    for (int c = 0; c < C; ++c) {
        const float s = gamma[c] / sqrtf(var[c] + eps);
        scale[c] = s;
        shift[c] = ((bias ? bias[c] : 0.f) - mean[c]) * s + beta[c];
    }
}

}  // namespace ltk

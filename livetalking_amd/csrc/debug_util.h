// What the test and measurement hooks (engine_debug.hip, its only includer) share: owners for what a hook allocates next to DevBuf, the
// timing blocks, and the read-back of a channel-blocked tensor.  Every helper leaves the calling thread's error text set when it fails.
#pragma once
#include "engine_internal.h"

namespace ltk {

// host-mapped word a kernel reports through (gn_coop_kernel's error word)
struct HostWord {
    unsigned* host = nullptr;
    unsigned* dev = nullptr;
    hipError_t create() {
        hipError_t he = hipHostMalloc((void**)&host, sizeof(unsigned), hipHostMallocMapped);
        if (he == hipSuccess) he = hipHostGetDevicePointer((void**)&dev, host, 0);
        if (he == hipSuccess) *host = 0u;
        return he;
    }
    ~HostWord() { if (host) (void)hipHostFree(host); }
};

// timing-enabled events (Ev's cannot time), destroyed on every return path
struct TimedEvs {
    std::vector<hipEvent_t> ev;
    hipError_t create(size_t n) {
        ev.assign(n, nullptr);
        hipError_t he = hipSuccess;
        for (size_t i = 0; i < n && he == hipSuccess; ++i) he = hipEventCreate(&ev[i]);
        return he;
    }
    ~TimedEvs() { for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x); }
};

// *ms = time on `s` of up to `iters` calls of fn (0 or its error code, the text set; the first error ends the loop).  Records and waits
// for the closing event also behind an error: nothing of the calls is still running when this returns.  Returns fn's error or LTK_OK.
template <class Fn>
int time_iters(hipStream_t s, int iters, Fn fn, float* ms) {
    TimedEvs t;
    CHK(t.create(2));
    CHK(hipEventRecord(t.ev[0], s));
    int rc = LTK_OK;
    for (int i = 0; i < iters && !rc; ++i) rc = fn();
    CHK(hipEventRecord(t.ev[1], s));
    CHK(hipEventSynchronize(t.ev[1]));
    CHK(hipEventElapsedTime(ms, t.ev[0], t.ev[1]));
    return rc;
}

// ms_out[i] = mean over `iters` runs of interval i of n: run(&evs) records evs[i] in front of interval i and evs[n] behind the last
template <class Run>
int time_intervals(int n, int iters, Run run, float* ms_out) {
    TimedEvs t;
    CHK(t.create((size_t)n + 1));
    std::vector<double> acc((size_t)n, 0.0);
    for (int it = 0; it < iters; ++it) {
        const int rc = run(&t.ev);
        if (rc) return rc;
        CHK(hipEventSynchronize(t.ev.back()));
        for (int i = 0; i < n; ++i) {
            float ms = 0.f;
            CHK(hipEventElapsedTime(&ms, t.ev[i], t.ev[i + 1]));
            acc[i] += ms;
        }
    }
    for (int i = 0; i < n; ++i) ms_out[i] = (float)(acc[i] / iters);
    return LTK_OK;
}

// host bytes -> a device buffer of their size
inline int upload(const void* host, size_t bytes, DevBuf* d) {
    CHK(hipMalloc(&d->p, bytes));
    CHK(hipMemcpy(d->p, host, bytes, hipMemcpyHostToDevice));
    return LTK_OK;
}

// channels [coff, coff + C) of a CB16 tensor of `ld` channels on an H x W map, `frames` images, as it stands once the compute stream has
// drained -> host fp32 NCHW
inline int read_cb16(ltk_engine* e, const f16* t, int frames, int C, int ld, int coff, int H, int W, float* host_out) {
    const size_t bytes = (size_t)frames * C * H * W * sizeof(float);
    DevBuf tmp;
    CHK(hipMalloc(&tmp.p, bytes));
    launch_nhwc_to_nchw_f32(t, frames, H, W, ld, coff, C, (float*)tmp.p, e->compute);
    CHK(hipGetLastError());
    CHK(hipStreamSynchronize(e->compute));
    CHK(hipMemcpy(host_out, tmp.p, bytes, hipMemcpyDeviceToHost));
    return LTK_OK;
}

// ... of the tensor `g` holds under `name` (`model`, `per`: the words of the two error texts)
inline int read_named(ltk_engine* e, MtGraph* g, const char* model, const char* name, int frames, const char* per, float* out, size_t n_floats) {
    int C, ld, coff, H, W;
    f16* t = mt_named(g, name, &C, &ld, &coff, &H, &W);
    if (!t) return fail(LTK_E_STATE, std::string("no ") + model + " tensor named " + name);
    const size_t cnt = (size_t)frames * C * H * W;
    if (cnt != n_floats) return fail(LTK_E_INVALID, "size mismatch: tensor has " + std::to_string(cnt) + " floats" + per);
    return read_cb16(e, t, frames, C, ld, coff, H, W, out);
}
// an op's name into the caller's buffer
inline int copy_op_name(MtGraph* g, int op, char* buf, int buf_len, int* type) {
    const char* n = mt_op_name(g, op, type);
    if (!n) return fail(LTK_E_INVALID, "no such op");
    snprintf(buf, (size_t)buf_len, "%s", n);
    return LTK_OK;
}

}  // namespace ltk

// libaccel_hip, internal: what its translation units share -- accel_hip.cpp (plans: parser, tuner, executor) and accel_io.cpp (bytes in and
// out of a model's persistent buffers, frames and results).  Everything about plans stays private to accel_hip.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "../../include/accel_hip.h"

// ---------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------
// records the message accel_last_error returns (per thread) and returns `code`; not an export of the library
__attribute__((visibility("hidden"))) int fail(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                    \
    do {                                                                                 \
        hipError_t e__ = (expr);                                                         \
        if (e__ != hipSuccess)                                                           \
            return fail(ACCEL_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), \
                        __FILE__, __LINE__);                                             \
    } while (0)

// ---------------------------------------------------------------------------
// objects
// ---------------------------------------------------------------------------
struct accel_ctx {
    int device;
    hipStream_t stream;     // compute stream (the one callers order against)
    hipStream_t copy;       // host<->HBM prefetch stream (accel_model_prefetch)
};

struct HostParam {
    std::vector<int64_t> shape;
    std::vector<float> data;
    size_t numel() const { return data.size(); }
};

struct DevBuf {
    void* ptr = nullptr;
    size_t bytes = 0;
    // accel_model_bind_device: input buffers that only the prep kernels read are read THROUGH `slot` (a pointer in device
    // memory, initially = ptr), which the host may point at a caller-owned frame between two runs of a captured plan
    const void** slot = nullptr;
    const void* bound = nullptr;        // what the slot points at when it is not `ptr`
    int readers = 0, prep_readers = 0;  // plan operands resolved to this buffer / those of prep_rgb and prep_flow
    int img_h = 0, img_w = 0;           // an image input: the H x W its prep kernels read it at (bytes / (3 * H * W * 4) frames)
};

// device bytes that grow on demand and are kept otherwise.  A buffer that is too small is released with hipFree, which waits for the device: no
// kernel enqueued earlier is still reading the old one.
struct __attribute__((visibility("hidden"))) DevScratch {
    unsigned char* ptr = nullptr;
    size_t bytes = 0;
    DevScratch() = default;
    DevScratch(const DevScratch&) = delete;
    ~DevScratch() { if (ptr) hipFree(ptr); }
    int reserve(int device, size_t need)
    {
        HIP_TRY(hipSetDevice(device));
        if (bytes >= need) return 0;
        if (ptr) { HIP_TRY(hipFree(ptr)); ptr = nullptr; bytes = 0; }
        HIP_TRY(hipMalloc((void**)&ptr, need));
        bytes = need;
        return 0;
    }
};

struct accel_model {
    accel_ctx* ctx;
    std::map<std::string, HostParam> params;
    std::map<std::string, DevBuf> pbufs;
    std::vector<accel_plan*> plans;
    std::map<std::string, accel_plan*> roles;
    int feat_c = 0, feat_h = 0, feat_w = 0, feat_n = 1;   // shape of the propagated feature (`meta` line of the plans)
    // derived persistent buffers (`pbuf name=featG from=feat`): a linear image of another buffer that the plans keep
    // in step with it.  Writing the source from outside a plan that also writes the derived buffer makes it stale; a
    // plan that reads a stale derived buffer first runs the model's `init:<name>` plan (see accel_plan_run).
    std::map<std::string, std::string> derived_from;
    std::map<std::string, bool> derived_valid;
    std::map<std::string, uint64_t> generation;     // write generation per persistent buffer (accel_model_buffer_generation)
    struct Shadow {
        DevScratch mem;
        size_t filled = 0;
        hipEvent_t ready = nullptr, consumed = nullptr;
        bool was_consumed = false;
        ~Shadow() { if (ready) hipEventDestroy(ready); if (consumed) hipEventDestroy(consumed); }
    };
    std::map<std::string, Shadow> shadows;          // prefetch targets (accel_model_prefetch / accel_model_commit)
    // uint8 frames (accel_model_write_u8 / accel_model_prefetch_u8 / accel_model_commit_u8): the bytes of a frame wait in HBM for the
    // conversion kernel -- per buffer in a uint8 shadow of its own, never the fp32 shadow above (a prefetch of one kind cannot be
    // committed as the other), or in the one staging buffer of synchronous host writes
    std::map<std::string, Shadow> shadows_u8;
    DevScratch stage_u8;
    // finished frames (accel_model_labels_to_source / _hist_add / _hist_read / _labels_colour): the shape of `labels` (the score_tail op
    // of a plan, or a `meta labels_n= labels_h= labels_w=` line, says it), a staging buffer for results on their way to the host, and the
    // confusion matrix: 32 x 32 unsigned 64-bit words that persist across calls, for ncls = hist_ncls classes (0: empty since the last clear)
    int labels_n = 0, labels_h = 0, labels_w = 0;
    // accel_model_confidence: the shape of `logits` (n x ncls x H x W fp32), learnt the same way (`meta logits_n= logits_ncls= logits_h= logits_w=`)
    int logits_n = 0, logits_ncls = 0, logits_h = 0, logits_w = 0;
    DevScratch stage_out;
    unsigned long long* hist = nullptr;
    int hist_ncls = 0;
    // accel_model_band_hist_add / _scores_band_hist_add / _band_hist_read: the confusion matrix per band around the ground truth's boundaries, an
    // accumulator of its own -- 5 x 32 x 32 words (allocated on first use), of which (nwidths + 1) x ncls x ncls hold counts made under `widths`
    // (ncls = 0: empty since the last clear)
    struct BandHist {
        unsigned long long* words = nullptr;
        int ncls = 0, nwidths = 0, widths[4] = {0, 0, 0, 0};
        BandHist() = default;
        BandHist(const BandHist&) = delete;
        ~BandHist() { if (words) hipFree(words); }
    };
    BandHist band_hist;
    // accel_model_scores_hist_add / _scores_colour: the labels of the interpolated scores at the source size (n x h x w uint8, tight rows)
    // on their way to the counting / colouring kernel
    DevScratch interp_labels;
    // accel_model_frame_change / accel_model_frame_keep: the signature of the frame looked at last and the one kept at the last key frame
    // (n x gh x gw int32 each, allocated on first use), with the geometry they were made under (n = 0: none yet)
    struct FrameSig {
        DevScratch mem;
        int n = 0, out_h = 0, out_w = 0, cell = 0;
    };
    FrameSig sig_cur, sig_kept;
    // accel_model_labels_summary / _scores_summary with track = 1: the previous frame's labels at the source size (n x h x w uint8, tight rows,
    // allocated on first use), with what they were made under (n = 0: none; accel_model_labels_forget)
    struct KeptLabels {
        DevScratch mem;
        int n = 0, h = 0, w = 0, ncls = 0;
    };
    KeptLabels kept_labels;
    // accel_model_labels_components / _scores_components: the scratch of labels_components.hip, one allocation carved into the parent and the
    // area / slot word per source pixel and the counts per chunk (accel_io.cpp ComponentsScratch); kept for the next frame, freed with the model
    DevScratch components;
    // which buffer holds the current propagated feature: 0 = `feat`, 1 = `feat_b` (non-key graphs may be bound as a pair of
    // plans `cur` / `cur_b` that ping-pong between the two instead of copying the warped feature back; whoever wrote last)
    int feat_slot = 0;
    void source_written(const std::string& src) {
        ++generation[src];
        if (src == "feat") feat_slot = 0;
        else if (src == "feat_b") feat_slot = 1;
        for (auto& kv : derived_from) if (kv.second == src) derived_valid[kv.first] = false;
    }
};

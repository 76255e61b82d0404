// libaccel_hip: bytes in and out of a model's persistent buffers (bind, write, read, prefetch and commit), and the frame and result entry
// points behind them -- uint8, NV12, I420, P010 and YUY2 frames in, finished frames, confidence (of stored and of interpolated scores), interpolated labels and
// the overlay in the frame's own format and the per-class summary out, and the frame-change measure of an image input (see include/accel_hip.h).  Nothing here knows about plans.
#include <cstring>

#include "accel_objects.h"
#include "kernels.h"

// a write into the model's own buffer ends a binding made by accel_model_bind_device
static int unbind(accel_model* m, DevBuf& b)
{
    if (!b.bound) return 0;
    HIP_TRY(launch_set_slot(b.slot, b.ptr, m->ctx->stream));
    b.bound = nullptr;
    return 0;
}

extern "C" int accel_model_bind_device(accel_model* m, const char* buf, const void* devptr, size_t bytes)
{
    if (!m || !buf || !devptr) return fail(ACCEL_ERR_ARG, "accel_model_bind_device: NULL argument");
    auto it = m->pbufs.find(buf);
    if (it == m->pbufs.end()) return fail(ACCEL_ERR_ARG, "accel_model_bind_device: unknown buffer '%s'", buf);
    DevBuf& b = it->second;
    if (!b.slot || b.readers != b.prep_readers)
        return fail(ACCEL_ERR_ARG, "accel_model_bind_device: '%s' is not an image input of the finalized plans (only buffers that prep_rgb / "
                                   "prep_flow alone read can be bound)", buf);
    if (bytes != b.bytes) return fail(ACCEL_ERR_ARG, "accel_model_bind_device: %zu bytes, buffer '%s' has %zu", bytes, buf, b.bytes);
    if (b.bound != devptr) HIP_TRY(launch_set_slot(b.slot, devptr, m->ctx->stream));
    b.bound = devptr == b.ptr ? nullptr : devptr;
    m->source_written(buf);
    return 0;
}

extern "C" int accel_model_write(accel_model* m, const char* buf, const void* src, size_t bytes, int src_on_device)
{
    if (!m || !buf || !src) return fail(ACCEL_ERR_ARG, "accel_model_write: NULL argument");
    auto it = m->pbufs.find(buf);
    if (it == m->pbufs.end()) return fail(ACCEL_ERR_ARG, "accel_model_write: unknown buffer '%s'", buf);
    if (bytes > it->second.bytes) return fail(ACCEL_ERR_ARG, "accel_model_write: %zu bytes > buffer '%s' (%zu)", bytes, buf, it->second.bytes);
    if (int rc = unbind(m, it->second)) return rc;
    if (src_on_device) HIP_TRY(launch_copy_bytes(src, it->second.ptr, bytes, m->ctx->stream));      // own copy kernel: 4x the rate of the runtime's blit
    else HIP_TRY(hipMemcpyAsync(it->second.ptr, src, bytes, hipMemcpyHostToDevice, m->ctx->stream));
    if (!src_on_device) HIP_TRY(hipStreamSynchronize(m->ctx->stream));   // pageable source may be reused by the caller
    m->source_written(buf);
    return 0;
}

extern "C" int accel_model_read(accel_model* m, const char* buf, void* dst, size_t bytes, int dst_on_device)
{
    if (!m || !buf || !dst) return fail(ACCEL_ERR_ARG, "accel_model_read: NULL argument");
    auto it = m->pbufs.find(buf);
    if (it == m->pbufs.end()) return fail(ACCEL_ERR_ARG, "accel_model_read: unknown buffer '%s'", buf);
    if (bytes > it->second.bytes) return fail(ACCEL_ERR_ARG, "accel_model_read: %zu bytes > buffer '%s' (%zu)", bytes, buf, it->second.bytes);
    // a bound input is read where the plans read it (the caller's frame), not the model-owned copy an earlier write left behind
    const void* src = it->second.bound ? it->second.bound : it->second.ptr;
    if (dst_on_device) HIP_TRY(launch_copy_bytes(src, dst, bytes, m->ctx->stream));
    else HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, m->ctx->stream));
    if (!dst_on_device) HIP_TRY(hipStreamSynchronize(m->ctx->stream));
    return 0;
}

extern "C" int accel_model_buffer(accel_model* m, const char* buf, void** dev_ptr, size_t* bytes)
{
    if (!m || !buf) return fail(ACCEL_ERR_ARG, "accel_model_buffer: NULL argument");
    auto it = m->pbufs.find(buf);
    if (it == m->pbufs.end()) return fail(ACCEL_ERR_ARG, "accel_model_buffer: unknown buffer '%s'", buf);
    // the caller is about to write the model-owned buffer through the raw pointer: a binding made by accel_model_bind_device
    // ends here (the plans read the model's copy again), otherwise that write would be silently ignored
    if (dev_ptr) if (int rc = unbind(m, it->second)) return rc;
    if (dev_ptr) *dev_ptr = it->second.ptr;
    if (bytes) *bytes = it->second.bytes;
    if (dev_ptr) m->source_written(buf);   // the caller may write through the raw pointer: derived buffers become stale
    return 0;
}

extern "C" int accel_model_buffer_generation(accel_model* m, const char* buf, uint64_t* generation)
{
    if (!m || !buf || !generation) return fail(ACCEL_ERR_ARG, "accel_model_buffer_generation: NULL argument");
    if (!m->pbufs.count(buf)) return fail(ACCEL_ERR_ARG, "accel_model_buffer_generation: unknown buffer '%s'", buf);
    auto it = m->generation.find(buf);
    *generation = it == m->generation.end() ? 0 : it->second;
    return 0;
}

extern "C" int accel_host_alloc(size_t bytes, void** out)
{
    if (!out || !bytes) return fail(ACCEL_ERR_ARG, "accel_host_alloc: bad argument");
    HIP_TRY(hipHostMalloc(out, bytes, hipHostMallocDefault));
    return 0;
}

extern "C" int accel_host_free(void* p)
{
    if (p) HIP_TRY(hipHostFree(p));
    return 0;
}

// ---- prefetch and commit: what the fp32 route and the uint8 route (BGR and NV12 bytes) share ------------------------------------------------
typedef accel_model::Shadow Shadow;

// `bytes` from pinned memory into a shadow of at least `reserve` bytes, on the copy stream
static int prefetch_into(accel_model* m, Shadow& sh, size_t reserve, const void* pinned_src, size_t bytes)
{
    const bool grows = sh.mem.bytes < reserve;      // (hipFree waits for the device, so for whoever read the old shadow)
    if (int rc = sh.mem.reserve(m->ctx->device, reserve)) return rc;
    if (!sh.ready) {
        HIP_TRY(hipEventCreateWithFlags(&sh.ready, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&sh.consumed, hipEventDisableTiming));
    }
    // the previous commit read the shadow on the compute stream (event recorded right behind that copy or kernel, ahead of the
    // plan that followed): do not overwrite under it -- and wait for nothing else on that stream
    if (!grows && sh.was_consumed) HIP_TRY(hipStreamWaitEvent(m->ctx->copy, sh.consumed, 0));
    HIP_TRY(hipMemcpyAsync(sh.mem.ptr, pinned_src, bytes, hipMemcpyHostToDevice, m->ctx->copy));
    HIP_TRY(hipEventRecord(sh.ready, m->ctx->copy));
    sh.filled = bytes;
    return 0;
}

// the shadow of `buf` if a prefetch is waiting in it
static Shadow* prefetched(std::map<std::string, Shadow>& shadows, const char* buf)
{
    auto it = shadows.find(buf);
    return it == shadows.end() || !it->second.filled ? nullptr : &it->second;
}

// the compute stream waits for the prefetch, `launch(src, dst, stream)` moves the shadow into the model-owned buffer, the shadow is free again
template <class Launch>
static int commit_from(accel_model* m, const char* buf, DevBuf& b, Shadow& sh, Launch launch)
{
    HIP_TRY(hipStreamWaitEvent(m->ctx->stream, sh.ready, 0));
    if (int rc = unbind(m, b)) return rc;
    HIP_TRY(launch(sh.mem.ptr, b.ptr, m->ctx->stream));
    HIP_TRY(hipEventRecord(sh.consumed, m->ctx->stream));
    sh.was_consumed = true;
    sh.filled = 0;
    m->source_written(buf);
    return 0;
}

// host bytes on their way to a kernel (frames, ground truth, a frame to blend with): through the staging buffer, on the compute stream
static int stage_in(accel_model* m, const void* host, size_t bytes, const unsigned char** dev)
{
    if (int rc = m->stage_u8.reserve(m->ctx->device, bytes)) return rc;
    HIP_TRY(hipMemcpyAsync(m->stage_u8.ptr, host, bytes, hipMemcpyHostToDevice, m->ctx->stream));
    HIP_TRY(hipStreamSynchronize(m->ctx->stream));   // pageable source may be reused by the caller
    *dev = m->stage_u8.ptr;
    return 0;
}

extern "C" int accel_model_prefetch(accel_model* m, const char* buf, const void* pinned_src, size_t bytes)
{
    if (!m || !buf || !pinned_src) return fail(ACCEL_ERR_ARG, "accel_model_prefetch: NULL argument");
    auto it = m->pbufs.find(buf);
    if (it == m->pbufs.end()) return fail(ACCEL_ERR_ARG, "accel_model_prefetch: unknown buffer '%s'", buf);
    if (bytes > it->second.bytes) return fail(ACCEL_ERR_ARG, "accel_model_prefetch: %zu bytes > buffer '%s' (%zu)", bytes, buf, it->second.bytes);
    return prefetch_into(m, m->shadows[buf], it->second.bytes, pinned_src, bytes);       // sized to the whole buffer on first use
}

extern "C" int accel_model_commit(accel_model* m, const char* buf)
{
    if (!m || !buf) return fail(ACCEL_ERR_ARG, "accel_model_commit: NULL argument");
    Shadow* sh = prefetched(m->shadows, buf);
    if (!sh) return fail(ACCEL_ERR_ARG, "accel_model_commit: nothing was prefetched for '%s'", buf);
    return commit_from(m, buf, m->pbufs[buf], *sh, [&](const unsigned char* src, void* dst, hipStream_t st) {
        return launch_copy_bytes(src, dst, sh->filled, st);
    });
}

// device temporaries of the operator-level entry points
struct DevTemps {
    std::vector<void*> ptrs;
    ~DevTemps() { for (void* p : ptrs) hipFree(p); }
    void* get(size_t bytes) { void* p = nullptr; if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) return nullptr; ptrs.push_back(p); return p; }
    void* upload(const void* host, size_t bytes) { void* p = get(bytes); if (p && hipMemcpy(p, host, bytes, hipMemcpyHostToDevice) != hipSuccess) return nullptr; return p; }
};

// ---- frames in: what the BGR route and the YUV routes share --------------------------------------------------------------------------------
// The resize a frame conversion is told (out_h, out_w, step) and the padded size H x W, for an h x w source.
static int frame_resize_args(const char* fn, int h, int w, int out_h, int out_w, double step, int H, int W)
{
    if (!(step > 0.0) || step > 1e9) return fail(ACCEL_ERR_ARG, "%s: step = %g, must be a positive number of source pixels per output pixel", fn, step);
    if (H < 1 || W < 1) return fail(ACCEL_ERR_ARG, "%s: H x W = %d x %d, must be >= 1", fn, H, W);
    if (out_h < 1 || out_h > H) return fail(ACCEL_ERR_ARG, "%s: out_h = %d, must be in 1 .. H = %d", fn, out_h, H);
    if (out_w < 1 || out_w > W) return fail(ACCEL_ERR_ARG, "%s: out_w = %d, must be in 1 .. W = %d", fn, out_w, W);
    if (step == 1.0 && (out_h != h || out_w != w))
        return fail(ACCEL_ERR_ARG, "%s: step = 1 copies the frame, but out_h x out_w = %d x %d is not h x w = %d x %d", fn, out_h, out_w, h, w);
    return 0;
}

static int frame_u8_buf(const char* fn, accel_model* m, const char* buf, int n, int H, int W, DevBuf** out)
{
    auto it = m->pbufs.find(buf);
    if (it == m->pbufs.end()) return fail(ACCEL_ERR_ARG, "%s: unknown buffer '%s'", fn, buf);
    const size_t need = (size_t)n * 3 * H * W * 4;
    if (need != it->second.bytes)
        return fail(ACCEL_ERR_ARG, "%s: n x 3 x H x W fp32 = %d x 3 x %d x %d = %zu bytes, buffer '%s' has %zu", fn, n, H, W, need, buf, it->second.bytes);
    *out = &it->second;
    return 0;
}

// Host frames of `src_bytes` bytes, converted by `launch(src, dst, stream)` into n x 3 x H x W fp32 of host memory: the operator-level entry points
template <class Launch>
static int frames_to_host(const char* fn, accel_ctx* ctx, const void* src, size_t src_bytes, int n, int H, int W, float* out, Launch launch)
{
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t ob = (size_t)n * 3 * H * W * 4;
    DevTemps t;
    const unsigned char* s = static_cast<const unsigned char*>(t.upload(src, src_bytes));
    float* d = static_cast<float*>(t.get(ob));
    if (!s || !d) return fail(ACCEL_ERR_HIP, "%s: device allocation or upload failed", fn);
    HIP_TRY(launch(s, d, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(out, d, ob, hipMemcpyDeviceToHost));
    return 0;
}

// n frames of h x w pixels as BGR bytes, by `launch(src, dst, dst_pitch, stream)`.  on_device: enqueued from `src` into `bgr_out`, and that is
// all.  Host in, host out: the rows of the result are written `out_pitch` apart, the bytes between them are left as they are.
template <class Launch>
static int bgr_rows(const char* fn, accel_ctx* ctx, const uint8_t* src, size_t src_bytes, int n, int h, int w, uint8_t* bgr_out, size_t out_pitch,
                    int on_device, Launch launch)
{
    const size_t row = (size_t)3 * w;
    if (!bgr_out) return fail(ACCEL_ERR_ARG, "%s: bgr_out is NULL", fn);
    if (out_pitch < row || out_pitch > ((size_t)1 << 40))
        return fail(ACCEL_ERR_ARG, "%s: out_pitch = %zu bytes, a row of w = %d BGR pixels has %zu", fn, out_pitch, w, row);
    HIP_TRY(hipSetDevice(ctx->device));
    if (on_device) {
        HIP_TRY(launch(src, bgr_out, out_pitch, ctx->stream));
        return 0;
    }
    DevTemps t;
    const unsigned char* s = static_cast<const unsigned char*>(t.upload(src, src_bytes));
    unsigned char* d = static_cast<unsigned char*>(t.get((size_t)n * h * row));
    if (!s || !d) return fail(ACCEL_ERR_HIP, "%s: device allocation or upload failed", fn);
    HIP_TRY(launch(s, d, row, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy2D(bgr_out, out_pitch, d, row, row, (size_t)n * h, hipMemcpyDeviceToHost));
    return 0;
}

// Frames of `src_bytes` bytes, converted by `launch(src, dst, stream)` into the image input `buf` of n x 3 x H x W fp32, once their own arguments
// are checked.  A host source goes through the staging buffer.
template <class Launch>
static int write_frames(const char* fn, accel_model* m, const char* buf, int n, int H, int W, const unsigned char* src, size_t src_bytes,
                        int src_on_device, Launch launch)
{
    DevBuf* b = nullptr;
    if (int rc = frame_u8_buf(fn, m, buf, n, H, W, &b)) return rc;
    if (!src_on_device) if (int rc = stage_in(m, src, src_bytes, &src)) return rc;
    if (int rc = unbind(m, *b)) return rc;
    HIP_TRY(launch(src, static_cast<float*>(b->ptr), m->ctx->stream));
    m->source_written(buf);
    return 0;
}

// The bytes that accel_model_prefetch_u8 put into the uint8 shadow of `buf` (bytes are bytes: BGR, NV12, P010's words), converted by
// `launch(src, dst, stream)` into the image input.  `check(dev, &need)` is the family's own argument check: it is told the address the kernel
// will read (P010's alignment needs it) and says how many bytes the frames occupy; `formula` is how the family words that size.
template <class Check, class Launch>
static int commit_frames(const char* fn, accel_model* m, const char* buf, int n, int H, int W, const char* formula, Check check, Launch launch)
{
    if (!m->pbufs.count(buf)) return fail(ACCEL_ERR_ARG, "%s: unknown buffer '%s'", fn, buf);
    Shadow* sh = prefetched(m->shadows_u8, buf);
    if (!sh) return fail(ACCEL_ERR_ARG, "%s: no uint8 frames were prefetched for '%s'", fn, buf);
    size_t need = 0;
    if (int rc = check(sh->mem.ptr, &need)) return rc;
    DevBuf* b = nullptr;
    if (int rc = frame_u8_buf(fn, m, buf, n, H, W, &b)) return rc;
    if (need > sh->filled) return fail(ACCEL_ERR_ARG, "%s: %s = %zu bytes, %zu were prefetched for '%s'", fn, formula, need, sh->filled, buf);
    return commit_from(m, buf, *b, *sh, [&](const unsigned char* src, void* dst, hipStream_t st) { return launch(src, static_cast<float*>(dst), st); });
}

// ---- BGR frames (frames_u8.hip) ------------------------------------------------------------------------------------------------------------
// Geometry of a uint8 frame conversion, checked before anything is enqueued: every message names the argument at fault.
static int frame_u8_args(const char* fn, const void* bgr, int n, int h, int w, size_t pitch, const double* means_bgr, int out_h, int out_w, double step,
                         int H, int W)
{
    if (!bgr) return fail(ACCEL_ERR_ARG, "%s: bgr is NULL", fn);
    if (!means_bgr) return fail(ACCEL_ERR_ARG, "%s: means_bgr is NULL", fn);
    if (n < 1) return fail(ACCEL_ERR_ARG, "%s: n = %d, must be >= 1", fn, n);
    if (h < 1) return fail(ACCEL_ERR_ARG, "%s: h = %d, must be >= 1", fn, h);
    if (w < 1) return fail(ACCEL_ERR_ARG, "%s: w = %d, must be >= 1", fn, w);
    if (pitch < (size_t)3 * w) return fail(ACCEL_ERR_ARG, "%s: pitch = %zu bytes, a row of w = %d pixels has %zu", fn, pitch, w, (size_t)3 * w);
    return frame_resize_args(fn, h, w, out_h, out_w, step, H, W);
}

extern "C" int accel_frame_u8(accel_ctx* ctx, const uint8_t* bgr, int n, int h, int w, size_t pitch, const double* means_bgr,
                              int out_h, int out_w, double step, int H, int W, float* out)
{
    const char* fn = "accel_frame_u8";
    if (!ctx || !out) return fail(ACCEL_ERR_ARG, "accel_frame_u8: NULL argument");
    if (int rc = frame_u8_args(fn, bgr, n, h, w, pitch, means_bgr, out_h, out_w, step, H, W)) return rc;
    return frames_to_host(fn, ctx, bgr, (size_t)n * h * pitch, n, H, W, out, [&](const unsigned char* src, float* dst, hipStream_t st) {
        return launch_frames_u8(src, n, h, w, pitch, means_bgr, out_h, out_w, step, H, W, dst, st);
    });
}

extern "C" int accel_model_write_u8(accel_model* m, const char* buf, const uint8_t* bgr, int n, int h, int w, size_t pitch, const double* means_bgr,
                                    int out_h, int out_w, double step, int H, int W, int src_on_device)
{
    const char* fn = "accel_model_write_u8";
    if (!m || !buf) return fail(ACCEL_ERR_ARG, "accel_model_write_u8: NULL argument");
    if (int rc = frame_u8_args(fn, bgr, n, h, w, pitch, means_bgr, out_h, out_w, step, H, W)) return rc;
    return write_frames(fn, m, buf, n, H, W, bgr, (size_t)n * h * pitch, src_on_device, [&](const unsigned char* src, float* dst, hipStream_t st) {
        return launch_frames_u8(src, n, h, w, pitch, means_bgr, out_h, out_w, step, H, W, dst, st);
    });
}

extern "C" int accel_model_prefetch_u8(accel_model* m, const char* buf, const void* pinned_src, size_t bytes)
{
    if (!m || !buf || !pinned_src) return fail(ACCEL_ERR_ARG, "accel_model_prefetch_u8: NULL argument");
    if (!m->pbufs.count(buf)) return fail(ACCEL_ERR_ARG, "accel_model_prefetch_u8: unknown buffer '%s'", buf);
    if (!bytes) return fail(ACCEL_ERR_ARG, "accel_model_prefetch_u8: bytes = 0");
    return prefetch_into(m, m->shadows_u8[buf], bytes, pinned_src, bytes);       // frames of another size: the shadow grows to the bytes asked for
}

extern "C" int accel_model_commit_u8(accel_model* m, const char* buf, int n, int h, int w, size_t pitch, const double* means_bgr,
                                     int out_h, int out_w, double step, int H, int W)
{
    const char* fn = "accel_model_commit_u8";
    if (!m || !buf) return fail(ACCEL_ERR_ARG, "accel_model_commit_u8: NULL argument");
    return commit_frames(fn, m, buf, n, H, W, "n x h x pitch", [&](const void* dev, size_t* need) {
        *need = (size_t)n * h * pitch;
        return frame_u8_args(fn, dev, n, h, w, pitch, means_bgr, out_h, out_w, step, H, W);
    }, [&](const unsigned char* src, float* dst, hipStream_t st) {
        return launch_frames_u8(src, n, h, w, pitch, means_bgr, out_h, out_w, step, H, W, dst, st);
    });
}

// ---- YUV frames: I420, P010, YUY2 and NV12, replicated or sited chroma (frames_yuv.h; frames_yuv.hip, frames_sited.hip) --------------------
extern "C" int accel_nv12_coefficients(int colour, int32_t out[6])
{
    if (!out) return fail(ACCEL_ERR_ARG, "accel_nv12_coefficients: out is NULL");
    const int32_t* c = nv12_coefficients(colour);
    if (!c) return fail(ACCEL_ERR_ARG, "accel_nv12_coefficients: colour = %d, must be in 0 .. 3", colour);
    for (int i = 0; i < 6; ++i) out[i] = c[i];
    return 0;
}

extern "C" int accel_yuv10_coefficients(int colour, int32_t out[6])
{
    if (!out) return fail(ACCEL_ERR_ARG, "accel_yuv10_coefficients: out is NULL");
    const int32_t* c = yuv10_coefficients(colour);
    if (!c) return fail(ACCEL_ERR_ARG, "accel_yuv10_coefficients: colour = %d, must be in 0 .. 3", colour);
    for (int i = 0; i < 6; ++i) out[i] = c[i];
    return 0;
}

enum { YUV_I420 = 0, YUV_P010 = 1, YUV_YUY2 = 2, YUV_NV12 = 3 };

// the bytes one frame occupies: one past the last byte of the last row of its last plane (planes of I420 may interleave, so no whole pitch is
// counted for the last row; the last chroma row of format 3 ends after w bytes)
static size_t yuv_extent(const accel_yuv_layout& y)
{
    const size_t h = (size_t)y.h, w = (size_t)y.w;
    if (y.format == YUV_I420) return (y.u_offset > y.v_offset ? y.u_offset : y.v_offset) + (h / 2 - 1) * y.pitch_c + w / 2;
    if (y.format == YUV_P010) return y.u_offset + (h / 2 - 1) * y.pitch + 2 * w;
    if (y.format == YUV_NV12) return y.u_offset + (h / 2 - 1) * y.pitch + w;
    return (h - 1) * y.pitch + 2 * w;
}

// the same for the accel_*_nv12 entry points, which ask for a whole pitch of the last chroma row (include/accel_hip.h)
static size_t nv12_extent(const accel_yuv_layout& y)
{
    return y.u_offset + (size_t)(y.h / 2) * y.pitch;
}

// What tells the families of entry points apart when a layout is checked: what their signatures call the frames and the chroma offset, the
// highest format they take, and where a frame ends.
struct LayoutRules { const char* src; const char* chroma; int max_format; size_t (*extent)(const accel_yuv_layout&); };
static const LayoutRules NV12_ARGS = {"nv12", "uv_offset", YUV_NV12, nv12_extent};      // accel_*_nv12: the layout is made of their scalars
static const LayoutRules YUV_ARGS = {"yuv", "u_offset", YUV_YUY2, yuv_extent};          // accel_*_yuv
static const LayoutRules SITED_ARGS = {"yuv", "u_offset", YUV_NV12, yuv_extent};        // accel_*_yuv_sited, and the overlay

static accel_yuv_layout nv12_layout(int h, int w, size_t pitch, size_t uv_offset, size_t frame_bytes, int colour)
{
    return {YUV_NV12, colour, h, w, pitch, 0, uv_offset, 0, frame_bytes};
}

static YuvLayout kernel_layout(const accel_yuv_layout& y)
{
    return {y.format, y.colour, y.h, y.w, y.pitch, y.pitch_c, y.u_offset, y.v_offset, y.frame_bytes};
}

// the bytes n frames occupy: the last one ends with its extent
static size_t frames_bytes(int n, const accel_yuv_layout& y, const LayoutRules& r)
{
    return (size_t)(n - 1) * y.frame_bytes + r.extent(y);
}

// Layout and siting of YUV frames, checked before anything is enqueued: every message names the argument at fault, as the caller's signature
// names it.  `dev`: the address the kernel will read if the caller's pointer is device memory, else NULL (host bytes are uploaded into an aligned
// buffer).
static int yuv_layout_args(const char* fn, const LayoutRules& r, const void* yuv, int n, const accel_yuv_layout* lay, int siting, const void* dev)
{
    const int lim = 32768;
    static const char* const names[4] = {"I420", "P010", "YUY2", "NV12"};
    if (!yuv) return fail(ACCEL_ERR_ARG, "%s: %s is NULL", fn, r.src);
    if (!lay) return fail(ACCEL_ERR_ARG, "%s: layout is NULL", fn);
    if (siting < 0 || siting > 3) return fail(ACCEL_ERR_ARG, "%s: siting = %d, must be 0 (replicate), 1 (left), 2 (centre) or 3 (topleft)", fn, siting);
    const accel_yuv_layout& y = *lay;
    if (n < 1) return fail(ACCEL_ERR_ARG, "%s: n = %d, must be >= 1", fn, n);
    if (y.format < 0 || y.format > r.max_format)
        return fail(ACCEL_ERR_ARG, "%s: format = %d, must be 0 (I420), 1 (P010)%s", fn, y.format, r.max_format == YUV_NV12 ? ", 2 (YUY2) or 3 (NV12)" : " or 2 (YUY2)");
    const char* name = names[y.format];
    if (y.colour < 0 || y.colour > 3)
        return fail(ACCEL_ERR_ARG, "%s: colour = %d, must be in 0 .. 3 (BT.601 limited / full, BT.709 limited / full)", fn, y.colour);
    const bool even_h = y.format != YUV_YUY2, words = y.format == YUV_P010 || y.format == YUV_YUY2;
    if (y.h < 1 || y.h > lim || (even_h && y.h % 2)) return fail(ACCEL_ERR_ARG, "%s: h = %d, must be %sin 1 .. %d for %s", fn, y.h, even_h ? "even and " : "", lim, name);
    if (y.w < 1 || y.w > lim || y.w % 2) return fail(ACCEL_ERR_ARG, "%s: w = %d, must be even and in 1 .. %d for %s", fn, y.w, lim, name);
    const size_t row = words ? (size_t)2 * y.w : (size_t)y.w;
    if (y.pitch < row) return fail(ACCEL_ERR_ARG, "%s: pitch = %zu bytes, a row of w = %d %s pixels has %zu", fn, y.pitch, y.w, name, row);
    if (y.pitch > ((size_t)1 << 40)) return fail(ACCEL_ERR_ARG, "%s: pitch = %zu bytes is not a row pitch", fn, y.pitch);
    const size_t luma_end = (size_t)y.h * y.pitch;
    if (y.format == YUV_I420) {
        if (y.pitch_c < (size_t)y.w / 2) return fail(ACCEL_ERR_ARG, "%s: pitch_c = %zu bytes, a chroma row of w = %d I420 pixels has %d", fn, y.pitch_c, y.w, y.w / 2);
        if (y.pitch_c > ((size_t)1 << 40)) return fail(ACCEL_ERR_ARG, "%s: pitch_c = %zu bytes is not a row pitch", fn, y.pitch_c);
    } else {
        if (y.pitch_c) return fail(ACCEL_ERR_ARG, "%s: pitch_c = %zu, but %s has no such field: it must be 0", fn, y.pitch_c, name);
        if (y.v_offset) return fail(ACCEL_ERR_ARG, "%s: v_offset = %zu, but %s has no such field: it must be 0", fn, y.v_offset, name);
        if (y.format == YUV_YUY2 && y.u_offset) return fail(ACCEL_ERR_ARG, "%s: u_offset = %zu, but YUY2 has no such field: it must be 0", fn, y.u_offset);
    }
    if (y.format != YUV_YUY2 && (y.u_offset < luma_end || y.u_offset > ((size_t)1 << 60)))
        return fail(ACCEL_ERR_ARG, "%s: %s = %zu bytes, the luma plane of h x pitch = %d x %zu ends at %zu", fn, r.chroma, y.u_offset, y.h, y.pitch, luma_end);
    if (y.format == YUV_I420 && (y.v_offset < luma_end || y.v_offset > ((size_t)1 << 60)))
        return fail(ACCEL_ERR_ARG, "%s: v_offset = %zu bytes, the luma plane of h x pitch = %d x %zu ends at %zu", fn, y.v_offset, y.h, y.pitch, luma_end);
    if (y.frame_bytes < r.extent(y))
        return fail(ACCEL_ERR_ARG, "%s: frame_bytes = %zu, the last plane of a frame ends at %zu", fn, y.frame_bytes, r.extent(y));
    if (y.frame_bytes > ((size_t)1 << 61) / (size_t)n) return fail(ACCEL_ERR_ARG, "%s: n x frame_bytes = %d x %zu bytes is not a buffer size", fn, n, y.frame_bytes);
    if (y.format == YUV_P010) {       // every 16-bit word is read as one
        if (y.pitch % 2) return fail(ACCEL_ERR_ARG, "%s: pitch = %zu, P010 words are 2-byte aligned: it must be even", fn, y.pitch);
        if (y.u_offset % 2) return fail(ACCEL_ERR_ARG, "%s: u_offset = %zu, P010 words are 2-byte aligned: it must be even", fn, y.u_offset);
        if (y.frame_bytes % 2) return fail(ACCEL_ERR_ARG, "%s: frame_bytes = %zu, P010 words are 2-byte aligned: it must be even", fn, y.frame_bytes);
        if (reinterpret_cast<uintptr_t>(dev) % 2) return fail(ACCEL_ERR_ARG, "%s: %s = %p, P010 words are 2-byte aligned: a device address must be even", fn, r.src, dev);
    }
    return 0;
}

static int frame_yuv_args(const char* fn, const LayoutRules& r, const void* yuv, int n, const accel_yuv_layout* lay, int siting, const void* dev,
                          const double* means_bgr, int out_h, int out_w, double step, int H, int W)
{
    if (int rc = yuv_layout_args(fn, r, yuv, n, lay, siting, dev)) return rc;
    if (!means_bgr) return fail(ACCEL_ERR_ARG, "%s: means_bgr is NULL", fn);
    return frame_resize_args(fn, lay->h, lay->w, out_h, out_w, step, H, W);
}

// the `launch(src, dst, stream)` of the YUV routes into the image tensor (`lay` is read at the launch: after the checks)
static auto frames_yuv_launch(int n, const accel_yuv_layout* lay, int siting, const double* means_bgr, int out_h, int out_w, double step, int H, int W)
{
    return [=](const unsigned char* src, float* dst, hipStream_t st) {
        return launch_frames_yuv(src, n, kernel_layout(*lay), siting, means_bgr, out_h, out_w, step, H, W, dst, st);
    };
}

// and their `launch(src, dst, dst_pitch, stream)` into BGR bytes
static auto yuv_to_bgr_launch(int n, const accel_yuv_layout* lay, int siting)
{
    return [=](const unsigned char* src, unsigned char* dst, size_t dst_pitch, hipStream_t st) {
        return launch_yuv_to_bgr(src, n, kernel_layout(*lay), siting, dst, dst_pitch, st);
    };
}

extern "C" int accel_frame_nv12(accel_ctx* ctx, const uint8_t* nv12, int n, int h, int w, size_t pitch, size_t uv_offset, size_t frame_bytes, int colour,
                                const double* means_bgr, int out_h, int out_w, double step, int H, int W, float* out)
{
    const char* fn = "accel_frame_nv12";
    const accel_yuv_layout lay = nv12_layout(h, w, pitch, uv_offset, frame_bytes, colour);
    if (!ctx || !out) return fail(ACCEL_ERR_ARG, "accel_frame_nv12: NULL argument");
    if (int rc = frame_yuv_args(fn, NV12_ARGS, nv12, n, &lay, 0, nullptr, means_bgr, out_h, out_w, step, H, W)) return rc;
    return frames_to_host(fn, ctx, nv12, frames_bytes(n, lay, NV12_ARGS), n, H, W, out, frames_yuv_launch(n, &lay, 0, means_bgr, out_h, out_w, step, H, W));
}

extern "C" int accel_nv12_to_bgr(accel_ctx* ctx, const uint8_t* nv12, int n, int h, int w, size_t pitch, size_t uv_offset, size_t frame_bytes, int colour,
                                 uint8_t* bgr_out, size_t out_pitch, int on_device)
{
    const char* fn = "accel_nv12_to_bgr";
    const accel_yuv_layout lay = nv12_layout(h, w, pitch, uv_offset, frame_bytes, colour);
    if (!ctx) return fail(ACCEL_ERR_ARG, "accel_nv12_to_bgr: NULL argument");
    if (int rc = yuv_layout_args(fn, NV12_ARGS, nv12, n, &lay, 0, nullptr)) return rc;
    return bgr_rows(fn, ctx, nv12, frames_bytes(n, lay, NV12_ARGS), n, h, w, bgr_out, out_pitch, on_device, yuv_to_bgr_launch(n, &lay, 0));
}

extern "C" int accel_model_write_nv12(accel_model* m, const char* buf, const uint8_t* nv12, int n, int h, int w, size_t pitch, size_t uv_offset,
                                      size_t frame_bytes, int colour, const double* means_bgr, int out_h, int out_w, double step, int H, int W,
                                      int src_on_device)
{
    const char* fn = "accel_model_write_nv12";
    const accel_yuv_layout lay = nv12_layout(h, w, pitch, uv_offset, frame_bytes, colour);
    if (!m || !buf) return fail(ACCEL_ERR_ARG, "accel_model_write_nv12: NULL argument");
    if (int rc = frame_yuv_args(fn, NV12_ARGS, nv12, n, &lay, 0, nullptr, means_bgr, out_h, out_w, step, H, W)) return rc;
    return write_frames(fn, m, buf, n, H, W, nv12, frames_bytes(n, lay, NV12_ARGS), src_on_device,
                        frames_yuv_launch(n, &lay, 0, means_bgr, out_h, out_w, step, H, W));
}

extern "C" int accel_model_commit_nv12(accel_model* m, const char* buf, int n, int h, int w, size_t pitch, size_t uv_offset, size_t frame_bytes, int colour,
                                       const double* means_bgr, int out_h, int out_w, double step, int H, int W)
{
    const char* fn = "accel_model_commit_nv12";
    const accel_yuv_layout lay = nv12_layout(h, w, pitch, uv_offset, frame_bytes, colour);
    if (!m || !buf) return fail(ACCEL_ERR_ARG, "accel_model_commit_nv12: NULL argument");
    return commit_frames(fn, m, buf, n, H, W, "(n - 1) x frame_bytes + uv_offset + h/2 x pitch", [&](const void* dev, size_t* need) {
        *need = frames_bytes(n, lay, NV12_ARGS);
        return frame_yuv_args(fn, NV12_ARGS, dev, n, &lay, 0, dev, means_bgr, out_h, out_w, step, H, W);
    }, frames_yuv_launch(n, &lay, 0, means_bgr, out_h, out_w, step, H, W));
}

extern "C" int accel_frame_yuv(accel_ctx* ctx, const uint8_t* yuv, int n, const accel_yuv_layout* layout, const double* means_bgr, int out_h, int out_w,
                               double step, int H, int W, float* out)
{
    const char* fn = "accel_frame_yuv";
    if (!ctx || !out) return fail(ACCEL_ERR_ARG, "accel_frame_yuv: NULL argument");
    if (int rc = frame_yuv_args(fn, YUV_ARGS, yuv, n, layout, 0, nullptr, means_bgr, out_h, out_w, step, H, W)) return rc;
    return frames_to_host(fn, ctx, yuv, frames_bytes(n, *layout, YUV_ARGS), n, H, W, out, frames_yuv_launch(n, layout, 0, means_bgr, out_h, out_w, step, H, W));
}

extern "C" int accel_yuv_to_bgr(accel_ctx* ctx, const uint8_t* yuv, int n, const accel_yuv_layout* layout, uint8_t* bgr_out, size_t out_pitch, int on_device)
{
    const char* fn = "accel_yuv_to_bgr";
    if (!ctx) return fail(ACCEL_ERR_ARG, "accel_yuv_to_bgr: NULL argument");
    if (int rc = yuv_layout_args(fn, YUV_ARGS, yuv, n, layout, 0, on_device ? yuv : nullptr)) return rc;
    return bgr_rows(fn, ctx, yuv, frames_bytes(n, *layout, YUV_ARGS), n, layout->h, layout->w, bgr_out, out_pitch, on_device, yuv_to_bgr_launch(n, layout, 0));
}

extern "C" int accel_model_write_yuv(accel_model* m, const char* buf, const uint8_t* yuv, int n, const accel_yuv_layout* layout, const double* means_bgr,
                                     int out_h, int out_w, double step, int H, int W, int src_on_device)
{
    const char* fn = "accel_model_write_yuv";
    if (!m || !buf) return fail(ACCEL_ERR_ARG, "accel_model_write_yuv: NULL argument");
    if (int rc = frame_yuv_args(fn, YUV_ARGS, yuv, n, layout, 0, src_on_device ? yuv : nullptr, means_bgr, out_h, out_w, step, H, W)) return rc;
    return write_frames(fn, m, buf, n, H, W, yuv, frames_bytes(n, *layout, YUV_ARGS), src_on_device,
                        frames_yuv_launch(n, layout, 0, means_bgr, out_h, out_w, step, H, W));
}

extern "C" int accel_model_commit_yuv(accel_model* m, const char* buf, int n, const accel_yuv_layout* layout, const double* means_bgr, int out_h,
                                      int out_w, double step, int H, int W)
{
    const char* fn = "accel_model_commit_yuv";
    if (!m || !buf) return fail(ACCEL_ERR_ARG, "accel_model_commit_yuv: NULL argument");
    return commit_frames(fn, m, buf, n, H, W, "(n - 1) x frame_bytes + the extent of a frame", [&](const void* dev, size_t* need) {
        if (int rc = frame_yuv_args(fn, YUV_ARGS, dev, n, layout, 0, dev, means_bgr, out_h, out_w, step, H, W)) return rc;
        *need = frames_bytes(n, *layout, YUV_ARGS);
        return 0;
    }, frames_yuv_launch(n, layout, 0, means_bgr, out_h, out_w, step, H, W));
}

// the same frames, and NV12 as format 3, with the chroma siting the caller names
extern "C" int accel_frame_yuv_sited(accel_ctx* ctx, const uint8_t* yuv, int n, const accel_yuv_layout* layout, const double* means_bgr, int out_h,
                                     int out_w, double step, int H, int W, float* out, int siting)
{
    const char* fn = "accel_frame_yuv_sited";
    if (!ctx || !out) return fail(ACCEL_ERR_ARG, "accel_frame_yuv_sited: NULL argument");
    if (int rc = frame_yuv_args(fn, SITED_ARGS, yuv, n, layout, siting, nullptr, means_bgr, out_h, out_w, step, H, W)) return rc;
    return frames_to_host(fn, ctx, yuv, frames_bytes(n, *layout, SITED_ARGS), n, H, W, out,
                          frames_yuv_launch(n, layout, siting, means_bgr, out_h, out_w, step, H, W));
}

extern "C" int accel_yuv_to_bgr_sited(accel_ctx* ctx, const uint8_t* yuv, int n, const accel_yuv_layout* layout, uint8_t* bgr_out, size_t out_pitch,
                                      int siting, int on_device)
{
    const char* fn = "accel_yuv_to_bgr_sited";
    if (!ctx) return fail(ACCEL_ERR_ARG, "accel_yuv_to_bgr_sited: NULL argument");
    if (int rc = yuv_layout_args(fn, SITED_ARGS, yuv, n, layout, siting, on_device ? yuv : nullptr)) return rc;
    return bgr_rows(fn, ctx, yuv, frames_bytes(n, *layout, SITED_ARGS), n, layout->h, layout->w, bgr_out, out_pitch, on_device,
                    yuv_to_bgr_launch(n, layout, siting));
}

extern "C" int accel_model_write_yuv_sited(accel_model* m, const char* buf, const uint8_t* yuv, int n, const accel_yuv_layout* layout,
                                           const double* means_bgr, int out_h, int out_w, double step, int H, int W, int siting, int src_on_device)
{
    const char* fn = "accel_model_write_yuv_sited";
    if (!m || !buf) return fail(ACCEL_ERR_ARG, "accel_model_write_yuv_sited: NULL argument");
    if (int rc = frame_yuv_args(fn, SITED_ARGS, yuv, n, layout, siting, src_on_device ? yuv : nullptr, means_bgr, out_h, out_w, step, H, W)) return rc;
    return write_frames(fn, m, buf, n, H, W, yuv, frames_bytes(n, *layout, SITED_ARGS), src_on_device,
                        frames_yuv_launch(n, layout, siting, means_bgr, out_h, out_w, step, H, W));
}

extern "C" int accel_model_commit_yuv_sited(accel_model* m, const char* buf, int n, const accel_yuv_layout* layout, const double* means_bgr, int out_h,
                                            int out_w, double step, int H, int W, int siting)
{
    const char* fn = "accel_model_commit_yuv_sited";
    if (!m || !buf) return fail(ACCEL_ERR_ARG, "accel_model_commit_yuv_sited: NULL argument");
    return commit_frames(fn, m, buf, n, H, W, "(n - 1) x frame_bytes + the extent of a frame", [&](const void* dev, size_t* need) {
        if (int rc = frame_yuv_args(fn, SITED_ARGS, dev, n, layout, siting, dev, means_bgr, out_h, out_w, step, H, W)) return rc;
        *need = frames_bytes(n, *layout, SITED_ARGS);
        return 0;
    }, frames_yuv_launch(n, layout, siting, means_bgr, out_h, out_w, step, H, W));
}

// ---- finished frames: labels at the source size, confusion matrix, colour image (results_u8.hip) ---------------------------------------
// Geometry shared by the three, checked before anything is enqueued: every message names the argument at fault.
static int results_args(const char* fn, int n, int H, int W, int out_h, int out_w, int h, int w)
{
    const int lim = 32768;       // the kernels index with 32-bit products of two sizes
    if (n < 1) return fail(ACCEL_ERR_ARG, "%s: n = %d, must be >= 1", fn, n);
    if (H < 1 || W < 1 || H > lim || W > lim) return fail(ACCEL_ERR_ARG, "%s: H x W = %d x %d, must be in 1 .. %d", fn, H, W, lim);
    if (h < 1 || h > lim) return fail(ACCEL_ERR_ARG, "%s: h = %d, must be in 1 .. %d", fn, h, lim);
    if (w < 1 || w > lim) return fail(ACCEL_ERR_ARG, "%s: w = %d, must be in 1 .. %d", fn, w, lim);
    if (out_h < 1 || out_h > H) return fail(ACCEL_ERR_ARG, "%s: out_h = %d, must be in 1 .. H = %d", fn, out_h, H);
    if (out_w < 1 || out_w > W) return fail(ACCEL_ERR_ARG, "%s: out_w = %d, must be in 1 .. W = %d", fn, out_w, W);
    return 0;
}

// the same for the entry points that interpolate the scores (scores_labels.hip): the class count first
static int scores_labels_args(const char* fn, int n, int ncls, int H, int W, int out_h, int out_w, int h, int w)
{
    if (ncls != 2 && ncls != 19 && ncls != 21) return fail(ACCEL_ERR_ARG, "%s: ncls = %d, the scores must have 2, 19 or 21 classes", fn, ncls);
    if (int rc = results_args(fn, n, H, W, out_h, out_w, h, w)) return rc;
    if (n > 32768) return fail(ACCEL_ERR_ARG, "%s: n = %d, must be in 1 .. 32768", fn, n);
    return 0;
}

static int pitch_arg(const char* fn, const char* name, size_t pitch, int w, int bytes_per_pixel)
{
    if (pitch < (size_t)bytes_per_pixel * w)
        return fail(ACCEL_ERR_ARG, "%s: %s = %zu bytes, a row of w = %d pixels has %zu", fn, name, pitch, w, (size_t)bytes_per_pixel * w);
    return 0;
}

static int ncls_arg(const char* fn, int ncls)
{
    if (ncls < 1 || ncls > 32) return fail(ACCEL_ERR_ARG, "%s: ncls = %d, must be in 1 .. 32", fn, ncls);
    return 0;
}

static int alpha_arg(const char* fn, int alpha)
{
    if (alpha < 0 || alpha > 256) return fail(ACCEL_ERR_ARG, "%s: alpha = %d, must be in 0 .. 256", fn, alpha);
    return 0;
}

// rows of `row` bytes, `pitch` apart on the host, tightly packed in device memory: only the bytes of the rows are written
static hipError_t rows_to_host(void* dst, size_t pitch, const void* dev, size_t row, size_t rows, hipStream_t st)
{
    if (pitch == row) return hipMemcpyAsync(dst, dev, row * rows, hipMemcpyDeviceToHost, st);
    return hipMemcpy2DAsync(dst, pitch, dev, row, row, rows, hipMemcpyDeviceToHost, st);
}

extern "C" int accel_labels_to_source(accel_ctx* ctx, const uint8_t* labels, int n, int H, int W, int out_h, int out_w, int h, int w,
                                      uint8_t* dst, size_t dst_pitch)
{
    const char* fn = "accel_labels_to_source";
    if (!ctx) return fail(ACCEL_ERR_ARG, "%s: ctx is NULL", fn);
    if (!labels) return fail(ACCEL_ERR_ARG, "%s: labels is NULL", fn);
    if (!dst) return fail(ACCEL_ERR_ARG, "%s: dst is NULL", fn);
    if (int rc = results_args(fn, n, H, W, out_h, out_w, h, w)) return rc;
    if (int rc = pitch_arg(fn, "dst_pitch", dst_pitch, w, 1)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    DevTemps t;
    const unsigned char* l = static_cast<const unsigned char*>(t.upload(labels, (size_t)n * H * W));
    unsigned char* d = static_cast<unsigned char*>(t.get((size_t)n * h * w));
    if (!l || !d) return fail(ACCEL_ERR_HIP, "%s: device allocation or upload failed", fn);
    HIP_TRY(launch_labels_source(l, n, H, W, out_h, out_w, h, w, d, (size_t)w, ctx->stream));
    HIP_TRY(rows_to_host(dst, dst_pitch, d, (size_t)w, (size_t)n * h, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int accel_labels_hist(accel_ctx* ctx, const uint8_t* labels, int n, int H, int W, int out_h, int out_w,
                                 const uint8_t* gt, int h, int w, size_t gt_pitch, int ncls, uint64_t* hist)
{
    const char* fn = "accel_labels_hist";
    if (!ctx) return fail(ACCEL_ERR_ARG, "%s: ctx is NULL", fn);
    if (!labels) return fail(ACCEL_ERR_ARG, "%s: labels is NULL", fn);
    if (!gt) return fail(ACCEL_ERR_ARG, "%s: gt is NULL", fn);
    if (!hist) return fail(ACCEL_ERR_ARG, "%s: hist is NULL", fn);
    if (int rc = results_args(fn, n, H, W, out_h, out_w, h, w)) return rc;
    if (int rc = pitch_arg(fn, "gt_pitch", gt_pitch, w, 1)) return rc;
    if (int rc = ncls_arg(fn, ncls)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    DevTemps t;
    const size_t hb = (size_t)ncls * ncls * sizeof(uint64_t);
    const unsigned char* l = static_cast<const unsigned char*>(t.upload(labels, (size_t)n * H * W));
    const unsigned char* g = static_cast<const unsigned char*>(t.upload(gt, (size_t)n * h * gt_pitch));
    unsigned long long* d = static_cast<unsigned long long*>(t.upload(hist, hb));
    if (!l || !g || !d) return fail(ACCEL_ERR_HIP, "%s: device allocation or upload failed", fn);
    HIP_TRY(launch_labels_hist(l, n, H, W, out_h, out_w, g, h, w, gt_pitch, ncls, d, ctx->stream));
    HIP_TRY(hipMemcpyAsync(hist, d, hb, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int accel_labels_colour(accel_ctx* ctx, const uint8_t* labels, int n, int H, int W, int out_h, int out_w, int h, int w,
                                   const uint8_t* palette_rgb, int rgb_order, const uint8_t* frame_bgr, size_t frame_pitch, int alpha,
                                   uint8_t* dst, size_t dst_pitch)
{
    const char* fn = "accel_labels_colour";
    if (!ctx) return fail(ACCEL_ERR_ARG, "%s: ctx is NULL", fn);
    if (!labels) return fail(ACCEL_ERR_ARG, "%s: labels is NULL", fn);
    if (!palette_rgb) return fail(ACCEL_ERR_ARG, "%s: palette_rgb is NULL", fn);
    if (!dst) return fail(ACCEL_ERR_ARG, "%s: dst is NULL", fn);
    if (int rc = results_args(fn, n, H, W, out_h, out_w, h, w)) return rc;
    if (int rc = pitch_arg(fn, "dst_pitch", dst_pitch, w, 3)) return rc;
    if (frame_bgr) if (int rc = pitch_arg(fn, "frame_pitch", frame_pitch, w, 3)) return rc;
    if (int rc = alpha_arg(fn, alpha)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    DevTemps t;
    const unsigned char* l = static_cast<const unsigned char*>(t.upload(labels, (size_t)n * H * W));
    const unsigned char* f = frame_bgr ? static_cast<const unsigned char*>(t.upload(frame_bgr, (size_t)n * h * frame_pitch)) : nullptr;
    unsigned char* d = static_cast<unsigned char*>(t.get((size_t)n * h * w * 3));
    if (!l || !d || (frame_bgr && !f)) return fail(ACCEL_ERR_HIP, "%s: device allocation or upload failed", fn);
    HIP_TRY(launch_labels_colour(l, n, H, W, out_h, out_w, h, w, palette_rgb, rgb_order, f, frame_pitch, alpha, d, (size_t)3 * w, ctx->stream));
    HIP_TRY(rows_to_host(dst, dst_pitch, d, (size_t)3 * w, (size_t)n * h, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

// the model's label maps: the `labels` buffer and the shape the plans write it in
static int model_labels(const char* fn, accel_model* m, int n, const unsigned char** labels)
{
    auto it = m->pbufs.find("labels");
    if (it == m->pbufs.end() || m->labels_h < 1 || m->labels_w < 1)
        return fail(ACCEL_ERR_ARG, "%s: this model has no `labels` buffer of a known shape (no plan with a score_tail op is bound)", fn);
    if (n < 1) return fail(ACCEL_ERR_ARG, "%s: n = %d, must be >= 1", fn, n);
    if (n > m->labels_n || (size_t)n * m->labels_h * m->labels_w > it->second.bytes)
        return fail(ACCEL_ERR_ARG, "%s: n = %d, the model is bound for a batch of %d", fn, n, m->labels_n);
    *labels = static_cast<const unsigned char*>(it->second.ptr);
    return 0;
}

// the model's scores: the `logits` buffer and the shape the plans write it in
static int model_scores(const char* fn, accel_model* m, int n, const float** scores, int* ncls, int* H, int* W)
{
    auto it = m->pbufs.find("logits");
    if (it == m->pbufs.end() || m->logits_h < 1 || m->logits_w < 1)
        return fail(ACCEL_ERR_ARG, "%s: this model has no `logits` buffer of a known shape (no plan with a score_tail op is bound)", fn);
    if (n < 1) return fail(ACCEL_ERR_ARG, "%s: n = %d, must be >= 1", fn, n);
    *ncls = m->logits_ncls; *H = m->logits_h; *W = m->logits_w;
    if (n > m->logits_n || (size_t)n * *ncls * *H * *W * sizeof(float) > it->second.bytes)
        return fail(ACCEL_ERR_ARG, "%s: n = %d, the model is bound for a batch of %d", fn, n, m->logits_n);
    *scores = static_cast<const float*>(it->second.ptr);
    return 0;
}

// Where the label maps of a model-level result come from, in one of two kinds:
//   NEAREST        the `labels` buffer the plans write -- n maps of H x W whose valid region out_h x out_w the consumer takes to the source size by
//                  the nearest rule: the consumer's geometry is the map's own H, W, out_h, out_w
//   INTERPOLATED   the argmax of the `logits` interpolated to the source size h x w (launch_scores_labels), which enqueue() writes into the model's
//                  scratch as tight rows: the consumer's geometry is the identity h, w, h, w
// An entry point uses it in this order: find (the buffer, n against the bound batch), geometry (INTERPOLATED: the class count of the scores first),
// its own checks, reserve (the scratch), and enqueue in front of the consumer's kernel -- or write alone, for the labels themselves.
struct LabelSource {
    enum Kind { NEAREST, INTERPOLATED };
    accel_model* m;
    Kind kind;
    const unsigned char* maps = nullptr;            // what the consumer reads (INTERPOLATED: from reserve() on) ...
    int n = 0, H = 0, W = 0, out_h = 0, out_w = 0, h = 0, w = 0;       // ... and the geometry it reads it in
    const float* scores = nullptr;                  // INTERPOLATED: the logits
    int ncls = 0, bH = 0, bW = 0, b_out_h = 0, b_out_w = 0;            // the buffer's own shape and valid region

    LabelSource(accel_model* m_, Kind kind_) : m(m_), kind(kind_) {}

    int find(const char* fn, int n_)
    {
        n = n_;
        if (kind == INTERPOLATED) return model_scores(fn, m, n, &scores, &ncls, &bH, &bW);
        bH = m->labels_h; bW = m->labels_w;
        return model_labels(fn, m, n, &maps);
    }
    int geometry(const char* fn, int out_h_, int out_w_, int h_, int w_)
    {
        b_out_h = out_h_; b_out_w = out_w_; h = h_; w = w_;
        const bool own = kind == NEAREST;
        H = own ? bH : h; W = own ? bW : w; out_h = own ? out_h_ : h; out_w = own ? out_w_ : w;
        return own ? results_args(fn, n, bH, bW, out_h_, out_w_, h, w) : scores_labels_args(fn, n, ncls, bH, bW, out_h_, out_w_, h, w);
    }
    int reserve()
    {
        if (kind == NEAREST) return 0;
        if (int rc = m->interp_labels.reserve(m->ctx->device, (size_t)n * h * w)) return rc;
        maps = m->interp_labels.ptr;
        return 0;
    }
    // the labels at the source size straight into `dst`
    hipError_t write(unsigned char* dst, size_t pitch, hipStream_t st) const
    {
        if (kind == NEAREST) return launch_labels_source(maps, n, bH, bW, b_out_h, b_out_w, h, w, dst, pitch, st);
        return launch_scores_labels(scores, n, ncls, bH, bW, b_out_h, b_out_w, h, w, dst, pitch, st);
    }
    hipError_t enqueue(hipStream_t st) const { return kind == NEAREST ? hipSuccess : write(m->interp_labels.ptr, (size_t)w, st); }
};

// Where the `rows` rows of `row` bytes of a result go.  Into the caller's device memory at the caller's pitch: `launch(dst, pitch, stream)` is enqueued
// and that is all.  To the host: the kernel writes tight rows into the staging buffer, they are copied `dst_pitch` apart, and the call waits.
template <class Launch>
static int result_rows(accel_model* m, uint8_t* dst, size_t dst_pitch, int dst_on_device, size_t row, size_t rows, Launch launch)
{
    hipStream_t st = m->ctx->stream;
    if (dst_on_device) {
        HIP_TRY(launch(dst, dst_pitch, st));
        return 0;
    }
    if (int rc = m->stage_out.reserve(m->ctx->device, row * rows)) return rc;
    HIP_TRY(launch(m->stage_out.ptr, row, st));
    HIP_TRY(rows_to_host(dst, dst_pitch, m->stage_out.ptr, row, rows, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// the model's confusion matrix for counts of `ncls` classes: refused while it holds counts of another number of classes, allocated and zeroed on first use
static int model_hist(const char* fn, accel_model* m, int ncls, unsigned long long** hist)
{
    if (m->hist_ncls && m->hist_ncls != ncls)
        return fail(ACCEL_ERR_ARG, "%s: ncls = %d, the accumulator holds counts of %d classes since its last clear", fn, ncls, m->hist_ncls);
    HIP_TRY(hipSetDevice(m->ctx->device));
    if (!m->hist) {
        HIP_TRY(hipMalloc((void**)&m->hist, 32 * 32 * sizeof(unsigned long long)));
        HIP_TRY(hipMemsetAsync(m->hist, 0, 32 * 32 * sizeof(unsigned long long), m->ctx->stream));
    }
    *hist = m->hist;
    return 0;
}

// the labels themselves: written straight to the destination (or the staging buffer), never through the scratch
static int model_labels_out(const char* fn, accel_model* m, LabelSource::Kind kind, int n, int out_h, int out_w, int h, int w, uint8_t* dst, size_t dst_pitch,
                            int dst_on_device)
{
    if (!m) return fail(ACCEL_ERR_ARG, "%s: m is NULL", fn);
    if (!dst) return fail(ACCEL_ERR_ARG, "%s: dst is NULL", fn);
    LabelSource src(m, kind);
    if (int rc = src.find(fn, n)) return rc;
    if (int rc = src.geometry(fn, out_h, out_w, h, w)) return rc;
    if (int rc = pitch_arg(fn, "dst_pitch", dst_pitch, w, 1)) return rc;
    if (dst_on_device) HIP_TRY(hipSetDevice(m->ctx->device));
    return result_rows(m, dst, dst_pitch, dst_on_device, (size_t)w, (size_t)n * h, [&](unsigned char* d, size_t pitch, hipStream_t st) {
        return src.write(d, pitch, st);
    });
}

extern "C" int accel_model_labels_to_source(accel_model* m, int n, int out_h, int out_w, int h, int w, uint8_t* dst, size_t dst_pitch, int dst_on_device)
{
    return model_labels_out("accel_model_labels_to_source", m, LabelSource::NEAREST, n, out_h, out_w, h, w, dst, dst_pitch, dst_on_device);
}

extern "C" int accel_model_scores_labels(accel_model* m, int n, int out_h, int out_w, int h, int w, uint8_t* dst, size_t dst_pitch, int dst_on_device)
{
    return model_labels_out("accel_model_scores_labels", m, LabelSource::INTERPOLATED, n, out_h, out_w, h, w, dst, dst_pitch, dst_on_device);
}

static int model_hist_add(const char* fn, accel_model* m, LabelSource::Kind kind, const uint8_t* gt, int n, int h, int w, size_t gt_pitch, int out_h,
                          int out_w, int ncls, int gt_on_device)
{
    if (!m) return fail(ACCEL_ERR_ARG, "%s: m is NULL", fn);
    if (!gt) return fail(ACCEL_ERR_ARG, "%s: gt is NULL", fn);
    LabelSource src(m, kind);
    if (int rc = src.find(fn, n)) return rc;
    if (int rc = src.geometry(fn, out_h, out_w, h, w)) return rc;
    if (int rc = pitch_arg(fn, "gt_pitch", gt_pitch, w, 1)) return rc;
    if (int rc = ncls_arg(fn, ncls)) return rc;
    unsigned long long* hist = nullptr;
    if (int rc = model_hist(fn, m, ncls, &hist)) return rc;
    hipStream_t st = m->ctx->stream;
    if (int rc = src.reserve()) return rc;
    const unsigned char* g = gt;
    if (!gt_on_device) if (int rc = stage_in(m, gt, (size_t)n * h * gt_pitch, &g)) return rc;
    HIP_TRY(src.enqueue(st));
    HIP_TRY(launch_labels_hist(src.maps, n, src.H, src.W, src.out_h, src.out_w, g, h, w, gt_pitch, ncls, hist, st));
    m->hist_ncls = ncls;
    return 0;
}

extern "C" int accel_model_hist_add(accel_model* m, const uint8_t* gt, int n, int h, int w, size_t gt_pitch, int out_h, int out_w, int ncls, int gt_on_device)
{
    return model_hist_add("accel_model_hist_add", m, LabelSource::NEAREST, gt, n, h, w, gt_pitch, out_h, out_w, ncls, gt_on_device);
}

extern "C" int accel_model_scores_hist_add(accel_model* m, const uint8_t* gt, int n, int h, int w, size_t gt_pitch, int out_h, int out_w, int ncls,
                                           int gt_on_device)
{
    return model_hist_add("accel_model_scores_hist_add", m, LabelSource::INTERPOLATED, gt, n, h, w, gt_pitch, out_h, out_w, ncls, gt_on_device);
}

extern "C" int accel_model_hist_read(accel_model* m, uint64_t* out, int ncls, int clear)
{
    const char* fn = "accel_model_hist_read";
    if (!m) return fail(ACCEL_ERR_ARG, "%s: m is NULL", fn);
    if (!out) return fail(ACCEL_ERR_ARG, "%s: out is NULL", fn);
    if (int rc = ncls_arg(fn, ncls)) return rc;
    const size_t hb = (size_t)ncls * ncls * sizeof(uint64_t);
    if (!m->hist_ncls) { memset(out, 0, hb); return 0; }      // nothing added since the last clear: any class count may be asked for
    unsigned long long* hist = nullptr;
    if (int rc = model_hist(fn, m, ncls, &hist)) return rc;
    hipStream_t st = m->ctx->stream;
    HIP_TRY(hipMemcpyAsync(out, hist, hb, hipMemcpyDeviceToHost, st));
    if (clear) {
        HIP_TRY(hipMemsetAsync(hist, 0, 32 * 32 * sizeof(unsigned long long), st));
        m->hist_ncls = 0;
    }
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

static int model_colour(const char* fn, accel_model* m, LabelSource::Kind kind, int n, int out_h, int out_w, int h, int w, const uint8_t* palette_rgb,
                        int rgb_order, const uint8_t* frame_bgr, size_t frame_pitch, int alpha, int frame_on_device, uint8_t* dst, size_t dst_pitch,
                        int dst_on_device)
{
    if (!m) return fail(ACCEL_ERR_ARG, "%s: m is NULL", fn);
    if (!palette_rgb) return fail(ACCEL_ERR_ARG, "%s: palette_rgb is NULL", fn);
    if (!dst) return fail(ACCEL_ERR_ARG, "%s: dst is NULL", fn);
    LabelSource src(m, kind);
    if (int rc = src.find(fn, n)) return rc;
    if (int rc = src.geometry(fn, out_h, out_w, h, w)) return rc;
    if (int rc = pitch_arg(fn, "dst_pitch", dst_pitch, w, 3)) return rc;
    if (frame_bgr) if (int rc = pitch_arg(fn, "frame_pitch", frame_pitch, w, 3)) return rc;
    if (int rc = alpha_arg(fn, alpha)) return rc;
    if (int rc = src.reserve()) return rc;
    const unsigned char* f = frame_bgr;
    if (frame_bgr && !frame_on_device) if (int rc = stage_in(m, frame_bgr, (size_t)n * h * frame_pitch, &f)) return rc;
    return result_rows(m, dst, dst_pitch, dst_on_device, (size_t)3 * w, (size_t)n * h, [&](unsigned char* d, size_t pitch, hipStream_t st) {
        const hipError_t e = src.enqueue(st);
        if (e != hipSuccess) return e;
        return launch_labels_colour(src.maps, n, src.H, src.W, src.out_h, src.out_w, h, w, palette_rgb, rgb_order, f, frame_pitch, alpha, d, pitch, st);
    });
}

extern "C" int accel_model_labels_colour(accel_model* m, int n, int out_h, int out_w, int h, int w, const uint8_t* palette_rgb, int rgb_order,
                                         const uint8_t* frame_bgr, size_t frame_pitch, int alpha, int frame_on_device,
                                         uint8_t* dst, size_t dst_pitch, int dst_on_device)
{
    return model_colour("accel_model_labels_colour", m, LabelSource::NEAREST, n, out_h, out_w, h, w, palette_rgb, rgb_order, frame_bgr, frame_pitch, alpha,
                        frame_on_device, dst, dst_pitch, dst_on_device);
}

extern "C" int accel_model_scores_colour(accel_model* m, int n, int out_h, int out_w, int h, int w, const uint8_t* palette_rgb, int rgb_order,
                                         const uint8_t* frame_bgr, size_t frame_pitch, int alpha, int frame_on_device,
                                         uint8_t* dst, size_t dst_pitch, int dst_on_device)
{
    return model_colour("accel_model_scores_colour", m, LabelSource::INTERPOLATED, n, out_h, out_w, h, w, palette_rgb, rgb_order, frame_bgr, frame_pitch, alpha,
                        frame_on_device, dst, dst_pitch, dst_on_device);
}

// ---- confidence of finished frames: of the stored scores (nearest) and of the interpolated ones, with their labels (confidence.hip) ---------
// The outputs of a call are one ConfOut (kernels.h): five pointers and four pitches, on the host or on the device; `labels` exists in the
// interpolated forms only and is NULL in the nearest ones.
// What the four entry points share, checked before anything is enqueued: every message names the argument at fault.
static int confidence_args(const char* fn, bool interp, int n, int ncls, int H, int W, int out_h, int out_w, int h, int w, const ConfOut& o)
{
    if (!o.labels && !o.conf && !o.margin && !o.second && !o.hist)
        return fail(ACCEL_ERR_ARG, "%s: %sconf, margin, second and hist are all NULL: nothing to compute", fn, interp ? "labels, " : "");
    if (ncls != 2 && ncls != 19 && ncls != 21) return fail(ACCEL_ERR_ARG, "%s: ncls = %d, must be 2, 19 or 21", fn, ncls);
    if (int rc = results_args(fn, n, H, W, out_h, out_w, h, w)) return rc;
    if (n > 32768) return fail(ACCEL_ERR_ARG, "%s: n = %d, must be in 1 .. 32768", fn, n);
    if (o.labels) if (int rc = pitch_arg(fn, "labels_pitch", o.labels_pitch, w, 1)) return rc;
    if (o.conf) if (int rc = pitch_arg(fn, "conf_pitch", o.conf_pitch, w, 1)) return rc;
    if (o.margin) {
        if (int rc = pitch_arg(fn, "margin_pitch", o.margin_pitch, w, 4)) return rc;
        if (o.margin_pitch % 4) return fail(ACCEL_ERR_ARG, "%s: margin_pitch = %zu bytes, must be a multiple of 4", fn, o.margin_pitch);
    }
    if (o.second) if (int rc = pitch_arg(fn, "second_pitch", o.second_pitch, w, 1)) return rc;
    return 0;
}

// a staging buffer carved into parts, each 256-byte aligned: take(bytes) -> the offset of the next part
struct Carved {
    size_t bytes = 0;
    size_t take(size_t b) { const size_t at = bytes; bytes += (b + 255) / 256 * 256; return at; }
};

// the device side of a call whose results go to the host: tight rows (labels, conf, second: n * h * w bytes; margin: 4 times that; hist: n * 256
// words) for the outputs `host` asks for
struct ConfStage : Carved {
    size_t labels = 0, conf = 0, second = 0, margin = 0, hist = 0;
    ConfStage(int n, int h, int w, const ConfOut& host)
    {
        const size_t px = (size_t)n * h * w;
        if (host.labels) labels = take(px);
        if (host.conf) conf = take(px);
        if (host.second) second = take(px);
        if (host.margin) margin = take(px * 4);
        if (host.hist) hist = take((size_t)n * 256 * sizeof(uint64_t));
    }
    ConfOut at(unsigned char* base, int w, const ConfOut& host) const
    {
        return {host.labels ? base + labels : nullptr, (size_t)w, host.conf ? base + conf : nullptr, (size_t)w,
                host.margin ? reinterpret_cast<float*>(base + margin) : nullptr, (size_t)4 * w, host.second ? base + second : nullptr, (size_t)w,
                host.hist ? reinterpret_cast<unsigned long long*>(base + hist) : nullptr};
    }
};

// the kernel into the stage at `base`, its results copied to the host; the call waits
static int confidence_to_host(const float* scores, unsigned char* base, const ConfStage& cs, int n, int ncls, int H, int W, int out_h, int out_w, int h, int w,
                              int is_prob, bool interp, const ConfOut& host, hipStream_t st)
{
    const ConfOut d = cs.at(base, w, host);
    const size_t rows = (size_t)n * h;
    HIP_TRY(launch_confidence(scores, n, ncls, H, W, out_h, out_w, h, w, is_prob, interp, d, st));
    if (host.labels) HIP_TRY(rows_to_host(host.labels, host.labels_pitch, d.labels, (size_t)w, rows, st));
    if (host.conf) HIP_TRY(rows_to_host(host.conf, host.conf_pitch, d.conf, (size_t)w, rows, st));
    if (host.second) HIP_TRY(rows_to_host(host.second, host.second_pitch, d.second, (size_t)w, rows, st));
    if (host.margin) HIP_TRY(rows_to_host(host.margin, host.margin_pitch, d.margin, (size_t)4 * w, rows, st));
    if (host.hist) HIP_TRY(hipMemcpyAsync(host.hist, d.hist, (size_t)n * 256 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

static int ctx_confidence(const char* fn, accel_ctx* ctx, const float* scores, bool interp, int n, int ncls, int H, int W, int out_h, int out_w, int h, int w,
                          int is_prob, const ConfOut& o)
{
    if (!ctx) return fail(ACCEL_ERR_ARG, "%s: ctx is NULL", fn);
    if (!scores) return fail(ACCEL_ERR_ARG, "%s: scores is NULL", fn);
    if (int rc = confidence_args(fn, interp, n, ncls, H, W, out_h, out_w, h, w, o)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    DevTemps t;
    const ConfStage cs(n, h, w, o);
    const float* s = static_cast<const float*>(t.upload(scores, (size_t)n * ncls * H * W * sizeof(float)));
    unsigned char* base = static_cast<unsigned char*>(t.get(cs.bytes));
    if (!s || !base) return fail(ACCEL_ERR_HIP, "%s: device allocation or upload failed", fn);
    return confidence_to_host(s, base, cs, n, ncls, H, W, out_h, out_w, h, w, is_prob, interp, o, ctx->stream);
}

static int model_confidence(const char* fn, accel_model* m, bool interp, int n, int out_h, int out_w, int h, int w, int is_prob, const ConfOut& o,
                            int dst_on_device)
{
    if (!m) return fail(ACCEL_ERR_ARG, "%s: m is NULL", fn);
    const float* scores = nullptr;
    int ncls = 0, H = 0, W = 0;
    if (int rc = model_scores(fn, m, n, &scores, &ncls, &H, &W)) return rc;
    if (int rc = confidence_args(fn, interp, n, ncls, H, W, out_h, out_w, h, w, o)) return rc;
    hipStream_t st = m->ctx->stream;
    if (dst_on_device) {
        if (reinterpret_cast<uintptr_t>(o.margin) % 4) return fail(ACCEL_ERR_ARG, "%s: margin = %p, device floats must be 4-byte aligned", fn, (void*)o.margin);
        if (reinterpret_cast<uintptr_t>(o.hist) % 8) return fail(ACCEL_ERR_ARG, "%s: hist = %p, device words must be 8-byte aligned", fn, (void*)o.hist);
        HIP_TRY(hipSetDevice(m->ctx->device));
        HIP_TRY(launch_confidence(scores, n, ncls, H, W, out_h, out_w, h, w, is_prob, interp, o, st));
        return 0;
    }
    const ConfStage cs(n, h, w, o);
    if (int rc = m->stage_out.reserve(m->ctx->device, cs.bytes)) return rc;
    return confidence_to_host(scores, m->stage_out.ptr, cs, n, ncls, H, W, out_h, out_w, h, w, is_prob, interp, o, st);
}

extern "C" int accel_scores_confidence(accel_ctx* ctx, const float* scores, int n, int ncls, int H, int W, int out_h, int out_w, int h, int w, int is_prob,
                                       uint8_t* conf, size_t conf_pitch, float* margin, size_t margin_pitch, uint8_t* second, size_t second_pitch,
                                       uint64_t* hist)
{
    return ctx_confidence("accel_scores_confidence", ctx, scores, false, n, ncls, H, W, out_h, out_w, h, w, is_prob,
                          {nullptr, 0, conf, conf_pitch, margin, margin_pitch, second, second_pitch, reinterpret_cast<unsigned long long*>(hist)});
}

extern "C" int accel_model_confidence(accel_model* m, int n, int out_h, int out_w, int h, int w, int is_prob, uint8_t* conf, size_t conf_pitch,
                                      float* margin, size_t margin_pitch, uint8_t* second, size_t second_pitch, uint64_t* hist, int dst_on_device)
{
    return model_confidence("accel_model_confidence", m, false, n, out_h, out_w, h, w, is_prob,
                            {nullptr, 0, conf, conf_pitch, margin, margin_pitch, second, second_pitch, reinterpret_cast<unsigned long long*>(hist)},
                            dst_on_device);
}

extern "C" int accel_scores_confidence_interp(accel_ctx* ctx, const float* scores, int n, int ncls, int H, int W, int out_h, int out_w, int h, int w,
                                              int is_prob, uint8_t* labels, size_t labels_pitch, uint8_t* conf, size_t conf_pitch, float* margin,
                                              size_t margin_pitch, uint8_t* second, size_t second_pitch, uint64_t* hist)
{
    return ctx_confidence("accel_scores_confidence_interp", ctx, scores, true, n, ncls, H, W, out_h, out_w, h, w, is_prob,
                          {labels, labels_pitch, conf, conf_pitch, margin, margin_pitch, second, second_pitch, reinterpret_cast<unsigned long long*>(hist)});
}

extern "C" int accel_model_confidence_interp(accel_model* m, int n, int out_h, int out_w, int h, int w, int is_prob, uint8_t* labels, size_t labels_pitch,
                                             uint8_t* conf, size_t conf_pitch, float* margin, size_t margin_pitch, uint8_t* second, size_t second_pitch,
                                             uint64_t* hist, int dst_on_device)
{
    return model_confidence("accel_model_confidence_interp", m, true, n, out_h, out_w, h, w, is_prob,
                            {labels, labels_pitch, conf, conf_pitch, margin, margin_pitch, second, second_pitch, reinterpret_cast<unsigned long long*>(hist)},
                            dst_on_device);
}

// ---- labels from interpolated scores (scores_labels.hip) ------------------------------------------------------------------------------------
extern "C" int accel_scores_labels(accel_ctx* ctx, const float* scores, int n, int ncls, int H, int W, int out_h, int out_w, int h, int w,
                                   uint8_t* dst, size_t dst_pitch)
{
    const char* fn = "accel_scores_labels";
    if (!ctx) return fail(ACCEL_ERR_ARG, "%s: ctx is NULL", fn);
    if (!scores) return fail(ACCEL_ERR_ARG, "%s: scores is NULL", fn);
    if (!dst) return fail(ACCEL_ERR_ARG, "%s: dst is NULL", fn);
    if (int rc = scores_labels_args(fn, n, ncls, H, W, out_h, out_w, h, w)) return rc;
    if (int rc = pitch_arg(fn, "dst_pitch", dst_pitch, w, 1)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    DevTemps t;
    const float* s = static_cast<const float*>(t.upload(scores, (size_t)n * ncls * H * W * sizeof(float)));
    unsigned char* d = static_cast<unsigned char*>(t.get((size_t)n * h * w));
    if (!s || !d) return fail(ACCEL_ERR_HIP, "%s: device allocation or upload failed", fn);
    HIP_TRY(launch_scores_labels(s, n, ncls, H, W, out_h, out_w, h, w, d, (size_t)w, ctx->stream));
    HIP_TRY(rows_to_host(dst, dst_pitch, d, (size_t)w, (size_t)n * h, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

// ---- the overlay in the frame's own format (overlay_yuv.hip) ---------------------------------------------------------------------------------
// What the three entry points share besides the geometry, checked before anything is enqueued: every message names the argument at fault.  The
// layout by the rules of the frame routes (format 3 = NV12; its `colour` is not looked at: the table holds the colours), `frame_dev` / `dst_dev`:
// the addresses the kernel will use if the caller's pointers are device memory, else NULL.
static int overlay_args(const char* fn, int n, const accel_yuv_layout* layout, const uint16_t* palette_ycc, int alpha, const void* frame,
                        const void* frame_dev, const void* dst, const void* dst_dev, accel_yuv_layout* lay)
{
    if (!frame) return fail(ACCEL_ERR_ARG, "%s: frame is NULL", fn);
    if (!dst) return fail(ACCEL_ERR_ARG, "%s: dst is NULL", fn);
    if (!palette_ycc) return fail(ACCEL_ERR_ARG, "%s: palette_ycc is NULL", fn);
    if (!layout) return fail(ACCEL_ERR_ARG, "%s: layout is NULL", fn);
    *lay = *layout;
    lay->colour = 0;
    if (int rc = yuv_layout_args(fn, SITED_ARGS, frame, n, lay, 0, nullptr)) return rc;
    if (lay->format == YUV_P010 && reinterpret_cast<uintptr_t>(frame_dev) % 2)
        return fail(ACCEL_ERR_ARG, "%s: frame = %p, P010 words are 2-byte aligned: a device address must be even", fn, frame_dev);
    if (lay->format == YUV_P010 && reinterpret_cast<uintptr_t>(dst_dev) % 2)
        return fail(ACCEL_ERR_ARG, "%s: dst = %p, P010 words are 2-byte aligned: a device address must be even", fn, dst_dev);
    if (int rc = alpha_arg(fn, alpha)) return rc;
    const int top = lay->format == YUV_P010 ? 1023 : 255;
    for (int i = 0; i < 768; ++i)
        if (palette_ycc[i] > top)
            return fail(ACCEL_ERR_ARG, "%s: palette_ycc[%d] = %d (label %d, %s), must be in 0 .. %d for this format", fn, i, (int)palette_ycc[i], i / 3,
                        i % 3 == 0 ? "Y" : i % 3 == 1 ? "Cb" : "Cr", top);
    if (frame_dev && dst_dev && frame_dev != dst_dev) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(frame_dev), b = reinterpret_cast<uintptr_t>(dst_dev), bytes = (size_t)n * lay->frame_bytes;
        if (a < b + bytes && b < a + bytes)
            return fail(ACCEL_ERR_ARG, "%s: dst = %p overlaps frame = %p (n x frame_bytes = %zu bytes each): dst must be the frame itself (in place) "
                                       "or disjoint from it", fn, dst_dev, frame_dev, (size_t)bytes);
    }
    return 0;
}

extern "C" int accel_labels_overlay_yuv(accel_ctx* ctx, const uint8_t* labels, int n, int H, int W, int out_h, int out_w, const accel_yuv_layout* layout,
                                        const uint16_t* palette_ycc, int alpha, const uint8_t* frame, uint8_t* dst)
{
    const char* fn = "accel_labels_overlay_yuv";
    if (!ctx) return fail(ACCEL_ERR_ARG, "%s: ctx is NULL", fn);
    if (!labels) return fail(ACCEL_ERR_ARG, "%s: labels is NULL", fn);
    accel_yuv_layout lay;
    if (int rc = overlay_args(fn, n, layout, palette_ycc, alpha, frame, nullptr, dst, nullptr, &lay)) return rc;
    if (int rc = results_args(fn, n, H, W, out_h, out_w, lay.h, lay.w)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    // host in, host out: the destination starts as a copy of the frame, so the bytes that are not samples are the input's
    DevTemps t;
    const size_t bytes = frames_bytes(n, lay, SITED_ARGS);
    const unsigned char* l = static_cast<const unsigned char*>(t.upload(labels, (size_t)n * H * W));
    const unsigned char* s = static_cast<const unsigned char*>(t.upload(frame, bytes));
    unsigned char* d = static_cast<unsigned char*>(t.upload(frame, bytes));
    if (!l || !s || !d) return fail(ACCEL_ERR_HIP, "%s: device allocation or upload failed", fn);
    HIP_TRY(launch_overlay_yuv(l, n, H, W, out_h, out_w, kernel_layout(lay), palette_ycc, alpha, s, d, ctx->stream));
    HIP_TRY(hipMemcpyAsync(dst, d, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

// The frames blended with `lab` (n maps of H x W, valid out_h x out_w) wherever source and destination are.  Device to device: one kernel, and
// that is all.  A host destination: the frame is brought into the staging buffer (its gaps with it), blended there in place, copied out, and the
// call waits.  A host frame into device memory goes through the input staging buffer.
template <class Labels>
static int overlay_frames(accel_model* m, int n, const accel_yuv_layout& lay, const uint16_t* palette_ycc, int alpha, const uint8_t* frame,
                          int frame_on_device, uint8_t* dst, int dst_on_device, Labels labels)
{
    hipStream_t st = m->ctx->stream;
    const YuvLayout y = kernel_layout(lay);
    const size_t bytes = frames_bytes(n, lay, SITED_ARGS);
    HIP_TRY(hipSetDevice(m->ctx->device));
    if (dst_on_device) {
        const unsigned char* f = frame;
        if (!frame_on_device) if (int rc = stage_in(m, frame, bytes, &f)) return rc;
        return labels(f, dst, y, st);
    }
    if (int rc = m->stage_out.reserve(m->ctx->device, bytes)) return rc;
    unsigned char* d = m->stage_out.ptr;
    if (frame_on_device) HIP_TRY(launch_copy_bytes(frame, d, bytes, st));
    else HIP_TRY(hipMemcpyAsync(d, frame, bytes, hipMemcpyHostToDevice, st));
    if (int rc = labels(d, d, y, st)) return rc;
    HIP_TRY(hipMemcpyAsync(dst, d, bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

static int model_overlay_yuv(const char* fn, accel_model* m, LabelSource::Kind kind, int n, int out_h, int out_w, const accel_yuv_layout* layout,
                             const uint16_t* palette_ycc, int alpha, const uint8_t* frame, int frame_on_device, uint8_t* dst, int dst_on_device)
{
    if (!m) return fail(ACCEL_ERR_ARG, "%s: m is NULL", fn);
    LabelSource src(m, kind);
    if (int rc = src.find(fn, n)) return rc;
    accel_yuv_layout lay;
    if (int rc = overlay_args(fn, n, layout, palette_ycc, alpha, frame, frame_on_device ? frame : nullptr, dst, dst_on_device ? dst : nullptr, &lay)) return rc;
    if (int rc = src.geometry(fn, out_h, out_w, lay.h, lay.w)) return rc;
    if (int rc = src.reserve()) return rc;
    return overlay_frames(m, n, lay, palette_ycc, alpha, frame, frame_on_device, dst, dst_on_device,
                          [&](const unsigned char* f, unsigned char* d, const YuvLayout& y, hipStream_t st) -> int {
        HIP_TRY(src.enqueue(st));
        HIP_TRY(launch_overlay_yuv(src.maps, n, src.H, src.W, src.out_h, src.out_w, y, palette_ycc, alpha, f, d, st));
        return 0;
    });
}

extern "C" int accel_model_labels_overlay_yuv(accel_model* m, int n, int out_h, int out_w, const accel_yuv_layout* layout, const uint16_t* palette_ycc,
                                              int alpha, const uint8_t* frame, int frame_on_device, uint8_t* dst, int dst_on_device)
{
    return model_overlay_yuv("accel_model_labels_overlay_yuv", m, LabelSource::NEAREST, n, out_h, out_w, layout, palette_ycc, alpha, frame,
                             frame_on_device, dst, dst_on_device);
}

extern "C" int accel_model_scores_overlay_yuv(accel_model* m, int n, int out_h, int out_w, const accel_yuv_layout* layout, const uint16_t* palette_ycc,
                                              int alpha, const uint8_t* frame, int frame_on_device, uint8_t* dst, int dst_on_device)
{
    return model_overlay_yuv("accel_model_scores_overlay_yuv", m, LabelSource::INTERPOLATED, n, out_h, out_w, layout, palette_ycc, alpha, frame,
                             frame_on_device, dst, dst_on_device);
}

// ---- frame change: the measure behind content-adaptive key frames (frame_change.hip) ------------------------------------------------------------
// What the two entry points share, checked before anything is enqueued: every message names the argument at fault.  `any_out`: at least one output
// is given (the model level always writes its current signature).
static int frame_change_args(const char* fn, int n, int H, int W, int out_h, int out_w, int cell, int level_q, bool has_key, bool any_out,
                             const void* changed, const void* sad, const void* mask, size_t mask_pitch)
{
    const int lim = 32768;
    if (n < 1 || n > lim) return fail(ACCEL_ERR_ARG, "%s: n = %d, must be in 1 .. %d", fn, n, lim);
    if (H < 1 || W < 1 || H > lim || W > lim) return fail(ACCEL_ERR_ARG, "%s: H x W = %d x %d, must be in 1 .. %d", fn, H, W, lim);
    if (out_h < 1 || out_h > H) return fail(ACCEL_ERR_ARG, "%s: out_h = %d, must be in 1 .. H = %d", fn, out_h, H);
    if (out_w < 1 || out_w > W) return fail(ACCEL_ERR_ARG, "%s: out_w = %d, must be in 1 .. W = %d", fn, out_w, W);
    if (cell != 8 && cell != 16 && cell != 32 && cell != 64) return fail(ACCEL_ERR_ARG, "%s: cell = %d, must be 8, 16, 32 or 64", fn, cell);
    if (level_q < 0 || level_q > 32768) return fail(ACCEL_ERR_ARG, "%s: level_q = %d, must be in 0 .. 32768 (64 per grey level)", fn, level_q);
    if (!any_out && !changed && !sad && !mask) return fail(ACCEL_ERR_ARG, "%s: sig_out, changed, sad and mask are all NULL: nothing to compute", fn);
    if (!has_key && (changed || sad || mask))
        return fail(ACCEL_ERR_ARG, "%s: sig_key is NULL, but %s is asked for: a comparison needs the signature of a key frame", fn,
                    changed ? "changed" : sad ? "sad" : "mask");
    const int gw = (out_w + cell - 1) / cell;
    if (mask && mask_pitch < (size_t)gw) return fail(ACCEL_ERR_ARG, "%s: mask_pitch = %zu bytes, a row of gw = %d cells has %d", fn, mask_pitch, gw, gw);
    return 0;
}

// the device side of a comparison whose results go to the host: changed (n words), sad (n words), mask (tight rows of gw bytes), each part 256-byte aligned
struct ChangeStage : Carved {
    size_t changed = 0, sad = 0, mask = 0;
    ChangeStage(int n, int gh, int gw, bool c, bool s, bool m)
    {
        if (c) changed = take((size_t)n * sizeof(uint32_t));
        if (s) sad = take((size_t)n * sizeof(uint64_t));
        if (m) mask = take((size_t)n * gh * gw);
    }
};

// the comparison of `img` with `key` into the stage at `base`, its results copied to the host; the call waits
static int frame_change_to_host(const float* img, const int* key, unsigned char* base, const ChangeStage& cs, int n, int H, int W, int out_h, int out_w,
                                int cell, int level_q, int* sig_dev, uint32_t* changed, uint64_t* sad, uint8_t* mask, size_t mask_pitch, hipStream_t st)
{
    const int gh = (out_h + cell - 1) / cell, gw = (out_w + cell - 1) / cell;
    unsigned* dc = changed ? reinterpret_cast<unsigned*>(base + cs.changed) : nullptr;
    unsigned long long* ds = sad ? reinterpret_cast<unsigned long long*>(base + cs.sad) : nullptr;
    unsigned char* dm = mask ? base + cs.mask : nullptr;
    HIP_TRY(launch_frame_change(img, key, n, H, W, out_h, out_w, cell, level_q, sig_dev, dc, ds, dm, (size_t)gw, st));
    if (changed) HIP_TRY(hipMemcpyAsync(changed, dc, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (sad) HIP_TRY(hipMemcpyAsync(sad, ds, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (mask) HIP_TRY(rows_to_host(mask, mask_pitch, dm, (size_t)gw, (size_t)n * gh, st));
    return 0;
}

extern "C" int accel_frame_change(accel_ctx* ctx, const float* img, const int32_t* sig_key, int n, int H, int W, int out_h, int out_w, int cell, int level_q,
                                  int32_t* sig_out, uint32_t* changed, uint64_t* sad, uint8_t* mask, size_t mask_pitch)
{
    const char* fn = "accel_frame_change";
    if (!ctx) return fail(ACCEL_ERR_ARG, "%s: ctx is NULL", fn);
    if (!img) return fail(ACCEL_ERR_ARG, "%s: img is NULL", fn);
    if (int rc = frame_change_args(fn, n, H, W, out_h, out_w, cell, level_q, sig_key != nullptr, sig_out != nullptr, changed, sad, mask, mask_pitch)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const int gh = (out_h + cell - 1) / cell, gw = (out_w + cell - 1) / cell;
    const size_t sb = (size_t)n * gh * gw * sizeof(int32_t);
    DevTemps t;
    const ChangeStage cs(n, gh, gw, changed, sad, mask);
    const float* x = static_cast<const float*>(t.upload(img, (size_t)n * 3 * H * W * sizeof(float)));
    const int* key = sig_key ? static_cast<const int*>(t.upload(sig_key, sb)) : nullptr;
    int* sig = sig_out ? static_cast<int*>(t.get(sb)) : nullptr;
    unsigned char* base = static_cast<unsigned char*>(t.get(cs.bytes));
    if (!x || !base || (sig_key && !key) || (sig_out && !sig)) return fail(ACCEL_ERR_HIP, "%s: device allocation or upload failed", fn);
    if (int rc = frame_change_to_host(x, key, base, cs, n, H, W, out_h, out_w, cell, level_q, sig, changed, sad, mask, mask_pitch, ctx->stream)) return rc;
    if (sig_out) HIP_TRY(hipMemcpyAsync(sig_out, sig, sb, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int accel_model_frame_change(accel_model* m, const char* buf, int n, int out_h, int out_w, int cell, int level_q, uint32_t* changed,
                                        uint64_t* sad, uint8_t* mask, size_t mask_pitch, int dst_on_device, int* compared)
{
    const char* fn = "accel_model_frame_change";
    if (!m) return fail(ACCEL_ERR_ARG, "%s: m is NULL", fn);
    if (!buf) return fail(ACCEL_ERR_ARG, "%s: buf is NULL", fn);
    if (!compared) return fail(ACCEL_ERR_ARG, "%s: compared is NULL", fn);
    auto it = m->pbufs.find(buf);
    if (it == m->pbufs.end()) return fail(ACCEL_ERR_ARG, "%s: unknown buffer '%s'", fn, buf);
    const DevBuf& b = it->second;
    if (!b.slot || b.readers != b.prep_readers || b.img_h < 1 || b.img_w < 1)
        return fail(ACCEL_ERR_ARG, "%s: '%s' is not an image input of the finalized plans (only buffers that prep_rgb / prep_flow alone read hold frames)", fn, buf);
    const int H = b.img_h, W = b.img_w;
    if (int rc = frame_change_args(fn, n, H, W, out_h, out_w, cell, level_q, true, true, changed, sad, mask, mask_pitch)) return rc;
    if ((size_t)n * 3 * H * W * sizeof(float) > b.bytes)
        return fail(ACCEL_ERR_ARG, "%s: n = %d, the model is bound for a batch of %zu", fn, n, b.bytes / ((size_t)3 * H * W * sizeof(float)));
    if (dst_on_device) {
        if (reinterpret_cast<uintptr_t>(changed) % 4) return fail(ACCEL_ERR_ARG, "%s: changed = %p, device words must be 4-byte aligned", fn, (void*)changed);
        if (reinterpret_cast<uintptr_t>(sad) % 8) return fail(ACCEL_ERR_ARG, "%s: sad = %p, device words must be 8-byte aligned", fn, (void*)sad);
    }
    const int gh = (out_h + cell - 1) / cell, gw = (out_w + cell - 1) / cell;
    const size_t sb = (size_t)n * gh * gw * sizeof(int32_t);
    accel_model::FrameSig &cur = m->sig_cur, &kept = m->sig_kept;
    cur.n = 0;      // (whatever happens below, the old signature is gone)
    if (int rc = cur.mem.reserve(m->ctx->device, sb)) return rc;
    hipStream_t st = m->ctx->stream;
    // a bound input is read where the plans read it (the caller's frame), not the model-owned copy an earlier write left behind
    const float* img = static_cast<const float*>(b.bound ? b.bound : b.ptr);
    int* sig = reinterpret_cast<int*>(cur.mem.ptr);
    const bool cmp = kept.n == n && kept.out_h == out_h && kept.out_w == out_w && kept.cell == cell;
    const int* key = cmp ? reinterpret_cast<const int*>(kept.mem.ptr) : nullptr;
    if (!cmp || (!changed && !sad && !mask)) {
        HIP_TRY(launch_frame_change(img, nullptr, n, H, W, out_h, out_w, cell, level_q, sig, nullptr, nullptr, nullptr, 0, st));
    } else if (dst_on_device) {
        HIP_TRY(launch_frame_change(img, key, n, H, W, out_h, out_w, cell, level_q, sig, changed, reinterpret_cast<unsigned long long*>(sad), mask, mask_pitch, st));
    } else {
        const ChangeStage cs(n, gh, gw, changed, sad, mask);
        if (int rc = m->stage_out.reserve(m->ctx->device, cs.bytes)) return rc;
        if (int rc = frame_change_to_host(img, key, m->stage_out.ptr, cs, n, H, W, out_h, out_w, cell, level_q, sig, changed, sad, mask, mask_pitch, st)) return rc;
        HIP_TRY(hipStreamSynchronize(st));
    }
    cur.n = n; cur.out_h = out_h; cur.out_w = out_w; cur.cell = cell;
    *compared = cmp ? 1 : 0;
    return 0;
}

extern "C" int accel_model_frame_keep(accel_model* m)
{
    const char* fn = "accel_model_frame_keep";
    if (!m) return fail(ACCEL_ERR_ARG, "%s: m is NULL", fn);
    accel_model::FrameSig &cur = m->sig_cur, &kept = m->sig_kept;
    if (!cur.n) return fail(ACCEL_ERR_ARG, "%s: no signature has been made yet (accel_model_frame_change makes one)", fn);
    const int gh = (cur.out_h + cur.cell - 1) / cur.cell, gw = (cur.out_w + cur.cell - 1) / cur.cell;
    const size_t sb = (size_t)cur.n * gh * gw * sizeof(int32_t);
    kept.n = 0;
    if (int rc = kept.mem.reserve(m->ctx->device, sb)) return rc;
    HIP_TRY(launch_copy_bytes(cur.mem.ptr, kept.mem.ptr, sb, m->ctx->stream));
    kept.n = cur.n; kept.out_h = cur.out_h; kept.out_w = cur.out_w; kept.cell = cur.cell;
    return 0;
}

// ---- summary of finished frames: areas, coordinate sums, boxes and class transitions (labels_summary.hip) --------------------------------------
// What the three entry points share, checked before anything is enqueued: every message names the argument at fault.
static int summary_args(const char* fn, int n, int H, int W, int out_h, int out_w, int h, int w, int ncls)
{
    if (int rc = results_args(fn, n, H, W, out_h, out_w, h, w)) return rc;
    if (n > 32768) return fail(ACCEL_ERR_ARG, "%s: n = %d, must be in 1 .. 32768", fn, n);
    return ncls_arg(fn, ncls);
}

// the device side of a summary whose results go to the host: stats (n x ncls x 3 words), box (n x ncls x 4), trans (n x ncls x ncls), each part 256-byte aligned
struct SummaryStage : Carved {
    size_t stats = 0, box = 0, trans = 0, sb, bb, tb;
    SummaryStage(int n, int ncls, bool s, bool b, bool t)
        : sb((size_t)n * ncls * 3 * sizeof(uint64_t)), bb((size_t)n * ncls * 4 * sizeof(int32_t)), tb((size_t)n * ncls * ncls * sizeof(uint64_t))
    {
        if (s) stats = take(sb);
        if (b) box = take(bb);
        if (t) trans = take(tb);
        if (!bytes) bytes = 256;
    }
};

// the summary of `labels` into the stage at `base`, its results copied to the host; the caller waits
static int summary_to_host(const unsigned char* labels, int n, int H, int W, int out_h, int out_w, int h, int w, int ncls, const unsigned char* prev,
                           size_t prev_pitch, unsigned char* base, const SummaryStage& ss, uint64_t* stats, int32_t* box, uint64_t* trans, unsigned char* kept,
                           size_t kept_pitch, hipStream_t st)
{
    unsigned long long* ds = stats ? reinterpret_cast<unsigned long long*>(base + ss.stats) : nullptr;
    int* db = box ? reinterpret_cast<int*>(base + ss.box) : nullptr;
    unsigned long long* dt = trans ? reinterpret_cast<unsigned long long*>(base + ss.trans) : nullptr;
    HIP_TRY(launch_labels_summary(labels, n, H, W, out_h, out_w, h, w, ncls, prev, prev_pitch, ds, db, dt, kept, kept_pitch, st));
    if (stats) HIP_TRY(hipMemcpyAsync(stats, ds, ss.sb, hipMemcpyDeviceToHost, st));
    if (box) HIP_TRY(hipMemcpyAsync(box, db, ss.bb, hipMemcpyDeviceToHost, st));
    if (trans) HIP_TRY(hipMemcpyAsync(trans, dt, ss.tb, hipMemcpyDeviceToHost, st));
    return 0;
}

extern "C" int accel_labels_summary(accel_ctx* ctx, const uint8_t* labels, int n, int H, int W, int out_h, int out_w, int h, int w, int ncls,
                                    const uint8_t* prev, size_t prev_pitch, uint64_t* stats, int32_t* box, uint64_t* trans, uint8_t* kept_out,
                                    size_t kept_pitch)
{
    const char* fn = "accel_labels_summary";
    if (!ctx) return fail(ACCEL_ERR_ARG, "%s: ctx is NULL", fn);
    if (!labels) return fail(ACCEL_ERR_ARG, "%s: labels is NULL", fn);
    if (int rc = summary_args(fn, n, H, W, out_h, out_w, h, w, ncls)) return rc;
    if (!stats && !box && !trans && !kept_out) return fail(ACCEL_ERR_ARG, "%s: stats, box, trans and kept_out are all NULL: nothing to compute", fn);
    if (trans && !prev) return fail(ACCEL_ERR_ARG, "%s: prev is NULL, but trans is asked for: transitions need the previous frame's labels", fn);
    if (prev) if (int rc = pitch_arg(fn, "prev_pitch", prev_pitch, w, 1)) return rc;
    if (kept_out) if (int rc = pitch_arg(fn, "kept_pitch", kept_pitch, w, 1)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    DevTemps t;
    const SummaryStage ss(n, ncls, stats, box, trans);
    const unsigned char* l = static_cast<const unsigned char*>(t.upload(labels, (size_t)n * H * W));
    const unsigned char* p = prev && trans ? static_cast<const unsigned char*>(t.upload(prev, (size_t)n * h * prev_pitch)) : nullptr;
    unsigned char* k = kept_out ? static_cast<unsigned char*>(t.get((size_t)n * h * w)) : nullptr;
    unsigned char* base = static_cast<unsigned char*>(t.get(ss.bytes));
    if (!l || !base || (prev && trans && !p) || (kept_out && !k)) return fail(ACCEL_ERR_HIP, "%s: device allocation or upload failed", fn);
    if (int rc = summary_to_host(l, n, H, W, out_h, out_w, h, w, ncls, p, prev_pitch, base, ss, stats, box, trans, k, (size_t)w, ctx->stream)) return rc;
    if (kept_out) HIP_TRY(rows_to_host(kept_out, kept_pitch, k, (size_t)w, (size_t)n * h, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

// what the two model-level forms share: the summary of the n maps of `src` at the source size, tracked against the model's kept map if asked
static int model_summary(const char* fn, accel_model* m, LabelSource::Kind kind, int n, int out_h, int out_w, int h, int w, int ncls, int track,
                         uint64_t* stats, int32_t* box, uint64_t* trans, int dst_on_device, int* compared)
{
    if (!m) return fail(ACCEL_ERR_ARG, "%s: m is NULL", fn);
    LabelSource src(m, kind);
    if (int rc = src.find(fn, n)) return rc;
    if (int rc = src.geometry(fn, out_h, out_w, h, w)) return rc;
    if (n > 32768) return fail(ACCEL_ERR_ARG, "%s: n = %d, must be in 1 .. 32768", fn, n);
    if (int rc = ncls_arg(fn, ncls)) return rc;
    if (!compared) return fail(ACCEL_ERR_ARG, "%s: compared is NULL", fn);
    if (!stats && !box && !trans) return fail(ACCEL_ERR_ARG, "%s: stats, box and trans are all NULL: nothing to compute", fn);
    if (trans && !track) return fail(ACCEL_ERR_ARG, "%s: trans is asked for with track = 0: transitions need the kept map", fn);
    if (dst_on_device) {
        if (reinterpret_cast<uintptr_t>(stats) % 8) return fail(ACCEL_ERR_ARG, "%s: stats = %p, device words must be 8-byte aligned", fn, (void*)stats);
        if (reinterpret_cast<uintptr_t>(trans) % 8) return fail(ACCEL_ERR_ARG, "%s: trans = %p, device words must be 8-byte aligned", fn, (void*)trans);
        if (reinterpret_cast<uintptr_t>(box) % 4) return fail(ACCEL_ERR_ARG, "%s: box = %p, device words must be 4-byte aligned", fn, (void*)box);
    }
    hipStream_t st = m->ctx->stream;
    HIP_TRY(hipSetDevice(m->ctx->device));
    if (int rc = src.reserve()) return rc;
    HIP_TRY(src.enqueue(st));
    accel_model::KeptLabels& k = m->kept_labels;
    bool cmp = false;
    unsigned char* kept = nullptr;
    if (track) {
        cmp = k.n == n && k.h == h && k.w == w && k.ncls == ncls;       // (then the map is large enough: nothing is reallocated)
        k.n = 0;      // (whatever happens below, the old map is gone)
        if (int rc = k.mem.reserve(m->ctx->device, (size_t)n * h * w)) return rc;
        kept = k.mem.ptr;
    }
    if (!cmp) trans = nullptr;
    const unsigned char* prev = trans ? kept : nullptr;
    if (dst_on_device) {
        HIP_TRY(launch_labels_summary(src.maps, n, src.H, src.W, src.out_h, src.out_w, h, w, ncls, prev, (size_t)w,
                                      reinterpret_cast<unsigned long long*>(stats), box, reinterpret_cast<unsigned long long*>(trans), kept, (size_t)w, st));
    } else {
        const SummaryStage ss(n, ncls, stats, box, trans);
        if (int rc = m->stage_out.reserve(m->ctx->device, ss.bytes)) return rc;
        if (int rc = summary_to_host(src.maps, n, src.H, src.W, src.out_h, src.out_w, h, w, ncls, prev, (size_t)w, m->stage_out.ptr, ss, stats, box, trans,
                                     kept, (size_t)w, st))
            return rc;
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (track) { k.n = n; k.h = h; k.w = w; k.ncls = ncls; }
    *compared = cmp ? 1 : 0;
    return 0;
}

extern "C" int accel_model_labels_summary(accel_model* m, int n, int out_h, int out_w, int h, int w, int ncls, int track, uint64_t* stats, int32_t* box,
                                          uint64_t* trans, int dst_on_device, int* compared)
{
    return model_summary("accel_model_labels_summary", m, LabelSource::NEAREST, n, out_h, out_w, h, w, ncls, track, stats, box, trans, dst_on_device, compared);
}

extern "C" int accel_model_scores_summary(accel_model* m, int n, int out_h, int out_w, int h, int w, int ncls, int track, uint64_t* stats, int32_t* box,
                                          uint64_t* trans, int dst_on_device, int* compared)
{
    return model_summary("accel_model_scores_summary", m, LabelSource::INTERPOLATED, n, out_h, out_w, h, w, ncls, track, stats, box, trans, dst_on_device,
                         compared);
}

extern "C" int accel_model_labels_forget(accel_model* m)
{
    if (!m) return fail(ACCEL_ERR_ARG, "accel_model_labels_forget: m is NULL");
    m->kept_labels.n = 0;      // (the memory stays for the next clip)
    return 0;
}

// ---- connected components of finished frames: objects per class (labels_components.hip) -------------------------------------------------------------
// What the three entry points share beyond the geometry, checked before anything is enqueued: every message names the argument at fault.
static int components_args(const char* fn, int n, int w, int ncls, int connectivity, int min_area, int max_components, const int32_t* count,
                           const int32_t* ids, size_t ids_pitch)
{
    if (n > 32768) return fail(ACCEL_ERR_ARG, "%s: n = %d, must be in 1 .. 32768", fn, n);
    if (int rc = ncls_arg(fn, ncls)) return rc;
    if (connectivity != 4 && connectivity != 8) return fail(ACCEL_ERR_ARG, "%s: connectivity = %d, must be 4 or 8", fn, connectivity);
    if (min_area < 1) return fail(ACCEL_ERR_ARG, "%s: min_area = %d, must be >= 1", fn, min_area);
    if (max_components < 1 || max_components > 65536)
        return fail(ACCEL_ERR_ARG, "%s: max_components = %d, must be in 1 .. 65536", fn, max_components);
    if (!count) return fail(ACCEL_ERR_ARG, "%s: count is NULL", fn);
    if (ids) {
        if (int rc = pitch_arg(fn, "ids_pitch", ids_pitch, w, 4)) return rc;
        if (ids_pitch % 4) return fail(ACCEL_ERR_ARG, "%s: ids_pitch = %zu bytes, must be a multiple of 4", fn, ids_pitch);
    }
    return 0;
}

// the device side of a components call whose results go to the host: count (n words), comp (n x max_components x 8), sums (n x max_components x 2
// words of 8 bytes), ids (n * h tight rows of w words), each part 256-byte aligned
struct ComponentsStage : Carved {
    size_t count = 0, comp = 0, sums = 0, ids = 0, nb, cb, sb, ib;
    ComponentsStage(int n, int h, int w, int max_components, bool c, bool s, bool i)
        : nb((size_t)n * sizeof(int32_t)), cb((size_t)n * max_components * 8 * sizeof(int32_t)), sb((size_t)n * max_components * 2 * sizeof(uint64_t)),
          ib((size_t)n * h * w * sizeof(int32_t))
    {
        count = take(nb);
        if (c) comp = take(cb);
        if (s) sums = take(sb);
        if (i) ids = take(ib);
    }
};

// the scratch of launch_labels_components for n frames of h x w, carved out of one allocation: parent, area, blocks
struct ComponentsScratch : Carved {
    size_t parent, area, blocks;
    ComponentsScratch(int n, int h, int w)
    {
        parent = take((size_t)n * h * w * sizeof(int32_t));
        area = take((size_t)n * h * w * sizeof(int32_t));
        blocks = take((size_t)n * labels_components_chunks(h, w) * sizeof(int32_t));
    }
};

struct ComponentsOut { int32_t* count; int32_t* comp; uint64_t* sums; int32_t* ids; size_t ids_pitch; };

static hipError_t components_launch(const unsigned char* labels, int n, int H, int W, int out_h, int out_w, int h, int w, int ncls, int connectivity,
                                    int min_area, int max_components, unsigned char* scratch, const ComponentsOut& o, hipStream_t st)
{
    const ComponentsScratch cs(n, h, w);
    return launch_labels_components(labels, n, H, W, out_h, out_w, h, w, ncls, connectivity, min_area, max_components,
                                    reinterpret_cast<int*>(scratch + cs.parent), reinterpret_cast<int*>(scratch + cs.area),
                                    reinterpret_cast<int*>(scratch + cs.blocks), o.count, o.comp, reinterpret_cast<unsigned long long*>(o.sums), o.ids,
                                    o.ids_pitch, st);
}

// the components of `labels` into the stage at `base`, the results copied to the host; the caller waits
static int components_to_host(const unsigned char* labels, int n, int H, int W, int out_h, int out_w, int h, int w, int ncls, int connectivity,
                              int min_area, int max_components, unsigned char* scratch, unsigned char* base, const ComponentsStage& cs,
                              const ComponentsOut& host, hipStream_t st)
{
    const ComponentsOut dev = {reinterpret_cast<int32_t*>(base + cs.count), host.comp ? reinterpret_cast<int32_t*>(base + cs.comp) : nullptr,
                               host.sums ? reinterpret_cast<uint64_t*>(base + cs.sums) : nullptr,
                               host.ids ? reinterpret_cast<int32_t*>(base + cs.ids) : nullptr, (size_t)4 * w};
    HIP_TRY(components_launch(labels, n, H, W, out_h, out_w, h, w, ncls, connectivity, min_area, max_components, scratch, dev, st));
    HIP_TRY(hipMemcpyAsync(host.count, dev.count, cs.nb, hipMemcpyDeviceToHost, st));
    if (host.comp) HIP_TRY(hipMemcpyAsync(host.comp, dev.comp, cs.cb, hipMemcpyDeviceToHost, st));
    if (host.sums) HIP_TRY(hipMemcpyAsync(host.sums, dev.sums, cs.sb, hipMemcpyDeviceToHost, st));
    if (host.ids) HIP_TRY(rows_to_host(host.ids, host.ids_pitch, dev.ids, (size_t)4 * w, (size_t)n * h, st));
    return 0;
}

extern "C" int accel_labels_components(accel_ctx* ctx, const uint8_t* labels, int n, int H, int W, int out_h, int out_w, int h, int w, int ncls,
                                       int connectivity, int min_area, int max_components, int32_t* count, int32_t* comp, uint64_t* sums, int32_t* ids,
                                       size_t ids_pitch)
{
    const char* fn = "accel_labels_components";
    if (!ctx) return fail(ACCEL_ERR_ARG, "%s: ctx is NULL", fn);
    if (!labels) return fail(ACCEL_ERR_ARG, "%s: labels is NULL", fn);
    if (int rc = results_args(fn, n, H, W, out_h, out_w, h, w)) return rc;
    if (int rc = components_args(fn, n, w, ncls, connectivity, min_area, max_components, count, ids, ids_pitch)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    DevTemps t;
    const ComponentsStage cs(n, h, w, max_components, comp, sums, ids);
    const ComponentsScratch sc(n, h, w);
    const unsigned char* l = static_cast<const unsigned char*>(t.upload(labels, (size_t)n * H * W));
    unsigned char* scratch = static_cast<unsigned char*>(t.get(sc.bytes));
    unsigned char* base = static_cast<unsigned char*>(t.get(cs.bytes));
    if (!l || !scratch || !base) return fail(ACCEL_ERR_HIP, "%s: device allocation or upload failed", fn);
    const ComponentsOut host = {count, comp, sums, ids, ids_pitch};
    if (int rc = components_to_host(l, n, H, W, out_h, out_w, h, w, ncls, connectivity, min_area, max_components, scratch, base, cs, host, ctx->stream))
        return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

// what the two model-level forms share: the components of the n maps of `src` at the source size
static int model_components(const char* fn, accel_model* m, LabelSource::Kind kind, int n, int out_h, int out_w, int h, int w, int ncls, int connectivity,
                            int min_area, int max_components, int dst_on_device, int32_t* count, int32_t* comp, uint64_t* sums, int32_t* ids,
                            size_t ids_pitch)
{
    if (!m) return fail(ACCEL_ERR_ARG, "%s: m is NULL", fn);
    LabelSource src(m, kind);
    if (int rc = src.find(fn, n)) return rc;
    if (int rc = src.geometry(fn, out_h, out_w, h, w)) return rc;
    if (int rc = components_args(fn, n, w, ncls, connectivity, min_area, max_components, count, ids, ids_pitch)) return rc;
    if (kind == LabelSource::INTERPOLATED && ncls != src.ncls)
        return fail(ACCEL_ERR_ARG, "%s: ncls = %d, the scores have %d classes", fn, ncls, src.ncls);
    if (dst_on_device) {
        if (reinterpret_cast<uintptr_t>(count) % 4) return fail(ACCEL_ERR_ARG, "%s: count = %p, device words must be 4-byte aligned", fn, (void*)count);
        if (reinterpret_cast<uintptr_t>(comp) % 4) return fail(ACCEL_ERR_ARG, "%s: comp = %p, device words must be 4-byte aligned", fn, (void*)comp);
        if (reinterpret_cast<uintptr_t>(sums) % 8) return fail(ACCEL_ERR_ARG, "%s: sums = %p, device words must be 8-byte aligned", fn, (void*)sums);
        if (reinterpret_cast<uintptr_t>(ids) % 4) return fail(ACCEL_ERR_ARG, "%s: ids = %p, device words must be 4-byte aligned", fn, (void*)ids);
    }
    hipStream_t st = m->ctx->stream;
    HIP_TRY(hipSetDevice(m->ctx->device));
    if (int rc = src.reserve()) return rc;
    const ComponentsScratch sc(n, h, w);
    if (int rc = m->components.reserve(m->ctx->device, sc.bytes)) return rc;
    const ComponentsOut out = {count, comp, sums, ids, ids_pitch};
    if (dst_on_device) {
        HIP_TRY(src.enqueue(st));
        HIP_TRY(components_launch(src.maps, n, src.H, src.W, src.out_h, src.out_w, h, w, ncls, connectivity, min_area, max_components,
                                  m->components.ptr, out, st));
        return 0;
    }
    const ComponentsStage cs(n, h, w, max_components, comp, sums, ids);
    if (int rc = m->stage_out.reserve(m->ctx->device, cs.bytes)) return rc;
    HIP_TRY(src.enqueue(st));
    if (int rc = components_to_host(src.maps, n, src.H, src.W, src.out_h, src.out_w, h, w, ncls, connectivity, min_area, max_components,
                                    m->components.ptr, m->stage_out.ptr, cs, out, st))
        return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int accel_model_labels_components(accel_model* m, int n, int out_h, int out_w, int h, int w, int ncls, int connectivity, int min_area,
                                             int max_components, int dst_on_device, int32_t* count, int32_t* comp, uint64_t* sums, int32_t* ids,
                                             size_t ids_pitch)
{
    return model_components("accel_model_labels_components", m, LabelSource::NEAREST, n, out_h, out_w, h, w, ncls, connectivity, min_area, max_components,
                            dst_on_device, count, comp, sums, ids, ids_pitch);
}

extern "C" int accel_model_scores_components(accel_model* m, int n, int out_h, int out_w, int h, int w, int ncls, int connectivity, int min_area,
                                             int max_components, int dst_on_device, int32_t* count, int32_t* comp, uint64_t* sums, int32_t* ids,
                                             size_t ids_pitch)
{
    return model_components("accel_model_scores_components", m, LabelSource::INTERPOLATED, n, out_h, out_w, h, w, ncls, connectivity, min_area,
                            max_components, dst_on_device, count, comp, sums, ids, ids_pitch);
}

// ---- trimap evaluation: the distance to the ground truth's boundaries and the confusion matrix per band of it (labels_band.hip) ---------------------
static int widths_arg(const char* fn, const int* widths, int nwidths)
{
    if (!widths) return fail(ACCEL_ERR_ARG, "%s: widths is NULL", fn);
    if (nwidths < 1 || nwidths > 4) return fail(ACCEL_ERR_ARG, "%s: nwidths = %d, must be in 1 .. 4", fn, nwidths);
    for (int i = 0; i < nwidths; ++i) {
        if (widths[i] < 1 || widths[i] > 16) return fail(ACCEL_ERR_ARG, "%s: widths[%d] = %d, a width must be in 1 .. 16", fn, i, widths[i]);
        if (i && widths[i] <= widths[i - 1])
            return fail(ACCEL_ERR_ARG, "%s: widths[%d] = %d after %d, widths must be strictly ascending", fn, i, widths[i], widths[i - 1]);
    }
    return 0;
}

static int batch_arg(const char* fn, int n)
{
    if (n < 1 || n > 32768) return fail(ACCEL_ERR_ARG, "%s: n = %d, must be in 1 .. 32768", fn, n);
    return 0;
}

extern "C" int accel_boundary_distance(accel_ctx* ctx, const uint8_t* maps, int n, int h, int w, size_t pitch, int cap, uint8_t* dst, size_t dst_pitch)
{
    const char* fn = "accel_boundary_distance";
    if (!ctx) return fail(ACCEL_ERR_ARG, "%s: ctx is NULL", fn);
    if (!maps) return fail(ACCEL_ERR_ARG, "%s: maps is NULL", fn);
    if (!dst) return fail(ACCEL_ERR_ARG, "%s: dst is NULL", fn);
    if (int rc = batch_arg(fn, n)) return rc;
    if (h < 1 || h > 32768) return fail(ACCEL_ERR_ARG, "%s: h = %d, must be in 1 .. 32768", fn, h);
    if (w < 1 || w > 32768) return fail(ACCEL_ERR_ARG, "%s: w = %d, must be in 1 .. 32768", fn, w);
    if (int rc = pitch_arg(fn, "pitch", pitch, w, 1)) return rc;
    if (int rc = pitch_arg(fn, "dst_pitch", dst_pitch, w, 1)) return rc;
    if (cap < 1 || cap > 16) return fail(ACCEL_ERR_ARG, "%s: cap = %d, must be in 1 .. 16", fn, cap);
    HIP_TRY(hipSetDevice(ctx->device));
    DevTemps t;
    const unsigned char* g = static_cast<const unsigned char*>(t.upload(maps, (size_t)n * h * pitch));
    unsigned char* d = static_cast<unsigned char*>(t.get((size_t)n * h * w));
    if (!g || !d) return fail(ACCEL_ERR_HIP, "%s: device allocation or upload failed", fn);
    HIP_TRY(launch_boundary_distance(g, n, h, w, pitch, cap, d, (size_t)w, ctx->stream));
    HIP_TRY(rows_to_host(dst, dst_pitch, d, (size_t)w, (size_t)n * h, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int accel_labels_band_hist(accel_ctx* ctx, const uint8_t* labels, int n, int H, int W, int out_h, int out_w, const uint8_t* gt, int h, int w,
                                      size_t gt_pitch, int ncls, const int* widths, int nwidths, uint64_t* hist)
{
    const char* fn = "accel_labels_band_hist";
    if (!ctx) return fail(ACCEL_ERR_ARG, "%s: ctx is NULL", fn);
    if (!labels) return fail(ACCEL_ERR_ARG, "%s: labels is NULL", fn);
    if (!gt) return fail(ACCEL_ERR_ARG, "%s: gt is NULL", fn);
    if (!hist) return fail(ACCEL_ERR_ARG, "%s: hist is NULL", fn);
    if (int rc = batch_arg(fn, n)) return rc;
    if (int rc = results_args(fn, n, H, W, out_h, out_w, h, w)) return rc;
    if (int rc = pitch_arg(fn, "gt_pitch", gt_pitch, w, 1)) return rc;
    if (int rc = ncls_arg(fn, ncls)) return rc;
    if (int rc = widths_arg(fn, widths, nwidths)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    DevTemps t;
    const size_t hb = (size_t)(nwidths + 1) * ncls * ncls * sizeof(uint64_t);
    const unsigned char* l = static_cast<const unsigned char*>(t.upload(labels, (size_t)n * H * W));
    const unsigned char* g = static_cast<const unsigned char*>(t.upload(gt, (size_t)n * h * gt_pitch));
    unsigned long long* d = static_cast<unsigned long long*>(t.upload(hist, hb));
    if (!l || !g || !d) return fail(ACCEL_ERR_HIP, "%s: device allocation or upload failed", fn);
    HIP_TRY(launch_labels_band_hist(l, n, H, W, out_h, out_w, g, h, w, gt_pitch, ncls, widths, nwidths, d, ctx->stream));
    HIP_TRY(hipMemcpyAsync(hist, d, hb, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

// the model's band accumulator for counts of `ncls` classes in the bands of `widths`: refused while it holds counts made under other values, allocated and
// zeroed on first use.  (nwidths + 1) * ncls * ncls words of the 5 * 32 * 32 are in use
static const size_t BAND_HIST_BYTES = 5 * 32 * 32 * sizeof(unsigned long long);

static int model_band_hist(const char* fn, accel_model* m, int ncls, const int* widths, int nwidths, unsigned long long** hist)
{
    accel_model::BandHist& b = m->band_hist;
    if (b.ncls) {
        if (b.ncls != ncls)
            return fail(ACCEL_ERR_ARG, "%s: ncls = %d, the band accumulator holds counts of %d classes since its last clear", fn, ncls, b.ncls);
        bool same = b.nwidths == nwidths;
        for (int i = 0; same && widths && i < nwidths; ++i) same = b.widths[i] == widths[i];
        if (!same) return fail(ACCEL_ERR_ARG, "%s: the band accumulator holds counts of %d other widths since its last clear", fn, b.nwidths);
    }
    HIP_TRY(hipSetDevice(m->ctx->device));
    if (!b.words) {
        HIP_TRY(hipMalloc((void**)&b.words, BAND_HIST_BYTES));
        HIP_TRY(hipMemsetAsync(b.words, 0, BAND_HIST_BYTES, m->ctx->stream));
    }
    *hist = b.words;
    return 0;
}

static int model_band_hist_add(const char* fn, accel_model* m, LabelSource::Kind kind, const uint8_t* gt, int n, int h, int w, size_t gt_pitch, int out_h,
                               int out_w, int ncls, const int* widths, int nwidths, int gt_on_device)
{
    if (!m) return fail(ACCEL_ERR_ARG, "%s: m is NULL", fn);
    if (!gt) return fail(ACCEL_ERR_ARG, "%s: gt is NULL", fn);
    LabelSource src(m, kind);
    if (int rc = src.find(fn, n)) return rc;
    if (int rc = src.geometry(fn, out_h, out_w, h, w)) return rc;
    if (int rc = batch_arg(fn, n)) return rc;
    if (int rc = pitch_arg(fn, "gt_pitch", gt_pitch, w, 1)) return rc;
    if (int rc = ncls_arg(fn, ncls)) return rc;
    if (int rc = widths_arg(fn, widths, nwidths)) return rc;
    unsigned long long* hist = nullptr;
    if (int rc = model_band_hist(fn, m, ncls, widths, nwidths, &hist)) return rc;
    hipStream_t st = m->ctx->stream;
    if (int rc = src.reserve()) return rc;
    const unsigned char* g = gt;
    if (!gt_on_device) if (int rc = stage_in(m, gt, (size_t)n * h * gt_pitch, &g)) return rc;
    HIP_TRY(src.enqueue(st));
    HIP_TRY(launch_labels_band_hist(src.maps, n, src.H, src.W, src.out_h, src.out_w, g, h, w, gt_pitch, ncls, widths, nwidths, hist, st));
    accel_model::BandHist& b = m->band_hist;
    b.ncls = ncls; b.nwidths = nwidths;
    for (int i = 0; i < nwidths; ++i) b.widths[i] = widths[i];
    return 0;
}

extern "C" int accel_model_band_hist_add(accel_model* m, const uint8_t* gt, int n, int h, int w, size_t gt_pitch, int out_h, int out_w, int ncls,
                                         const int* widths, int nwidths, int gt_on_device)
{
    return model_band_hist_add("accel_model_band_hist_add", m, LabelSource::NEAREST, gt, n, h, w, gt_pitch, out_h, out_w, ncls, widths, nwidths, gt_on_device);
}

extern "C" int accel_model_scores_band_hist_add(accel_model* m, const uint8_t* gt, int n, int h, int w, size_t gt_pitch, int out_h, int out_w, int ncls,
                                                const int* widths, int nwidths, int gt_on_device)
{
    return model_band_hist_add("accel_model_scores_band_hist_add", m, LabelSource::INTERPOLATED, gt, n, h, w, gt_pitch, out_h, out_w, ncls, widths, nwidths,
                               gt_on_device);
}

extern "C" int accel_model_band_hist_read(accel_model* m, uint64_t* out, int ncls, int nwidths, int clear)
{
    const char* fn = "accel_model_band_hist_read";
    if (!m) return fail(ACCEL_ERR_ARG, "%s: m is NULL", fn);
    if (!out) return fail(ACCEL_ERR_ARG, "%s: out is NULL", fn);
    if (int rc = ncls_arg(fn, ncls)) return rc;
    if (nwidths < 1 || nwidths > 4) return fail(ACCEL_ERR_ARG, "%s: nwidths = %d, must be in 1 .. 4", fn, nwidths);
    const size_t hb = (size_t)(nwidths + 1) * ncls * ncls * sizeof(uint64_t);
    accel_model::BandHist& b = m->band_hist;
    if (!b.ncls) { memset(out, 0, hb); return 0; }      // nothing added since the last clear: any class count and number of widths may be asked for
    unsigned long long* hist = nullptr;
    if (int rc = model_band_hist(fn, m, ncls, nullptr, nwidths, &hist)) return rc;
    hipStream_t st = m->ctx->stream;
    HIP_TRY(hipMemcpyAsync(out, hist, hb, hipMemcpyDeviceToHost, st));
    if (clear) {
        HIP_TRY(hipMemsetAsync(hist, 0, BAND_HIST_BYTES, st));
        b.ncls = 0; b.nwidths = 0;
    }
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int accel_model_read_async(accel_model* m, const char* buf, void* pinned_dst, size_t bytes)
{
    if (!m || !buf || !pinned_dst) return fail(ACCEL_ERR_ARG, "accel_model_read_async: NULL argument");
    auto it = m->pbufs.find(buf);
    if (it == m->pbufs.end()) return fail(ACCEL_ERR_ARG, "accel_model_read_async: unknown buffer '%s'", buf);
    if (bytes > it->second.bytes) return fail(ACCEL_ERR_ARG, "accel_model_read_async: %zu bytes > buffer '%s' (%zu)", bytes, buf, it->second.bytes);
    HIP_TRY(hipMemcpyAsync(pinned_dst, it->second.ptr, bytes, hipMemcpyDeviceToHost, m->ctx->stream));
    return 0;
}

/*
 * accel_hip.h -- C ABI of libaccel_hip.so, the MI355X (gfx950) execution engine
 * of the Accel (dff_deeplab) video-segmentation inference path.
 *
 * What it replaces in the reference (SamvitJ/Accel, /root/reference):
 *   the reference has NO C ABI on this path; its Python symbol files describe a
 *   graph and MXNet (un-vendored, README.md:76) executes it.  The boundary a
 *   maintainer binds is therefore the executor contract of
 *     dff_deeplab/core/tester.py:22-35        Predictor(bind, init_params, forward, get_outputs)
 *     dff_deeplab/core/module.py:791-845,1011-1044  bind at max shape / forward
 *     dff_deeplab/core/DataParallelExecutorGroup.py:18-27,330-378  copy-in, forward, collect
 *   and, per operator, the MXNet ops the symbol files call
 *     (dff_deeplab/symbols/resnet_v1_101_flownet_deeplab.py, accel_18.py:121-239).
 *   Each entry point below names the reference interface it stands in for.
 *
 * Conventions: every function returns 0 on success and a negative code on
 * failure (never throws, never prints); accel_last_error() gives the message of
 * the last failure on the calling thread.  Tensors crossing the boundary are
 * fp32 NCHW (label maps uint8 HxW), exactly the reference's layouts; `on_device`
 * flags whether a caller pointer is HBM or host memory.  The caller owns all
 * I/O buffers; the library owns weights, the activation arena and the named
 * persistent buffers.  Calls enqueue on the context's HIP stream; only
 * accel_sync() and copies to host memory block.  Objects are re-entrant across
 * instances, not thread-safe within one instance (same as one MXNet executor).
 */
#ifndef ACCEL_HIP_H
#define ACCEL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct accel_ctx accel_ctx;       /* one GPU + one HIP stream            */
typedef struct accel_model accel_model;   /* parameters + persistent buffers     */
typedef struct accel_plan accel_plan;     /* one bound graph (key or cur)        */

#define ACCEL_OK 0
#define ACCEL_ERR_ARG (-1)
#define ACCEL_ERR_HIP (-2)
#define ACCEL_ERR_PLAN (-3)
#define ACCEL_ERR_PARAM (-4)
#define ACCEL_ERR_COMM (-5)
#define ACCEL_ERR_RANGE (-6)   /* fp16x2 form: a convolution input was not finite in an earlier run (accel_plan_run) */

const char* accel_last_error(void);
const char* accel_version(void);

/* context: stands in for `context=[mx.gpu(i)]` (demo.py:197,201) */
int accel_ctx_create(int device_id, accel_ctx** out);
int accel_ctx_destroy(accel_ctx* ctx);
int accel_sync(accel_ctx* ctx);                       /* = NDArray.asnumpy()'s implicit wait */
void* accel_ctx_stream(accel_ctx* ctx);               /* hipStream_t, for interop (RCCL / torch ExternalStream) */

/* model: parameter store shared by the key and cur graphs
 * (demo.py:192-195 arg_params/aux_params dicts; tester.py:30 init_params) */
int accel_model_create(accel_ctx* ctx, accel_model** out);
int accel_model_destroy(accel_model* m);
/* name = MXNet parameter name (`arg:`/`aux:` prefix already stripped), data = fp32
 * host memory in MXNet layout (OIHW conv, (Cin,Cout/g,kh,kw) deconv, (C,) BN);
 * the library repacks at plan finalisation. */
int accel_model_set_param(accel_model* m, const char* name, const float* data,
                          int ndim, const int64_t* shape);
int accel_model_has_param(accel_model* m, const char* name);

/* plan: a lowered, fused kernel sequence (text form, produced by
 * accel_amd/lower.py from the symbol graph) bound to static shapes -- the
 * counterpart of Module.bind (module.py:791-845).  `role` is "key", "cur" or any
 * label; plans of one model share the model's persistent buffers by name. */
int accel_model_add_plan(accel_model* m, const char* role, const char* plan_text, accel_plan** out);
int accel_plan_finalize(accel_plan* p);   /* repack weights, allocate arena, capture hipGraph */
/* enqueue one forward (Module.forward, module.py:1011).
 * Derived persistent buffers: a plan line `pbuf name=featG bytes=.. from=feat` declares featG a function of
 * `feat` that the plans keep in step with it (featG = fc6_weight * feat: non-key plans warp it instead of
 * re-running fc6 on the warped feature; Accel-101's plans have featC = corr_weight[:, :2048] * feat, the left half of
 * the feature fusion, the same way).  A plan that writes both leaves featG valid; any other write of `feat`
 * (accel_model_write, a raw pointer from accel_model_buffer, a plan that writes only `feat`) makes it stale, and
 * the next plan that READS featG first runs the plan registered under the role "init:featG" -- or fails with
 * ACCEL_ERR_PLAN if there is none.  Never silently reads a stale buffer. */
int accel_plan_run(accel_plan* p);
int accel_plan_num_ops(accel_plan* p);
/* kind: up to 31 chars + NUL; flops/bytes: algorithmic work of op i (0 if n/a) */
int accel_plan_op_info(accel_plan* p, int i, char* kind32, char* name64, double* flops, double* bytes);
/* launch decisions of op i after finalize (autotuned or heuristic): conv tile id (conv_igemm.hip, -1 for
 * non-conv ops), split-K factor, 1 if the narrow-N kernel runs it.  Diagnostic only. */
int accel_plan_op_launch(accel_plan* p, int i, int* tile, int* ksplit, int* narrow);
/* arithmetic mode of conv op i: 0 = fp32 layer (its launch geometry may still execute on the bf16 matrix cores as an exact
 * three-term split: tile 70-87), 1 = fp16-MFMA layer (plan option dtype=f16: ONE half product per multiply-add whatever the
 * geometry), 2 = bf16x3 layer (plan option dtype=bf16x3), 3 = fp32 layer whose matrix-core geometries run the fp16x2 form (two half
 * terms per operand, THREE half products per multiply-add; the default, plan option split=h2); -1 for non-conv ops.  Diagnostic only
 * (bench.py prices families by it). */
int accel_plan_op_mode(accel_plan* p, int i, int* mode);
/* fp16x2 form: the power of two conv op i's pixels were multiplied by before the split in the plan's LAST run (0 if the op has no such
 * form) and where the range behind it came from: 0 = no run yet / an all-zero input (scale 1), 1 = raised by the epilogues of the ops
 * that wrote the tensor, 2 = measured by a pass over the op's input view (tensors written outside the plan).  The scale is derived by
 * the convolution itself, in its prologue, from the largest |value| of its input tensor in THAT run (the largest lands in
 * [2^13, 2^14)): a plan run is a pure function of its inputs and parameters, like an executor forward of the reference
 * (dff_deeplab/core/module.py:1011-1044) -- nothing is calibrated, nothing survives a run.  A tensor such a convolution reads whose
 * largest stored |value| was an INFINITY in some run makes the NEXT accel_plan_run fail with ACCEL_ERR_RANGE (once); so does a NaN in a
 * tensor written by a byte mover (image converters, pools, warps, the deformable sampler, view copies) or measured by a pass of its
 * own.  A NaN that a matrix-core convolution produces mid-plan is NOT reported: its range epilogue takes floating-point maxima, which
 * drop NaNs (csrc/conv_epilogue.h); behind a ReLU the NaN itself becomes 0 (fmaxf -- the reference's relu `a > 0 ? a : 0` does the
 * same), without one it reaches the outputs through the matrix instructions as in fp32 arithmetic.
 * Diagnostic only. */
int accel_plan_op_range(accel_plan* p, int i, float* scale, int* source);
/* Diagnostic (scripts/debug/range_nan.py): the 1088 words of conv op i's input range slot after the plan's last run -- word 0 = the
 * largest |value| stored into the tensor, as a bit pattern (what the convolution read), words 64 .. 1087 = the partial words the
 * writers raised (csrc/range.h).  n_words must be at least 1088. */
int accel_plan_op_range_words(accel_plan* p, int i, unsigned* words, int n_words);
/* Launch geometries are REPRODUCIBLE: decisions come from the table shipped beside the library (tune/gfx950.tune, covers
 * the BASELINE workloads) or from the user's table ($ACCEL_TUNE_CACHE, else ~/.cache/accel_amd/gfx950.tune); a shape in
 * neither is timed once and appended to the user's table.  Counters of this process: decisions replayed, decisions
 * taken by timing, entries of the shipped table (0 = not found).  Diagnostic only. */
int accel_tune_stats(int* replayed, int* timed, int* shipped_entries);
/* runs the plan `iters` times eagerly with a HIP event pair around every op on
 * the context stream; ms[i] = mean duration of op i */
int accel_plan_profile(accel_plan* p, int iters, float* ms, int n_ms);

/* Diagnostics (scripts/debug, tests): the ops of a finalized plan launched one after the other on the context stream --
 * no captured graph -- followed by a host wait; and a host copy of a byte range of the plan's activation
 * arena (arena_bytes, if given, receives its size; host_dst may be NULL to query only).  Comparing the arena after a
 * normal accel_plan_run with the arena after accel_plan_run_serial of the same bound plan names the first op whose
 * output depends on the schedule. */
int accel_plan_run_serial(accel_plan* p);
int accel_plan_arena_read(accel_plan* p, size_t offset, void* host_dst, size_t bytes, size_t* arena_bytes);

/* persistent buffers (inputs `data`/`data_key`, outputs `logits`/`labels`, the
 * propagated feature `feat`): DataParallelExecutorGroup._load_general copy-in
 * (:18-27) and get_outputs (:357-378) */
int accel_model_write(accel_model* m, const char* buf, const void* src, size_t bytes, int src_on_device);
int accel_model_read(accel_model* m, const char* buf, void* dst, size_t bytes, int dst_on_device);
/* Zero-copy input: the image input `buf` (`data`, `data_key` -- a buffer that only the input-conversion kernels of the
 * finalized plans read) is read from the caller's device buffer `devptr` (`bytes` = the size of `buf`, same layout) by every
 * plan run that follows, until the next accel_model_write / accel_model_commit into `buf` or the next bind.  Stream-ordered
 * on the context stream like a write; the caller keeps `devptr` alive and unchanged until those runs have completed.
 * An EXTENSION, not the reference's behaviour: DataParallelExecutorGroup._load_general (executor_group.py:18-27) ALWAYS copies
 * the source array into the executor's bound input (d_src.copyto(d_targets)), also when the source already lives on the
 * device -- accel_model_write(src_on_device = 1) is that copy, and bench.py's headline uses it; the zero-copy binding is
 * reported separately (secondary.*_zero_copy_inputs).  accel_model_buffer(buf) and accel_model_read(buf) of a bound buffer:
 * a raw pointer hand-out ends the binding (the caller is about to write the model's own copy), a read returns the bytes the
 * plans would read (the bound frame). */
int accel_model_bind_device(accel_model* m, const char* buf, const void* devptr, size_t bytes);
int accel_model_buffer(accel_model* m, const char* buf, void** dev_ptr, size_t* bytes);
/* Write generation of a persistent buffer: starts at 0, bumped by every accel_plan_run of a plan that writes the
 * buffer, every accel_model_write / accel_model_commit into it and every raw-pointer hand-out.  A device handle to an
 * output (the `feat` a Predictor returns, tester.py:158-171) records the generation it was produced at; a consumer
 * that finds another generation knows the bytes are no longer that output (MXNet: "outputs are valid until the next
 * forward") and must fall back to a host copy or fail -- never read whatever the buffer holds now. */
int accel_model_buffer_generation(accel_model* m, const char* buf, uint64_t* generation);

/* ---- host I/O overlapped with compute ------------------------------------------------------------------------------
 * The reference's timed loop (demo.py:234-250) moves the frame in and the label map out synchronously through pageable
 * memory.  Here: page-locked staging memory, the NEXT frame's upload on a copy stream while the current frame computes,
 * and an asynchronous download of the outputs.
 *   accel_host_alloc / _free      page-locked host memory (hipHostMalloc)
 *   accel_model_prefetch(buf,src) enqueue H2D of `src` (page-locked, must stay valid until the matching commit) into a
 *                                 library-owned shadow of `buf` on the copy stream; returns immediately
 *   accel_model_commit(buf)       compute stream waits for the prefetch and copies the shadow into `buf` (HBM to HBM)
 *   accel_model_read_async        enqueue D2H of `buf` into page-locked `dst` on the compute stream, no host wait:
 *                                 the bytes are valid after accel_sync() */
int accel_host_alloc(size_t bytes, void** out);
int accel_host_free(void* p);
int accel_model_prefetch(accel_model* m, const char* buf, const void* pinned_src, size_t bytes);
int accel_model_commit(accel_model* m, const char* buf);
int accel_model_read_async(accel_model* m, const char* buf, void* pinned_dst, size_t bytes);

/* ---- uint8 video frames ---------------------------------------------------------------------------------------------
 * A camera, a decoder or a PNG gives uint8 h x w x 3 BGR; the image inputs are fp32 n x 3 x H x W RGB, mean-subtracted
 * and padded (lib/utils/image.py:194-235, resize + transform -- numpy float64 on one host thread in the reference's
 * harness, and 4x the bytes of the frame over PCIe afterwards).  Here the bytes are uploaded as they are and one kernel
 * (csrc/frames_u8.hip) writes the fp32 tensor, bit for bit what accel_amd/utils/image.py computes on the host:
 *   bgr, n, h, w, pitch   n frames of h rows of w pixels, 3 bytes each in B, G, R order; `pitch` bytes from row to row
 *                         (>= 3 * w) and h * pitch bytes from frame to frame
 *   means_bgr             three float64 means in B, G, R order (PIXEL_MEANS): value = fp32(double(grey) - mean), ONE rounding
 *   out_h, out_w, step    the resized image and the source pixels per output pixel (1 / scale) of the bilinear resize
 *                         (half-pixel centres, float64, rounded to a grey level like the host's uint8 resize); step == 1
 *                         copies the bytes and needs out_h == h, out_w == w.  The CALLER derives the three from the resize
 *                         rule (utils/image.py resize_geometry): the library does not re-derive it, so two `round`
 *                         implementations cannot disagree
 *   H, W                  the padded size (out_h <= H, out_w <= W); padding holds fp32(0 - mean), not 0: the reference
 *                         pads with zeros BEFORE it removes the mean
 * Argument errors return ACCEL_ERR_ARG before anything is enqueued, with a message that names the argument.
 *   accel_frame_u8           operator level: host bytes in, host tensor out (the parity tests)
 *   accel_model_write_u8     accel_model_write for uint8 frames into an image input `buf` of n x 3 x H x W fp32: host bytes go
 *                            through a library-owned uint8 staging buffer on the compute stream (src_on_device = 0), device
 *                            bytes -- a frame a GPU decoder left in HBM -- are read in place (src_on_device = 1: the caller keeps
 *                            them unchanged until the kernel has run).  Ends a zero-copy binding and bumps the write
 *                            generation exactly as accel_model_write does
 *   accel_model_prefetch_u8  accel_model_prefetch for uint8 bytes: page-locked `pinned_src` crosses PCIe on the copy stream
 *                            into a uint8 shadow of `buf` -- a shadow of its own, not the fp32 one of accel_model_prefetch
 *   accel_model_commit_u8    the compute stream waits for that upload, then the kernel converts the shadow into `buf`
 *                            (n * h * pitch <= the bytes prefetched) */
int accel_frame_u8(accel_ctx* ctx, const uint8_t* bgr, int n, int h, int w, size_t pitch, const double* means_bgr,
                   int out_h, int out_w, double step, int H, int W, float* out);
int accel_model_write_u8(accel_model* m, const char* buf, const uint8_t* bgr, int n, int h, int w, size_t pitch, const double* means_bgr,
                         int out_h, int out_w, double step, int H, int W, int src_on_device);
int accel_model_prefetch_u8(accel_model* m, const char* buf, const void* pinned_src, size_t bytes);
int accel_model_commit_u8(accel_model* m, const char* buf, int n, int h, int w, size_t pitch, const double* means_bgr,
                          int out_h, int out_w, double step, int H, int W);

/* ---- NV12 video frames -------------------------------------------------------------------------------------------
 * What a hardware or software video decoder hands out: a full-size 8-bit luma plane followed by a half-height plane of
 * interleaved Cb, Cr at half resolution.  The bytes are uploaded as they are (1.5 per pixel) and one kernel
 * (csrc/frames_yuv.hip) converts the colour, resizes, removes the mean and pads: the tensor is, bit for bit,
 * transform(resize(nv12_to_bgr_host(frame))) of accel_amd/utils/image.py -- what the uint8 route above gives for the
 * BGR frames the conversion below makes.
 *   nv12, n, h, w         n frames; h and w are even, 2 .. 32768
 *   pitch                 bytes from row to row, in both planes (>= w)
 *   uv_offset             the byte of a frame at which its h/2 rows of w/2 (Cb, Cr) pairs begin (>= h * pitch)
 *   frame_bytes           bytes from frame to frame (>= uv_offset + (h/2) * pitch); n frames occupy
 *                         (n - 1) * frame_bytes + uv_offset + (h/2) * pitch bytes.  Bytes in the gaps -- between rows,
 *                         between the planes, after a frame -- are never read
 *   colour                0 BT.601 limited range, 1 BT.601 full range, 2 BT.709 limited range, 3 BT.709 full range
 *   means_bgr .. W        as for uint8 frames
 * Pixel (x, y) takes Y at (x, y) and Cb, Cr at (x >> 1, y >> 1) (replicated chroma; interpolated chroma siting is what
 * the _sited entry points below offer, NV12 being their format 3).  With c = Y - yoff, d = Cb - 128, e = Cr - 128 in int32 and arithmetic right shifts:
 *     R = clip((ky*c + krv*e         + 32768) >> 16, 0, 255)
 *     G = clip((ky*c - kgu*d - kgv*e + 32768) >> 16, 0, 255)
 *     B = clip((ky*c + kbu*d         + 32768) >> 16, 0, 255)
 * (yoff, ky, krv, kgu, kgv, kbu) = round(65536 x the standard's value).  When the frame is resized, each of the four
 * taps is converted to B, G, R bytes first and the bilinear arithmetic of the uint8 route runs on them.
 * Argument errors return ACCEL_ERR_ARG before anything is enqueued, with a message that names the argument.
 *   accel_nv12_coefficients  the six integers (yoff, ky, krv, kgu, kgv, kbu) of a colour mode; host only, touches no GPU
 *   accel_frame_nv12         operator level: host bytes in, host tensor out (the parity tests)
 *   accel_nv12_to_bgr        n x h x w x 3 BGR bytes, rows `out_pitch` apart (>= 3 * w; bytes between rows are not
 *                            written) and h * out_pitch from frame to frame.  on_device = 0: host in, host out;
 *                            on_device = 1: both pointers are HBM and the kernel is only enqueued on the context's stream
 *   accel_model_write_nv12   accel_model_write_u8 for NV12 bytes (src_on_device = 1: a decoder's output in HBM, read in
 *                            place; the caller keeps it unchanged until the kernel has run)
 *   accel_model_commit_nv12  accel_model_commit_u8 for NV12 bytes that accel_model_prefetch_u8 uploaded -- bytes are
 *                            bytes, the uint8 shadow serves both (the bytes n frames occupy <= the bytes prefetched) */
int accel_nv12_coefficients(int colour, int32_t out[6]);
int accel_frame_nv12(accel_ctx* ctx, const uint8_t* nv12, int n, int h, int w, size_t pitch, size_t uv_offset, size_t frame_bytes, int colour,
                     const double* means_bgr, int out_h, int out_w, double step, int H, int W, float* out);
int accel_nv12_to_bgr(accel_ctx* ctx, const uint8_t* nv12, int n, int h, int w, size_t pitch, size_t uv_offset, size_t frame_bytes, int colour,
                      uint8_t* bgr_out, size_t out_pitch, int on_device);
int accel_model_write_nv12(accel_model* m, const char* buf, const uint8_t* nv12, int n, int h, int w, size_t pitch, size_t uv_offset,
                           size_t frame_bytes, int colour, const double* means_bgr, int out_h, int out_w, double step, int H, int W,
                           int src_on_device);
int accel_model_commit_nv12(accel_model* m, const char* buf, int n, int h, int w, size_t pitch, size_t uv_offset, size_t frame_bytes, int colour,
                            const double* means_bgr, int out_h, int out_w, double step, int H, int W);

/* ---- I420, P010 and YUY2 video frames -------------------------------------------------------------------------------
 * What a software decoder (I420; YV12 is I420 with the chroma planes in the other order), a 10-bit hardware decoder
 * (P010) and a capture card or USB camera (YUY2) hand out.  The bytes are uploaded as they are (1.5, 3 and 2 per pixel)
 * and one kernel (csrc/frames_yuv.hip) converts the colour, resizes, removes the mean and pads: the tensor is, bit for
 * bit, transform(resize(yuv_to_bgr_host(frame))) of accel_amd/utils/image.py.  The entry points mirror the NV12 ones
 * argument for argument, with `n, const accel_yuv_layout*` in place of the flat layout:
 *   format                0 I420, 1 P010, 2 YUY2
 *   colour                as for NV12
 *   h, w                  1 .. 32768; w even; h even for I420 and P010
 *   pitch                 bytes from row to row of the luma plane (I420: >= w), of both planes (P010: >= 2 * w) or of the
 *                         one plane (YUY2: >= 2 * w, rows of Y0 Cb Y1 Cr quads)
 *   pitch_c               I420: bytes from row to row of each chroma plane (>= w / 2)
 *   u_offset, v_offset    I420: the bytes of a frame at which its Cb and Cr planes begin, each h/2 rows of w/2 bytes; both
 *                         >= h * pitch, in either order, and not required to be disjoint from each other (rows may interleave:
 *                         pitch_c == pitch, v_offset == u_offset + pitch / 2).  P010: u_offset is where the h/2 rows of w/2
 *                         (Cb, Cr) word pairs begin
 *   frame_bytes           bytes from frame to frame, >= the extent of a frame: one past the last byte of the last row of
 *                         its last plane.  n frames occupy (n - 1) * frame_bytes + extent bytes; a host buffer may end there
 * A field the format does not use (pitch_c and v_offset for P010 and YUY2, u_offset for YUY2) must be 0.  P010 holds
 * little-endian 16-bit words whose sample is word >> 6 (the low six bits are never looked at); its pitch, u_offset,
 * frame_bytes and a device source address are multiples of 2.  Bytes in the gaps are never read.
 * Chroma is replicated: I420 and P010 pixel (x, y) takes it at (x >> 1, y >> 1), YUY2 from quad x >> 1 of its own row
 * (interpolated siting: the _sited entry points below).
 * The 8-bit formats convert with the rule and the integers of NV12.  P010, with c = Y10 - 4 * yoff, d = Cb10 - 512,
 * e = Cr10 - 512 in int32:
 *     R = clip((ky*c + krv*e         + (1 << 17)) >> 18, 0, 255)
 *     G = clip((ky*c - kgu*d - kgv*e + (1 << 17)) >> 18, 0, 255)
 *     B = clip((ky*c + kbu*d         + (1 << 17)) >> 18, 0, 255)
 * with NV12's integers for the limited-range modes and round(65536 x the standard's value x 1020 / 1023) for the
 * full-range ones (1023 is white).  The output is 8-bit BGR; from there on nothing differs from the other routes.
 * Argument errors return ACCEL_ERR_ARG before anything is enqueued, with a message that names the argument.
 *   accel_yuv10_coefficients  the six integers (yoff, ky, krv, kgu, kgv, kbu) of a colour mode for P010; host only
 *   accel_frame_yuv, accel_yuv_to_bgr, accel_model_write_yuv, accel_model_commit_yuv
 *                             as their NV12 namesakes; the bytes a commit converts were uploaded by
 *                             accel_model_prefetch_u8 (P010's words travel as bytes) */
typedef struct { int format, colour, h, w; size_t pitch, pitch_c, u_offset, v_offset, frame_bytes; } accel_yuv_layout;
int accel_yuv10_coefficients(int colour, int32_t out[6]);
int accel_frame_yuv(accel_ctx* ctx, const uint8_t* yuv, int n, const accel_yuv_layout* layout, const double* means_bgr,
                    int out_h, int out_w, double step, int H, int W, float* out);
int accel_yuv_to_bgr(accel_ctx* ctx, const uint8_t* yuv, int n, const accel_yuv_layout* layout, uint8_t* bgr_out, size_t out_pitch, int on_device);
int accel_model_write_yuv(accel_model* m, const char* buf, const uint8_t* yuv, int n, const accel_yuv_layout* layout, const double* means_bgr,
                          int out_h, int out_w, double step, int H, int W, int src_on_device);
int accel_model_commit_yuv(accel_model* m, const char* buf, int n, const accel_yuv_layout* layout, const double* means_bgr,
                           int out_h, int out_w, double step, int H, int W);

/* ---- interpolated chroma siting ----------------------------------------------------------------------------------------
 * The routes above replicate chroma: the nearest-neighbour upsampling, which shifts the colour planes by up to half a
 * chroma sample against the luma plane.  These entry points interpolate Cb and Cr to every luma pixel first, as the
 * siting of the source says (H.273 chroma_sample_loc_type 0, 1, 2), and hand the result to the colour rule of the format
 * where the replicated sample enters it above (csrc/frames_sited.hip): the tensor is, bit for bit,
 * transform(resize(yuv_to_bgr_host(frame, siting = s))) of accel_amd/utils/image.py.  They mirror the four yuv entry
 * points argument for argument, with a trailing `int siting` (before on_device / src_on_device where those exist):
 *   siting                0 replicate: the kernels above, bit for bit;  1 left: horizontally co-sited, vertically centred
 *                         (H.264 / HEVC);  2 centre: centred on both axes (JPEG);  3 topleft: co-sited on both (BT.2020).
 *                         For YUY2, which has no vertical step, left and topleft coincide.  Interlaced siting is not offered
 *   format                0 I420, 1 P010, 2 YUY2 as above, and 3 NV12: h rows of w luma bytes `pitch` apart and, at
 *                         `u_offset` (>= h * pitch), h/2 rows of w/2 (Cb, Cr) byte pairs at the same pitch; pitch_c and
 *                         v_offset must be 0; h, w even, 2 .. 32768; frame_bytes >= u_offset + (h/2 - 1) * pitch + w
 * The chroma planes have cw = w/2 columns and ch = h/2 rows (YUY2: ch = h, weight 4 on the pixel's own row).  For luma
 * pixel (x, y), k = x >> 1 and j = y >> 1, each axis takes two neighbouring samples with weights that sum to 4:
 *     co-sited (sample k lies on luma 2k)          even coordinate: (k: 4)             odd: (k: 2, k+1: 2)
 *     centred  (sample k lies on luma 2k + 0.5)    even coordinate: (k-1: 1, k: 3)     odd: (k: 3, k+1: 1)
 * with indices clamped to [0, cw-1] and [0, ch-1], and for Cb and Cr alike
 *     C(x, y) = (sum_rows sum_cols wy * wx * c[row][col] + 8) >> 4
 * -- one rounding, none between the axes; for P010 on the 10-bit word >> 6 samples.  When the frame is resized, each of
 * the four taps is converted to B, G, R bytes with sited chroma first.
 * Argument errors (those of the yuv entry points; siting outside 0 .. 3; format outside 0 .. 3; NV12's fields) return
 * ACCEL_ERR_ARG before anything is enqueued, with a message that names the argument. */
int accel_frame_yuv_sited(accel_ctx* ctx, const uint8_t* yuv, int n, const accel_yuv_layout* layout, const double* means_bgr,
                          int out_h, int out_w, double step, int H, int W, float* out, int siting);
int accel_yuv_to_bgr_sited(accel_ctx* ctx, const uint8_t* yuv, int n, const accel_yuv_layout* layout, uint8_t* bgr_out, size_t out_pitch,
                           int siting, int on_device);
int accel_model_write_yuv_sited(accel_model* m, const char* buf, const uint8_t* yuv, int n, const accel_yuv_layout* layout,
                                const double* means_bgr, int out_h, int out_w, double step, int H, int W, int siting, int src_on_device);
int accel_model_commit_yuv_sited(accel_model* m, const char* buf, int n, const accel_yuv_layout* layout, const double* means_bgr,
                                 int out_h, int out_w, double step, int H, int W, int siting);

/* ---- finished frames: labels at the source size, confusion matrix, colour image ------------------------------------
 * The output side of the loop (demo.py:245-266: `.asnumpy()` of the label map, fast_hist, the palette PNG) on the GPU
 * (csrc/results_u8.hip).  A label map is n x H x W uint8; its valid (unpadded) region is out_h x out_w in the top-left
 * corner; the source frame is h x w.  Source pixel (y, x) takes
 *     labels[min(y * out_h / h, out_h - 1)][min(x * out_w / w, out_w - 1)]          (integer division)
 * -- the nearest-neighbour rule of the reference's evaluator (lib/dataset/cityscape.py:227) applied to the cropped
 * region; a crop or a copy when h x w == out_h x out_w.  out_h, out_w are what accel_model_write_u8 was told.
 *   labels at the source size   n x h x w uint8, rows `dst_pitch` bytes apart (>= w), h * dst_pitch from frame to frame;
 *                               bytes between rows are not written
 *   confusion matrix            hist[gt * ncls + pred] += 1 for every source pixel with gt < ncls and pred < ncls (255 and
 *                               any other id >= ncls are ignored, as fast_hist of demo.py:50-53 ignores them): rows are
 *                               ground truth, columns prediction; ncls in 1 .. 32; gt is n x h x w uint8 with `gt_pitch`;
 *                               unsigned 64-bit counts, exact, independent of the order of arrival
 *   colour image                n x h x w x 3 uint8 = palette_rgb[label] for a 256 x 3 R, G, B table (768 host bytes, passed
 *                               to the kernel by value), stored R, G, B (rgb_order = 1: what PIL wants) or B, G, R
 *                               (rgb_order = 0: what the frames are).  With frame_bgr (n x h x w x 3 B, G, R, `frame_pitch`)
 *                               every channel is (alpha * colour + (256 - alpha) * frame + 128) >> 8, alpha in 0 .. 256;
 *                               alpha = 256 or frame_bgr = NULL gives the pure colour
 * Sizes are at most 32768.  Argument errors (a NULL pointer, a size < 1, out_h > H, out_w > W, a pitch smaller than a row,
 * ncls outside 1 .. 32, alpha outside 0 .. 256, n larger than the bound batch, ncls other than the accumulator's since its
 * last clear) return ACCEL_ERR_ARG before anything is enqueued, with a message that names the argument.
 *   accel_labels_to_source, accel_labels_hist, accel_labels_colour
 *                               operator level: host bytes in, host bytes out (the parity tests); `hist` is ncls * ncls
 *                               words that are ADDED to
 *   accel_model_labels_to_source, accel_model_hist_add, accel_model_hist_read, accel_model_labels_colour
 *                               the same on the model's `labels` buffer (n x H x W as the bound plans write it), enqueued
 *                               on the context stream after the run that wrote it.  They only read `labels`: no write
 *                               generation changes, no captured graph is touched.  Host gt / frame bytes go through a
 *                               library-owned staging buffer (*_on_device = 0), device bytes are read in place (= 1: the
 *                               caller keeps them unchanged until the kernel has run); a host `dst` is filled when the
 *                               call returns, a device `dst` (dst_on_device = 1) when the stream reaches it.
 *                               The confusion matrix accumulates in the model, across calls, until
 *                               accel_model_hist_read(.., clear = 1); hist_read waits for the stream and copies
 *                               ncls * ncls words to the host (zeros when nothing was added since the last clear) */
int accel_labels_to_source(accel_ctx* ctx, const uint8_t* labels, int n, int H, int W, int out_h, int out_w, int h, int w,
                           uint8_t* dst, size_t dst_pitch);
int accel_labels_hist(accel_ctx* ctx, const uint8_t* labels, int n, int H, int W, int out_h, int out_w,
                      const uint8_t* gt, int h, int w, size_t gt_pitch, int ncls, uint64_t* hist);
int accel_labels_colour(accel_ctx* ctx, const uint8_t* labels, int n, int H, int W, int out_h, int out_w, int h, int w,
                        const uint8_t* palette_rgb, int rgb_order, const uint8_t* frame_bgr, size_t frame_pitch, int alpha,
                        uint8_t* dst, size_t dst_pitch);
int accel_model_labels_to_source(accel_model* m, int n, int out_h, int out_w, int h, int w, uint8_t* dst, size_t dst_pitch, int dst_on_device);
int accel_model_hist_add(accel_model* m, const uint8_t* gt, int n, int h, int w, size_t gt_pitch, int out_h, int out_w, int ncls, int gt_on_device);
int accel_model_hist_read(accel_model* m, uint64_t* out, int ncls, int clear);
int accel_model_labels_colour(accel_model* m, int n, int out_h, int out_w, int h, int w, const uint8_t* palette_rgb, int rgb_order,
                              const uint8_t* frame_bgr, size_t frame_pitch, int alpha, int frame_on_device,
                              uint8_t* dst, size_t dst_pitch, int dst_on_device);

/* ---- finished frames: per-pixel confidence ------------------------------------------------------------------------
 * How sure the network was, made where the scores are (csrc/confidence.hip) instead of `logits.asnumpy()` plus a softmax
 * on the host.  `scores` is n x ncls x H x W fp32 (NCHW, the layout of `logits`), ncls in {2, 19, 21}; the geometry is
 * that of the block above (valid region out_h x out_w, source size h x w, the same integer nearest rule), so every output
 * lines up pixel for pixel with accel_labels_to_source.  Per source pixel, any subset of (a NULL pointer leaves one out):
 *   conf     n x h x w uint8    min(255, floor(256 * p)), p = 1 / sum_k exp(l_k - l_max) the largest softmax probability;
 *                               differences, exp, sum (classes in ascending order), reciprocal and scaling in float64
 *   margin   n x h x w fp32     l_top1 - l_top2, one fp32 subtraction of two stored values; top2 is the largest value among
 *                               the classes other than the winner: 0 on a tie at the top
 *   second   n x h x w uint8    the runner-up: the first maximal index among the classes other than `best`, the first-max
 *                               argmax (= `labels`)
 *   hist     n x 256 uint64     per frame, the number of source pixels at each conf level: OVERWRITTEN, exact, independent
 *                               of the order of arrival (any threshold and the mean confidence follow on the host)
 * is_prob = 1: the stored values are probabilities already (a tail lowered with softmax=1): conf =
 * min(255, floor(256 * double(top1))), no exponential; margin and second as above, on the stored values.
 * Rows are `*_pitch` BYTES apart (>= a row; margin_pitch a multiple of 4), h * pitch from frame to frame; bytes between
 * rows are not written.  Argument errors (a NULL input, all outputs NULL, a size < 1 or > 32768, out_h > H, out_w > W, a
 * pitch smaller than a row, a misaligned margin pitch, an unsupported ncls, n larger than the bound batch, no `logits`
 * buffer) return ACCEL_ERR_ARG before anything is enqueued, with a message that names the argument.
 *   accel_scores_confidence     operator level: host scores in, host results out (the parity tests)
 *   accel_model_confidence      the same on the model's `logits` buffer (n, ncls, H, W as the bound plans write it),
 *                               enqueued on the context stream after the run that wrote it.  It only reads `logits`: no
 *                               write generation changes, no captured graph is touched.  A host destination
 *                               (dst_on_device = 0) is filled when the call returns, device destinations (= 1: all of
 *                               them, margin 4-byte and hist 8-byte aligned) when the stream reaches it */
int accel_scores_confidence(accel_ctx* ctx, const float* scores, int n, int ncls, int H, int W, int out_h, int out_w, int h, int w, int is_prob,
                            uint8_t* conf, size_t conf_pitch, float* margin, size_t margin_pitch, uint8_t* second, size_t second_pitch,
                            uint64_t* hist);
int accel_model_confidence(accel_model* m, int n, int out_h, int out_w, int h, int w, int is_prob, uint8_t* conf, size_t conf_pitch,
                           float* margin, size_t margin_pitch, uint8_t* second, size_t second_pitch, uint64_t* hist, int dst_on_device);

/* ---- finished frames: labels from interpolated scores ---------------------------------------------------------------
 * Labels at the source frame's size the way segmentation is usually evaluated: every class plane of the scores is
 * interpolated bilinearly to the source pixel and the argmax is taken THERE (csrc/scores_labels.hip), instead of copying
 * the finished label of the nearest map pixel (accel_labels_to_source) -- and instead of `logits.asnumpy()` plus a blend
 * of ncls planes on the host.  `scores` is n x ncls x H x W fp32 (NCHW, the layout of `logits`), ncls in {2, 19, 21}; the
 * geometry vocabulary is that of the blocks above (valid region out_h x out_w, source size h x w).  The specification is
 * accel_amd/utils/image.py labels_interpolated_host; the kernel restates it bit for bit.
 *   taps     in integer arithmetic, for source row y of h rows over a region of out_h rows (columns alike with w, out_w):
 *                num = clamp((2 * y + 1) * out_h - h, 0, 2 * h * (out_h - 1))           (< 2^31: sizes are <= 32768)
 *                y0 = num / (2 * h),  y1 = min(y0 + 1, out_h - 1),  fy = double(num - 2 * h * y0) / double(2 * h)
 *            (ONE IEEE division): the half-pixel-centre coordinate (y + 0.5) * out_h / h - 0.5 clamped to the region, the
 *            inverse of the resize of the input side.  Taps never leave the valid region: the padding is never read
 *   blend    in float64, each operation rounded on its own (no fma), a<row><col> the four fp32 taps as doubles:
 *                gx = 1 - fx, gy = 1 - fy, top = a00 * gx + a01 * fx, bot = a10 * gx + a11 * fx, v_k = top * gy + bot * fy
 *   label    the first k with the largest v_k (ascending scan, strict >): the tie rule of `labels`
 * At h x w == out_h x out_w, fx = fy = 0 and v_k is the stored score: the result is the crop of `labels`, which is what
 * accel_labels_to_source gives there.  Scores are assumed FINITE: a pixel with a non-finite tap is unspecified (inf * 0
 * arises in the blend).  Rows of dst are `dst_pitch` bytes apart; bytes between rows are not written.
 * Argument errors (a NULL pointer, a size < 1 or > 32768, out_h > H, out_w > W, a pitch smaller than a row, an unsupported
 * ncls, n larger than the bound batch, no `logits` buffer, and for _hist_add / _colour those of their label forms) return
 * ACCEL_ERR_ARG before anything is enqueued, with a message that names the argument.
 *   accel_scores_labels         operator level: host scores in, host labels out (the parity tests)
 *   accel_model_scores_labels, accel_model_scores_hist_add, accel_model_scores_colour
 *                               on the model's `logits` buffer (n, ncls, H, W as the bound plans write it), enqueued on the
 *                               context stream after the run that wrote it.  They only read `logits`: no write generation
 *                               changes, no captured graph is touched.  _hist_add and _colour write the interpolated labels
 *                               into a model-owned n x h x w scratch (grown on demand, freed with the model) and then run
 *                               the kernels of accel_model_hist_add / accel_model_labels_colour on it at the identity
 *                               geometry: _hist_add adds into the SAME accumulator under the same ncls rule (its `ncls` is
 *                               the evaluation's class count, 1 .. 32; the class count of the scores is that of `logits`);
 *                               *_on_device as in the label forms */
int accel_scores_labels(accel_ctx* ctx, const float* scores, int n, int ncls, int H, int W, int out_h, int out_w, int h, int w,
                        uint8_t* dst, size_t dst_pitch);
int accel_model_scores_labels(accel_model* m, int n, int out_h, int out_w, int h, int w, uint8_t* dst, size_t dst_pitch, int dst_on_device);
int accel_model_scores_hist_add(accel_model* m, const uint8_t* gt, int n, int h, int w, size_t gt_pitch, int out_h, int out_w, int ncls, int gt_on_device);
int accel_model_scores_colour(accel_model* m, int n, int out_h, int out_w, int h, int w, const uint8_t* palette_rgb, int rgb_order,
                              const uint8_t* frame_bgr, size_t frame_pitch, int alpha, int frame_on_device,
                              uint8_t* dst, size_t dst_pitch, int dst_on_device);

/* ---- finished frames: confidence of interpolated scores, with their labels ---------------------------------------------
 * The confidence block above describes the NEAREST map pixel; the labels of the block above are the argmax of INTERPOLATED
 * scores.  For a frame that was resampled on the way in the two do not speak of the same winner.  These two calls finish a
 * source pixel from the interpolated values themselves, in ONE pass over the scores (the interpolated form of csrc/confidence.hip), and can
 * hand out the label found on the way.  `scores`, ncls and the geometry as above; v_k are the ncls values of the pixel,
 * taps and blend exactly as in the block above (float64).  Any subset of (a NULL pointer leaves one out, at least one):
 *   labels   n x h x w uint8    the first k with the largest v_k: what accel_scores_labels writes
 *   conf     n x h x w uint8    min(255, floor(256 * p)), p = 1 / sum_k exp(v_k - v_best), classes in ascending order, all
 *                               in float64: the softmax of the interpolated logits, whose argmax is `labels`
 *   margin   n x h x w fp32     float(v_best - v_second): one float64 subtraction, rounded once to fp32; 0 on a tie at the top
 *   second   n x h x w uint8    the first maximal index among the classes other than `labels`, compared on the float64 v_k
 *   hist     n x 256 uint64     per frame, the number of source pixels at each conf level: OVERWRITTEN
 * is_prob = 1: the stored values are probabilities and are blended the same way; conf = min(255, floor(256 * v_best)), no
 * exponential.  The specification is accel_amd/utils/image.py confidence_interpolated_host; the kernel restates it bit for
 * bit up to the exp.  At h x w == out_h x out_w every weight is 0: the outputs are those of accel_scores_confidence and the
 * crop of `labels`.  Scores are assumed FINITE.  Pitches, argument errors and dst_on_device as for accel_model_confidence,
 * with labels / labels_pitch checked like conf / conf_pitch.
 *   accel_scores_confidence_interp   operator level: host scores in, host results out (the parity tests)
 *   accel_model_confidence_interp    on the model's `logits` buffer; it only reads `logits` */
int accel_scores_confidence_interp(accel_ctx* ctx, const float* scores, int n, int ncls, int H, int W, int out_h, int out_w, int h, int w, int is_prob,
                                   uint8_t* labels, size_t labels_pitch, uint8_t* conf, size_t conf_pitch, float* margin, size_t margin_pitch,
                                   uint8_t* second, size_t second_pitch, uint64_t* hist);
int accel_model_confidence_interp(accel_model* m, int n, int out_h, int out_w, int h, int w, int is_prob, uint8_t* labels, size_t labels_pitch,
                                  uint8_t* conf, size_t conf_pitch, float* margin, size_t margin_pitch, uint8_t* second, size_t second_pitch,
                                  uint64_t* hist, int dst_on_device);

/* ---- frame change: the measure behind content-adaptive key frames ------------------------------------------------------
 * How much a frame differs from the frame kept at the last key frame, made where every input route (fp32, BGR bytes, NV12,
 * I420, P010, YUY2, a zero-copy binding) leaves the frame: the image input, n x 3 x H x W fp32, planes R, G, B,
 * mean-subtracted, of which the valid region out_h x out_w in the top-left corner is looked at and nothing else is read
 * (csrc/frame_change.hip).  Integer arithmetic; the specification is accel_amd/utils/image.py frame_signature_host /
 * frame_change_host and the kernel equals it bit for bit.  With cell in {8, 16, 32, 64}, gh = ceil(out_h / cell) and
 * gw = ceil(out_w / cell):
 *   q        int(rint(fmin(fmax(x, -512), 512) * 8)), fp32 round-half-to-even; NaN gives -4096, +-inf gives +-4096
 *   v        2 qR + 5 qG + qB per pixel: 64 units per grey level
 *   sig      n x gh x gw int32   the SIGNATURE: S = the sum of v over the valid pixels of the cell (|S| <= 2^27)
 * and against the signature sig_key of another frame (frame i with frame i), per cell d = |S - S_key| and the cell is CHANGED
 * iff d > level_q * area (strict, 64-bit; area = the valid pixels of the cell: edge cells are smaller; level_q in
 * 0 .. 32768, 64 per grey level of mean absolute change):
 *   changed  n uint32            the number of changed cells of the frame (changed / (gh * gw) is the share)
 *   sad      n uint64            the sum of d over the cells (sad / (64 * out_h * out_w) is the mean absolute change per pixel)
 *   mask     n x gh x gw uint8   1 where a cell changed; rows `mask_pitch` bytes apart (>= gw), gh * mask_pitch from frame to
 *                                frame; bytes between rows are not written
 * changed and sad are OVERWRITTEN; being integer sums they are exact and independent of the order of arrival.  A NULL output
 * is left out.  Sizes are at most 32768.  Argument errors (a NULL input, a size < 1 or > 32768, out_h > H, out_w > W, a cell
 * other than 8 / 16 / 32 / 64, level_q outside 0 .. 32768, all outputs NULL, a result asked for without a key, a mask pitch
 * smaller than a row, n larger than the bound batch, a buffer that is not an image input) return ACCEL_ERR_ARG before
 * anything is enqueued, with a message that names the argument.
 *   accel_frame_change          operator level: host image (and key signature) in, host results out (the parity tests).
 *                               sig_key = NULL: the signature only -- asking for changed, sad or mask is then an error
 *   accel_model_frame_change    on the image input `buf` (`data` or `data_key`; H, W as the bound plans read it) of a model,
 *                               enqueued on the context stream.  What is read is what the plans would read: the frame bound
 *                               with accel_model_bind_device if there is one.  It only reads `buf`: no write generation
 *                               changes, no captured graph is touched.  It writes the model-owned CURRENT signature (allocated
 *                               on first use, freed with the model) and compares it with the model's KEPT signature if one
 *                               exists that was made under the same (n, out_h, out_w, cell): *compared is then 1 and the
 *                               results are written -- host destinations (dst_on_device = 0) are filled when the call
 *                               returns, device destinations (= 1: all of them, changed 4-byte and sad 8-byte aligned) when
 *                               the stream reaches them.  Otherwise *compared is 0 and the result pointers are not written
 *   accel_model_frame_keep      the current signature becomes the kept one: a stream-ordered copy inside HBM of gh * gw words
 *                               per frame.  An argument error while no signature has been made */
int accel_frame_change(accel_ctx* ctx, const float* img, const int32_t* sig_key /* NULL: signature only */, int n, int H, int W, int out_h, int out_w,
                       int cell, int level_q, int32_t* sig_out, uint32_t* changed, uint64_t* sad, uint8_t* mask, size_t mask_pitch);
int accel_model_frame_change(accel_model* m, const char* buf, int n, int out_h, int out_w, int cell, int level_q, uint32_t* changed, uint64_t* sad,
                             uint8_t* mask, size_t mask_pitch, int dst_on_device, int* compared);
int accel_model_frame_keep(accel_model* m);

/* ---- finished frames: per-class areas, boxes, centroids and label churn -------------------------------------------------
 * What is in a finished frame, where, and did it just change -- with no ground truth and no label map crossing PCIe: a few
 * hundred bytes per frame (csrc/labels_summary.hip).  The geometry vocabulary is that of the finished-frames block: `labels`
 * is n x H x W uint8, its valid region out_h x out_w, the source frame h x w, and source pixel (y, x) has the label
 *   L(f, y, x) = labels[f][min(y * out_h / h, out_h - 1)][min(x * out_w / w, out_w - 1)]
 * For every frame f and class k in 0 .. ncls - 1 (ncls in 1 .. 32; ids >= ncls are ignored, as the confusion matrix ignores
 * them), integers throughout:
 *   stats    n x ncls x 3 uint64      (area, sum_x, sum_y) over the source pixels with L == k; a sum reaches 2^15 * 2^30.  The
 *                                     centroid is (sum_x / area, sum_y / area)
 *   box      n x ncls x 4 int32       (x0, y0, x1, y1), the INCLUSIVE extremes of those pixels in source coordinates; a class
 *                                     with no pixel has (w, h, -1, -1), the identities of min and max
 *   trans    n x ncls x ncls uint64   against `prev`, the previous frame's labels AT THE SOURCE SIZE (n x h x w, frame i with
 *                                     frame i): trans[f][p * ncls + c] = the source pixels with prev == p < ncls and L == c < ncls
 *                                     (rows the previous frame, columns the current one).  Its off-diagonal share is the label
 *                                     churn; the IoU per class of it is the temporal IoU
 *   kept     n x h x w uint8          the current map at the source size: what accel_labels_to_source writes, and the `prev` of
 *                                     the next frame.  Rows `kept_pitch` bytes apart; bytes between rows are not written
 * All of them are OVERWRITTEN; being integer sums, minima and maxima they are exact and independent of the order of arrival.
 * A NULL output is left out; at least one of stats / box / trans is given (or kept_out, at operator level).  One pass over
 * the source pixels computes all of them; nothing outside out_h x out_w of `labels` is read.  The specification is
 * accel_amd/utils/image.py labels_summary_host and the kernel equals it bit for bit.
 * Argument errors (a NULL input, a size < 1 or > 32768, out_h > H, out_w > W, ncls outside 1 .. 32, a pitch smaller than a
 * row, all outputs NULL, trans without prev -- at model level: with track = 0 --, n larger than the bound batch, no `labels`
 * / `logits` buffer) return ACCEL_ERR_ARG before anything is enqueued, with a message that names the argument.
 *   accel_labels_summary          operator level: host bytes in, host results out (the parity tests)
 *   accel_model_labels_summary    on the model's `labels` buffer (H, W as the bound plans write it), enqueued on the context
 *                                 stream after the run that wrote it.  It only reads `labels`: no write generation changes, no
 *                                 captured graph is touched.  track = 1 compares with the model-owned KEPT map (n x h x w,
 *                                 allocated on first use, freed with the model) if that was made under the same (n, h, w,
 *                                 ncls): *compared is then 1 and trans is written; otherwise *compared is 0 and trans is not
 *                                 written.  Either way the current map becomes the kept one, in the same pass.  track = 0
 *                                 neither reads nor writes the kept map (*compared = 0).  Host destinations (dst_on_device =
 *                                 0) are filled when the call returns, device destinations (= 1: all of them, stats and trans
 *                                 8-byte and box 4-byte aligned) when the stream reaches them
 *   accel_model_scores_summary    the same of the labels of the bilinearly INTERPOLATED scores (accel_model_scores_labels):
 *                                 they are written into the model's n x h x w scratch and summarised at the identity geometry.
 *                                 `ncls` is the summary's class count, 1 .. 32; the class count of the scores is that of
 *                                 `logits`.  It only reads `logits`.  One kept map serves both forms
 *   accel_model_labels_forget     drops the kept map (a new clip, a cut): the next tracked call compares with nothing.  Not an
 *                                 error when there is none */
int accel_labels_summary(accel_ctx* ctx, const uint8_t* labels, int n, int H, int W, int out_h, int out_w, int h, int w, int ncls,
                         const uint8_t* prev /* NULL, or n x h x w */, size_t prev_pitch,
                         uint64_t* stats, int32_t* box, uint64_t* trans, uint8_t* kept_out /* NULL, or n x h x w */, size_t kept_pitch);
int accel_model_labels_summary(accel_model* m, int n, int out_h, int out_w, int h, int w, int ncls, int track,
                               uint64_t* stats, int32_t* box, uint64_t* trans, int dst_on_device, int* compared);
int accel_model_scores_summary(accel_model* m, int n, int out_h, int out_w, int h, int w, int ncls, int track,
                               uint64_t* stats, int32_t* box, uint64_t* trans, int dst_on_device, int* compared);
int accel_model_labels_forget(accel_model* m);

/* ---- finished frames: connected components, the objects of every class ---------------------------------------------------
 * The summary above says "class car covers 3 % of the frame, inside this box"; this says "four cars, here, here, here and
 * here" (csrc/labels_components.hip).  The geometry vocabulary and L(f, y, x) are those of the summary.  A source pixel with
 * L >= ncls (ncls in 1 .. 32) is background: it belongs to no component and separates components.  Two other pixels of one
 * frame are joined when their labels are equal and they are 4-adjacent -- with connectivity = 8 also when they are diagonally
 * adjacent; a component is a class of the transitive closure and its ANCHOR is its first pixel in raster order (the smallest
 * y * w + x).  Frames never join.  The REPORTED components of a frame are those with area >= min_area (>= 1), in ascending
 * anchor order:
 *   count    n int32                        the reported components of the frame: the full number, also above max_components
 *   comp     n x max_components x 8 int32   (class, area, x0, y0, x1, y1, ax, ay) of the first min(count, max_components) of
 *                                           them: the inclusive box and the anchor; -1 in the records after them
 *   sums     n x max_components x 2 uint64  (sum_x, sum_y) over the component's source pixels (the centroid is sum / area); 0
 *                                           in the unused records
 *   ids      n x h rows of w int32, `ids_pitch` bytes apart (>= 4 * w, a multiple of 4): per source pixel the index of its
 *            component's record; -1 for background, for components below min_area and for components beyond
 *            max_components.  Only the w words of a row are written
 * count is required; comp, sums and ids may each be NULL.  max_components is in 1 .. 65536.  All of it is integer and exact:
 * the specification is accel_amd/utils/image.py labels_components_host and the kernels equal it bit for bit.  Nothing outside
 * out_h x out_w of `labels` is read.  Argument errors (a NULL handle, labels or count, a size < 1 or > 32768, out_h > H,
 * out_w > W, ncls outside 1 .. 32, connectivity other than 4 or 8, min_area < 1, max_components outside 1 .. 65536, an
 * ids_pitch below 4 * w or not a multiple of 4, a misaligned device destination, n larger than the bound batch, no `labels` /
 * `logits` buffer, scores of another class count than ncls) return ACCEL_ERR_ARG before anything is enqueued.
 *   accel_labels_components         operator level: host bytes in, host results out (the parity tests)
 *   accel_model_labels_components   on the model's `labels` buffer, enqueued on the context stream after the run that wrote it.
 *                                   It only reads `labels`.  The scratch (two int32 per source pixel and one per 1024 of them)
 *                                   is model-owned, allocated on first use, kept for the next frame and freed with the model.
 *                                   Host destinations (dst_on_device = 0) go through the staging buffer and the call waits;
 *                                   device destinations (4-byte aligned, sums 8-byte) are enqueued only
 *   accel_model_scores_components   the same with the labels of the bilinearly interpolated scores (accel_model_scores_labels):
 *                                   ncls must be the class count of `logits`.  It only reads `logits` */
int accel_labels_components(accel_ctx* ctx, const uint8_t* labels, int n, int H, int W, int out_h, int out_w, int h, int w, int ncls,
                            int connectivity, int min_area, int max_components,
                            int32_t* count, int32_t* comp, uint64_t* sums, int32_t* ids, size_t ids_pitch);
int accel_model_labels_components(accel_model* m, int n, int out_h, int out_w, int h, int w, int ncls, int connectivity, int min_area,
                                  int max_components, int dst_on_device, int32_t* count, int32_t* comp, uint64_t* sums, int32_t* ids,
                                  size_t ids_pitch);
int accel_model_scores_components(accel_model* m, int n, int out_h, int out_w, int h, int w, int ncls, int connectivity, int min_area,
                                  int max_components, int dst_on_device, int32_t* count, int32_t* comp, uint64_t* sums, int32_t* ids,
                                  size_t ids_pitch);

/* ---- finished frames: trimap evaluation, the confusion matrix in bands around the ground truth's boundaries ------------
 * Whole-frame mIoU is dominated by interior pixels; what feature propagation costs sits at object boundaries.  For a
 * ground-truth map g (h x w uint8, rows `gt_pitch` apart; the frames of a batch are independent):
 *   edge pixel    one of its 4-neighbours INSIDE the frame holds another byte (raw bytes: the border between a class and an
 *                 ignored id is an edge; a neighbour outside the frame is never different)
 *   d(y, x)       min(cap, min over edge pixels (y', x') of max(|y - y'|, |x - x'|)): the Chebyshev distance to the nearest
 *                 edge pixel, 0 on one, cap where none lies closer and where the map has no edge
 *   widths        1 .. 4 strictly ascending ints in 1 .. 16; cap = the last one.  Bucket b < nwidths holds the pixels with
 *                 widths[b - 1] <= d < widths[b] (0 for b = 0), bucket nwidths the rest
 *   counting      a source pixel adds 1 to hist[b][gt * ncls + pred] when gt < ncls and pred < ncls, pred by the nearest rule
 *                 of accel_labels_hist: (nwidths + 1) * ncls * ncls uint64.  The band of width widths[b] is the sum of the
 *                 buckets 0 .. b (taken by the caller); the sum of ALL buckets is the matrix accel_labels_hist gives
 * (accel_amd/utils/image.py boundary_distance_host, band_hist_host; csrc/labels_band.hip).  Integer arithmetic: exact.
 * Argument errors (a NULL pointer, nwidths outside 1 .. 4, a width or cap outside 1 .. 16, widths not strictly ascending,
 * ncls outside 1 .. 32, a size < 1 or > 32768, out_h > H, out_w > W, a pitch smaller than a row, a model without `labels` /
 * `logits` of n frames, other ncls or widths than the accumulator's since its last clear) return ACCEL_ERR_ARG before
 * anything is enqueued, with a message that names the argument.
 *   accel_boundary_distance       host maps (n x h rows, `pitch` apart) in, d out as bytes (rows `dst_pitch` apart; bytes
 *                                 between rows are not written).  Any label maps: ground truth or fetched predictions;
 *                                 d == 0 is the outline a viewer draws.  Stateless
 *   accel_labels_band_hist        operator level, host bytes: the buckets are ADDED to `hist`.  Stateless
 *   accel_model_band_hist_add     the same on the model's `labels` buffer, enqueued on the context stream (gt_on_device as
 *                                 in accel_model_hist_add), into an accumulator of the model's own that is SEPARATE from
 *                                 the one of accel_model_hist_add: it remembers ncls and widths and refuses other values
 *                                 until it has been cleared; freed with the model
 *   accel_model_scores_band_hist_add   with the labels of the bilinearly INTERPOLATED scores (accel_model_scores_labels),
 *                                 through the model's n x h x w scratch: the same accumulator
 *   accel_model_band_hist_read    waits for the stream and copies (nwidths + 1) * ncls * ncls words to the host (zeros
 *                                 when nothing was added since the last clear); clear = 1 zeroes the accumulator */
int accel_boundary_distance(accel_ctx* ctx, const uint8_t* maps, int n, int h, int w, size_t pitch, int cap, uint8_t* dst, size_t dst_pitch);
int accel_labels_band_hist(accel_ctx* ctx, const uint8_t* labels, int n, int H, int W, int out_h, int out_w,
                           const uint8_t* gt, int h, int w, size_t gt_pitch, int ncls, const int* widths, int nwidths, uint64_t* hist);
int accel_model_band_hist_add(accel_model* m, const uint8_t* gt, int n, int h, int w, size_t gt_pitch, int out_h, int out_w, int ncls,
                              const int* widths, int nwidths, int gt_on_device);
int accel_model_scores_band_hist_add(accel_model* m, const uint8_t* gt, int n, int h, int w, size_t gt_pitch, int out_h, int out_w, int ncls,
                                     const int* widths, int nwidths, int gt_on_device);
int accel_model_band_hist_read(accel_model* m, uint64_t* out, int ncls, int nwidths, int clear);

/* ---- finished frames: the overlay in the frame's own format ------------------------------------------------------------
 * The label map blended over NV12, I420 / YV12, P010 or YUY2 frames and written as the same format in the same layout
 * (csrc/overlay_yuv.hip): what an encoder, a compositor or a capture-card output takes, with no BGR picture in between.
 * `layout` as for the frame routes, checked by their rules, with format 3 = NV12 as for the _sited entry points (u_offset =
 * the chroma plane, rows `pitch` apart, pitch_c = v_offset = 0); h x w of the geometry above are layout->h x layout->w.
 * `layout->colour` is NOT looked at: the colours arrive as palette_ycc, 256 x 3 uint16 (Y, Cb, Cr) per label in the units
 * of the samples (0 .. 255; 0 .. 1023 for P010), which the caller makes once from an R, G, B palette with the standard's
 * forward matrix -- accel_amd/utils/image.py palette_ycbcr, INTEGRATION.md has the formula.  With a = alpha in 0 .. 256,
 * T the table and L(x, y) the label of source pixel (x, y) under the nearest rule above:
 *   luma            Y'  = (a * T[L(x, y)].Y + (256 - a) * Y + 128) >> 8
 *   4:2:0 chroma    Cb' = (a * S + (256 - a) * 4 * Cb + 512) >> 10 with S the sum of T[L].Cb over the 2 x 2 luma pixels
 *                   (2cx .. 2cx + 1, 2cy .. 2cy + 1) of sample (cx, cy); Cr alike                (NV12, I420 / YV12, P010)
 *   4:2:2 chroma    Cb' = (a * S2 + (256 - a) * 2 * Cb + 256) >> 9 with S2 over the two pixels of the quad; Cr alike  (YUY2)
 *   P010            the operands are word >> 6; the stored word is sample << 6, its low six bits are zero
 * Integer arithmetic, one rounding per sample, no clip needed; alpha = 0 returns every sample unchanged.  The overlay's
 * chroma is the block mean of the palette colours whatever the siting of the frame's own samples, which are blended where
 * they are and are not resited.  The specification is accel_amd/utils/image.py overlay_yuv_host, bit for bit.
 * `dst` has the layout of `frame`.  Bytes that are not samples -- between rows, between planes, after a frame -- are never
 * written in a device `dst`; a host `dst` of (n - 1) * frame_bytes + the extent of a frame bytes holds the input's bytes
 * there.  A device `dst` may be the device `frame` itself (in place on a decoder's surface); any other overlap of the two
 * n * frame_bytes ranges is an error.  The samples of a layout must be distinct bytes (I420 planes that interleave row by
 * row are; planes laid over each other are not, and the result is then undefined).
 * Argument errors (a NULL frame, dst, palette_ycc or layout, a table entry above 255 -- above 1023 for P010 --, an odd
 * device address for P010, and those of the layout, the geometry and alpha) return ACCEL_ERR_ARG before anything is
 * enqueued, with a message that names the argument.
 *   accel_labels_overlay_yuv         operator level: host labels (n x H x W) and frames in, host bytes out (the parity tests)
 *   accel_model_labels_overlay_yuv   on the model's `labels` buffer; frame_on_device / dst_on_device as for
 *                                    accel_model_labels_colour.  It only reads `labels`: no write generation changes
 *   accel_model_scores_overlay_yuv   the same with the labels of the interpolated scores (accel_model_scores_labels), made
 *                                    into a library-owned scratch first; it only reads `logits` */
int accel_labels_overlay_yuv(accel_ctx* ctx, const uint8_t* labels, int n, int H, int W, int out_h, int out_w, const accel_yuv_layout* layout,
                             const uint16_t* palette_ycc, int alpha, const uint8_t* frame, uint8_t* dst);
int accel_model_labels_overlay_yuv(accel_model* m, int n, int out_h, int out_w, const accel_yuv_layout* layout, const uint16_t* palette_ycc,
                                   int alpha, const uint8_t* frame, int frame_on_device, uint8_t* dst, int dst_on_device);
int accel_model_scores_overlay_yuv(accel_model* m, int n, int out_h, int out_w, const accel_yuv_layout* layout, const uint16_t* palette_ycc,
                                   int alpha, const uint8_t* frame, int frame_on_device, uint8_t* dst, int dst_on_device);

/* whole-frame entry points, the two Predictor.predict calls of the demo loop
 * (demo.py:235-245; tester.py:158-171 im_segment).  img_*: fp32 1x3xHxW already
 * mean-subtracted (lib/utils/image.py:224-235).  Any output pointer may be NULL.
 * feat_out / logits_out are NCHW fp32, labels_out uint8 HxW (first-max argmax).
 * The propagated feature stays in HBM between calls: in persistent buffer
 * `feat`, or -- when the non-key graph was bound as the plan pair `cur` /
 * `cur_b` (accel_amd/lower.py, feat_slot) -- alternately in `feat` and
 * `feat_b`; accel_cur_forward runs the plan that reads the buffer written
 * last, so callers never see the difference.  A host upload goes to `feat`. */
int accel_key_forward(accel_model* m, const float* img, int img_on_device,
                      float* feat_out, float* logits_out, uint8_t* labels_out, int out_on_device);
int accel_cur_forward(accel_model* m, const float* img_cur, const float* img_prev, int img_on_device,
                      float* feat_out, float* logits_out, uint8_t* labels_out, int out_on_device);

/* ---- operator level (host fp32 NCHW in / out; used by the parity tests) --------
 * Each is the single MXNet operator named, run through the same kernels and the
 * same weight repacking as the plans.  N >= 1 for conv / deconv / deformable conv / pool (the
 * convolution kernel runs the batch as one GEMM with M = N*Ho*Wo). */
/* mx.symbol.Convolution (+ optional per-channel scale/shift, residual, activation:
 * the fused epilogue).  act: 0 none, 1 relu, 2 leaky(slope).  force_tile: -1 = the library's choice, otherwise a launch
 * geometry id of conv_igemm.hip (every accepted id computes the same contraction; ids the build does not carry are
 * rejected with ACCEL_ERR_ARG -- timing-only ablation variants exist only in the diagnostics build). */
int accel_conv2d(accel_ctx* ctx, const float* x, int N, int C, int H, int W,
                 const float* w, const float* bias, int K, int kh, int kw,
                 int sh, int sw, int ph, int pw, int dh, int dw,
                 const float* scale, const float* shift, const float* residual,
                 int act, float slope, int force_tile, float* y);
/* mx.symbol.Deconvolution 4x4 stride 2 pad 1 (== pad 0 + Crop(offset 1,1)) */
int accel_deconv2d_4x4s2(accel_ctx* ctx, const float* x, int N, int C, int H, int W,
                         const float* w, const float* bias, int K, int act, float slope, float* y);
/* mx.contrib.symbol.DeformableConvolution, no bias */
int accel_deform_conv2d(accel_ctx* ctx, const float* x, int N, int C, int H, int W,
                        const float* offset, const float* w, int K, int kh, int kw,
                        int sh, int sw, int ph, int pw, int dh, int dw, int dg, float* y);
/* mx.symbol.Pooling; optional BN scale/shift + relu epilogue */
int accel_pool2d(accel_ctx* ctx, const float* x, int N, int C, int H, int W, int is_max, int full,
                 int kh, int kw, int sh, int sw, int ph, int pw,
                 const float* scale, const float* shift, int relu, float* y);
/* GridGenerator(transform_type='warp') + BilinearSampler == the "FlowWarp" op */
int accel_flow_warp(accel_ctx* ctx, const float* feat, int C, int H, int W, const float* flow, float* out);
/* Deconvolution 32x32/16 group=ncls + Crop(8,8) [+ Concat + correction 1x1] + argmax.
 * right/wr/cw/cb may be NULL (single head). Hs,Ws = score size; output H=16*Hs, W=16*Ws */
int accel_score_fuse(accel_ctx* ctx, const float* left, const float* right, int ncls, int Hs, int Ws,
                     const float* wl, const float* wr, const float* cw, const float* cb,
                     float* logits, uint8_t* labels);
/* mx.ndarray.argmax(axis=1) of an NCHW tensor (first maximal index) */
int accel_argmax_c(accel_ctx* ctx, const float* logits, int C, int H, int W, uint8_t* labels);
/* FlowNet input stage: avgpool2(concat(cur/255, prev/255)) -> 6 x H/2 x W/2 */
int accel_flow_input(accel_ctx* ctx, const float* cur, const float* prev, int H, int W, float* out);

/* ---- multi-GPU: the one collective of the path -------------------------------------------------------
 * Clips are sharded over ranks with no activation exchange; each frame's logits (or label map) are gathered to a root
 * rank.  Stands in for the host-side merge of per-GPU results in the reference's multi-GPU tester
 * (dff_rfcn/function/test_rcnn.py:62-82, dff_rfcn/core/tester.py:290-298: one thread per GPU, results appended on the
 * host).  One process per GPU; RCCL (librccl, resolved at run time) point-to-point send/recv over xGMI: every peer
 * uses its own direct link to the root, no ring.
 *   accel_comm_available   0 if THIS process can resolve librccl and every entry point the gather uses (no communicator, no
 *                          network activity); else an error whose text says what is missing.  Every rank calls it and the
 *                          ranks agree on the outcome BEFORE any of them enters accel_comm_create (ncclCommInitRank blocks
 *                          until all ranks have arrived: a rank that cannot load the library must not leave the others there)
 *   accel_comm_unique_id   128-byte id, made on one rank and distributed by the caller (file, socket, torch.distributed)
 *   accel_comm_create      communicator of `nranks` processes, this one being `rank`, bound to ctx's device; owns a
 *                          communication stream and two staging slots
 *   accel_gather_logits    every rank contributes `bytes` at `sendbuf` (HBM); the root receives rank r's block at
 *                          recvbuf + r*bytes (recvbuf is NULL on the other ranks).  Asynchronous: sendbuf is copied
 *                          into a staging slot in compute-stream order (so the next frame may overwrite it at once), the
 *                          transfer runs on the communication stream beside the next frame's kernels.  recvbuf must
 *                          stay untouched until accel_comm_sync() or the second-next gather.
 *   accel_comm_sync        host wait for all gathers issued so far */
typedef struct accel_comm accel_comm;
int accel_comm_available(void);
int accel_comm_unique_id(void* id128);
int accel_comm_create(accel_ctx* ctx, int rank, int nranks, const void* id128, accel_comm** out);
int accel_comm_destroy(accel_comm* comm);
int accel_gather_logits(accel_comm* comm, const void* sendbuf, void* recvbuf_or_null, size_t bytes, int root);
/* the same with a ROOT that contributes fewer bytes than a full slot (`bytes` = slot size = what every peer sends; the root, which
 * also receives all the others' frames, may be given fewer clips: send_bytes <= bytes on the root, == bytes elsewhere) */
int accel_gather_frames(accel_comm* comm, const void* sendbuf, size_t send_bytes, void* recvbuf_or_null, size_t bytes, int root);
/* The gather at SCORE resolution -- the default payload of bench.py --gpus N.  When the two upsampling filters are the same for every
 * class (the reference freezes them at the bilinear initialisation, accel_18.py:153) the plans fuse the two heads at score resolution
 * and leave the fused map in the model's persistent buffer `scores` ([images][H/16][W/16][ncls rounded up to 4] fp32, 0.66 MB per
 * 1024x2048 frame); the fp32 logits (159 MB) are a pure function of it.
 *   (A key plan's tail has ONE head and no correction bias, a non-key plan's the fused two: the expansion belongs to a PLAN.  Both leave
 *   their map in the same `scores` buffer; every rank passes the plan it has just run -- the ranks of a job run the same schedule.)
 *   accel_expand_scores   logits + labels of n_images maps at scores_dev (HBM, layout of `scores`) by the very launch plan p ends
 *                         with: bit-identical to the logits the producing GPU computed.  Enqueued on the model's compute
 *                         stream, or on a communicator's communication stream (on_comm_stream_of != NULL).
 *   accel_gather_scores   accel_gather_frames of the `scores` buffer (own_images of the slot_images a rank's slot holds; only the
 *                         root may contribute fewer) followed, on the root and on the communication stream, by the expansion of every
 *                         rank's block into logits_out / labels_out ([nranks * slot_images] images); valid after accel_comm_sync.
 * ACCEL_ERR_PLAN if the model has no `scores` buffer (filters not uniform): gather the logits then.  (Reference pattern: per-device
 * results merged on the host, dff_rfcn/function/test_rcnn.py:62-82.) */
int accel_expand_scores(accel_plan* p, const void* scores_dev, int n_images, float* logits_dev, unsigned char* labels_dev, accel_comm* on_comm_stream_of);
int accel_gather_scores(accel_comm* comm, accel_plan* p, int own_images, int slot_images, void* recv_scores_or_null, float* logits_out_or_null,
                        unsigned char* labels_out_or_null, int root);
int accel_comm_sync(accel_comm* comm);

#ifdef __cplusplus
}
#endif
#endif

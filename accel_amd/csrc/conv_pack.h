// Host side of a convolution's parameter block: weight repacking, the tap table and the epilogue constants.  Standard C++ on host
// vectors, no HIP: accel_hip.cpp (finalize_conv) uploads what these functions return, tests/host/conv_pack_check.cpp checks them on the
// CPU.  The Winograd, stem and weight-stationary packers stay beside their kernels (kernels.h).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

// ---- packed fp32 weights: [class][rows][K_pad] -------------------------------------------------------------------------------------
// conv weights (Cout, Cin, kh, kw) -> [rows][K_pad], k = (ky*kw + kx)*cin_pad + ci
void pack_conv_w(const float* w, int Cout, int Cin, int kh, int kw, int cin_pad, int rows, int K_pad, std::vector<float>& out);
// deconv 4x4 s2 p1 weights (Cin, Cout, 4, 4) -> [4 classes][rows][K_pad]; class (py,px), tap (ty,tx):
// ky = 3 - py - 2*ty, kx = 3 - px - 2*tx ; k = (ty*2 + tx)*cin_pad + ci
void pack_deconv2x_w(const float* w, int Cin, int Cout, int cin_pad, int rows, int K_pad, std::vector<float>& out);

// ---- the planes the matrix-core kernels read -----------------------------------------------------------------------------------------
// One plane holds every (class, row, k) of the packed weights once, K in steps of 32, in one of two orders:
//   CONV_ORDER_STEP  [class][K step][row][32]: the tile a block fetches per K step (BN rows x 32 k) is ONE contiguous run of BN x 64
//                    bytes -- whole cache lines, where the row-major order gave 64-byte pieces 2 * K_pad bytes apart (conv_igemm.hip)
//   CONV_ORDER_FRAG  [class][K step][half step][row][16], the MFMA fragment order: the 16 bytes lane (row, half) feeds to one
//                    v_mfma_f32_32x32x16_bf16 are contiguous (k = 32*step + 16*halfstep + 8*half .. +8), a wavefront's fragment fetch
//                    is one contiguous kilobyte; weights go global -> VGPR, never through LDS (conv_b3r.hip, conv_b3d.hip)
// and ends in two K steps of slack (2 * rows * 32 zero elements): the kernels prefetch past the end.
enum ConvOrder { CONV_ORDER_STEP, CONV_ORDER_FRAG };

inline size_t conv_plane_elems(int classes, int rows, int K_pad) { return (size_t)classes * rows * K_pad + 2 * (size_t)rows * 32; }

inline size_t conv_plane_index(ConvOrder order, int rows, int K_pad, int c, int n, int k)
{
    const int steps = K_pad / 32;
    if (order == CONV_ORDER_STEP) return (((size_t)c * steps + k / 32) * rows + n) * 32 + (k & 31);
    return ((((size_t)c * steps + k / 32) * 2 + ((k >> 4) & 1)) * rows + n) * 16 + (k & 15);
}

// the exact three-term bf16 split of an fp32 value: the top 16 bits, then those of the residual, twice (t[0] + t[1] + t[2] == v)
void bf16_split3(float v, uint16_t t[3]);

// bf16x3 form (ConvParams::wb3 in CONV_ORDER_STEP, ::wb3r in CONV_ORDER_FRAG): three planes of conv_plane_elems, term by term
void pack_bf16x3(const std::vector<float>& packed, int classes, int rows, int K_pad, ConvOrder order, std::vector<uint16_t>& out);
// f16-mode layers: the half-rounded weights [class][rows][K_pad] once more as one plane in fragment order, for the fp16 form of
// conv_b3r.hip and for conv_b3d.hip
void pack_f16r(const std::vector<_Float16>& half, int classes, int rows, int K_pad, std::vector<_Float16>& out);
// fp16x2 form (ConvParams::wh2r): two planes in fragment order, every weight as hi + lo, two half terms of w * 2^q[row], the
// exponent q[row] chosen so that the largest weight of the output channel (over all parity classes) lands in [2^14, 2^15) -- the
// top of the half range, where lo keeps its full 11 bits (the pair: 2^-23 relative) for every weight down to 2^-16 of the channel's
// largest; below that the absolute error is 2^-25 of the scaled value, i.e. 2^-39 to 2^-40 of the largest: a bit lost per octave
// (tests/test_h2_model_cpu.py; on the device, half subnormals included: tests/test_h2_octaves_gpu.py).  The Winograd planes
// (conv_wino_b3_pack_h2) split U = G g G^T the same way, one octave higher, because they pay that absolute error at 16 positions
// against |V| <= 4 max|x|.
// qexp receives q per row; the epilogue scale is multiplied by 2^-q (exact: conv_h2_scale).
void pack_h2r(const std::vector<float>& packed, int classes, int rows, int K_pad, std::vector<uint16_t>& out, std::vector<int>& qexp);

// ---- tap table ---------------------------------------------------------------------------------------------------------------------
// One int4 per 4-wide K granule g (k = 4 g, tap = k / Cin = ky * kw + kx, ci = k % Cin), per parity class G + CONV_TAP_SLACK of them
// with G = K_pad / 4:
//   {ky * dh, kx * dw, ((ky * dh * W + kx * dw) * xCs + ci) * esize, 0}      dy, dx, input byte offset relative to tap 0 / channel 0
// FAST shapes read it wave-uniformly through the scalar unit, the others per lane.  Padded K (tap >= kh * kw) and the slack entries
// (the pipelined kernels prefetch up to two K steps past the end) carry CONV_TAP_OUT in their first word and zeros behind it.
constexpr int CONV_TAP_SLACK = 48;
constexpr int CONV_TAP_OUT = -(1 << 28);
void conv_tap_table(int classes, int K_pad, int Cin, int kh, int kw, int dh, int dw, int W, int xCs, int esize, std::vector<int>& tab);

// ---- epilogue constants ------------------------------------------------------------------------------------------------------------
// BatchNorm inference folding -- identical expressions to oracle orc_bn_fold (MXNet mshadow inference form):
// scale = g/sqrt(var+eps), shift = beta - g*mean/sqrt(var+eps); gamma null: fixed at 1
void bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, float eps, int C,
             std::vector<float>& scale, std::vector<float>& shift);
// y = conv * scale + shift over `rows` channels of which `cout` are real (1 / 0; the padding rows 0 / 0): the folded BatchNorm
// (bn_scale / bn_shift, null: none), then the bias (shift += bias * scale), then mul on both
void conv_fold_epilogue(int rows, int cout, const std::vector<float>* bn_scale, const std::vector<float>* bn_shift, const float* bias,
                        const float* mul, std::vector<float>& scale, std::vector<float>& shift);
// the second output's pair: out2 = relu(v + bias2) (scale 1), or the folded BatchNorm bn2
void conv_fold_epilogue2(int rows, int cout, const float* bias2, const std::vector<float>* bn_scale, const std::vector<float>* bn_shift,
                         std::vector<float>& scale2, std::vector<float>& shift2);
// the epilogue scale of an fp16x2 form: scale[i] * 2^(k - q[i]) for the first n channels (exact), 0 behind them
void conv_h2_scale(const std::vector<float>& scale, const std::vector<int>& q, int n, int k, std::vector<float>& out);

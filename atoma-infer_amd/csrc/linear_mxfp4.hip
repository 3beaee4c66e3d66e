// MXFP4 (OCP microscaling: e2m1 elements, one e8m0 scale per block of 32 inputs) WEIGHTS for the decode-step projections, "W4A16":
//   y[b][n] = round(sum_k x[b][k] * e2m1(nibble[n][k]) * 2^(w_scale[n][k / 32] - 127)), batch <= 16.
//
// The next step after linear_fp8w.hip in the same direction: at 1..16 rows a projection is a stream over the weights, so the only thing left to
// win is moving fewer bytes -- 0.53 bytes per weight (K/2 nibble bytes + K/32 scale bytes per row) against fp8's 1.  w4 [n][k / 2]: byte i of a
// row holds input 2i in its low nibble and input 2i + 1 in its high nibble (bit 3 the sign, bits 0..2 index {0, .5, 1, 1.5, 2, 3, 4, 6});
// w_scale [n][k / 32] bytes.  e2m1 x 2^e is an exact bf16 / f16 number and gfx950 converts a byte to a packed pair with the block scale applied
// in one instruction (v_cvt_scalef32_pk_{bf16,f16}_fp4, scale operand as_float(byte << 23)), so everything behind the conversion is the 16-bit
// kernels' arithmetic (v_dot2c / v_mfma_f32_16x16x32, fp32 accumulation); nothing is scaled per element afterwards and nothing after the sum.
// The kernels (1..4 rows linear_wq_gemv_kernel, 5..16 rows linear_wq_wg_kernel), their launchers and the entry are linear_wq.h's, the ones fp8
// weights run, instantiated with the format below (Mx4Blocks): a 16-byte load is exactly one MX block (32 inputs, one scale) and four operand
// fragments, one per word; a slab is therefore 512 inputs, and its last one may hold 128, 256 or 384.  The scale bytes of a slab come with ONE
// more load instruction per 16 rows (against four for the nibbles): a dword is the four scales of a 128-input chunk.  More than 16 rows is
// refused: the fp8 17..64-row structure loses to 16-bit weights and is not copied.
// Out of scope here: the fused RMSNorm and q/k/v + RoPE + cache forms, 17 rows and more, MX activations (the mfma_scale_*_f8f6f4 path).
// atoma_quantize_weight_mxfp4 at the bottom: round to nearest, ties to the even code, saturating at 6; one thread per block of 32 inputs.
#include "linear_wq.h"

namespace atoma {

// byte SEL of `word` (inputs 2.SEL and 2.SEL + 1 of the word's 8: low nibble, then high nibble) -> one packed pair of T, times the block scale
template <typename T, int SEL> __device__ __forceinline__ uint32_t w4_pair(uint32_t word, float scale);
#define ATOMA_W4_PAIR(SEL)                                                                                                                          \
    template <> __device__ __forceinline__ uint32_t w4_pair<bf16_t, SEL>(uint32_t word, float scale) {                                              \
        return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, scale, SEL));                                           \
    }                                                                                                                                               \
    template <> __device__ __forceinline__ uint32_t w4_pair<f16_t, SEL>(uint32_t word, float scale) {                                               \
        return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(word, scale, SEL));                                            \
    }
ATOMA_W4_PAIR(0)
ATOMA_W4_PAIR(1)
ATOMA_W4_PAIR(2)
ATOMA_W4_PAIR(3)
#undef ATOMA_W4_PAIR
// one word (8 nibbles) -> 8 values of T in element order: one MFMA A operand, or four dot2 operands
template <typename T> __device__ __forceinline__ lu32x4 w4_frag(uint32_t word, float scale) {
    return lu32x4{w4_pair<T, 0>(word, scale), w4_pair<T, 1>(word, scale), w4_pair<T, 2>(word, scale), w4_pair<T, 3>(word, scale)};
}

// ---- the format of linear_wq.h's kernels -----------------------------------------------------------------------------------------------------
// A slab is 512 inputs = 4 KiB per load round of a wavefront, the same bytes as a 256-input slab of fp8 weights; a row of W is a quarter of the
// 16-bit row, so K = 4096 is 8 slabs.  The depth rule of waves_per_workgroup (at least 4 units per wavefront) is fed `units per slab` units for
// each slab, measured per kernel: the VALU kernel 2 (two slabs per wavefront: q/k/v at 1 row 5.9 us against 6.5) under at most
// 16 wavefronts per CU (gate/up at 1 row: two wavefronts per workgroup 13.2 us, four 15.5), the MFMA kernel 1 (four slabs per wavefront, as
// everywhere else).
struct Mx4Blocks {
    static constexpr int CH = 4;                                 // a slab: 512 inputs
    static constexpr bool kBlockScales = true;                   // one e8m0 byte per 32 inputs, applied in the conversion
    struct Args { LinearParams p; Mx4Scales sp; };
    static Args args(const LinearParams &p, const void *w_scale, int64_t scale_row_stride) { return Args{p, Mx4Scales{static_cast<const uint8_t *>(w_scale), scale_row_stride}}; }
    // one fragment per word, all under the block's scale
    template <typename T> static __device__ __forceinline__ lu32x4 frag(const lu32x4 &v, int h, float scale) { return w4_frag<T>(v[h], scale); }

    static constexpr const char *kName = "linear_decode_mxfp4", *kW = "w4";
    static constexpr int kMaxBatch = 16, kInputsPerByte = 2;
    static constexpr const char *kBatchRule = "batch must be in [0, 16] (the MXFP4-weight kernels serve 1..16 rows; more than 16 rows is not supported)";
    static constexpr const char *kScaleRule = "w_scale must be 4-byte aligned e8m0 bytes [out_features, in_features / 32]";
    static constexpr WqPlan kGemvPlan{"ATOMA_MXFP4_GEMV_WAVES_PER_CU", 16, "ATOMA_MXFP4_GEMV_UNITS_PER_SLAB", 2},
                            kWgPlan{"ATOMA_MXFP4_WG_WAVES_PER_CU", 8, "ATOMA_MXFP4_WG_UNITS_PER_SLAB", 1};
    static constexpr int gemv_depth(bool pair, int nb) { return pair ? (nb > 1 ? 1 : 2) : (nb > 2 ? 1 : 2); }
    static constexpr int wg_depth(bool pair) { return pair ? 1 : 2; }
    static int gemv_rows() { static const int v = env_int("ATOMA_MXFP4_GEMV_MAX_BATCH", 4); return v; }
};

// ---- the quantiser -------------------------------------------------------------------------------------------------------------------------
// |v| = |w| . 2^-e (exact) -> the nearest of {0, .5, 1, 1.5, 2, 3, 4, 6}, ties to the even code, saturating at 6 (code 7)
__device__ __forceinline__ uint32_t e2m1_code(float v) {
    return v <= 0.25f ? 0u : v < 0.75f ? 1u : v <= 1.25f ? 2u : v < 1.75f ? 3u : v <= 2.5f ? 4u : v < 3.5f ? 5u : v <= 5.0f ? 6u : 7u;
}

// One thread per (row, block of 32 inputs): amax of the block, e = exponent(amax) - 2 raised to E_MIN (0.5 . 2^e stays a normal number of T;
// 127 for an all-zero block), then 32 codes = 16 bytes and the scale byte e + 127.  The sign bit is the source's sign bit.
template <typename T>
__global__ void __launch_bounds__(256) quantize_weight_mxfp4_kernel(const uint16_t *__restrict__ w, uint8_t *__restrict__ w4, uint8_t *__restrict__ scale_out,
                                                                    int64_t out_features, int blocks_per_row, int64_t w_row_stride, int64_t w4_row_stride,
                                                                    int64_t scale_row_stride) {
    constexpr int E_MIN = std::is_same<T, bf16_t>::value ? -125 : -13;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = i / blocks_per_row;
    const int j = (int)(i - row * blocks_per_row);
    if (row >= out_features) return;
    const uint16_t *src = w + row * w_row_stride + j * 32;
    uint32_t u[16];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        const uint4 v = *reinterpret_cast<const uint4 *>(src + h * 8);
        u[4 * h] = v.x; u[4 * h + 1] = v.y; u[4 * h + 2] = v.z; u[4 * h + 3] = v.w;
    }
    float amax = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) amax = fmaxf(amax, fmaxf(fabsf(lo_to_f32<T>(u[e])), fabsf(hi_to_f32<T>(u[e]))));
    int e = 0;
    if (amax > 0.f) e = max((int)((__float_as_uint(amax) >> 23) & 0xffu) - 127 - 2, E_MIN);
    const float inv = __uint_as_float((uint32_t)(127 - e) << 23);   // 2^-e: e in [-125, 125]
    uint32_t out[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        uint32_t word = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const uint32_t pr = u[4 * h + t];
            const uint32_t lo = e2m1_code(fabsf(lo_to_f32<T>(pr)) * inv) | ((pr >> 12) & 8u);
            const uint32_t hi = e2m1_code(fabsf(hi_to_f32<T>(pr)) * inv) | ((pr >> 28) & 8u);
            word |= (lo | (hi << 4)) << (8 * t);
        }
        out[h] = word;
    }
    *reinterpret_cast<uint4 *>(w4 + row * w4_row_stride + j * 16) = make_uint4(out[0], out[1], out[2], out[3]);
    scale_out[row * scale_row_stride + j] = (uint8_t)(e + 127);
}

}  // namespace atoma

extern "C" int atoma_linear_decode_mxfp4(const void *x, const void *w4, const void *w_scale, void *y, int64_t batch, int64_t in_features,
                                         int64_t out_features, int64_t x_row_stride, int64_t w4_row_stride, int64_t scale_row_stride,
                                         int64_t y_row_stride, int dtype, void *stream) {
    return atoma::linear_wq_entry<atoma::Mx4Blocks>(x, w4, w_scale, y, batch, in_features, out_features, x_row_stride, w4_row_stride, scale_row_stride, y_row_stride, 0, nullptr, 0, dtype, stream);
}
extern "C" int atoma_linear_decode_mxfp4_residual(const void *x, const void *w4, const void *w_scale, const void *residual, void *y, int64_t batch,
                                                  int64_t in_features, int64_t out_features, int64_t x_row_stride, int64_t w4_row_stride,
                                                  int64_t scale_row_stride, int64_t residual_row_stride, int64_t y_row_stride, int dtype, void *stream) {
    return atoma::linear_wq_entry<atoma::Mx4Blocks>(x, w4, w_scale, y, batch, in_features, out_features, x_row_stride, w4_row_stride, scale_row_stride, y_row_stride, 1, residual, residual_row_stride, dtype, stream);
}
extern "C" int atoma_linear_decode_mxfp4_silu_mul(const void *x, const void *w4_gate_up, const void *w_scale, void *y, int64_t batch, int64_t in_features,
                                                  int64_t intermediate, int64_t x_row_stride, int64_t w4_row_stride, int64_t scale_row_stride,
                                                  int64_t y_row_stride, int dtype, void *stream) {
    return atoma::linear_wq_entry<atoma::Mx4Blocks>(x, w4_gate_up, w_scale, y, batch, in_features, 2 * intermediate, x_row_stride, w4_row_stride, scale_row_stride, y_row_stride, 2, nullptr, 0, dtype, stream);
}

extern "C" int atoma_quantize_weight_mxfp4(const void *w, int64_t out_features, int64_t in_features, int64_t w_row_stride, int dtype, void *w4_out,
                                           int64_t w4_row_stride, void *scale_out, int64_t scale_row_stride, void *stream) {
    using namespace atoma;
    clear_error();
    if (dtype != ATOMA_F16 && dtype != ATOMA_BF16) { set_error("quantize_weight_mxfp4: dtype (of the source weights) must be f16 or bf16"); return -1; }
    if (out_features < 0 || out_features > 0x7fffffff) { set_error("quantize_weight_mxfp4: out_features must be in [0, 2^31)"); return -1; }
    if (in_features <= 0 || in_features % 32 != 0 || in_features > 0x7fffffff) { set_error("quantize_weight_mxfp4: in_features must be a positive multiple of 32"); return -1; }
    if (w_row_stride < in_features || w4_row_stride < in_features / 2 || scale_row_stride < in_features / 32) {
        set_error("quantize_weight_mxfp4: row strides must cover a row");
        return -1;
    }
    if (w_row_stride % 8 || w4_row_stride % 16) { set_error("quantize_weight_mxfp4: w_row_stride (elements) must be a multiple of 8, w4_row_stride (bytes) of 16"); return -1; }
    if (!w || !w4_out || (reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(w4_out)) & 15u) {
        set_error("quantize_weight_mxfp4: w and w4_out must be 16-byte aligned");
        return -1;
    }
    if (!scale_out) { set_error("quantize_weight_mxfp4: scale_out must be e8m0 bytes [out_features, in_features / 32]"); return -1; }
    const int64_t blocks = out_features * (in_features / 32);
    if (cdiv(blocks, 256) > 0x7fffffff) { set_error("quantize_weight_mxfp4: out_features * in_features / 32 must stay below 2^39 (one launch)"); return -1; }
    if (out_features == 0) return 0;
    const auto s = static_cast<hipStream_t>(stream);
    const auto src = static_cast<const uint16_t *>(w);
    const auto dst = static_cast<uint8_t *>(w4_out);
    const auto sc = static_cast<uint8_t *>(scale_out);
    const dim3 grid((unsigned)cdiv(blocks, 256));
    if (dtype == ATOMA_BF16)
        hipLaunchKernelGGL((quantize_weight_mxfp4_kernel<bf16_t>), grid, dim3(256), 0, s, src, dst, sc, out_features, (int)(in_features / 32), w_row_stride, w4_row_stride, scale_row_stride);
    else
        hipLaunchKernelGGL((quantize_weight_mxfp4_kernel<f16_t>), grid, dim3(256), 0, s, src, dst, sc, out_features, (int)(in_features / 32), w_row_stride, w4_row_stride, scale_row_stride);
    return ATOMA_CHECK_LAUNCH("quantize_weight_mxfp4_kernel") ? 0 : -1;
}

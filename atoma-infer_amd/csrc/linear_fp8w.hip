// fp8 (OCP e4m3fn) WEIGHTS for the decode-step projections, "W8A16": y[b][n] = round(scale[n] * sum_k x[b][k] * e4m3(w8[n][k])), batch <= 64.
//
// No counterpart in the reference beyond its roadmap item "quantization" (its README); the weight-side sibling of the fp8 KV
// cache (kv_fp8.hip, paged_decode_fp8.hip).  At 1..64 rows a projection is a stream over the weights (linear_decode.hip), and the 16-bit
// kernels already run near the HBM rate, so the only thing left to win is moving fewer bytes: one byte per weight, one f32 scale per output
// feature.  fp8 -> bf16 / f16 is exact (3 mantissa bits), so the inner loops are the 16-bit kernels' arithmetic (v_dot2c / v_mfma_f32_16x16x32
// with fp32 accumulation) on operands converted in registers (v_cvt_scalef32_pk_{bf16,f16}_fp8, scale 1.0); nothing is scaled per element:
// scale[n] multiplies the fp32 sum once, where the output is rounded -- in the single-launch kernels' store, otherwise in the kernel that adds
// the K splits, never before they are summed.  A 16-byte load holds 16 inputs instead of 8.  The three regimes:
//   * 1..4 rows   linear_wq_gemv_kernel<T, Fp8Rows, ..> and
//   * 5..16 rows  linear_wq_wg_kernel<T, Fp8Rows, ..>: the quantised-weight kernels of linear_wq.h, written once for every format, with their
//                 launchers and the entry; this file gives them the format (Fp8Rows: slabs of 256 inputs, one 16-byte load = two operand
//                 fragments, its low and its high 8 bytes);
//   * 17..64 rows linear_fp8w_mma_kernel, here: loads in the MFMA operand order, K split over wavefronts into the fp32 workspace, and
//                 linear_reduce_kernel<T, SCALED> (sum, scale, round, epilogue).
// The split counts derive from the W rows, never from the epilogue, so _residual and _silu_mul are bit-identical to the plain call followed by
// atoma_add / atoma_silu_mul.  Pipeline and the reduce kernel are those of the 16-bit kernels (linear_stream.h), the parameters are LinearParams
// with byte weights and w_scale, the launch plans and the shared argument checks are linear_plan.h's.
// Out of scope here: the fused RMSNorm and q/k/v + RoPE + cache forms, 65..256 rows and prefill-sized products (16-bit weights only).
// atoma_quantize_weight_fp8 at the bottom: the KV-cache write's arithmetic (kv_fp8.hip) with one scale per output row, amax / 448.
#include "linear_wq.h"

namespace atoma {

// two fp8 bytes of `word` (bytes 0,1 or, hi, bytes 2,3) -> one packed pair of T, exact
template <typename T> __device__ __forceinline__ uint32_t w8_pair(uint32_t word, bool hi);
template <> __device__ __forceinline__ uint32_t w8_pair<bf16_t>(uint32_t word, bool hi) {
    return hi ? __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(word, 1.0f, true))
              : __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(word, 1.0f, false));
}
template <> __device__ __forceinline__ uint32_t w8_pair<f16_t>(uint32_t word, bool hi) {
    return hi ? __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(word, 1.0f, true))
              : __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(word, 1.0f, false));
}
// 8 fp8 bytes (two words) -> 8 values of T in element order: one MFMA A operand
template <typename T> __device__ __forceinline__ lu32x4 w8_frag(uint32_t w0, uint32_t w1) {
    return lu32x4{w8_pair<T>(w0, false), w8_pair<T>(w0, true), w8_pair<T>(w1, false), w8_pair<T>(w1, true)};
}

// 17..64 rows.  One wavefront per (16.RT output features, K split), loads in the MFMA operand order: lane 16.grp + col loads bytes
// 64q + 16.grp ..+15 of row 16r + col of a 128-input chunk (q = 0, 1) -- two A operands -- and the matching 32 bytes of x rows 16c + col.
// CT column tiles of 16 batch rows share every converted A operand.  Unscaled fp32 sums go to the workspace [split][batch][n] when K is
// split or an epilogue follows (linear_reduce_kernel<T, SCALED>); otherwise scaled, rounded and stored here.
template <typename T, int RT, int CT, int P>
__global__ void __launch_bounds__(64) linear_fp8w_mma_kernel(const LinearParams p) {
    const int lane = threadIdx.x, grp = lane >> 4, col = lane & 15;
    const int tiles_n = p.n / (16 * RT);
    const int tile = blockIdx.x % tiles_n, split = blockIdx.x / tiles_n;
    const int n0 = tile * 16 * RT;
    const int c0 = split * p.chunks_per_split, c1 = min(c0 + p.chunks_per_split, p.k >> 7);

    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(wq_bytes(p) + (int64_t)n0 * p.w_row_stride), 0, 0x7fffffff, 0x00020000);
    uint32_t w_lane[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) w_lane[r] = (uint32_t)((16 * r + col) * p.w_row_stride + grp * 16);
    bool has_x[CT];
    const uint16_t *xrow[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        has_x[c] = 16 * c + col < p.batch;
        xrow[c] = p.x + (int64_t)(has_x[c] ? 16 * c + col : 0) * p.x_row_stride + grp * 16;
    }

    lu32x4 wb[P][RT][2], xb[P][CT][2][2];
    auto issue = [&](int s, int chunk) {
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
            for (int q = 0; q < 2; ++q) wb[s][r][q] = __builtin_amdgcn_raw_buffer_load_b128(wr, w_lane[r], chunk * 128 + q * 64, 2 /* nt */);
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int h = 0; h < 2; ++h)
                    xb[s][c][q][h] = has_x[c] ? *reinterpret_cast<const lu32x4 *>(xrow[c] + chunk * 128 + q * 64 + h * 8) : lu32x4{0, 0, 0, 0};
    };
    lf32x4 acc[RT][CT];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[r][c] = lf32x4{0.f, 0.f, 0.f, 0.f};
    auto compute = [&](int s) {
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int r = 0; r < RT; ++r) {
                const lu32x4 lo = w8_frag<T>(wb[s][r][q][0], wb[s][r][q][1]), hi = w8_frag<T>(wb[s][r][q][2], wb[s][r][q][3]);
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    acc[r][c] = lin_mfma<T>(lo, xb[s][c][q][0], acc[r][c]);
                    acc[r][c] = lin_mfma<T>(hi, xb[s][c][q][1], acc[r][c]);
                }
            }
    };
    ATOMA_STREAM_PIPELINE(P, c0, c1, issue, compute, stream_no_op);
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        if (!has_x[ct]) continue;
        const int brow = 16 * ct + col;
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const int n = n0 + 16 * r + 4 * grp;
            const lf32x4 a = acc[r][ct];
            if (p.partial) {
                *reinterpret_cast<float4 *>(p.partial + ((int64_t)split * p.batch + brow) * p.n + n) = make_float4(a[0], a[1], a[2], a[3]);
            } else {
                uint2 o;
                o.x = pack2<T>(a[0] * p.w_scale[n], a[1] * p.w_scale[n + 1]);
                o.y = pack2<T>(a[2] * p.w_scale[n + 2], a[3] * p.w_scale[n + 3]);
                *reinterpret_cast<uint2 *>(p.y + (int64_t)brow * p.y_row_stride + n) = o;
            }
        }
    }
}

template <typename T> static int launch_fp8w_mma(LinearParams &p, hipStream_t stream) {
    const int ct = (p.batch + 15) / 16;
    const int rt = p.n % 32 == 0 ? 2 : 1;
    const int64_t tiles_n = p.n / (16 * rt);
    // Split K until about 4 (two row tiles) / 8 wavefronts per CU stream the weights, never below 8 chunks per split: 1 KiB per weight row and
    // split, the bytes the 16-bit kernel's floor of 4 chunks stands for.  An epilogue always runs in the reduce kernel (it needs whole rows of y).
    if (!plan_k_splits(p, tiles_n, (int64_t)device_num_cus() * (rt > 1 ? 4 : 8), 8, stream, p.epilogue != 0)) return -1;
    const dim3 grid((unsigned)(tiles_n * p.splits));
    auto launch = [&](auto RT_, auto CT_) { hipLaunchKernelGGL((linear_fp8w_mma_kernel<T, decltype(RT_)::value, decltype(CT_)::value, 2>), grid, dim3(64), 0, stream, p); };
    auto cols = [&](auto RT_) { if (ct <= 1) launch(RT_, int_c<1>{}); else if (ct == 2) launch(RT_, int_c<2>{}); else if (ct == 3) launch(RT_, int_c<3>{}); else launch(RT_, int_c<4>{}); };
    if (rt == 2) cols(int_c<2>{}); else cols(int_c<1>{});
    if (!ATOMA_CHECK_LAUNCH("linear_fp8w_mma_kernel")) return -1;
    return !p.partial || launch_reduce<T, true>(p, stream) ? 0 : -1;
}

// ---- the format of linear_wq.h's kernels -----------------------------------------------------------------------------------------------------
// A slab is 256 inputs = 4 KiB per load round of a wavefront, the same bytes as a 128-input chunk of the 16-bit kernels, so the depth rule carries
// over in slabs: at least 4 slabs (1024 inputs) per wavefront -- half the K split of the 16-bit kernel at the same K, and the same bytes in
// flight per wavefront (P x 4 KiB per row tile).
struct Fp8Rows {
    static constexpr int CH = 2;                                 // a slab: 256 inputs
    static constexpr bool kBlockScales = false;                  // one f32 per output row, applied to the fp32 sum
    struct Args { LinearParams p; };
    static Args args(LinearParams p, const void *w_scale, int64_t) { p.w_scale = static_cast<const float *>(w_scale); return Args{p}; }
    // fragment 0: bytes 0..7 of the load, fragment 1: bytes 8..15
    template <typename T> static __device__ __forceinline__ lu32x4 frag(const lu32x4 &v, int h, float) { return w8_frag<T>(v[2 * h], v[2 * h + 1]); }

    static constexpr const char *kName = "linear_decode_fp8w", *kW = "w8";
    static constexpr int kMaxBatch = 64, kInputsPerByte = 1;
    static constexpr const char *kBatchRule = "batch must be in [0, 64] (the fp8-weight kernels serve the decode range only; more than 64 rows is not supported)";
    static constexpr const char *kScaleRule = "w_scale must be a 4-byte aligned f32 [out_features]";
    static constexpr WqPlan kGemvPlan{"ATOMA_FP8W_GEMV_WAVES_PER_CU", 32, nullptr, 1}, kWgPlan{"ATOMA_FP8W_WG_WAVES_PER_CU", 8, nullptr, 1};
    static constexpr int gemv_depth(bool pair, int nb) { return pair ? (nb > 2 ? 1 : 2) : (nb > 2 ? 2 : 3); }
    static constexpr int wg_depth(bool pair) { return pair ? 2 : 3; }
    static int gemv_rows() { static const int v = env_int("ATOMA_FP8W_GEMV_MAX_BATCH", 4); return v; }
    static int wg_rows() { static const int v = env_int("ATOMA_FP8W_WG_MAX_BATCH", 16); return v; }
    template <typename T> static int launch_above_wg(LinearParams &p, hipStream_t stream) { return launch_fp8w_mma<T>(p, stream); }
};

// ---- the quantiser -------------------------------------------------------------------------------------------------------------------------
// 8 source elements -> 8 fp8 bytes: quantize8 of kv_fp8.hip (clamp to +-448, v_cvt_pk_fp8_f32: round to nearest even)
template <typename T> __device__ __forceinline__ uint2 w8_quantize8(const uint4 &v, float inv_scale) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    float f[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        f[2 * e] = lo_to_f32<T>(w[e]) * inv_scale;
        f[2 * e + 1] = hi_to_f32<T>(w[e]) * inv_scale;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = __builtin_amdgcn_fmed3f(f[e], -448.f, 448.f);
    uint32_t lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], lo, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], hi, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
    return make_uint2(lo, hi);
}

// one workgroup per output row: amax over the row, scale = amax / 448 (1 for an all-zero row), then the bytes (the row is re-read from L2)
template <typename T>
__global__ void __launch_bounds__(256) quantize_weight_fp8_kernel(const uint16_t *__restrict__ w, uint8_t *__restrict__ w8, float *__restrict__ scale_out,
                                                                  int in_features, int64_t w_row_stride, int64_t w8_row_stride) {
    __shared__ float wave_max[4];
    const uint16_t *src = w + (int64_t)blockIdx.x * w_row_stride;
    uint8_t *dst = w8 + (int64_t)blockIdx.x * w8_row_stride;
    const int pieces = in_features >> 4;                         // 16 elements: two 16-byte loads, one 16-byte store
    float m = 0.f;
    for (int i = threadIdx.x; i < 2 * pieces; i += 256) {
        const uint4 v = *reinterpret_cast<const uint4 *>(src + i * 8);
        const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) m = fmaxf(m, fmaxf(fabsf(lo_to_f32<T>(u[e])), fabsf(hi_to_f32<T>(u[e]))));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = m;
    __syncthreads();
    const float amax = fmaxf(fmaxf(wave_max[0], wave_max[1]), fmaxf(wave_max[2], wave_max[3]));
    const float scale = amax > 0.f ? amax / 448.f : 1.f;
    const float inv = 1.0f / scale;
    if (threadIdx.x == 0) scale_out[blockIdx.x] = scale;
    for (int i = threadIdx.x; i < pieces; i += 256) {
        const uint2 a = w8_quantize8<T>(*reinterpret_cast<const uint4 *>(src + i * 16), inv);
        const uint2 b = w8_quantize8<T>(*reinterpret_cast<const uint4 *>(src + i * 16 + 8), inv);
        *reinterpret_cast<uint4 *>(dst + i * 16) = make_uint4(a.x, a.y, b.x, b.y);
    }
}

}  // namespace atoma

extern "C" int atoma_linear_decode_fp8w(const void *x, const void *w8, const float *w_scale, void *y, int64_t batch, int64_t in_features,
                                        int64_t out_features, int64_t x_row_stride, int64_t w8_row_stride, int64_t y_row_stride, int dtype,
                                        void *stream) {
    return atoma::linear_wq_entry<atoma::Fp8Rows>(x, w8, w_scale, y, batch, in_features, out_features, x_row_stride, w8_row_stride, 0, y_row_stride, 0, nullptr, 0, dtype, stream);
}
extern "C" int atoma_linear_decode_fp8w_residual(const void *x, const void *w8, const float *w_scale, const void *residual, void *y, int64_t batch,
                                                 int64_t in_features, int64_t out_features, int64_t x_row_stride, int64_t w8_row_stride,
                                                 int64_t residual_row_stride, int64_t y_row_stride, int dtype, void *stream) {
    return atoma::linear_wq_entry<atoma::Fp8Rows>(x, w8, w_scale, y, batch, in_features, out_features, x_row_stride, w8_row_stride, 0, y_row_stride, 1, residual, residual_row_stride, dtype, stream);
}
extern "C" int atoma_linear_decode_fp8w_silu_mul(const void *x, const void *w8_gate_up, const float *w_scale, void *y, int64_t batch,
                                                 int64_t in_features, int64_t intermediate, int64_t x_row_stride, int64_t w8_row_stride,
                                                 int64_t y_row_stride, int dtype, void *stream) {
    return atoma::linear_wq_entry<atoma::Fp8Rows>(x, w8_gate_up, w_scale, y, batch, in_features, 2 * intermediate, x_row_stride, w8_row_stride, 0, y_row_stride, 2, nullptr, 0, dtype, stream);
}

extern "C" int atoma_quantize_weight_fp8(const void *w, int64_t out_features, int64_t in_features, int64_t w_row_stride, int dtype, void *w8_out,
                                         int64_t w8_row_stride, float *scale_out, void *stream) {
    using namespace atoma;
    clear_error();
    if (dtype != ATOMA_F16 && dtype != ATOMA_BF16) { set_error("quantize_weight_fp8: dtype (of the source weights) must be f16 or bf16"); return -1; }
    if (out_features < 0 || out_features > 0x7fffffff) { set_error("quantize_weight_fp8: out_features must be in [0, 2^31)"); return -1; }
    if (in_features <= 0 || in_features % 16 != 0 || in_features > 0x7fffffff) { set_error("quantize_weight_fp8: in_features must be a positive multiple of 16"); return -1; }
    if (w_row_stride < in_features || w8_row_stride < in_features) { set_error("quantize_weight_fp8: row strides must cover a row"); return -1; }
    if (w_row_stride % 8 || w8_row_stride % 16) { set_error("quantize_weight_fp8: w_row_stride (elements) must be a multiple of 8, w8_row_stride (bytes) of 16"); return -1; }
    if (!w || !w8_out || (reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(w8_out)) & 15u) {
        set_error("quantize_weight_fp8: w and w8_out must be 16-byte aligned");
        return -1;
    }
    if (!scale_out || reinterpret_cast<uintptr_t>(scale_out) & 3u) { set_error("quantize_weight_fp8: scale_out must be a 4-byte aligned f32 [out_features]"); return -1; }
    if (out_features == 0) return 0;
    const auto s = static_cast<hipStream_t>(stream);
    const auto src = static_cast<const uint16_t *>(w);
    const auto dst = static_cast<uint8_t *>(w8_out);
    if (dtype == ATOMA_BF16)
        hipLaunchKernelGGL((quantize_weight_fp8_kernel<bf16_t>), dim3((unsigned)out_features), dim3(256), 0, s, src, dst, scale_out, (int)in_features, w_row_stride, w8_row_stride);
    else
        hipLaunchKernelGGL((quantize_weight_fp8_kernel<f16_t>), dim3((unsigned)out_features), dim3(256), 0, s, src, dst, scale_out, (int)in_features, w_row_stride, w8_row_stride);
    return ATOMA_CHECK_LAUNCH("quantize_weight_fp8_kernel") ? 0 : -1;
}

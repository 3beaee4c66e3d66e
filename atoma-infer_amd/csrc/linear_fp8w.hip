// fp8 (OCP e4m3fn) WEIGHTS for the decode-step projections, "W8A16": y[b][n] = round(scale[n] * sum_k x[b][k] * e4m3(w8[n][k])), batch <= 64.
//
// No counterpart in the reference beyond its roadmap item "quantization" (its README); the weight-side sibling of the fp8 KV
// cache (kv_fp8.hip, paged_decode_fp8.hip).  At 1..64 rows a projection is a stream over the weights (linear_decode.hip), and the 16-bit
// kernels already run near the HBM rate, so the only thing left to win is moving fewer bytes: one byte per weight, one f32 scale per output
// feature.  fp8 -> bf16 / f16 is exact (3 mantissa bits), so the inner loops are the 16-bit kernels' arithmetic (v_dot2c / v_mfma_f32_16x16x32
// with fp32 accumulation) on operands converted in registers (v_cvt_scalef32_pk_{bf16,f16}_fp8, scale 1.0); nothing is scaled per element:
// scale[n] multiplies the fp32 sum once, where the output is rounded -- in the single-launch kernels' store, otherwise in the kernel that adds
// the K splits, never before they are summed.  A 16-byte load now holds 16 inputs instead of 8, which is what changes in the three regimes:
//   * 1..4 rows   linear_fp8w_gemv_kernel: 4 rows x 256 contiguous bytes (= 256 inputs) per load instruction, v_dot2c, one launch;
//   * 5..16 rows  linear_fp8w_wg_kernel: the same loads re-laid into the MFMA A-operand order through a 4 KiB LDS tile per wavefront; one
//                 16-byte LDS read feeds two MFMAs (its low and its high 8 bytes: the k order inside an MFMA is free as long as x agrees);
//   * 17..64 rows linear_fp8w_mma_kernel: loads in the MFMA operand order, K split over wavefronts into the fp32 workspace, and
//                 linear_reduce_kernel<T, SCALED> (sum, scale, round, epilogue).
// W by non-temporal buffer loads (read once), x from L2.  in_features is a multiple of 128, so the last 256-input slab of the first two kernels
// may be half a slab: its upper half is not loaded (zeros for W and x).  The split counts derive from the W rows, never from the epilogue, so
// _residual and _silu_mul are bit-identical to the plain call followed by atoma_add / atoma_silu_mul.
// Pipeline, row sum and the reduce kernel are those of the 16-bit kernels (linear_stream.h), the parameters are LinearParams with
// byte weights and w_scale, the launch plans and the shared argument checks are linear_plan.h's.
// Out of scope here: the fused RMSNorm and q/k/v + RoPE + cache forms, 65..256 rows and prefill-sized products (16-bit weights only).
// atoma_quantize_weight_fp8 at the bottom: the KV-cache write's arithmetic (kv_fp8.hip) with one scale per output row, amax / 448.
#include "linear_plan.h"
#include <stdlib.h>

namespace atoma {

// LinearParams here: w = e4m3fn bytes [n][k] (w8_bytes), w_row_stride in bytes, w_scale [n], partial = UNSCALED fp32 sums
__device__ __forceinline__ const uint8_t *w8_bytes(const LinearParams &p) { return reinterpret_cast<const uint8_t *>(p.w); }

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

// 1..4 rows.  Workgroup = NW wavefronts x 16 output features (PAIR: + the 16 matching up features); wavefront w streams the w-th part of K
// in slabs of 256 inputs: lane 16.g + c loads bytes 16c..16c+15 of row 4.rg + g (4 rows x 256 B per instruction), converts them to 8 pairs
// and multiplies with the matching 16 inputs of every batch row (two 16-byte loads of x).  Merge over LDS and epilogues as linear_gemv_kernel.
template <typename T, int NW, bool PAIR, int NB, int P>
__global__ void __launch_bounds__(64 * NW) linear_fp8w_gemv_kernel(const LinearParams p) {
    constexpr int RT = PAIR ? 2 : 1;
    __shared__ float red[NW][RT][16][4];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), g = lane >> 4, c = lane & 15;
    const int n0 = blockIdx.x * 16;
    const int out_n = PAIR ? p.n / 2 : p.n;
    const int slabs = (p.k + 255) >> 8, per = (slabs + NW - 1) / NW;
    const int half_slab = (p.k & 255) ? slabs - 1 : -1;          // the slab that holds 128 inputs only
    const int c0 = wave * per, c1 = min(c0 + per, slabs);
    const int64_t row_bytes = p.w_row_stride;

    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(w8_bytes(p) + (int64_t)n0 * row_bytes), 0, 0x7fffffff, 0x00020000);
    uint32_t w_lane[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) w_lane[r] = (uint32_t)(((int64_t)r * out_n + g) * row_bytes + c * 16);
    const uint16_t *xrow[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) xrow[b] = p.x + (int64_t)min(b, p.batch - 1) * p.x_row_stride + c * 16;   // rows beyond the batch: recomputed, never stored

    lu32x4 wb[P][RT][4], xb[P][NB][2];
    auto issue = [&](int s, int slab) {
        const bool ok = slab != half_slab || c < 8;
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg)
                wb[s][r][rg] = ok ? __builtin_amdgcn_raw_buffer_load_b128(wr, w_lane[r], (int)(rg * 4 * row_bytes + slab * 256), 2 /* nt */) : lu32x4{0, 0, 0, 0};
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int h = 0; h < 2; ++h) xb[s][b][h] = ok ? *reinterpret_cast<const lu32x4 *>(xrow[b] + slab * 256 + h * 8) : lu32x4{0, 0, 0, 0};
    };
    float acc[RT][4][NB];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg)
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[r][rg][b] = 0.f;
    auto compute = [&](int s) {
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                const lu32x4 lo = w8_frag<T>(wb[s][r][rg][0], wb[s][r][rg][1]), hi = w8_frag<T>(wb[s][r][rg][2], wb[s][r][rg][3]);
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    float a = acc[r][rg][b];
#pragma unroll
                    for (int e = 0; e < 4; ++e) a = dot2<T>(lo[e], xb[s][b][0][e], a);
#pragma unroll
                    for (int e = 0; e < 4; ++e) a = dot2<T>(hi[e], xb[s][b][1][e], a);
                    acc[r][rg][b] = a;
                }
            }
    };
    ATOMA_STREAM_PIPELINE(P, c0, c1, issue, compute, stream_no_op);
    // sum the 16 lanes of every row; lane c == 0 of group g then holds row 4.rg + g
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg)
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const float v = row16_sum(acc[r][rg][b]);
                if (c == 0) red[wave][r][rg * 4 + g][b] = v;
            }
    __syncthreads();
    if (wave > 0) return;
    const int row = lane & 15, n = n0 + row, b = lane >> 4;      // 16 features x 4 batch rows on the 64 lanes of wavefront 0
    if (b >= NB || b >= p.batch) return;
    float v[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        float t = red[0][r][row][b];
#pragma unroll
        for (int w = 1; w < NW; ++w) t += red[w][r][row][b];     // fixed order: deterministic
        v[r] = round_through<T>(t * p.w_scale[(int64_t)r * out_n + n]);
    }
    float out = v[0];
    if (p.epilogue == 1) out += lo_to_f32<T>((uint32_t)p.aux[(int64_t)b * p.aux_row_stride + n]);
    if constexpr (PAIR) out = silu_round<T>(out) * v[1];
    p.y[(int64_t)b * p.y_row_stride + n] = (uint16_t)f32_to_bits<T>(out);
}

// 5..16 rows.  The loads of the kernel above (4 rows x 256 B per instruction), re-laid through a 4 KiB LDS tile per wavefront and row tile as
// in linear_wg_kernel<RELAY>: lane 16.g + c writes its 16 bytes of row 4.q + g to [row][piece c ^ row], lane 16.grp + col reads
// [row col][piece (4q + grp) ^ col] = inputs 16.(4q + grp) ..+15 of the slab; the low 8 bytes are the A operand of one MFMA, the high 8 of the
// next, against x[col][the same inputs].  Result tile: lane holds y^T[n0 + 4.grp + i][batch row col].
template <typename T, int NW, bool PAIR, int P>
__global__ void __launch_bounds__(64 * NW) linear_fp8w_wg_kernel(const LinearParams p) {
    constexpr int RT = PAIR ? 2 : 1;
    __shared__ float red[NW > 1 ? NW - 1 : 1][RT][64][4];
    __shared__ __attribute__((aligned(16))) char relay[NW][RT][4096];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), grp = lane >> 4, col = lane & 15;
    const int n0 = blockIdx.x * 16;
    const int out_n = PAIR ? p.n / 2 : p.n;
    const int slabs = (p.k + 255) >> 8, per = (slabs + NW - 1) / NW;
    const int half_slab = (p.k & 255) ? slabs - 1 : -1;
    const int c0 = wave * per, c1 = min(c0 + per, slabs);
    const int64_t row_bytes = p.w_row_stride;

    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(w8_bytes(p) + (int64_t)n0 * row_bytes), 0, 0x7fffffff, 0x00020000);
    uint32_t w_lane[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) w_lane[r] = (uint32_t)(((int64_t)r * out_n + grp) * row_bytes + col * 16);   // row 4.q + grp, piece col
    const bool has_x = col < p.batch;
    const uint16_t *xrow = p.x + (int64_t)(has_x ? col : 0) * p.x_row_stride + grp * 16;

    lu32x4 wb[P][RT][4], xb[P][4][2];
    auto issue = [&](int s, int slab) {
        const bool half = slab == half_slab;
        const bool ok = !half || col < 8;
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                wb[s][r][q] = ok ? __builtin_amdgcn_raw_buffer_load_b128(wr, w_lane[r], (int)(q * 4 * row_bytes + slab * 256), 2 /* nt */) : lu32x4{0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int h = 0; h < 2; ++h)          // piece 4q + grp of the slab: in the lower half (pieces 0..7) for q < 2
                xb[s][q][h] = (has_x && !(half && q >= 2)) ? *reinterpret_cast<const lu32x4 *>(xrow + slab * 256 + q * 64 + h * 8) : lu32x4{0, 0, 0, 0};
    };
    lf32x4 acc[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) acc[r] = lf32x4{0.f, 0.f, 0.f, 0.f};
    auto compute = [&](int s) {
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            char *tile = relay[wave][r];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = 4 * q + grp;
                *reinterpret_cast<lu32x4 *>(tile + row * 256 + ((col ^ row) & 15) * 16) = wb[s][r][q];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const char *tile = relay[wave][r];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const lu32x4 a = *reinterpret_cast<const lu32x4 *>(tile + col * 256 + (((4 * q + grp) ^ col) & 15) * 16);
                acc[r] = lin_mfma<T>(w8_frag<T>(a[0], a[1]), xb[s][q][0], acc[r]);
                acc[r] = lin_mfma<T>(w8_frag<T>(a[2], a[3]), xb[s][q][1], acc[r]);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    ATOMA_STREAM_PIPELINE(P, c0, c1, issue, compute, stream_no_op);
    // add the NW accumulator tiles: wavefronts 1.. write, wavefront 0 sums (fixed order: deterministic)
    if constexpr (NW > 1) {
        if (wave > 0) {
#pragma unroll
            for (int r = 0; r < RT; ++r) *reinterpret_cast<lf32x4 *>(red[wave - 1][r][lane]) = acc[r];
        }
        __syncthreads();
        if (wave > 0) return;
#pragma unroll
        for (int w = 0; w < NW - 1; ++w)
#pragma unroll
            for (int r = 0; r < RT; ++r) {
                const lf32x4 o = *reinterpret_cast<const lf32x4 *>(red[w][r][lane]);
                acc[r] += o;
            }
    }
    if (!has_x) return;
    const int n = n0 + 4 * grp;
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = round_through<T>(acc[0][i] * p.w_scale[n + i]);
    if (p.epilogue == 1) {
        const uint2 r = *reinterpret_cast<const uint2 *>(p.aux + (int64_t)col * p.aux_row_stride + n);
        v[0] += lo_to_f32<T>(r.x); v[1] += hi_to_f32<T>(r.x); v[2] += lo_to_f32<T>(r.y); v[3] += hi_to_f32<T>(r.y);
    }
    if constexpr (PAIR) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = silu_round<T>(v[i]) * round_through<T>(acc[1][i] * p.w_scale[(int64_t)out_n + n + i]);
    }
    uint2 o;
    o.x = pack2<T>(v[0], v[1]);
    o.y = pack2<T>(v[2], v[3]);
    *reinterpret_cast<uint2 *>(p.y + (int64_t)col * p.y_row_stride + n) = o;
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

    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(w8_bytes(p) + (int64_t)n0 * p.w_row_stride), 0, 0x7fffffff, 0x00020000);
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

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------
// Wavefronts per workgroup (the K split inside it) from the W ROWS, as launch_linear_gemv / launch_linear_wg do, so that the stacked gate / up
// launch splits K exactly like the plain projection of the same matrix.  A slab is 256 inputs = 4 KiB per load round of a wavefront, the same
// bytes as a 128-input chunk of the 16-bit kernels, so the depth rule carries over in slabs: at least 4 slabs (1024 inputs) per wavefront --
// half the K split of the 16-bit kernel at the same K, and the same bytes in flight per wavefront (P x 4 KiB per row tile).
static const int fp8w_gemv_max_batch = env_int("ATOMA_FP8W_GEMV_MAX_BATCH", 4);
static const int fp8w_wg_max_batch = env_int("ATOMA_FP8W_WG_MAX_BATCH", 16);

template <typename T> static int launch_fp8w_gemv(LinearParams &p, hipStream_t stream) {
    static const int wpc = env_int("ATOMA_FP8W_GEMV_WAVES_PER_CU", 32);
    const bool pair = p.epilogue == 2;
    const int nw = waves_per_workgroup(p.n / 16, (p.k + 255) / 256, wpc);
    const dim3 grid((unsigned)((pair ? p.n / 2 : p.n) / 16)), block(64 * nw);
    dispatch_nw(nw, [&](auto NW_) {
        constexpr int NW = decltype(NW_)::value;
        auto rows = [&](auto NB_) {
            constexpr int NB = decltype(NB_)::value;
            if (pair) hipLaunchKernelGGL((linear_fp8w_gemv_kernel<T, NW, true, NB, (NB > 2 ? 1 : 2)>), grid, block, 0, stream, p);
            else hipLaunchKernelGGL((linear_fp8w_gemv_kernel<T, NW, false, NB, (NB > 2 ? 2 : 3)>), grid, block, 0, stream, p);
        };
        if (p.batch == 1) rows(int_c<1>{}); else if (p.batch == 2) rows(int_c<2>{}); else rows(int_c<4>{});
    });
    return ATOMA_CHECK_LAUNCH("linear_fp8w_gemv_kernel") ? 0 : -1;
}

template <typename T> static int launch_fp8w_wg(LinearParams &p, hipStream_t stream) {
    static const int wpc = env_int("ATOMA_FP8W_WG_WAVES_PER_CU", 8);
    const bool pair = p.epilogue == 2;
    const int nw = waves_per_workgroup(p.n / 16, (p.k + 255) / 256, wpc);
    const dim3 grid((unsigned)((pair ? p.n / 2 : p.n) / 16)), block(64 * nw);
    dispatch_nw(nw, [&](auto NW_) {
        constexpr int NW = decltype(NW_)::value;
        if (pair) hipLaunchKernelGGL((linear_fp8w_wg_kernel<T, NW, true, 2>), grid, block, 0, stream, p);
        else hipLaunchKernelGGL((linear_fp8w_wg_kernel<T, NW, false, 3>), grid, block, 0, stream, p);
    });
    return ATOMA_CHECK_LAUNCH("linear_fp8w_wg_kernel") ? 0 : -1;
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

template <typename T> static int launch_fp8w(LinearParams &p, hipStream_t stream) {
    if (p.batch <= std::min(fp8w_gemv_max_batch, 4)) return launch_fp8w_gemv<T>(p, stream);
    if (p.batch <= std::min(fp8w_wg_max_batch, 16)) return launch_fp8w_wg<T>(p, stream);
    return launch_fp8w_mma<T>(p, stream);
}

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

static int linear_fp8w_entry(const void *x, const void *w8, const void *w_scale, void *y, int64_t batch, int64_t in_features, int64_t out_features,
                             int64_t x_row_stride, int64_t w8_row_stride, int64_t y_row_stride, int epilogue, const void *aux, int64_t aux_row_stride,
                             int dtype, void *stream) {
    using namespace atoma;
    clear_error();
    if (dtype != ATOMA_F16 && dtype != ATOMA_BF16) { set_error("linear_decode_fp8w: dtype (the activation dtype) must be f16 or bf16"); return -1; }
    if (batch < 0 || batch > 64) {
        set_error("linear_decode_fp8w: batch must be in [0, 64] (the fp8-weight kernels serve the decode range only; more than 64 rows is not supported)");
        return -1;
    }
    if (!check_linear_args("linear_decode_fp8w", in_features, out_features, x_row_stride, w8_row_stride, y_row_stride, epilogue, aux, aux_row_stride)) return -1;
    if (x_row_stride % 8 || y_row_stride % 4) { set_error("linear_decode_fp8w: strides must keep rows 16-byte (x) / 8-byte (y) aligned"); return -1; }
    if (w8_row_stride % 16) { set_error("linear_decode_fp8w: w8_row_stride (bytes) must be a multiple of 16"); return -1; }
    if (!x || !w8 || !y || (reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w8)) & 15u || reinterpret_cast<uintptr_t>(y) & 7u) {
        set_error("linear_decode_fp8w: x and w8 must be 16-byte aligned, y 8-byte aligned");
        return -1;
    }
    if (!w_scale || reinterpret_cast<uintptr_t>(w_scale) & 3u) { set_error("linear_decode_fp8w: w_scale must be a 4-byte aligned f32 [out_features]"); return -1; }
    // a row tile (and the up rows of the stacked gate / up kernels) is reached through a 32-bit buffer offset from the tile's base
    if (((epilogue == 2 ? out_features / 2 : 0) + 32) * w8_row_stride >= ((int64_t)1 << 31)) {
        set_error("linear_decode_fp8w: the weight rows a workgroup reaches must stay below 2 GiB (32-bit buffer offsets)");
        return -1;
    }
    if (batch == 0) return 0;
    LinearParams p = linear_params_of(x, w8, y, batch, in_features, out_features, x_row_stride, w8_row_stride, y_row_stride, epilogue, aux, aux_row_stride);
    p.w_scale = static_cast<const float *>(w_scale);
    const auto s = static_cast<hipStream_t>(stream);
    return dtype == ATOMA_BF16 ? launch_fp8w<bf16_t>(p, s) : launch_fp8w<f16_t>(p, s);
}

extern "C" int atoma_linear_decode_fp8w(const void *x, const void *w8, const float *w_scale, void *y, int64_t batch, int64_t in_features,
                                        int64_t out_features, int64_t x_row_stride, int64_t w8_row_stride, int64_t y_row_stride, int dtype,
                                        void *stream) {
    return linear_fp8w_entry(x, w8, w_scale, y, batch, in_features, out_features, x_row_stride, w8_row_stride, y_row_stride, 0, nullptr, 0, dtype, stream);
}
extern "C" int atoma_linear_decode_fp8w_residual(const void *x, const void *w8, const float *w_scale, const void *residual, void *y, int64_t batch,
                                                 int64_t in_features, int64_t out_features, int64_t x_row_stride, int64_t w8_row_stride,
                                                 int64_t residual_row_stride, int64_t y_row_stride, int dtype, void *stream) {
    return linear_fp8w_entry(x, w8, w_scale, y, batch, in_features, out_features, x_row_stride, w8_row_stride, y_row_stride, 1, residual,
                             residual_row_stride, dtype, stream);
}
extern "C" int atoma_linear_decode_fp8w_silu_mul(const void *x, const void *w8_gate_up, const float *w_scale, void *y, int64_t batch,
                                                 int64_t in_features, int64_t intermediate, int64_t x_row_stride, int64_t w8_row_stride,
                                                 int64_t y_row_stride, int dtype, void *stream) {
    return linear_fp8w_entry(x, w8_gate_up, w_scale, y, batch, in_features, 2 * intermediate, x_row_stride, w8_row_stride, y_row_stride, 2, nullptr, 0,
                             dtype, stream);
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

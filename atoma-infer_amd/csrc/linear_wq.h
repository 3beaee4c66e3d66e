// QUANTISED WEIGHTS ("wq") for the decode-step projections at 1..16 rows, each thing once for every weight format: the 1..4-row VALU kernel, the
// 5..16-row MFMA kernel, their launchers and the entry behind the C ABI.  Users: linear_fp8w.hip (Fp8Rows) and linear_mxfp4.hip (Mx4Blocks).
//
// A wavefront streams W in slabs of 4 rows x 256 contiguous bytes per load instruction, whatever a byte holds.  What differs between the formats
// is a trait F:
//   F::CH            128-input chunks in a slab: 2 (fp8, 256 inputs) or 4 (MXFP4, 512 inputs).  A lane's 16 bytes of W are 8.CH inputs, multiplied
//                    with CH 16-byte loads of x; in_features is a multiple of 128, so the last slab may hold fewer than CH chunks: the lanes
//                    beyond them load nothing (zeros for W and x).  A chunk is 16 / CH pieces of 16 bytes.
//   F::frag<T>       fragment h of the CH operand fragments a 16-byte load holds (8 values of T: one MFMA A operand, or four dot2 operands).
//   F::kBlockScales  true: one e8m0 byte per 32 inputs, loaded in issue() and applied inside the conversion, nothing after the sum;
//                    false: one f32 per output row (p.w_scale), multiplied into the merged fp32 sum once, where it is rounded.
//   F::Args          the kernel argument: {LinearParams p;}, with block scales {LinearParams p; Mx4Scales sp;}.
//   host             the entry's name and words, the batch bound and the row limit of each regime, the environment knobs with their defaults,
//                    the pipeline depth per (PAIR, NB).
// W by non-temporal buffer loads (read once), x from L2.  The wavefront count per workgroup derives from the W rows, never from the epilogue, and
// the merge across wavefronts runs in a fixed order, so _residual and _silu_mul are bit-identical to the plain call followed by atoma_add /
// atoma_silu_mul, and results are deterministic.  Pipeline and row sum are linear_stream.h's, the launch plan and the shared checks linear_plan.h's.
#pragma once
#include "linear_plan.h"
#include <stdlib.h>

namespace atoma {

// LinearParams here: w = the format's bytes [n][...] (wq_bytes), w_row_stride in bytes; block scales travel next to it
__device__ __forceinline__ const uint8_t *wq_bytes(const LinearParams &p) { return reinterpret_cast<const uint8_t *>(p.w); }
struct Mx4Scales {
    const uint8_t *scale;        // [n][k / 32] e8m0 bytes, rows 4-byte aligned
    int64_t row_stride;          // bytes
};
constexpr uint32_t kUnitScales = 0x7f7f7f7fu;   // four scale bytes 127 (2^0): what a lane holds where a partial slab has no scales to load
__device__ __forceinline__ float e8m0_scale(uint32_t dword, int shift) { return __uint_as_float(((dword >> shift) & 0xffu) << 23); }
typedef lu32x4 __attribute__((aligned(4))) lu32x4_a4;

// 1..4 rows.  Workgroup = NW wavefronts x 16 output features (PAIR: + the 16 matching up features); wavefront w streams the w-th part of K
// in slabs: lane 16.g + c loads bytes 16c..16c+15 of row 4.rg + g (4 rows x 256 B per instruction), converts them to CH fragments and multiplies
// with the matching 8.CH inputs of every batch row (CH 16-byte loads of x).  Block scales: the scales of a slab, all 16 rows, are one dword load:
// lane 4.row + j holds the scales of chunk j (blocks 4j..4j+3) of row `row`; lane (g, c) fetches the dword of lane 4.(4.rg + g) + (c >> 2) with
// ds_bpermute and takes byte c & 3.  Merge over LDS and epilogues as linear_gemv_kernel.
template <typename T, typename F, int NW, bool PAIR, int NB, int P>
__global__ void __launch_bounds__(64 * NW) linear_wq_gemv_kernel(const typename F::Args a) {
    static_assert(F::CH == 2 || F::CH == 4, "a slab is 2 or 4 chunks of 128 inputs");
    constexpr int RT = PAIR ? 2 : 1, CH = F::CH, LOG2_CH = CH == 2 ? 1 : 2, SHIFT = 4 - LOG2_CH;   // piece c lies in chunk c >> SHIFT
    const LinearParams &p = a.p;
    __shared__ float red[NW][RT][16][4];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), g = lane >> 4, c = lane & 15;
    const int n0 = blockIdx.x * 16;
    const int out_n = PAIR ? p.n / 2 : p.n;
    const int slabs = (p.k + 128 * CH - 1) >> (7 + LOG2_CH), per = (slabs + NW - 1) / NW;
    const int part_chunks = (p.k >> 7) & (CH - 1);               // 128-input chunks in the partial last slab; 0: every slab is whole
    const int part_slab = part_chunks ? slabs - 1 : -1;
    const int part_held = CH == 2 ? 1 : part_chunks;             // ... as the partial slab sees it: of two chunks it holds one, known at compile time
    const int c0 = wave * per, c1 = min(c0 + per, slabs);
    const int64_t row_bytes = p.w_row_stride;

    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(wq_bytes(p) + (int64_t)n0 * row_bytes), 0, 0x7fffffff, 0x00020000);
    uint32_t w_lane[RT];
    [[maybe_unused]] const uint32_t *s_lane[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        w_lane[r] = (uint32_t)(((int64_t)r * out_n + g) * row_bytes + c * 16);
        if constexpr (F::kBlockScales) s_lane[r] = reinterpret_cast<const uint32_t *>(a.sp.scale + ((int64_t)r * out_n + n0 + (lane >> 2)) * a.sp.row_stride) + (lane & 3);
    }
    const uint16_t *xrow[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) xrow[b] = p.x + (int64_t)min(b, p.batch - 1) * p.x_row_stride + c * 8 * CH;   // rows beyond the batch: recomputed, never stored
    [[maybe_unused]] const int s_shift = (c & 3) * 8;
    [[maybe_unused]] int s_from[4];                                               // ds_bpermute address of the lane that holds row 4.rg + g, chunk c >> 2
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) s_from[rg] = (4 * (4 * rg + g) + (c >> 2)) * 4;

    lu32x4 wb[P][RT][4], xb[P][NB][CH];
    uint32_t sb[P][RT];
    auto issue = [&](int s, int slab) {
        const bool part = slab == part_slab;
        const bool ok = !part || (c >> SHIFT) < part_held;
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg)
                wb[s][r][rg] = ok ? __builtin_amdgcn_raw_buffer_load_b128(wr, w_lane[r], (int)(rg * 4 * row_bytes + slab * 256), 2 /* nt */) : lu32x4{0, 0, 0, 0};
        if constexpr (F::kBlockScales) {
#pragma unroll
            for (int r = 0; r < RT; ++r) sb[s][r] = (!part || (lane & 3) < part_held) ? s_lane[r][slab * 4] : kUnitScales;
        }
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int h = 0; h < CH; ++h) xb[s][b][h] = ok ? *reinterpret_cast<const lu32x4 *>(xrow[b] + slab * 128 * CH + h * 8) : lu32x4{0, 0, 0, 0};
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
                float scale = 1.0f;
                if constexpr (F::kBlockScales) scale = e8m0_scale((uint32_t)__builtin_amdgcn_ds_bpermute(s_from[rg], (int)sb[s][r]), s_shift);
#pragma unroll
                for (int h = 0; h < CH; ++h) {                   // fragment by fragment into the same accumulators
                    const lu32x4 w = F::template frag<T>(wb[s][r][rg], h, scale);
#pragma unroll
                    for (int b = 0; b < NB; ++b) {
                        float t = acc[r][rg][b];
#pragma unroll
                        for (int e = 0; e < 4; ++e) t = dot2<T>(w[e], xb[s][b][h][e], t);
                        acc[r][rg][b] = t;
                    }
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
        if constexpr (!F::kBlockScales) t *= p.w_scale[(int64_t)r * out_n + n];
        v[r] = round_through<T>(t);
    }
    float out = v[0];
    if (p.epilogue == 1) out += lo_to_f32<T>((uint32_t)p.aux[(int64_t)b * p.aux_row_stride + n]);
    if constexpr (PAIR) out = silu_round<T>(out) * v[1];
    p.y[(int64_t)b * p.y_row_stride + n] = (uint16_t)f32_to_bits<T>(out);
}

// 5..16 rows.  The loads of the kernel above (4 rows x 256 B per instruction), re-laid through a 4 KiB LDS tile per wavefront and row tile as
// in linear_wg_kernel<RELAY>: lane 16.g + c writes its 16 bytes of row 4.q + g to [row][piece c ^ row], lane 16.grp + col reads
// [row col][piece (4q + grp) ^ col] = inputs 8.CH.(4q + grp) ..+8.CH-1 of the slab; fragment h of it is the A operand of one MFMA against
// x[col][the same 8 inputs] (the k order inside an MFMA is free as long as x agrees).  Block scales: piece 4q + grp is one block, byte grp of scale
// dword q: lane (grp, col) loads the 16 scale bytes of row col and this slab itself (one load instruction per slab; dword by dword in a partial
// slab).  Result tile: lane holds y^T[n0 + 4.grp + i][batch row col].
template <typename T, typename F, int NW, bool PAIR, int P>
__global__ void __launch_bounds__(64 * NW) linear_wq_wg_kernel(const typename F::Args a) {
    constexpr int RT = PAIR ? 2 : 1, CH = F::CH, LOG2_CH = CH == 2 ? 1 : 2, SHIFT = 4 - LOG2_CH;
    const LinearParams &p = a.p;
    __shared__ float red[NW > 1 ? NW - 1 : 1][RT][64][4];
    __shared__ __attribute__((aligned(16))) char relay[NW][RT][4096];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), grp = lane >> 4, col = lane & 15;
    const int n0 = blockIdx.x * 16;
    const int out_n = PAIR ? p.n / 2 : p.n;
    const int slabs = (p.k + 128 * CH - 1) >> (7 + LOG2_CH), per = (slabs + NW - 1) / NW;
    const int part_chunks = (p.k >> 7) & (CH - 1);
    const int part_slab = part_chunks ? slabs - 1 : -1;
    const int part_held = CH == 2 ? 1 : part_chunks;
    const int c0 = wave * per, c1 = min(c0 + per, slabs);
    const int64_t row_bytes = p.w_row_stride;

    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(wq_bytes(p) + (int64_t)n0 * row_bytes), 0, 0x7fffffff, 0x00020000);
    uint32_t w_lane[RT];
    [[maybe_unused]] const uint8_t *s_lane[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        w_lane[r] = (uint32_t)(((int64_t)r * out_n + grp) * row_bytes + col * 16);   // row 4.q + grp, piece col
        if constexpr (F::kBlockScales) s_lane[r] = a.sp.scale + ((int64_t)r * out_n + n0 + col) * a.sp.row_stride;   // row col
    }
    const bool has_x = col < p.batch;
    const uint16_t *xrow = p.x + (int64_t)(has_x ? col : 0) * p.x_row_stride + grp * 8 * CH;
    [[maybe_unused]] const int s_shift = grp * 8;

    lu32x4 wb[P][RT][4], xb[P][4][CH], sb[P][RT];
    auto issue = [&](int s, int slab) {
        const bool part = slab == part_slab;
        const bool ok = !part || (col >> SHIFT) < part_held;
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                wb[s][r][q] = ok ? __builtin_amdgcn_raw_buffer_load_b128(wr, w_lane[r], (int)(q * 4 * row_bytes + slab * 256), 2 /* nt */) : lu32x4{0, 0, 0, 0};
        if constexpr (F::kBlockScales) {
#pragma unroll
            for (int r = 0; r < RT; ++r) {
                if (!part) {
                    sb[s][r] = *reinterpret_cast<const lu32x4_a4 *>(s_lane[r] + slab * 16);
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) sb[s][r][q] = q < part_held ? reinterpret_cast<const uint32_t *>(s_lane[r] + slab * 16)[q] : kUnitScales;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int h = 0; h < CH; ++h)         // piece 4q + grp of the slab lies in chunk 4q >> SHIFT: inside a partial slab below part_held
                xb[s][q][h] = (has_x && !(part && ((4 * q) >> SHIFT) >= part_held)) ? *reinterpret_cast<const lu32x4 *>(xrow + slab * 128 * CH + q * 32 * CH + h * 8)
                                                                                    : lu32x4{0, 0, 0, 0};
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
                const lu32x4 piece = *reinterpret_cast<const lu32x4 *>(tile + col * 256 + (((4 * q + grp) ^ col) & 15) * 16);
                float scale = 1.0f;
                if constexpr (F::kBlockScales) scale = e8m0_scale(sb[s][r][q], s_shift);
#pragma unroll
                for (int h = 0; h < CH; ++h) acc[r] = lin_mfma<T>(F::template frag<T>(piece, h, scale), xb[s][q][h], acc[r]);
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
    if constexpr (!F::kBlockScales) {
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[r][i] *= p.w_scale[(int64_t)r * out_n + n + i];
    }
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = round_through<T>(acc[0][i]);
    if (p.epilogue == 1) {
        const uint2 r = *reinterpret_cast<const uint2 *>(p.aux + (int64_t)col * p.aux_row_stride + n);
        v[0] += lo_to_f32<T>(r.x); v[1] += hi_to_f32<T>(r.x); v[2] += lo_to_f32<T>(r.y); v[3] += hi_to_f32<T>(r.y);
    }
    if constexpr (PAIR) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = silu_round<T>(v[i]) * round_through<T>(acc[1][i]);
    }
    uint2 o;
    o.x = pack2<T>(v[0], v[1]);
    o.y = pack2<T>(v[2], v[3]);
    *reinterpret_cast<uint2 *>(p.y + (int64_t)col * p.y_row_stride + n) = o;
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------
// Wavefronts per workgroup (the K split inside it) from the W ROWS, as launch_linear_gemv / launch_linear_wg do, so that the stacked gate / up
// launch splits K exactly like the plain projection of the same matrix.  A slab is 4 KiB per load round of a wavefront in every format, the same
// bytes as a 128-input chunk of the 16-bit kernels, so the depth rule of waves_per_workgroup (at least 4 units per wavefront) carries over in
// slabs, times the format's measured `units per slab` (F::kGemvPlan / F::kWgPlan; 1 unless the format says otherwise).
struct WqPlan {
    const char *waves_env; int waves_per_cu;     // wavefronts per CU that stream W, and the knob that overrides it
    const char *units_env; int units_per_slab;   // units a slab counts for in the depth rule, and its knob (null: none)
};
template <typename F, bool WG> static inline int wq_waves(const LinearParams &p) {
    static const WqPlan plan = WG ? F::kWgPlan : F::kGemvPlan;
    static const int wpc = env_int(plan.waves_env, plan.waves_per_cu);
    static const int ups = plan.units_env ? std::max(1, std::min(4, env_int(plan.units_env, plan.units_per_slab))) : plan.units_per_slab;
    return waves_per_workgroup(p.n / 16, (int64_t)((p.k + 128 * F::CH - 1) / (128 * F::CH)) * ups, wpc);
}

template <typename T, typename F> static int launch_wq_gemv(const typename F::Args &a, hipStream_t stream) {
    const LinearParams &p = a.p;
    const bool pair = p.epilogue == 2;
    const int nw = wq_waves<F, false>(p);
    const dim3 grid((unsigned)((pair ? p.n / 2 : p.n) / 16)), block(64 * nw);
    dispatch_nw(nw, [&](auto NW_) {
        constexpr int NW = decltype(NW_)::value;
        auto rows = [&](auto NB_) {
            constexpr int NB = decltype(NB_)::value;
            if (pair) hipLaunchKernelGGL((linear_wq_gemv_kernel<T, F, NW, true, NB, F::gemv_depth(true, NB)>), grid, block, 0, stream, a);
            else hipLaunchKernelGGL((linear_wq_gemv_kernel<T, F, NW, false, NB, F::gemv_depth(false, NB)>), grid, block, 0, stream, a);
        };
        if (p.batch == 1) rows(int_c<1>{}); else if (p.batch == 2) rows(int_c<2>{}); else rows(int_c<4>{});
    });
    return ATOMA_CHECK_LAUNCH("linear_wq_gemv_kernel") ? 0 : -1;
}

template <typename T, typename F> static int launch_wq_wg(const typename F::Args &a, hipStream_t stream) {
    const LinearParams &p = a.p;
    const bool pair = p.epilogue == 2;
    const int nw = wq_waves<F, true>(p);
    const dim3 grid((unsigned)((pair ? p.n / 2 : p.n) / 16)), block(64 * nw);
    dispatch_nw(nw, [&](auto NW_) {
        constexpr int NW = decltype(NW_)::value;
        if (pair) hipLaunchKernelGGL((linear_wq_wg_kernel<T, F, NW, true, F::wg_depth(true)>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((linear_wq_wg_kernel<T, F, NW, false, F::wg_depth(false)>), grid, block, 0, stream, a);
    });
    return ATOMA_CHECK_LAUNCH("linear_wq_wg_kernel") ? 0 : -1;
}

// 1..4 rows, 5..16 rows, and beyond them whatever the format has (F::launch_above_wg; a format whose batch bound is the MFMA kernel's has none)
template <typename T, typename F> static int launch_wq(typename F::Args &a, hipStream_t stream) {
    if (a.p.batch <= std::min(F::gemv_rows(), 4)) return launch_wq_gemv<T, F>(a, stream);
    if constexpr (F::kMaxBatch > 16) {
        if (a.p.batch > std::min(F::wg_rows(), 16)) return F::template launch_above_wg<T>(a.p, stream);
    }
    return launch_wq_wg<T, F>(a, stream);
}

// ---- the entry ---------------------------------------------------------------------------------------------------------------------------
// Behind the three extern "C" entries of a format.  w_row_stride counts bytes; scale_row_stride is read with block scales only.  The formats
// answer out_features == 0 differently: with block scales it is "nothing to do" once the entry's own checks pass, with row scales the shared
// checks refuse it.
template <typename F>
static int linear_wq_entry(const void *x, const void *w, const void *w_scale, void *y, int64_t batch, int64_t in_features, int64_t out_features,
                           int64_t x_row_stride, int64_t w_row_stride, int64_t scale_row_stride, int64_t y_row_stride, int epilogue, const void *aux,
                           int64_t aux_row_stride, int dtype, void *stream) {
    clear_error();
    const std::string name = F::kName, wn = F::kW;
    auto fail = [&](const std::string &what) { set_error(name + ": " + what); return false; };
    if (dtype != ATOMA_F16 && dtype != ATOMA_BF16) { fail("dtype (the activation dtype) must be f16 or bf16"); return -1; }
    if (batch < 0 || batch > F::kMaxBatch) { fail(F::kBatchRule); return -1; }
    auto own_checks = [&]() {
        if (F::kBlockScales && scale_row_stride < in_features / 32) return fail("row strides must cover a row (scale_row_stride: in_features / 32 bytes)");
        if (x_row_stride % 8 || y_row_stride % 4) return fail("strides must keep rows 16-byte (x) / 8-byte (y) aligned");
        if (w_row_stride % 16) return fail(wn + "_row_stride (bytes) must be a multiple of 16");
        if (F::kBlockScales && scale_row_stride % 4) return fail("scale_row_stride (bytes) must be a multiple of 4");
        if (!x || !w || !y || (reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w)) & 15u || reinterpret_cast<uintptr_t>(y) & 7u)
            return fail("x and " + wn + " must be 16-byte aligned, y 8-byte aligned");
        if (!w_scale || reinterpret_cast<uintptr_t>(w_scale) & 3u) return fail(F::kScaleRule);
        // a row tile (and the up rows of the stacked gate / up kernels) is reached through a 32-bit buffer offset from the tile's base
        if (((epilogue == 2 ? out_features / 2 : 0) + 32) * w_row_stride >= ((int64_t)1 << 31))
            return fail("the weight rows a workgroup reaches must stay below 2 GiB (32-bit buffer offsets)");
        return true;
    };
    if (F::kBlockScales && out_features == 0) return own_checks() ? 0 : -1;
    // the shared checks see the inputs a weight row's bytes cover.  The min() keeps the product from overflowing: a stride beyond in_features
    // covers the row whatever its size.
    if (!check_linear_args(F::kName, in_features, out_features, x_row_stride, F::kInputsPerByte * std::min(w_row_stride, std::max<int64_t>(in_features, 0)),
                           y_row_stride, epilogue, aux, aux_row_stride))
        return -1;
    if (!own_checks()) return -1;
    if (batch == 0) return 0;
    typename F::Args a = F::args(linear_params_of(x, w, y, batch, in_features, out_features, x_row_stride, w_row_stride, y_row_stride, epilogue, aux, aux_row_stride),
                                 w_scale, scale_row_stride);
    const auto s = static_cast<hipStream_t>(stream);
    return dtype == ATOMA_BF16 ? launch_wq<bf16_t, F>(a, s) : launch_wq<f16_t, F>(a, s);
}

}  // namespace atoma

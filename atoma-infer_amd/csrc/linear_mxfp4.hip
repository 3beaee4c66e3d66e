// MXFP4 (OCP microscaling: e2m1 elements, one e8m0 scale per block of 32 inputs) WEIGHTS for the decode-step projections, "W4A16":
//   y[b][n] = round(sum_k x[b][k] * e2m1(nibble[n][k]) * 2^(w_scale[n][k / 32] - 127)), batch <= 16.
//
// The next step after linear_fp8w.hip in the same direction: at 1..16 rows a projection is a stream over the weights, so the only thing left to
// win is moving fewer bytes -- 0.53 bytes per weight (K/2 nibble bytes + K/32 scale bytes per row) against fp8's 1.  w4 [n][k / 2]: byte i of a
// row holds input 2i in its low nibble and input 2i + 1 in its high nibble (bit 3 the sign, bits 0..2 index {0, .5, 1, 1.5, 2, 3, 4, 6});
// w_scale [n][k / 32] bytes.  e2m1 x 2^e is an exact bf16 / f16 number and gfx950 converts a byte to a packed pair with the block scale applied
// in one instruction (v_cvt_scalef32_pk_{bf16,f16}_fp4, scale operand as_float(byte << 23)), so everything behind the conversion is the 16-bit
// kernels' arithmetic (v_dot2c / v_mfma_f32_16x16x32, fp32 accumulation); nothing is scaled per element afterwards and nothing after the sum.
// A 16-byte load is exactly one MX block (32 inputs, one scale); the two regimes are linear_fp8w.hip's, one call one launch:
//   * 1..4 rows   linear_mxfp4_gemv_kernel: 4 rows x 256 contiguous bytes (= 512 inputs) per load instruction, v_dot2c;
//   * 5..16 rows  linear_mxfp4_wg_kernel: the same loads re-laid into the MFMA A-operand order through a 4 KiB LDS tile per wavefront; one
//                 16-byte LDS read (one block) feeds four MFMAs, one per word (the k order inside an MFMA is free as long as x agrees).
// A slab is therefore 512 inputs; in_features is a multiple of 128, so the last slab may hold 128, 256 or 384: lanes beyond it load nothing
// (zeros for W and x).  The scale bytes of a slab come with ONE more load instruction per 16 rows (against four for the nibbles): a dword is the
// four scales of a 128-input chunk.  W by non-temporal buffer loads (read once), x from L2.  More than 16 rows is refused: the fp8 17..64-row
// structure loses to 16-bit weights and is not copied a third time.
// The wavefront count per workgroup derives from the W rows, never from the epilogue, and the merge across wavefronts runs in a fixed order, so
// _residual and _silu_mul are bit-identical to the plain call followed by atoma_add / atoma_silu_mul, and results are deterministic.
// Pipeline and row sum are linear_stream.h's, the launch plan and the shared argument checks linear_plan.h's; the parameters are LinearParams
// with nibble bytes behind w, plus Mx4Scales as a second by-value argument.
// Out of scope here: the fused RMSNorm and q/k/v + RoPE + cache forms, 17 rows and more, MX activations (the mfma_scale_*_f8f6f4 path).
// atoma_quantize_weight_mxfp4 at the bottom: round to nearest, ties to the even code, saturating at 6; one thread per block of 32 inputs.
#include "linear_plan.h"
#include <stdlib.h>

namespace atoma {

// LinearParams here: w = nibble bytes [n][k / 2] (w4_bytes), w_row_stride in bytes; the block scales travel next to it
struct Mx4Scales {
    const uint8_t *scale;        // [n][k / 32] e8m0 bytes, rows 4-byte aligned
    int64_t row_stride;          // bytes
};
__device__ __forceinline__ const uint8_t *w4_bytes(const LinearParams &p) { return reinterpret_cast<const uint8_t *>(p.w); }

constexpr uint32_t kUnitScales = 0x7f7f7f7fu;   // four scale bytes 127 (2^0): what a lane holds where a partial slab has no scales to load

__device__ __forceinline__ float e8m0_scale(uint32_t dword, int shift) { return __uint_as_float(((dword >> shift) & 0xffu) << 23); }

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

// 1..4 rows.  Workgroup = NW wavefronts x 16 output features (PAIR: + the 16 matching up features); wavefront w streams the w-th part of K
// in slabs of 512 inputs: lane 16.g + c loads bytes 16c..16c+15 of row 4.rg + g (4 rows x 256 B per instruction) -- block 16.slab + c of that
// row -- converts them to 16 pairs and multiplies with the matching 32 inputs of every batch row (four 16-byte loads of x).  The scales of the
// slab, all 16 rows, are one dword load: lane 4.row + j holds the scales of chunk j (blocks 4j..4j+3) of row `row`; lane (g, c) fetches the
// dword of lane 4.(4.rg + g) + (c >> 2) with ds_bpermute and takes byte c & 3.  Merge over LDS and epilogues as linear_fp8w_gemv_kernel.
template <typename T, int NW, bool PAIR, int NB, int P>
__global__ void __launch_bounds__(64 * NW) linear_mxfp4_gemv_kernel(const LinearParams p, const Mx4Scales sp) {
    constexpr int RT = PAIR ? 2 : 1;
    __shared__ float red[NW][RT][16][4];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), g = lane >> 4, c = lane & 15;
    const int n0 = blockIdx.x * 16;
    const int out_n = PAIR ? p.n / 2 : p.n;
    const int slabs = (p.k + 511) >> 9, per = (slabs + NW - 1) / NW;
    const int part_chunks = (p.k >> 7) & 3;                      // 128-input chunks in the partial last slab; 0: every slab is whole
    const int part_slab = part_chunks ? slabs - 1 : -1;
    const int c0 = wave * per, c1 = min(c0 + per, slabs);
    const int64_t row_bytes = p.w_row_stride;

    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(w4_bytes(p) + (int64_t)n0 * row_bytes), 0, 0x7fffffff, 0x00020000);
    uint32_t w_lane[RT];
    const uint32_t *s_lane[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        w_lane[r] = (uint32_t)(((int64_t)r * out_n + g) * row_bytes + c * 16);
        s_lane[r] = reinterpret_cast<const uint32_t *>(sp.scale + ((int64_t)r * out_n + n0 + (lane >> 2)) * sp.row_stride) + (lane & 3);
    }
    const uint16_t *xrow[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) xrow[b] = p.x + (int64_t)min(b, p.batch - 1) * p.x_row_stride + c * 32;   // rows beyond the batch: recomputed, never stored
    const int s_shift = (c & 3) * 8;
    int s_from[4];                                               // ds_bpermute address of the lane that holds row 4.rg + g, chunk c >> 2
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) s_from[rg] = (4 * (4 * rg + g) + (c >> 2)) * 4;

    lu32x4 wb[P][RT][4], xb[P][NB][4];
    uint32_t sb[P][RT];
    auto issue = [&](int s, int slab) {
        const bool part = slab == part_slab;
        const bool ok = !part || (c >> 2) < part_chunks;
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg)
                wb[s][r][rg] = ok ? __builtin_amdgcn_raw_buffer_load_b128(wr, w_lane[r], (int)(rg * 4 * row_bytes + slab * 256), 2 /* nt */) : lu32x4{0, 0, 0, 0};
#pragma unroll
        for (int r = 0; r < RT; ++r) sb[s][r] = (!part || (lane & 3) < part_chunks) ? s_lane[r][slab * 4] : kUnitScales;
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int h = 0; h < 4; ++h) xb[s][b][h] = ok ? *reinterpret_cast<const lu32x4 *>(xrow[b] + slab * 512 + h * 8) : lu32x4{0, 0, 0, 0};
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
                const float scale = e8m0_scale((uint32_t)__builtin_amdgcn_ds_bpermute(s_from[rg], (int)sb[s][r]), s_shift);
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    const lu32x4 w = w4_frag<T>(wb[s][r][rg][h], scale);
#pragma unroll
                    for (int b = 0; b < NB; ++b) {
                        float a = acc[r][rg][b];
#pragma unroll
                        for (int e = 0; e < 4; ++e) a = dot2<T>(w[e], xb[s][b][h][e], a);
                        acc[r][rg][b] = a;
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
        v[r] = round_through<T>(t);
    }
    float out = v[0];
    if (p.epilogue == 1) out += lo_to_f32<T>((uint32_t)p.aux[(int64_t)b * p.aux_row_stride + n]);
    if constexpr (PAIR) out = silu_round<T>(out) * v[1];
    p.y[(int64_t)b * p.y_row_stride + n] = (uint16_t)f32_to_bits<T>(out);
}

// 5..16 rows.  The loads of the kernel above (4 rows x 256 B per instruction), re-laid through a 4 KiB LDS tile per wavefront and row tile as
// in linear_fp8w_wg_kernel: lane 16.g + c writes its 16 bytes of row 4.q + g to [row][piece c ^ row], lane 16.grp + col reads
// [row col][piece (4q + grp) ^ col] = block 4q + grp of the slab, inputs 32.(4q + grp) ..+31; word e of it is the A operand of one MFMA against
// x[col][the same 8 inputs].  Block 4q + grp is byte grp of scale dword q: lane (grp, col) loads the 16 scale bytes of row col and this slab
// itself (one load instruction per slab; dword by dword in a partial slab).  Result tile: lane holds y^T[n0 + 4.grp + i][batch row col].
typedef lu32x4 __attribute__((aligned(4))) lu32x4_a4;
template <typename T, int NW, bool PAIR, int P>
__global__ void __launch_bounds__(64 * NW) linear_mxfp4_wg_kernel(const LinearParams p, const Mx4Scales sp) {
    constexpr int RT = PAIR ? 2 : 1;
    __shared__ float red[NW > 1 ? NW - 1 : 1][RT][64][4];
    __shared__ __attribute__((aligned(16))) char relay[NW][RT][4096];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), grp = lane >> 4, col = lane & 15;
    const int n0 = blockIdx.x * 16;
    const int out_n = PAIR ? p.n / 2 : p.n;
    const int slabs = (p.k + 511) >> 9, per = (slabs + NW - 1) / NW;
    const int part_chunks = (p.k >> 7) & 3;
    const int part_slab = part_chunks ? slabs - 1 : -1;
    const int c0 = wave * per, c1 = min(c0 + per, slabs);
    const int64_t row_bytes = p.w_row_stride;

    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(w4_bytes(p) + (int64_t)n0 * row_bytes), 0, 0x7fffffff, 0x00020000);
    uint32_t w_lane[RT];
    const uint8_t *s_lane[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        w_lane[r] = (uint32_t)(((int64_t)r * out_n + grp) * row_bytes + col * 16);   // row 4.q + grp, piece col
        s_lane[r] = sp.scale + ((int64_t)r * out_n + n0 + col) * sp.row_stride;      // row col
    }
    const bool has_x = col < p.batch;
    const uint16_t *xrow = p.x + (int64_t)(has_x ? col : 0) * p.x_row_stride + grp * 32;
    const int s_shift = grp * 8;

    lu32x4 wb[P][RT][4], xb[P][4][4], sb[P][RT];
    auto issue = [&](int s, int slab) {
        const bool part = slab == part_slab;
        const bool ok = !part || (col >> 2) < part_chunks;
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                wb[s][r][q] = ok ? __builtin_amdgcn_raw_buffer_load_b128(wr, w_lane[r], (int)(q * 4 * row_bytes + slab * 256), 2 /* nt */) : lu32x4{0, 0, 0, 0};
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            if (!part) {
                sb[s][r] = *reinterpret_cast<const lu32x4_a4 *>(s_lane[r] + slab * 16);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) sb[s][r][q] = q < part_chunks ? reinterpret_cast<const uint32_t *>(s_lane[r] + slab * 16)[q] : kUnitScales;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e)          // block 4q + grp of the slab: inside a partial slab for q < part_chunks
                xb[s][q][e] = (has_x && !(part && q >= part_chunks)) ? *reinterpret_cast<const lu32x4 *>(xrow + slab * 512 + q * 128 + e * 8) : lu32x4{0, 0, 0, 0};
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
                const float scale = e8m0_scale(sb[s][r][q], s_shift);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[r] = lin_mfma<T>(w4_frag<T>(a[e], scale), xb[s][q][e], acc[r]);
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
// Wavefronts per workgroup (the K split inside it) from the W ROWS, as launch_fp8w_gemv / launch_fp8w_wg do.  A slab is 512 inputs = 4 KiB per
// load round of a wavefront, the same bytes as a 256-input slab of fp8 weights; a row of W is a quarter of the 16-bit row, so K = 4096 is 8 slabs.
// The depth rule of waves_per_workgroup (at least 4 units per wavefront) is fed `units per slab` units for each slab, measured per kernel
// (DESIGN.md 4.8f): the VALU kernel 2 (two slabs per wavefront: q/k/v at 1 row 5.9 us against 6.5) under at most 16 wavefronts per CU (gate/up at
// 1 row: two wavefronts per workgroup 13.2 us, four 15.5), the MFMA kernel 1 (four slabs per wavefront, as everywhere else).
static const int mxfp4_gemv_max_batch = env_int("ATOMA_MXFP4_GEMV_MAX_BATCH", 4);
static inline int64_t mxfp4_units(const LinearParams &p, int units_per_slab) { return (int64_t)((p.k + 511) / 512) * std::max(1, std::min(4, units_per_slab)); }

template <typename T> static int launch_mxfp4_gemv(LinearParams &p, const Mx4Scales &sp, hipStream_t stream) {
    static const int wpc = env_int("ATOMA_MXFP4_GEMV_WAVES_PER_CU", 16);
    const bool pair = p.epilogue == 2;
    static const int ups = env_int("ATOMA_MXFP4_GEMV_UNITS_PER_SLAB", 2);
    const int nw = waves_per_workgroup(p.n / 16, mxfp4_units(p, ups), wpc);
    const dim3 grid((unsigned)((pair ? p.n / 2 : p.n) / 16)), block(64 * nw);
    dispatch_nw(nw, [&](auto NW_) {
        constexpr int NW = decltype(NW_)::value;
        auto rows = [&](auto NB_) {
            constexpr int NB = decltype(NB_)::value;
            if (pair) hipLaunchKernelGGL((linear_mxfp4_gemv_kernel<T, NW, true, NB, (NB > 1 ? 1 : 2)>), grid, block, 0, stream, p, sp);
            else hipLaunchKernelGGL((linear_mxfp4_gemv_kernel<T, NW, false, NB, (NB > 2 ? 1 : 2)>), grid, block, 0, stream, p, sp);
        };
        if (p.batch == 1) rows(int_c<1>{}); else if (p.batch == 2) rows(int_c<2>{}); else rows(int_c<4>{});
    });
    return ATOMA_CHECK_LAUNCH("linear_mxfp4_gemv_kernel") ? 0 : -1;
}

template <typename T> static int launch_mxfp4_wg(LinearParams &p, const Mx4Scales &sp, hipStream_t stream) {
    static const int wpc = env_int("ATOMA_MXFP4_WG_WAVES_PER_CU", 8);
    const bool pair = p.epilogue == 2;
    static const int ups = env_int("ATOMA_MXFP4_WG_UNITS_PER_SLAB", 1);
    const int nw = waves_per_workgroup(p.n / 16, mxfp4_units(p, ups), wpc);
    const dim3 grid((unsigned)((pair ? p.n / 2 : p.n) / 16)), block(64 * nw);
    dispatch_nw(nw, [&](auto NW_) {
        constexpr int NW = decltype(NW_)::value;
        if (pair) hipLaunchKernelGGL((linear_mxfp4_wg_kernel<T, NW, true, 1>), grid, block, 0, stream, p, sp);
        else hipLaunchKernelGGL((linear_mxfp4_wg_kernel<T, NW, false, 2>), grid, block, 0, stream, p, sp);
    });
    return ATOMA_CHECK_LAUNCH("linear_mxfp4_wg_kernel") ? 0 : -1;
}

template <typename T> static int launch_mxfp4(LinearParams &p, const Mx4Scales &sp, hipStream_t stream) {
    if (p.batch <= std::min(mxfp4_gemv_max_batch, 4)) return launch_mxfp4_gemv<T>(p, sp, stream);
    return launch_mxfp4_wg<T>(p, sp, stream);
}

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

static int linear_mxfp4_entry(const void *x, const void *w4, const void *w_scale, void *y, int64_t batch, int64_t in_features, int64_t out_features,
                              int64_t x_row_stride, int64_t w4_row_stride, int64_t scale_row_stride, int64_t y_row_stride, int epilogue, const void *aux,
                              int64_t aux_row_stride, int dtype, void *stream) {
    using namespace atoma;
    clear_error();
    if (dtype != ATOMA_F16 && dtype != ATOMA_BF16) { set_error("linear_decode_mxfp4: dtype (the activation dtype) must be f16 or bf16"); return -1; }
    if (batch < 0 || batch > 16) {
        set_error("linear_decode_mxfp4: batch must be in [0, 16] (the MXFP4-weight kernels serve 1..16 rows; more than 16 rows is not supported)");
        return -1;
    }
    // what this entry checks itself; they also stand when out_features == 0 (nothing to do), which the shared checks would refuse
    auto own_checks = [&]() {
        if (scale_row_stride < in_features / 32) { set_error("linear_decode_mxfp4: row strides must cover a row (scale_row_stride: in_features / 32 bytes)"); return false; }
        if (x_row_stride % 8 || y_row_stride % 4) { set_error("linear_decode_mxfp4: strides must keep rows 16-byte (x) / 8-byte (y) aligned"); return false; }
        if (w4_row_stride % 16) { set_error("linear_decode_mxfp4: w4_row_stride (bytes) must be a multiple of 16"); return false; }
        if (scale_row_stride % 4) { set_error("linear_decode_mxfp4: scale_row_stride (bytes) must be a multiple of 4"); return false; }
        if (!x || !w4 || !y || (reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w4)) & 15u || reinterpret_cast<uintptr_t>(y) & 7u) {
            set_error("linear_decode_mxfp4: x and w4 must be 16-byte aligned, y 8-byte aligned");
            return false;
        }
        if (!w_scale || reinterpret_cast<uintptr_t>(w_scale) & 3u) { set_error("linear_decode_mxfp4: w_scale must be 4-byte aligned e8m0 bytes [out_features, in_features / 32]"); return false; }
        // a row tile (and the up rows of the stacked gate / up kernels) is reached through a 32-bit buffer offset from the tile's base
        if (((epilogue == 2 ? out_features / 2 : 0) + 32) * w4_row_stride >= ((int64_t)1 << 31)) {
            set_error("linear_decode_mxfp4: the weight rows a workgroup reaches must stay below 2 GiB (32-bit buffer offsets)");
            return false;
        }
        return true;
    };
    if (out_features == 0) return own_checks() ? 0 : -1;
    // w4_row_stride counts bytes, two inputs each: the shared checks see the inputs it covers.  The min() keeps 2 * stride from overflowing:
    // a stride beyond in_features covers the row whatever its size.
    if (!check_linear_args("linear_decode_mxfp4", in_features, out_features, x_row_stride, 2 * std::min(w4_row_stride, std::max<int64_t>(in_features, 0)),
                           y_row_stride, epilogue, aux, aux_row_stride))
        return -1;
    if (!own_checks()) return -1;
    if (batch == 0) return 0;
    LinearParams p = linear_params_of(x, w4, y, batch, in_features, out_features, x_row_stride, w4_row_stride, y_row_stride, epilogue, aux, aux_row_stride);
    const Mx4Scales sp{static_cast<const uint8_t *>(w_scale), scale_row_stride};
    const auto s = static_cast<hipStream_t>(stream);
    return dtype == ATOMA_BF16 ? launch_mxfp4<bf16_t>(p, sp, s) : launch_mxfp4<f16_t>(p, sp, s);
}

extern "C" int atoma_linear_decode_mxfp4(const void *x, const void *w4, const void *w_scale, void *y, int64_t batch, int64_t in_features,
                                         int64_t out_features, int64_t x_row_stride, int64_t w4_row_stride, int64_t scale_row_stride,
                                         int64_t y_row_stride, int dtype, void *stream) {
    return linear_mxfp4_entry(x, w4, w_scale, y, batch, in_features, out_features, x_row_stride, w4_row_stride, scale_row_stride, y_row_stride, 0, nullptr, 0,
                              dtype, stream);
}
extern "C" int atoma_linear_decode_mxfp4_residual(const void *x, const void *w4, const void *w_scale, const void *residual, void *y, int64_t batch,
                                                  int64_t in_features, int64_t out_features, int64_t x_row_stride, int64_t w4_row_stride,
                                                  int64_t scale_row_stride, int64_t residual_row_stride, int64_t y_row_stride, int dtype, void *stream) {
    return linear_mxfp4_entry(x, w4, w_scale, y, batch, in_features, out_features, x_row_stride, w4_row_stride, scale_row_stride, y_row_stride, 1, residual,
                              residual_row_stride, dtype, stream);
}
extern "C" int atoma_linear_decode_mxfp4_silu_mul(const void *x, const void *w4_gate_up, const void *w_scale, void *y, int64_t batch, int64_t in_features,
                                                  int64_t intermediate, int64_t x_row_stride, int64_t w4_row_stride, int64_t scale_row_stride,
                                                  int64_t y_row_stride, int dtype, void *stream) {
    return linear_mxfp4_entry(x, w4_gate_up, w_scale, y, batch, in_features, 2 * intermediate, x_row_stride, w4_row_stride, scale_row_stride, y_row_stride, 2,
                              nullptr, 0, dtype, stream);
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

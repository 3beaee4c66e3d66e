// What the projection kernels share on the device (linear_decode.hip, linear_wq.h with linear_fp8w.hip and linear_mxfp4.hip, linear_tile.hip, linear_wide.hip), each thing once: the
// software pipeline of the weight-streaming kernels, the 16-lane row sum, the tile kernels' plain rounded store, and the kernel that adds K splits.
#pragma once
#include "linear_params.h"

namespace atoma {

// Software pipeline of a weight stream over the chunks [c0, c1): P chunks in flight, stage s of the registers holds chunk c0 + s (mod P).
// issue(s, chunk) requests a chunk into stage s, compute(s) consumes stage s (lambdas of the kernel).  With at least 2.P chunks the loads of the
// steady state are unconditional, which keeps the vmcnt waits exact; shorter ranges and the last chunks run guarded.  after_prologue() runs behind
// the first round of loads on both paths (the self-normalising kernel derives its scales there, under the latency of the first weights).  The
// stage index is a compile-time constant everywhere (unrolled loops over s): the stage arrays of the callers stay in registers.
// A macro on purpose: hipcc optimises the body of a __forceinline__ function template first -- stage loops unrolled around the inlined lambdas
// while their captures are still opaque pointers -- and only then inlines it; the conditional x loads of a stage then no longer share a branch
// and the kernels come out longer.  Expanded in place, the kernels compile to what written-out loops give.  c0_ and c1_ are evaluated several
// times: pass plain locals.
__device__ __forceinline__ void stream_no_op() {}
#define ATOMA_STREAM_PIPELINE(P_, c0_, c1_, issue_, compute_, after_prologue_)                \
    do {                                                                                      \
        int c_ = (c0_);                                                                       \
        if ((c0_) + 2 * (P_) <= (c1_)) {                                                      \
            _Pragma("unroll") for (int s_ = 0; s_ < (P_); ++s_) issue_(s_, (c0_) + s_);       \
            after_prologue_();                                                                \
            for (; c_ + 2 * (P_) <= (c1_); c_ += (P_)) {                                      \
                _Pragma("unroll") for (int s_ = 0; s_ < (P_); ++s_) {                         \
                    compute_(s_);                                                             \
                    issue_(s_, c_ + s_ + (P_));                                               \
                }                                                                             \
            }                                                                                 \
        } else {                                                                              \
            _Pragma("unroll") for (int s_ = 0; s_ < (P_); ++s_)                               \
                if ((c0_) + s_ < (c1_)) issue_(s_, (c0_) + s_);                               \
            after_prologue_();                                                                \
        }                                                                                     \
        for (; c_ < (c1_); c_ += (P_)) {                                                      \
            _Pragma("unroll") for (int s_ = 0; s_ < (P_); ++s_)                               \
                if (c_ + s_ < (c1_)) {                                                        \
                    compute_(s_);                                                             \
                    if (c_ + s_ + (P_) < (c1_)) issue_(s_, c_ + s_ + (P_));                   \
                }                                                                             \
        }                                                                                     \
    } while (0)

__device__ __forceinline__ float row16_sum(float x) {   // sum over the 16 lanes of a DPP row
    x += __builtin_amdgcn_update_dpp(0.f, x, 0xB1, 0xf, 0xf, true);    // quad_perm [1,0,3,2]
    x += __builtin_amdgcn_update_dpp(0.f, x, 0x4E, 0xf, 0xf, true);    // quad_perm [2,3,0,1]
    x += __builtin_amdgcn_update_dpp(0.f, x, 0x141, 0xf, 0xf, true);   // row_half_mirror
    x += __builtin_amdgcn_update_dpp(0.f, x, 0x140, 0xf, 0xf, true);   // row_mirror
    return x;
}

// The rounded store of a plain projection: y[row][n ..+3] from four fp32 sums, + residual when p.epilogue == 1.  The epilogues keep the
// reference's rounding points: the projection's output is rounded to the storage dtype first, then the next op is applied and rounds again (a
// paired kernel: silu_round(gate) * round(up)).  Used by the tile kernels' plain stores only: in the other kernels hipcc schedules the code
// around an inlined helper differently from the written-out block (vgpr counts moved by up to 4), so they keep theirs.
template <typename T> __device__ __forceinline__ void linear_store4(const LinearParams &p, int64_t row, int n, lf32x4 sum) {
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = round_through<T>(sum[i]);
    if (p.epilogue == 1) {
        const uint2 r = *reinterpret_cast<const uint2 *>(p.aux + row * p.aux_row_stride + n);
        v[0] += lo_to_f32<T>(r.x); v[1] += hi_to_f32<T>(r.x); v[2] += lo_to_f32<T>(r.y); v[3] += hi_to_f32<T>(r.y);
    }
    uint2 o;
    o.x = pack2<T>(v[0], v[1]);
    o.y = pack2<T>(v[2], v[3]);
    *reinterpret_cast<uint2 *>(p.y + row * p.y_row_stride + n) = o;
}

// y[b][n] = round(sum over splits of the fp32 partials [x w_scale[n] where the weights are fp8: SCALED]); 4 outputs per thread, then the
// epilogue with the same rounding points.
template <typename T, bool SCALED> __device__ __forceinline__ float4 linear_sum_splits(const LinearParams &p, int64_t i, int64_t n, int64_t total) {
    float4 a = *reinterpret_cast<const float4 *>(p.partial + i);
    for (int s = 1; s < p.splits; ++s) {
        const float4 b = *reinterpret_cast<const float4 *>(p.partial + (int64_t)s * total + i);
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    if constexpr (SCALED) {
        const float *sc = p.w_scale + n;
        a.x *= sc[0]; a.y *= sc[1]; a.z *= sc[2]; a.w *= sc[3];
    }
    return make_float4(round_through<T>(a.x), round_through<T>(a.y), round_through<T>(a.z), round_through<T>(a.w));
}
template <typename T, bool SCALED> __global__ void __launch_bounds__(256) linear_reduce_kernel(const LinearParams p) {
    const int64_t total = (int64_t)p.batch * p.n;
    const int out_n = p.epilogue == 2 ? p.n / 2 : p.n;
    const int64_t o = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;      // index into the [batch, out_n] result
    if (o >= (int64_t)p.batch * out_n) return;
    const int64_t row = o / out_n, n = o - row * out_n;
    float4 a = linear_sum_splits<T, SCALED>(p, row * p.n + n, n, total);
    if (p.epilogue == 1) {
        const uint2 r = *reinterpret_cast<const uint2 *>(p.aux + row * p.aux_row_stride + n);
        a.x += lo_to_f32<T>(r.x); a.y += hi_to_f32<T>(r.x); a.z += lo_to_f32<T>(r.y); a.w += hi_to_f32<T>(r.y);
    } else if (p.epilogue == 2) {
        const float4 u = linear_sum_splits<T, SCALED>(p, row * p.n + out_n + n, out_n + n, total);
        a.x = silu_round<T>(a.x) * u.x; a.y = silu_round<T>(a.y) * u.y; a.z = silu_round<T>(a.z) * u.z; a.w = silu_round<T>(a.w) * u.w;
    }
    uint2 w;
    w.x = pack2<T>(a.x, a.y);
    w.y = pack2<T>(a.z, a.w);
    *reinterpret_cast<uint2 *>(p.y + row * p.y_row_stride + n) = w;
}

}  // namespace atoma

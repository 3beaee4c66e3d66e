// What the launchers of the streaming projection kernels share on the host (linear_decode.hip, linear_wq.h with linear_fp8w.hip and linear_mxfp4.hip), each thing once: the K-split plan
// with its fp32 workspace, the launch of the kernel that adds the splits, the wavefronts per workgroup, their dispatch, and the argument checks.
#pragma once
#include "linear_stream.h"
#include <algorithm>
#include <type_traits>

namespace atoma {

// K split over workgroups: as many splits as bring the grid to `target` workgroups (wavefronts) -- counted from the ROW TILES OF W, never from the
// epilogue, so that the stacked gate / up launch with its SiLU.up epilogue splits K exactly like the plain projection of the same matrix and stays
// bit-identical to projection + atoma_silu_mul -- never below min_chunks 128-input chunks per split.  Sets p.chunks_per_split, p.splits and
// p.partial: fp32 partials [splits][batch][n] in the stream's workspace when K is split or force_partial (an epilogue that needs the reduce kernel).
static inline bool plan_k_splits(LinearParams &p, int64_t row_tiles, int64_t target, int64_t min_chunks, hipStream_t stream, bool force_partial) {
    const int64_t chunks = p.k / 128;
    const int64_t splits = std::max<int64_t>(1, std::min<int64_t>(target / std::max<int64_t>(row_tiles, 1), chunks / min_chunks));
    p.chunks_per_split = (int)cdiv(chunks, splits);
    p.splits = (int)cdiv(chunks, p.chunks_per_split);
    p.partial = nullptr;
    if (p.splits > 1 || force_partial) {
        p.partial = static_cast<float *>(workspace(stream, (size_t)p.splits * p.batch * p.n * sizeof(float)));
        if (!p.partial) return false;
    }
    return true;
}

// the fp32 partials of p -> y (sum over the splits, scale where the weights are fp8, round, epilogue)
template <typename T, bool SCALED = false> static inline bool launch_reduce(const LinearParams &p, hipStream_t stream) {
    const int out_n = p.epilogue == 2 ? p.n / 2 : p.n;
    hipLaunchKernelGGL((linear_reduce_kernel<T, SCALED>), dim3((unsigned)cdiv((int64_t)p.batch * out_n, 1024)), dim3(256), 0, stream, p);
    return ATOMA_CHECK_LAUNCH(SCALED ? "linear_fp8w_reduce_kernel" : "linear_reduce_kernel");
}

// Wavefronts per workgroup of the single-launch kernels (the K split inside a workgroup): as many as keep waves_per_cu wavefronts per CU streaming,
// each with at least 4 units (128-input chunks, or the 4 KiB slabs of quantised weights, linear_wq.h: 4 KiB per load round either way).  From the W rows, as above.
static inline int waves_per_workgroup(int64_t row_tiles, int64_t units, int waves_per_cu) {
    int nw = 1;
    while (nw < 8 && row_tiles * nw * 2 <= (int64_t)device_num_cus() * waves_per_cu && units / (nw * 2) >= 4) nw *= 2;
    return nw;
}
// A run-time choice handed to a generic lambda as a compile-time constant: f(int_c<NW>{}) for nw = 1, 2, 4, 8
template <int N> using int_c = std::integral_constant<int, N>;
template <typename F> static inline void dispatch_nw(int nw, F &&f) {
    switch (nw) {
        case 1: f(int_c<1>{}); break;
        case 2: f(int_c<2>{}); break;
        case 4: f(int_c<4>{}); break;
        default: f(int_c<8>{}); break;
    }
}

// The argument checks every projection entry makes, in the order the entries report them (prefix: the entry's name in the message; the string is
// built only when a check fails).  What differs between the entries -- dtype, batch bound, alignment of the weights, 2 GiB rules -- stays with them.
static inline bool check_linear_args(const char *prefix, int64_t in_features, int64_t out_features, int64_t x_row_stride, int64_t w_row_stride,
                                     int64_t y_row_stride, int epilogue, const void *aux, int64_t aux_row_stride) {
    auto fail = [&](const char *what) { set_error(std::string(prefix) + ": " + what); return false; };
    if (in_features <= 0 || in_features % 128 != 0) return fail("in_features must be a positive multiple of 128");
    if (out_features <= 0 || out_features % 16 != 0) return fail("out_features must be a positive multiple of 16");
    if (epilogue < 0 || epilogue > 2) return fail("unknown epilogue");   // (the entries' callers pass 0, 1 or 2)
    if (epilogue == 2 && out_features % 32 != 0) return fail("the silu.up epilogue needs out_features to be a multiple of 32");
    if (epilogue == 1 && (!aux || aux_row_stride < out_features || aux_row_stride % 4 || (reinterpret_cast<uintptr_t>(aux) & 7u)))
        return fail("the residual epilogue needs an 8-byte aligned [batch, out_features] tensor");
    const int64_t y_width = epilogue == 2 ? out_features / 2 : out_features;
    if (x_row_stride < in_features || w_row_stride < in_features || y_row_stride < y_width) return fail("row strides must cover a row");
    return true;
}
// ... and the parameters both entries fill alike
static inline LinearParams linear_params_of(const void *x, const void *w, void *y, int64_t batch, int64_t in_features, int64_t out_features, int64_t x_row_stride,
                                            int64_t w_row_stride, int64_t y_row_stride, int epilogue, const void *aux, int64_t aux_row_stride) {
    LinearParams p{};
    p.x = static_cast<const uint16_t *>(x);
    p.w = static_cast<const uint16_t *>(w);
    p.y = static_cast<uint16_t *>(y);
    p.x_row_stride = x_row_stride; p.w_row_stride = w_row_stride; p.y_row_stride = y_row_stride;
    p.batch = (int)batch; p.n = (int)out_features; p.k = (int)in_features;
    p.epilogue = epilogue; p.aux = static_cast<const uint16_t *>(aux); p.aux_row_stride = aux_row_stride;
    return p;
}

}  // namespace atoma

// On-device greedy selection over the logits rows of a step.
//
// Replaces the per-sequence device->host copies of /root/reference/backends/vllm/src/model_executor.rs:
// 206-249 (`logits.i(idx)` -> `LogitsProcessor::sample` with Sampling::ArgMax -> `to_vec1::<f32>()[next_token]`):
// two 512 KB transfers per sequence per step at a 128k vocabulary become 8 bytes per sequence.  Index work:
// bit-exact against numpy argmax (smallest index among the maxima; NaNs are never selected).
// HBM-bound: rows * vocab * elt bytes read once.
#include "common.h"
#include "sampling_rows.h"
#include <cstdlib>

namespace atoma {

// the per-row code lives in sampling_rows.h (shared with sample_batch.hip); these kernels read the rows as they are in memory

// one workgroup per row; 16-byte loads when the row allows it
template <typename T, bool VEC>
__global__ void __launch_bounds__(1024) argmax_rows_kernel(const void *__restrict__ logits, int64_t row_stride_bytes, int vocab,
                                                           int32_t *__restrict__ out_idx, float *__restrict__ out_val) {
    __shared__ ArgmaxShared sh;
    const char *row = static_cast<const char *>(logits) + (int64_t)blockIdx.x * row_stride_bytes;
    argmax_row<T, VEC>(sh, row, vocab, NoPenalty{}, out_idx + blockIdx.x, out_val ? out_val + blockIdx.x : nullptr);
}

template <typename T>
__global__ void __launch_bounds__(TOPK_THREADS) topk_rows_kernel(const void *__restrict__ logits, int64_t row_stride_bytes, int vocab, int k,
                                                                 float *__restrict__ out_val, int32_t *__restrict__ out_idx) {
    __shared__ TopkShared sh;
    const char *row = static_cast<const char *>(logits) + (int64_t)blockIdx.x * row_stride_bytes;
    topk_row_hist<T>(sh, row, vocab, k, NoPenalty{}, out_val + (int64_t)blockIdx.x * k, out_idx + (int64_t)blockIdx.x * k);
}

// the one-pass register route (sampling_rows.h: topk_row_reg); the launcher guarantees vocab % EPV == 0 and aligned rows
template <typename T>
__global__ void __launch_bounds__(TOPK_THREADS) topk_rows_reg_kernel(const void *__restrict__ logits, int64_t row_stride_bytes, int vocab, int k,
                                                                     float *__restrict__ out_val, int32_t *__restrict__ out_idx) {
    __shared__ TopkShared sh;
    const char *row = static_cast<const char *>(logits) + (int64_t)blockIdx.x * row_stride_bytes;
    topk_row_reg<T>(sh, row, vocab, k, NoPenalty{}, out_val + (int64_t)blockIdx.x * k, out_idx + (int64_t)blockIdx.x * k);
}

template <typename T>
__global__ void __launch_bounds__(SAMPLE_THREADS) sample_full_kernel(const void *__restrict__ logits, int64_t row_stride_bytes, int vocab, float inv_temp,
                                                                     const float *__restrict__ u, int32_t *__restrict__ out_idx, float *__restrict__ out_logit) {
    __shared__ SampleFullShared sh;
    const char *row = static_cast<const char *>(logits) + (int64_t)blockIdx.x * row_stride_bytes;
    sample_full_row<T>(sh, row, vocab, inv_temp, u[blockIdx.x], NoPenalty{}, out_idx + blockIdx.x, out_logit ? out_logit + blockIdx.x : nullptr);
}

// top-k / top-p: `vals`, `idxs` [rows][k] from atoma_topk_rows (value descending, index ascending); one wave per row
template <typename T>
__global__ void __launch_bounds__(256) sample_topk_kernel(const void *__restrict__ logits, int64_t row_stride_bytes, int vocab, const float *__restrict__ vals,
                                                          const int32_t *__restrict__ idxs, int k, float inv_temp, float top_p, const float *__restrict__ u,
                                                          int32_t *__restrict__ out_idx, float *__restrict__ out_logit, int full_row_nucleus) {
    __shared__ SampleTopkShared sh;
    const char *row = static_cast<const char *>(logits) + (int64_t)blockIdx.x * row_stride_bytes;
    sample_topk_row<T>(sh, row, vocab, vals + (int64_t)blockIdx.x * k, idxs + (int64_t)blockIdx.x * k, k, inv_temp, top_p, u[blockIdx.x], full_row_nucleus,
                       NoPenalty{}, out_idx + blockIdx.x, out_logit ? out_logit + blockIdx.x : nullptr);
}

void *workspace(hipStream_t stream, size_t bytes);   // runtime.hip

}  // namespace atoma

extern "C" int atoma_argmax_rows(const void *logits, int64_t rows, int64_t vocab, int64_t row_stride, int dtype, int32_t *out_idx,
                                 float *out_val, void *stream) {
    using namespace atoma;
    clear_error();
    if (dtype != ATOMA_F16 && dtype != ATOMA_BF16 && dtype != ATOMA_F32) { set_error("argmax_rows: dtype must be f16, bf16 or f32"); return -1; }
    if (rows < 0 || vocab <= 0 || vocab > 0x7ffffffe) { set_error("argmax_rows: invalid shape"); return -1; }
    if (row_stride < vocab) { set_error("argmax_rows: row_stride must be >= vocab"); return -1; }
    if (!out_idx) { set_error("argmax_rows: out_idx is required"); return -1; }
    if (rows == 0) return 0;
    const int elt = dtype == ATOMA_F32 ? 4 : 2;
    const int64_t stride_bytes = row_stride * elt;
    const bool vec = (reinterpret_cast<uintptr_t>(logits) & 15u) == 0 && stride_bytes % 16 == 0;
    const int threads = vocab >= 32768 ? 1024 : (vocab >= 4096 ? 256 : 64);
    const auto s = static_cast<hipStream_t>(stream);
#define ATOMA_ARGMAX(TT)                                                                                                   \
    do {                                                                                                                   \
        if (vec) hipLaunchKernelGGL((argmax_rows_kernel<TT, true>), dim3((unsigned)rows), dim3(threads), 0, s, logits,     \
                                    stride_bytes, (int)vocab, out_idx, out_val);                                           \
        else hipLaunchKernelGGL((argmax_rows_kernel<TT, false>), dim3((unsigned)rows), dim3(threads), 0, s, logits,        \
                                stride_bytes, (int)vocab, out_idx, out_val);                                               \
    } while (0)
    if (dtype == ATOMA_F32) ATOMA_ARGMAX(float);
    else if (dtype == ATOMA_BF16) ATOMA_ARGMAX(bf16_t);
    else ATOMA_ARGMAX(f16_t);
#undef ATOMA_ARGMAX
    return ATOMA_CHECK_LAUNCH("argmax_rows") ? 0 : -1;
}

static bool topk_reg_enabled() {   // ATOMA_TOPK_REG=0: always the two-pass histogram kernel (A/B runs)
    static const bool on = [] { const char *e = getenv("ATOMA_TOPK_REG"); return !(e && e[0] == '0'); }();
    return on;
}

extern "C" int atoma_topk_rows(const void *logits, int64_t rows, int64_t vocab, int64_t row_stride, int dtype, int64_t k, float *out_val,
                               int32_t *out_idx, void *stream) {
    using namespace atoma;
    clear_error();
    if (dtype != ATOMA_F16 && dtype != ATOMA_BF16 && dtype != ATOMA_F32) { set_error("topk_rows: dtype must be f16, bf16 or f32"); return -1; }
    if (rows < 0 || vocab <= 0 || vocab > 0x7ffffffe) { set_error("topk_rows: invalid shape"); return -1; }
    if (k <= 0 || k > TOPK_MAX || k > vocab) { set_error("topk_rows: k must be in [1, min(vocab, 1024)]"); return -1; }
    if (row_stride < vocab) { set_error("topk_rows: row_stride must be >= vocab"); return -1; }
    if (!out_val || !out_idx) { set_error("topk_rows: out_val and out_idx are required"); return -1; }
    if (rows == 0) return 0;
    const int64_t stride_bytes = row_stride * (dtype == ATOMA_F32 ? 4 : 2);
    const auto s = static_cast<hipStream_t>(stream);
    const int epv = dtype == ATOMA_F32 ? 4 : 8;
    const bool reg = vocab <= TOPK_REG_MAX_VOCAB && k <= TOPK_REG_MAX_K && vocab % epv == 0 && vocab >= 4 * TOPK_THREADS &&
                     (reinterpret_cast<uintptr_t>(logits) & 15u) == 0 && stride_bytes % 16 == 0 && topk_reg_enabled();
#define ATOMA_TOPK(TT)                                                                                                                       \
    do {                                                                                                                                     \
        if (reg) hipLaunchKernelGGL((topk_rows_reg_kernel<TT>), dim3((unsigned)rows), dim3(TOPK_THREADS), 0, s, logits, stride_bytes, (int)vocab, (int)k, out_val, out_idx); \
        else hipLaunchKernelGGL((topk_rows_kernel<TT>), dim3((unsigned)rows), dim3(TOPK_THREADS), 0, s, logits, stride_bytes, (int)vocab, (int)k, out_val, out_idx);       \
    } while (0)
    if (dtype == ATOMA_F32) ATOMA_TOPK(float);
    else if (dtype == ATOMA_BF16) ATOMA_TOPK(bf16_t);
    else ATOMA_TOPK(f16_t);
#undef ATOMA_TOPK
    return ATOMA_CHECK_LAUNCH("topk_rows") ? 0 : -1;
}

extern "C" int atoma_sample_rows(const void *logits, int64_t rows, int64_t vocab, int64_t row_stride, int dtype, float temperature, int64_t top_k,
                                 float top_p, const float *u, int32_t *out_idx, float *out_logit, void *stream) {
    using namespace atoma;
    clear_error();
    if (dtype != ATOMA_F16 && dtype != ATOMA_BF16 && dtype != ATOMA_F32) { set_error("sample_rows: dtype must be f16, bf16 or f32"); return -1; }
    if (rows < 0 || vocab <= 0 || vocab > (int64_t)SAMPLE_CHUNK * SAMPLE_MAX_CHUNKS) { set_error("sample_rows: invalid shape"); return -1; }
    if (row_stride < vocab) { set_error("sample_rows: row_stride must be >= vocab"); return -1; }
    if (!(temperature > 0.f)) { set_error("sample_rows: temperature must be positive (greedy selection is atoma_argmax_rows)"); return -1; }
    if (top_k < 0 || top_k > TOPK_MAX) { set_error("sample_rows: top_k must be in [0, 1024] (0 = no top-k)"); return -1; }
    if (!(top_p > 0.f)) { set_error("sample_rows: top_p must be in (0, 1] (1 = no top-p)"); return -1; }
    if (!u || !out_idx) { set_error("sample_rows: u and out_idx are required"); return -1; }
    if (rows == 0) return 0;
    const int64_t stride_bytes = row_stride * (dtype == ATOMA_F32 ? 4 : 2);
    const auto s = static_cast<hipStream_t>(stream);
    const float inv_temp = 1.f / temperature;
    const bool restricted = (top_k > 0 && top_k < vocab) || top_p < 1.f;
    if (!restricted) {
#define ATOMA_SF(TT) hipLaunchKernelGGL((sample_full_kernel<TT>), dim3((unsigned)rows), dim3(SAMPLE_THREADS), 0, s, logits, stride_bytes, (int)vocab, inv_temp, u, out_idx, out_logit)
        if (dtype == ATOMA_F32) ATOMA_SF(float); else if (dtype == ATOMA_BF16) ATOMA_SF(bf16_t); else ATOMA_SF(f16_t);
#undef ATOMA_SF
        return ATOMA_CHECK_LAUNCH("sample_rows") ? 0 : -1;
    }
    // top-p without top-k: the nucleus is searched among the 1024 most probable tokens first (it ends there for any peaked
    // distribution); a row whose 1024 most probable tokens do not reach top_p continues over the whole row (sorted_crossing)
    const bool have_k = top_k > 0 && top_k < vocab;
    const int64_t k = std::min<int64_t>(have_k ? top_k : TOPK_MAX, vocab);
    const int full_row = !have_k && top_p < 1.f;
    char *ws = static_cast<char *>(workspace(s, (size_t)rows * k * 8));
    if (!ws) return -1;
    float *vals = reinterpret_cast<float *>(ws);
    int32_t *idxs = reinterpret_cast<int32_t *>(ws + (size_t)rows * k * 4);
    if (atoma_topk_rows(logits, rows, vocab, row_stride, dtype, k, vals, idxs, stream) != 0) return -1;
#define ATOMA_ST(TT) hipLaunchKernelGGL((sample_topk_kernel<TT>), dim3((unsigned)rows), dim3(256), 0, s, logits, stride_bytes, (int)vocab, vals, idxs, (int)k, inv_temp, top_p, u, out_idx, out_logit, full_row)
    if (dtype == ATOMA_F32) ATOMA_ST(float); else if (dtype == ATOMA_BF16) ATOMA_ST(bf16_t); else ATOMA_ST(f16_t);
#undef ATOMA_ST
    return ATOMA_CHECK_LAUNCH("sample_rows (top-k / top-p)") ? 0 : -1;
}

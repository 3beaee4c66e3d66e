// Per-request sampling of a whole step in one call: atoma_sample_batch (include/atoma_hip.h).
//
// The reference samples per sequence group (backends/vllm/src/model_executor.rs:173-278): its own LogitsProcessor (ArgMax / All /
// TopK / TopP / TopKThenTopP, temperature, k, p: llm_service.rs:346-372), its own repetition penalty over the tail of its
// token ids (:211-225), the log-prob read from the penalised row (:249) and the EOS test (:237-241).  Here every one of these
// settings is a device-side value of the row, so one captured graph serves any mix of them:
//   kernel 1 (one workgroup of 1024 per row): marks the row's history window in an LDS bitmap (one bit per vocabulary entry, dynamic LDS),
//     then takes the row's branch -- greedy: the argmax pass; All: the two-pass multinomial draw; restricted: the top-k list of
//     the row into the stream's workspace.  The penalty is applied in registers to the marked elements while the row streams
//     by (sampling_rows.h: WindowPenalty); the logits are never written and never read once more than without a penalty.
//   kernel 2 (one workgroup of 256 per row; exits at once for the rows kernel 1 finished): the top-k / top-p draw from the list.
// Whichever kernel chooses the token also writes the stop flag and appends to the history.  Two launches whatever the batch
// holds; no host synchronisation, no state outside the arguments and the stream's workspace.
#include "common.h"
#include "sampling_rows.h"
#include "../../include/atoma_hip.h"

namespace atoma {

void *workspace(hipStream_t stream, size_t bytes);   // runtime.hip

static_assert(sizeof(atoma_sampling_params) == 32, "atoma_sampling_params is 32 bytes without padding");

constexpr int SB_MAX_PENALTY_VOCAB = 262144;                 // one bit per entry: at most 32 KB of LDS
// the bitmap is dynamic LDS, sized by the launcher: vocab / 8 bytes when a history is given, nothing otherwise
extern __shared__ uint32_t sb_bits[];
constexpr int SB_MAX_EOS = 16;

// what a row asks for, decided the same way by both kernels
struct RowPlan {
    bool valid, greedy, restricted, pen_on, full_row;
    int k;                 // length of the row's top-k list (restricted rows)
    float inv_temp, top_p, penalty;
    int win_start, win_len, len_raw;
};

__device__ __forceinline__ bool is_nan_bits(float v) { return (__float_as_uint(v) & 0x7fffffffu) > 0x7f800000u; }

__device__ __forceinline__ RowPlan make_plan(const atoma_sampling_params &q, int vocab, const int32_t *history_len, int64_t history_stride, int r) {
    RowPlan p;
    p.greedy = q.mode == 0;
    p.pen_on = history_len != nullptr && __float_as_uint(q.repetition_penalty) != 0x3f800000u;
    bool ok = q.mode == 0 || q.mode == 1;
    if (q.mode == 1) {
        // comparisons with a NaN operand are not trusted (-fno-honor-nans): NaNs are rejected from the bits first
        if (is_nan_bits(q.temperature) || !(q.temperature > 0.f)) ok = false;
        if (q.top_k < 0 || q.top_k > TOPK_MAX) ok = false;
        if (is_nan_bits(q.top_p) || !(q.top_p > 0.f) || q.top_p > 1.f) ok = false;
    }
    if (p.pen_on && q.repeat_last_n <= 0) ok = false;
    if (q.reserved[0] != 0 || q.reserved[1] != 0) ok = false;   // kept free for later settings
    p.valid = ok;
    const bool have_k = q.top_k > 0 && q.top_k < vocab;
    p.restricted = !p.greedy && (have_k || q.top_p < 1.f);
    p.k = min(have_k ? q.top_k : TOPK_MAX, vocab);
    p.full_row = !have_k && q.top_p < 1.f;
    p.inv_temp = 1.f / q.temperature;
    p.top_p = q.top_p;
    p.penalty = q.repetition_penalty;
    p.len_raw = history_len ? history_len[r] : 0;
    const int len = (int)min((int64_t)max(p.len_raw, 0), history_stride);
    p.win_len = p.pen_on ? min(len, max(q.repeat_last_n, 0)) : 0;
    p.win_start = len - p.win_len;
    return p;
}

// one bit per vocabulary entry that occurs in the window; ids outside [0, vocab) are ignored.  Whole workgroup.
__device__ __forceinline__ void mark_window(uint32_t *bits, int vocab, const int32_t *hist_row, const RowPlan &p) {
    const int words = (vocab + 31) >> 5;
    for (int i = threadIdx.x; i < words; i += blockDim.x) bits[i] = 0u;
    __syncthreads();
    for (int i = threadIdx.x; i < p.win_len; i += blockDim.x) {
        const int t = hist_row[p.win_start + i];
        if (t >= 0 && t < vocab) atomicOr(&bits[t >> 5], 1u << (t & 31));
    }
    __syncthreads();
}

// thread 0, after it wrote out_idx[r]: stop flag and history append
__device__ __forceinline__ void finish_row(int r, int token, const RowPlan &p, int32_t *history, int64_t history_stride, int32_t *history_len, int append,
                                           const int32_t *eos_ids, int num_eos, uint8_t *out_stop) {
    if (out_stop) {
        bool stop = false;
        for (int e = 0; e < num_eos; ++e) stop = stop || eos_ids[e] == token;
        out_stop[r] = stop ? 1 : 0;
    }
    if (append && history && p.len_raw >= 0 && (int64_t)p.len_raw < history_stride) {
        history[(int64_t)r * history_stride + p.len_raw] = token;
        history_len[r] = p.len_raw + 1;
    }
}

union SelectShared {
    ArgmaxShared argmax;
    TopkShared topk;
    SampleFullShared full;
};

template <typename T, bool VEC>
__global__ void __launch_bounds__(1024) sample_batch_select_kernel(const void *__restrict__ logits, int64_t row_stride_bytes, int vocab,
                                                                   const atoma_sampling_params *__restrict__ params, const float *__restrict__ u,
                                                                   int32_t *history, int64_t history_stride, int32_t *history_len, int append, const int32_t *__restrict__ eos_ids,
                                                                   int num_eos, int reg_ok, float *__restrict__ ws_vals, int32_t *__restrict__ ws_idxs, int ws_k,
                                                                   int32_t *__restrict__ out_idx, float *__restrict__ out_logit, uint8_t *__restrict__ out_stop) {
    __shared__ SelectShared sh;
    uint32_t *bits = sb_bits;
    const int r = blockIdx.x;
    const char *row = static_cast<const char *>(logits) + (int64_t)r * row_stride_bytes;
    const atoma_sampling_params q = params[r];
    const RowPlan p = make_plan(q, vocab, history_len, history_stride, r);
    if (!p.valid) {   // workgroup-uniform
        if (threadIdx.x == 0) {
            out_idx[r] = -1;
            if (out_stop) out_stop[r] = 0;
        }
        return;
    }
    if (p.pen_on) mark_window(bits, vocab, history + (int64_t)r * history_stride, p);
    const WindowPenalty pen{bits, p.penalty, p.pen_on};
    float *ov = out_logit ? out_logit + r : nullptr;
    if (p.greedy) {
        argmax_row<T, VEC>(sh.argmax, row, vocab, pen, out_idx + r, ov);
    } else if (!p.restricted) {
        sample_full_row<T>(sh.full, row, vocab, p.inv_temp, u[r], pen, out_idx + r, ov);
    } else {
        // the list for kernel 2; a penalised f16 row takes the histogram route: its penalised values are f32
        // and no longer share the f16 patterns' 16-bit order, which is what the register route packs (sampling_rows.h)
        float *lv = ws_vals + (int64_t)r * ws_k;
        int32_t *li = ws_idxs + (int64_t)r * ws_k;
        const bool reg = reg_ok && p.k <= TOPK_REG_MAX_K && !(std::is_same<T, f16_t>::value && p.pen_on);
        if constexpr (VEC) {
            if (reg) { topk_row_reg<T>(sh.topk, row, vocab, p.k, pen, lv, li); return; }
        }
        topk_row_hist<T>(sh.topk, row, vocab, p.k, pen, lv, li);
        return;
    }
    if (threadIdx.x == 0) finish_row(r, out_idx[r], p, history, history_stride, history_len, append, eos_ids, num_eos, out_stop);
}

template <typename T>
__global__ void __launch_bounds__(256) sample_batch_draw_kernel(const void *__restrict__ logits, int64_t row_stride_bytes, int vocab,
                                                                const atoma_sampling_params *__restrict__ params, const float *__restrict__ u,
                                                                int32_t *history, int64_t history_stride, int32_t *history_len, int append, const int32_t *__restrict__ eos_ids,
                                                                int num_eos, const float *__restrict__ ws_vals, const int32_t *__restrict__ ws_idxs, int ws_k,
                                                                int32_t *__restrict__ out_idx, float *__restrict__ out_logit, uint8_t *__restrict__ out_stop) {
    __shared__ SampleTopkShared sh;
    uint32_t *bits = sb_bits;
    const int r = blockIdx.x;
    const atoma_sampling_params q = params[r];
    const RowPlan p = make_plan(q, vocab, history_len, history_stride, r);
    if (!p.valid || !p.restricted) return;   // kernel 1 finished this row
    const char *row = static_cast<const char *>(logits) + (int64_t)r * row_stride_bytes;
    if (p.pen_on) mark_window(bits, vocab, history + (int64_t)r * history_stride, p);   // the window again; the row's list is already penalised
    const WindowPenalty pen{bits, p.penalty, p.pen_on};
    sample_topk_row<T>(sh, row, vocab, ws_vals + (int64_t)r * ws_k, ws_idxs + (int64_t)r * ws_k, p.k, p.inv_temp, p.top_p, u[r], p.full_row ? 1 : 0, pen,
                       out_idx + r, out_logit ? out_logit + r : nullptr);
    if (threadIdx.x == 0) finish_row(r, out_idx[r], p, history, history_stride, history_len, append, eos_ids, num_eos, out_stop);
}

}  // namespace atoma

extern "C" int atoma_sample_batch(const void *logits, int64_t rows, int64_t vocab, int64_t row_stride, int dtype, const atoma_sampling_params *params,
                                  const float *u, int32_t *history, int64_t history_stride, int32_t *history_len, int append, const int32_t *eos_ids,
                                  int64_t num_eos, int32_t *out_idx, float *out_logit, uint8_t *out_stop, void *stream) {
    using namespace atoma;
    clear_error();
    if (dtype != ATOMA_F16 && dtype != ATOMA_BF16 && dtype != ATOMA_F32) { set_error("sample_batch: dtype must be f16, bf16 or f32"); return -1; }
    if (rows < 0 || vocab <= 0 || vocab > (int64_t)SAMPLE_CHUNK * SAMPLE_MAX_CHUNKS) { set_error("sample_batch: invalid shape"); return -1; }
    if (row_stride < vocab) { set_error("sample_batch: row_stride must be >= vocab"); return -1; }
    if (!logits || !params || !u || !out_idx) { set_error("sample_batch: logits, params, u and out_idx are required"); return -1; }
    if ((history == nullptr) != (history_len == nullptr)) { set_error("sample_batch: history and history_len come together"); return -1; }
    if (history && (history_stride <= 0 || history_stride > 0x7fffffff)) { set_error("sample_batch: history_stride must be positive"); return -1; }
    if (history && vocab > SB_MAX_PENALTY_VOCAB) { set_error("sample_batch: a history (repetition penalty) needs vocab <= 262144"); return -1; }
    if (append != 0 && append != 1) { set_error("sample_batch: append must be 0 or 1"); return -1; }
    if (num_eos < 0 || num_eos > SB_MAX_EOS) { set_error("sample_batch: num_eos must be in [0, 16]"); return -1; }
    if (num_eos > 0 && !eos_ids) { set_error("sample_batch: eos_ids is required when num_eos > 0"); return -1; }
    if (rows == 0) return 0;
    const auto s = static_cast<hipStream_t>(stream);
    const int elt = dtype == ATOMA_F32 ? 4 : 2;
    const int64_t stride_bytes = row_stride * elt;
    const int ws_k = (int)std::min<int64_t>(TOPK_MAX, vocab);
    char *ws = static_cast<char *>(workspace(s, (size_t)rows * ws_k * 8));   // the top-k lists of the restricted rows
    if (!ws) return -1;
    float *ws_vals = reinterpret_cast<float *>(ws);
    int32_t *ws_idxs = reinterpret_cast<int32_t *>(ws + (size_t)rows * ws_k * 4);
    const bool vec = (reinterpret_cast<uintptr_t>(logits) & 15u) == 0 && stride_bytes % 16 == 0;
    const int epv = dtype == ATOMA_F32 ? 4 : 8;
    const int reg_ok = vec && vocab <= TOPK_REG_MAX_VOCAB && vocab % epv == 0 && vocab >= 4 * TOPK_THREADS;
    const dim3 grid((unsigned)rows);
    const unsigned bitmap_bytes = history ? (unsigned)((vocab + 31) / 32) * 4u : 0u;
#define ATOMA_SB_SELECT(TT, VV)                                                                                                                     \
    hipLaunchKernelGGL((sample_batch_select_kernel<TT, VV>), grid, dim3(1024), bitmap_bytes, s, logits, stride_bytes, (int)vocab, params, u, history, history_stride, \
                       history_len, append, eos_ids, (int)num_eos, reg_ok, ws_vals, ws_idxs, ws_k, out_idx, out_logit, out_stop)
#define ATOMA_SB(TT)                                                                                                                                \
    do {                                                                                                                                            \
        if (vec) ATOMA_SB_SELECT(TT, true); else ATOMA_SB_SELECT(TT, false);                                                                        \
        hipLaunchKernelGGL((sample_batch_draw_kernel<TT>), grid, dim3(256), bitmap_bytes, s, logits, stride_bytes, (int)vocab, params, u, history, history_stride, \
                           history_len, append, eos_ids, (int)num_eos, ws_vals, ws_idxs, ws_k, out_idx, out_logit, out_stop);                       \
    } while (0)
    if (dtype == ATOMA_F32) ATOMA_SB(float);
    else if (dtype == ATOMA_BF16) ATOMA_SB(bf16_t);
    else ATOMA_SB(f16_t);
#undef ATOMA_SB
#undef ATOMA_SB_SELECT
    return ATOMA_CHECK_LAUNCH("sample_batch") ? 0 : -1;
}

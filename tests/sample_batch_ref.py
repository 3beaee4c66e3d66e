"""numpy restatement of atoma_sample_batch's per-row semantics (TEST INFRASTRUCTURE, like tests/fp8w_ref.py).

The reference: backends/vllm/src/model_executor.rs:211-225 calls candle's apply_repeat_penalty(logits, penalty, tail of the
sequence's token ids) before LogitsProcessor::sample, reads the log-prob from the penalised row (:249) and compares the token
with the EOS ids (:237-241).  The draw itself is oracle/sampling_oracle.py on the penalised row."""
import numpy as np

from oracle import sampling_oracle as SO

GREEDY, STOCHASTIC = 0, 1


def penalised(x32, history, history_len, penalty, repeat_last_n):
    """x32: one f32 row.  Every DISTINCT token t of the last min(history_len, repeat_last_n) history entries with 0 <= t < vocab:
    x_t = x_t / penalty if x_t >= 0 else x_t * penalty -- one correctly rounded f32 operation, once per token.  penalty == 1 (or
    no history) returns the row bit for bit.  NaN stays NaN (NaN >= 0 is false: NaN * penalty), -inf stays -inf."""
    x = np.array(x32, np.float32, copy=True)
    p = np.float32(penalty)
    if history is None or p == np.float32(1.0):
        return x
    n = min(int(history_len), int(repeat_last_n))
    window = np.asarray(history[:history_len], np.int64)[history_len - n:] if n > 0 else np.zeros(0, np.int64)
    toks = np.unique(window)
    toks = toks[(toks >= 0) & (toks < x.size)]
    with np.errstate(all="ignore"):
        v = x[toks]
        x[toks] = np.where(v >= 0, v / p, v * p).astype(np.float32)
    return x


def valid(prm):
    """prm: dict with mode, temperature, top_k, top_p, repetition_penalty, repeat_last_n (+ 'has_history')."""
    if prm["mode"] not in (GREEDY, STOCHASTIC) or any(prm.get("reserved", (0, 0))):
        return False
    if prm["mode"] == STOCHASTIC:
        if not (prm["temperature"] > 0) or not (0 <= prm["top_k"] <= 1024) or not (0 < prm["top_p"] <= 1):
            return False
    if prm.get("has_history", True) and np.float32(prm["repetition_penalty"]) != np.float32(1.0) and prm["repeat_last_n"] <= 0:
        return False
    return True


def argmax(x):
    """atoma_argmax_rows' rule: smallest index among the maxima, NaN never chosen (all -inf / NaN: index 0)."""
    return int(np.where(np.isnan(x), -np.inf, x).argmax())


def greedy_row(x32, history, history_len, prm):
    x = penalised(x32, history, history_len, prm["repetition_penalty"], prm["repeat_last_n"])
    t = argmax(x)
    return t, x[t], x


def bracket_row(x32, token, history, history_len, prm):
    """(lo, hi, x): u in [lo, hi) draws `token` from the penalised row x."""
    x = penalised(x32, history, history_len, prm["repetition_penalty"], prm["repeat_last_n"])
    lo, hi = SO.bracket(x, int(token), prm["temperature"], prm["top_k"], prm["top_p"])
    return lo, hi, x


def params_array(dtype, rows_of_params):
    """list of dicts -> structured array in the layout of atoma_sampling_params"""
    a = np.zeros(len(rows_of_params), dtype)
    for i, prm in enumerate(rows_of_params):
        for k in ("mode", "temperature", "top_k", "top_p", "repetition_penalty", "repeat_last_n"):
            a[k][i] = prm[k]
        a["reserved"][i] = prm.get("reserved", (0, 0))
    return a


def P(mode=GREEDY, temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0, repeat_last_n=64):
    return dict(mode=mode, temperature=temperature, top_k=top_k, top_p=top_p, repetition_penalty=repetition_penalty, repeat_last_n=repeat_last_n)


def hand_rows():
    """Hand-worked penalty rows: (name, x [8] f32, history, penalty, repeat_last_n, expected penalised row, expected argmax).
    Every expected value is written out, not computed by `penalised`.  Each row is built so that the penalty decides the argmax."""
    f = np.float32
    inf, nan = np.inf, np.nan
    rows = []
    # positive / negative / zero logits, a token seen three times is penalised once, ids -1 and vocab (8) are ignored
    rows.append(("signs_dups_range", [4.0, -2.0, 0.0, 3.0, 1.0, -1.0, 0.5, 2.5], [0, 0, 0, 1, 2, -1, 8], 2.0, 64,
                 [2.0, -4.0, 0.0, 3.0, 1.0, -1.0, 0.5, 2.5], 3))                      # the maximum (4.0 -> 2.0) falls below the runner-up 3.0
    # a token one position outside the tail is not penalised: the window is the last 3 of [5, 0, 1, 2]
    rows.append(("tail_only", [1.0, 6.0, 2.0, 0.0, 0.0, 8.0, 0.0, 0.0], [5, 0, 1, 2], 2.0, 3,
                 [0.5, 3.0, 1.0, 0.0, 0.0, 8.0, 0.0, 0.0], 5))                        # token 5 keeps 8.0
    # penalty < 1 on a negative row RAISES the seen token to the top: -4 * 0.25 = -1
    rows.append(("below_one_negative", [-2.0, -3.0, -4.0, -2.5, -6.0, -7.0, -8.0, -9.0], [2], 0.25, 1,
                 [-2.0, -3.0, -1.0, -2.5, -6.0, -7.0, -8.0, -9.0], 2))
    # penalty < 1 on a positive logit divides: 1.5 / 0.5 = 3
    rows.append(("below_one_positive", [2.0, 1.5, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0], [1, 3], 0.5, 8,
                 [2.0, 3.0, 0.0, -0.5, 0.0, 0.0, 0.0, 0.0], 1))
    # one correctly rounded division: 1 / 1.1 in f32, written as the two f32 operands' quotient rounded once
    rows.append(("rounded_division", [1.0, 0.9, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], [0], 1.1, 4,
                 [float(f(f(1.0) / f(1.1))), 0.9, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], 0))  # 0.90909094 > f32(0.9): still the maximum
    # -inf and NaN inside the window stay what they are; the finite maximum is penalised below token 4
    rows.append(("inf_nan", [-inf, nan, 5.0, -inf, 3.0, 1.0, nan, 0.0], [0, 1, 2], 2.0, 16,
                 [-inf, nan, 2.5, -inf, 3.0, 1.0, nan, 0.0], 4))
    # penalty 1: the identity on the bits (history present)
    rows.append(("identity", [0.1, -0.0, 7.0, -3.3, 0.0, 1e-40, -1e-40, 2.0], [1, 2, 5, 6], 1.0, 64,
                 [0.1, -0.0, 7.0, -3.3, 0.0, 1e-40, -1e-40, 2.0], 2))
    return [(n, np.array(x, f), np.array(h, np.int32), p, k, np.array(e, f), a) for n, x, h, p, k, e, a in rows]

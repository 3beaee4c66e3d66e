"""The numpy restatement of atoma_sample_batch's penalty (tests/sample_batch_ref.py) against hand-worked rows, and the layout of
the binding's parameter struct against the header."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_rust_ffi as G  # noqa: E402
import sample_batch_ref as R  # noqa: E402


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_penalty_against_hand_worked_rows():
    rows = R.hand_rows()
    assert {n for n, *_ in rows} >= {"signs_dups_range", "tail_only", "below_one_negative", "below_one_positive", "inf_nan", "identity"}
    for name, x, hist, penalty, last_n, expect, amax in rows:
        before = bits(x).copy()
        got = R.penalised(x, hist, len(hist), penalty, last_n)
        assert np.array_equal(bits(got), bits(expect)), (name, got, expect)
        assert R.argmax(got) == amax, name
        assert np.array_equal(bits(x), before), "the input row is not modified"


def test_penalty_details():
    x = np.array([4.0, -2.0, 0.0, 3.0], np.float32)
    # a token seen three times is penalised once
    assert R.penalised(x, np.array([0, 0, 0], np.int32), 3, 2.0, 8)[0] == 2.0
    # ids -1 and vocab are ignored
    assert np.array_equal(R.penalised(x, np.array([-1, 4], np.int32), 2, 2.0, 8), x)
    # one position outside the repeat_last_n tail
    assert np.array_equal(R.penalised(x, np.array([0, 1, 3], np.int32), 3, 2.0, 2), np.array([4.0, -4.0, 0.0, 1.5], np.float32))
    # history_len limits the window, not the buffer's length
    assert np.array_equal(R.penalised(x, np.array([1, 0, 0], np.int32), 1, 2.0, 8), np.array([4.0, -4.0, 0.0, 3.0], np.float32))
    # zero logit: 0 / p = 0
    assert R.penalised(x, np.array([2], np.int32), 1, 1.7, 8)[2] == 0.0
    # penalty < 1
    assert np.array_equal(R.penalised(x, np.array([0, 1], np.int32), 2, 0.5, 8), np.array([8.0, -1.0, 0.0, 3.0], np.float32))
    # penalty 1 is the identity on the bits, NaN payloads and signed zeros included
    odd = np.array([0x7fc01234, 0x80000000, 0xff800000, 0x00000001], np.uint32).view(np.float32)
    assert np.array_equal(bits(R.penalised(odd, np.array([0, 1, 2, 3], np.int32), 4, 1.0, 8)), bits(odd))
    # no history: the identity whatever the penalty
    assert np.array_equal(R.penalised(x, None, 0, 1.3, 8), x)


def test_valid_rows():
    ok = R.P(R.STOCHASTIC, 0.7, 50, 0.9, 1.1, 64)
    assert R.valid(ok) and R.valid(R.P())
    for bad in (dict(mode=2), dict(mode=-1), dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("nan")), dict(top_k=-1),
                dict(top_k=1025), dict(top_p=0.0), dict(top_p=1.5), dict(repeat_last_n=0), dict(reserved=(0, 1)), dict(reserved=(7, 0))):
        assert not R.valid({**ok, **bad}), bad
    assert R.valid({**ok, "repetition_penalty": 1.0, "repeat_last_n": 0})          # penalty off: repeat_last_n is not looked at
    assert R.valid(R.P(R.GREEDY, temperature=0.0, top_k=5000, top_p=0.0))           # greedy rows ignore the stochastic fields


def test_binding_struct_matches_the_header():
    sys.path.insert(0, os.path.join(ROOT, "atoma-infer_amd", "bindings"))
    import atoma_hip as ah
    assert hasattr(ah.lib, "atoma_sample_batch"), "the library does not export atoma_sample_batch"
    S = ah.SamplingParams
    assert C.sizeof(S) == 32
    _, structs, funcs = G.parse(open(G.HEADER).read())
    size = {"int32_t": 4, "float": 4}
    off, want = 0, []
    for ctype, name, n in structs["atoma_sampling_params"]:
        want.append((name, off, size[ctype.strip()] * (n or 1)))
        off += size[ctype.strip()] * (n or 1)
    assert off == 32
    assert [(n, getattr(S, n).offset, getattr(S, n).size) for n, _ in S._fields_] == want
    assert [(n, ah.SAMPLING_PARAMS_DTYPE.fields[n][1], ah.SAMPLING_PARAMS_DTYPE.fields[n][0].itemsize) for n, _ in S._fields_] == want
    assert ah.SAMPLING_PARAMS_DTYPE.itemsize == 32
    proto = [p for _, n, p in funcs if n == "atoma_sample_batch"]
    assert len(proto) == 1 and len(proto[0]) == len(ah.lib.atoma_sample_batch.argtypes) == 17

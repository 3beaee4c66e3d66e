"""atoma_sample_batch through the C ABI against its numpy restatement (tests/sample_batch_ref.py on oracle/sampling_oracle.py):
per-row modes, repetition penalty, stop flags, history append, invalid rows, strides, graph replay, argument checks."""
import inspect

import numpy as np
import pytest

import sample_batch_ref as R
from oracle.halfs import F16, BF16, to_f32
from test_sampling_gpu import check_draws, gpu_argmax
from util import rand_half

pytestmark = pytest.mark.gpu
F32 = 2
SLACK = inspect.signature(check_draws).parameters["slack"].default       # the slack of the existing draws' check, not re-chosen
POISON32, POISON8 = np.int32(0x5a5a5a5a), np.uint8(0xa5)


def make_logits(rng, shape, dtype, scale):
    if dtype == F32:
        x = (rng.standard_normal(shape) * scale).astype(np.float32)
        return x, x
    x = rand_half(rng, shape, dtype, scale)
    return x, to_f32(x, dtype)


class Call:
    """Device buffers of one atoma_sample_batch call, with guard words behind every output and every history row."""

    def __init__(self, gpu, logits, dtype, prms, u, hist=None, hlen=None, eos=(), vocab=None, stride=None, extra_rows=3, offset_elems=0,
                 want_logit=True, want_stop=True):
        self.gpu, self.dtype = gpu, dtype
        self.rows = len(prms)
        self.vocab = vocab or logits.shape[1]
        self.stride = stride or logits.shape[1]
        self.offset = offset_elems * (4 if dtype == F32 else 2)
        self.dl = gpu.DeviceBuffer.from_numpy(logits)
        self.logits_before = self.dl.numpy(np.uint8, (self.dl.nbytes,))
        self.dp = gpu.DeviceBuffer.from_numpy(R.params_array(gpu.SAMPLING_PARAMS_DTYPE, prms))
        self.du = gpu.DeviceBuffer.from_numpy(np.asarray(u, np.float32))
        n = self.rows + extra_rows
        self.di = gpu.DeviceBuffer.from_numpy(np.full(n, POISON32, np.int32))
        self.dv = gpu.DeviceBuffer.from_numpy(np.full(n, POISON32, np.int32)) if want_logit else None
        self.ds = gpu.DeviceBuffer.from_numpy(np.full(n + 13, POISON8, np.uint8)) if want_stop else None
        self.n_out = n
        self.hist = None
        if hist is not None:
            self.hstride = hist.shape[1]
            padded = np.full((self.rows, self.hstride), POISON32, np.int32)      # history rows are adjacent: row r + 1 guards row r
            padded[:, :] = hist
            self.hist = gpu.DeviceBuffer.from_numpy(np.concatenate([padded.ravel(), np.full(16, POISON32, np.int32)]))
            self.hlen = gpu.DeviceBuffer.from_numpy(np.concatenate([np.asarray(hlen, np.int32), np.full(16, POISON32, np.int32)]))
        self.eos = gpu.DeviceBuffer.from_numpy(np.asarray(list(eos) or [0], np.int32))
        self.num_eos = len(eos)

    def run(self, append=0, stream=None, sync=True):
        g = self.gpu
        rc = g.lib.atoma_sample_batch(self.dl.ptr + self.offset, self.rows, self.vocab, self.stride, self.dtype, self.dp.ptr, self.du.ptr,
                                      self.hist.ptr if self.hist else None, self.hstride if self.hist else 0, self.hlen.ptr if self.hist else None,
                                      append, self.eos.ptr if self.num_eos else None, self.num_eos, self.di.ptr, self.dv.ptr if self.dv else None,
                                      self.ds.ptr if self.ds else None, stream)
        assert rc == 0, g.last_error()
        if sync:
            g.synchronize()
        return self

    def out(self):
        idx = self.di.numpy(np.int32, (self.n_out,))
        assert (idx[self.rows:] == POISON32).all(), "out_idx written past `rows`"
        val = stop = None
        if self.dv:
            val = self.dv.numpy(np.float32, (self.n_out,))
            assert (val[self.rows:].view(np.int32) == POISON32).all(), "out_logit written past `rows`"
            val = val[: self.rows]
        if self.ds:
            stop = self.ds.numpy(np.uint8, (self.n_out + 13,))
            assert (stop[self.rows:] == POISON8).all(), "out_stop written past `rows`"
            stop = stop[: self.rows]
        return idx[: self.rows], val, stop

    def history(self):
        h = self.hist.numpy(np.int32, (self.rows * self.hstride + 16,))
        l = self.hlen.numpy(np.int32, (self.rows + 16,))
        assert (h[self.rows * self.hstride:] == POISON32).all() and (l[self.rows:] == POISON32).all(), "guard words after the history were written"
        return h[: self.rows * self.hstride].reshape(self.rows, self.hstride), l[: self.rows]

    def logits_unchanged(self):
        return np.array_equal(self.dl.numpy(np.uint8, (self.dl.nbytes,)), self.logits_before)


def check_rows(x32, prms, u, hist, hlen, idx, val, report=None):
    """Every valid row against the restatement: greedy rows equal, stochastic rows with u inside the token's interval (+- SLACK);
    out_logit bit-equal to the penalised value."""
    worst, inexact, n_st = 0.0, 0, 0
    for r, prm in enumerate(prms):
        h, n = (hist[r], int(hlen[r])) if hist is not None else (None, 0)
        if not R.valid({**prm, "has_history": hist is not None}):
            assert idx[r] == -1, (r, prm, idx[r])
            continue
        if prm["mode"] == R.GREEDY:
            t, v, _ = R.greedy_row(x32[r], h, n, prm)
            assert idx[r] == t, (r, prm, int(idx[r]), t)
        else:
            assert 0 <= idx[r] < x32.shape[1], (r, int(idx[r]))
            lo, hi, x = R.bracket_row(x32[r], idx[r], h, n, prm)
            worst = max(worst, lo - u[r], u[r] - hi)
            assert lo - SLACK <= u[r] < hi + SLACK, (r, prm, int(idx[r]), float(u[r]), lo, hi)
            n_st += 1
            inexact += not (lo <= u[r] < hi)
            v = x[idx[r]]
        if val is not None:
            assert np.float32(val[r]).view(np.uint32) == np.float32(v).view(np.uint32), (r, prm, val[r], v)
    print(f"sample_batch check: {n_st} stochastic rows, worst distance outside the interval {worst:.3e} (slack {SLACK}), {inexact} at an edge")
    assert inexact <= max(1, n_st // 25)       # as check_draws: a draw within rounding distance of an edge may fall on either side
    return worst


def mixed_params(rows, with_penalty=True):
    modes = [dict(mode=R.GREEDY), dict(mode=1), dict(mode=1, top_k=1), dict(mode=1, top_k=50), dict(mode=1, top_k=1024), dict(mode=1, top_p=0.5),
             dict(mode=1, top_p=0.9), dict(mode=1, top_k=50, top_p=0.9)]
    prms = []
    for r in range(rows):
        pen = [0.8, 1.1, 1.3, 2.0][(r // 32) % 4] if with_penalty and (r // 8) % 2 else 1.0      # half of the rows, every mode both ways
        prms.append(R.P(**{**dict(temperature=[0.7, 1.0, 2.0][(r // 16) % 3], repetition_penalty=pen, repeat_last_n=[64, 512, 4096][r % 3]), **modes[r % 8]}))
    return prms


def mixed_history(rng, x32, stride=2056):
    """1..2048 tokens per row, drawn with repetition from the row's 48 largest logits and random ids (so the penalty moves the top)."""
    rows, vocab = x32.shape
    hist = np.zeros((rows, stride), np.int32)
    hlen = np.zeros(rows, np.int32)
    for r in range(rows):
        n = 1 + (r * 37) % 2048 if r else 2048
        top = np.argsort(-x32[r])[:48]
        pool = np.concatenate([top, rng.integers(0, vocab, 200)])
        hist[r, :n] = rng.choice(pool, n)
        hlen[r] = n
    return hist, hlen


@pytest.mark.parametrize("dtype", [BF16, F16, F32])
def test_mixed_batch_at_full_size(gpu, dtype):
    rows, vocab = 256, 128256
    rng = np.random.default_rng(100 + dtype)
    logits, x32 = make_logits(rng, (rows, vocab), dtype, 4.0)
    prms = mixed_params(rows)
    hist, hlen = mixed_history(rng, x32)
    u = rng.random(rows).astype(np.float32)
    u[1], u[9] = 0.0, np.float32(1.0 - 2.0 ** -24)
    c = Call(gpu, logits, dtype, prms, u, hist, hlen).run()
    idx, val, _ = c.out()
    assert c.logits_unchanged()
    check_rows(x32, prms, u, hist, hlen, idx, val)
    for r in [r for r in range(rows) if prms[r]["mode"] == R.GREEDY and prms[r]["repetition_penalty"] == 1.0]:
        ai, av = gpu_argmax(gpu, logits[r:r + 1], dtype)
        assert idx[r] == ai[0] and val[r].view(np.uint32) == av[0].view(np.uint32)
    pen_greedy = [r for r in range(rows) if prms[r]["mode"] == R.GREEDY and prms[r]["repetition_penalty"] != 1.0]
    assert any(idx[r] != x32[r].argmax() for r in pen_greedy), "the histories must move some greedy row's argmax"


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
def test_penalty_semantics_on_the_device(gpu, dtype):
    hand = R.hand_rows()
    if dtype != F32:                       # the hand-worked values are exact in bf16 / f16 except these
        hand = [h for h in hand if h[0] not in ("rounded_division", "identity")]
    x32 = np.stack([h[1] for h in hand])
    if dtype == F32:
        logits = x32
    else:
        from oracle.halfs import from_f32
        logits = from_f32(x32, dtype)
        assert np.array_equal(to_f32(logits, dtype), x32, equal_nan=True)
    stride = 8
    hist = np.zeros((len(hand), stride), np.int32)
    hlen = np.zeros(len(hand), np.int32)
    for r, h in enumerate(hand):
        hist[r, : len(h[2])] = h[2]
        hlen[r] = len(h[2])
    prms = [R.P(R.GREEDY, repetition_penalty=h[3], repeat_last_n=h[4]) for h in hand]
    c = Call(gpu, logits, dtype, prms, np.zeros(len(hand), np.float32), hist, hlen).run()
    idx, val, _ = c.out()
    assert c.logits_unchanged(), "the logits buffer is modified"
    for r, h in enumerate(hand):
        assert idx[r] == h[6], (h[0], int(idx[r]), h[6])
        assert val[r].view(np.uint32) == h[5][h[6]].view(np.uint32), (h[0], val[r], h[5][h[6]])
    # the same rows as one-token-restricted stochastic rows (top_k = 1 draws the maximum of the penalised row)
    prms = [R.P(R.STOCHASTIC, 1.0, 1, 1.0, h[3], h[4]) for h in hand]
    idx2, val2, _ = Call(gpu, logits, dtype, prms, np.full(len(hand), 0.5, np.float32), hist, hlen).run().out()
    assert np.array_equal(idx2, idx) and np.array_equal(val2.view(np.uint32), val.view(np.uint32))


@pytest.mark.parametrize("dtype", [BF16, F32, F16])
@pytest.mark.parametrize("vocab", [128256, 1000])
def test_top_k_on_the_penalised_row(gpu, dtype, vocab):
    """Token `t` is the 3rd largest logit; the penalty pushes it below the 5 largest others, so top_k = 5 never draws it."""
    n = 64
    rng = np.random.default_rng(vocab)
    base = (rng.standard_normal(vocab) * 0.5).astype(np.float32)
    base = np.clip(base, -3, 3)
    top = rng.choice(vocab, 8, replace=False)
    base[top] = [9.0, 8.5, 8.0, 7.5, 7.0, 6.5, 6.0, 5.5]
    t = int(top[2])
    x32 = np.tile(base, (n, 1))
    if dtype == F32:
        logits = x32
    else:
        from oracle.halfs import from_f32
        logits = from_f32(x32, dtype)
        x32 = to_f32(logits, dtype)
    hist = np.full((n, 4), t, np.int32)
    hlen = np.full(n, 3, np.int32)
    prms = [R.P(R.STOCHASTIC, 2.0, 5, 1.0, 2.0, 8) for _ in range(n)]
    u = ((np.arange(n) + 0.5) / n).astype(np.float32)
    idx, val, _ = Call(gpu, logits, dtype, prms, u, hist, hlen).run().out()
    assert t in np.argsort(-x32[0])[:5]
    assert not (idx == t).any()
    assert set(idx.tolist()) <= {int(top[i]) for i in (0, 1, 3, 4, 5)} and int(top[5]) in idx.tolist()
    check_rows(x32, prms, u, hist, hlen, idx, val)
    # without the penalty the token is drawn
    prms0 = [R.P(R.STOCHASTIC, 2.0, 5, 1.0, 1.0, 8) for _ in range(n)]
    idx0, _, _ = Call(gpu, logits, dtype, prms0, u, hist, hlen).run().out()
    assert (idx0 == t).any()


def test_distribution_with_penalty(gpu):
    rng = np.random.default_rng(78)
    vocab, stride, n = 1000, 1024, 4096
    row = (rng.standard_normal(vocab) * 2).astype(np.float32)
    row[[3, 500]] = -np.inf
    row[7] = np.nan
    x = np.full((n, stride), 50.0, np.float32)
    x[:, :vocab] = row
    h = np.concatenate([np.argsort(-np.nan_to_num(row, nan=-np.inf))[:20], [3, 7, 999, 999]]).astype(np.int32)
    hist = np.tile(h, (n, 1))
    hlen = np.full(n, len(h), np.int32)
    prm = R.P(R.STOCHASTIC, 1.0, 0, 1.0, 1.3, 64)
    u = ((np.arange(n) + 0.5) / n).astype(np.float32)
    idx, _, _ = Call(gpu, x, F32, [prm] * n, u, hist, hlen, vocab=vocab, stride=stride).run().out()
    assert (idx < vocab).all() and (idx >= 0).all() and not np.isin(idx, [3, 500, 7]).any()
    xp = R.penalised(row, h, len(h), 1.3, 64)
    _, w = R.SO.kept_weights(xp, 1.0)
    p = w / w.sum()
    freq = np.bincount(idx, minlength=vocab) / n
    assert np.abs(freq - p).max() < 2.0 / n + 1e-6            # the bound of test_sample_rows_distribution_and_degenerate_rows
    _, w0 = R.SO.kept_weights(row, 1.0)
    assert np.abs(freq - w0 / w0.sum()).max() > 10.0 / n      # ... which the unpenalised distribution does not meet


@pytest.mark.parametrize("num_eos", [0, 1, 16])
def test_stop_flags(gpu, num_eos):
    rng = np.random.default_rng(num_eos)
    rows, vocab = 40, 5000
    logits, x32 = make_logits(rng, (rows, vocab), BF16, 3.0)
    prms = mixed_params(rows, with_penalty=False)
    u = rng.random(rows).astype(np.float32)
    base, _, _ = Call(gpu, logits, BF16, prms, u, want_logit=False, want_stop=False).run().out()     # NULL out_logit / out_stop are accepted
    assert (base >= 0).all()
    eos = list(dict.fromkeys(base[::3].tolist()))[:num_eos]
    eos += [vocab + 5 + i for i in range(num_eos - len(eos))]
    idx, val, stop = Call(gpu, logits, BF16, prms, u, eos=eos).run().out()
    assert np.array_equal(idx, base)
    assert np.array_equal(stop, np.isin(idx, eos).astype(np.uint8)) if num_eos else not stop.any()
    if num_eos:
        assert stop.any() and not stop.all()
    idx2, _, stop2 = Call(gpu, logits, BF16, prms, u, eos=eos, want_logit=False).run().out()
    assert np.array_equal(idx2, base) and np.array_equal(stop2, stop)


def test_history_append(gpu):
    rng = np.random.default_rng(6)
    rows, vocab, stride = 24, 3000, 12
    logits, x32 = make_logits(rng, (rows, vocab), F32, 3.0)
    prms = mixed_params(rows)
    for p in prms:
        p["repeat_last_n"] = 5
    hist = rng.integers(0, vocab, (rows, stride)).astype(np.int32)
    hlen = (np.arange(rows) % (stride + 1)).astype(np.int32)
    hlen[[0, 8, 11, 12]] = stride                                     # full rows: greedy, penalised, restricted
    u = rng.random(rows).astype(np.float32)
    c = Call(gpu, logits, F32, prms, u, hist, hlen).run(append=0)
    idx0, val0, _ = c.out()
    h0, l0 = c.history()
    assert np.array_equal(h0, hist) and np.array_equal(l0, hlen), "append = 0 must not touch the history"
    check_rows(x32, prms, u, hist, hlen, idx0, val0)
    c = Call(gpu, logits, F32, prms, u, hist, hlen).run(append=1)
    idx, val, _ = c.out()
    assert np.array_equal(idx, idx0)                                  # the window is read before the append
    h1, l1 = c.history()
    want_h, want_l = hist.copy(), hlen.copy()
    for r in range(rows):
        if hlen[r] < stride:
            want_h[r, hlen[r]] = idx[r]
            want_l[r] += 1
    assert np.array_equal(h1, want_h) and np.array_equal(l1, want_l)
    assert (l1 <= stride).all()


def test_invalid_rows(gpu):
    rng = np.random.default_rng(7)
    vocab, stride = 4000, 16
    good = mixed_params(8)
    bad = [dict(mode=2), dict(mode=-1), dict(mode=1, temperature=0.0), dict(mode=1, temperature=-1.0), dict(mode=1, temperature=float("nan")),
           dict(mode=1, top_k=-1), dict(mode=1, top_k=1025), dict(mode=1, top_p=0.0), dict(mode=1, top_p=1.25), dict(mode=1, top_p=float("nan")),
           dict(mode=0, repetition_penalty=1.2, repeat_last_n=0), dict(mode=1, repetition_penalty=1.2, repeat_last_n=-3),
           dict(mode=0, reserved=(1, 0)), dict(mode=1, reserved=(0, -1))]
    prms = []
    for i, b in enumerate(bad):
        prms += [good[i % 8], {**R.P(temperature=1.0), **b}]
    prms.append(good[3])
    rows = len(prms)
    logits, x32 = make_logits(rng, (rows, vocab), BF16, 3.0)
    hist = rng.integers(0, vocab, (rows, stride)).astype(np.int32)
    hlen = np.full(rows, 7, np.int32)
    u = rng.random(rows).astype(np.float32)
    c = Call(gpu, logits, BF16, prms, u, hist, hlen, eos=list(range(16))).run(append=1)
    idx, val, stop = c.out()
    h1, l1 = c.history()
    for r in range(1, rows, 2):
        assert not R.valid(prms[r])
        assert idx[r] == -1 and stop[r] == 0 and l1[r] == 7 and np.array_equal(h1[r], hist[r]), (r, prms[r])
    assert (idx[0::2] >= 0).all() and (l1[0::2] == 8).all()
    check_rows(x32, prms, u, hist, hlen, idx, None)


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_strides_guards_and_the_scalar_path(gpu, dtype):
    rng = np.random.default_rng(8)
    big = np.float32(3.3895314e38 if dtype == BF16 else np.finfo(np.float32).max)
    # row_stride > vocab, padding = the largest finite value and NaN; vocab not a multiple of 8; then an unaligned row start
    for rows, vocab, stride, offset in [(16, 5003, 5120, 0), (16, 5003, 5011, 1), (16, 40000, 40008, 0)]:
        body, x32 = make_logits(rng, (rows, vocab), dtype, 3.0)
        n_el = offset + rows * stride
        flat = np.empty(n_el, body.dtype)
        pad32 = np.where(np.arange(n_el) % 2 == 0, big, np.float32(np.nan)).astype(np.float32)
        if dtype == F32:
            flat[:] = pad32
        else:
            from oracle.halfs import from_f32
            flat[:] = from_f32(pad32, dtype)
        view = flat[offset:].reshape(rows, stride)
        view[:, :vocab] = body
        prms = mixed_params(rows)
        hist = np.stack([np.argsort(-x32[r])[:10] for r in range(rows)]).astype(np.int32)
        hlen = np.full(rows, 10, np.int32)
        u = rng.random(rows).astype(np.float32)
        c = Call(gpu, flat, dtype, prms, u, hist, hlen, vocab=vocab, stride=stride, offset_elems=offset).run()
        idx, val, _ = c.out()
        assert (idx < vocab).all()
        check_rows(x32, prms, u, hist, hlen, idx, val)


def test_graph_capture_and_replay(gpu):
    rng = np.random.default_rng(9)
    rows, vocab, stride = 32, 128256, 64
    logits, x32 = make_logits(rng, (rows, vocab), BF16, 4.0)
    st = gpu.Stream()

    def setting(seed):
        g = np.random.default_rng(seed)
        prms = mixed_params(rows)
        g.shuffle(prms)
        hist = np.stack([g.choice(np.argsort(-x32[r])[:24], stride) for r in range(rows)]).astype(np.int32)
        hlen = g.integers(1, stride, rows).astype(np.int32)
        return prms, g.random(rows).astype(np.float32), hist, hlen

    prms, u, hist, hlen = setting(0)
    c = Call(gpu, logits, BF16, prms, u, hist, hlen, eos=[int(x32[0].argmax())])
    c.run(append=1, stream=st.s, sync=False)          # eager once: the stream's workspace exists before the capture
    st.synchronize()
    with gpu.Graph.capture(st) as g:
        c.run(append=1, stream=st.s, sync=False)
    for seed in (1, 2, 3):
        prms, u, hist, hlen = setting(seed)
        c.dp.upload(R.params_array(gpu.SAMPLING_PARAMS_DTYPE, prms))
        c.du.upload(u)
        c.hist.upload(hist)
        c.hlen.upload(hlen)
        g.launch()
        st.synchronize()
        idx, val, stop = c.out()
        check_rows(x32, prms, u, hist, hlen, idx, val)
        h1, l1 = c.history()
        assert np.array_equal(l1, hlen + 1) and np.array_equal(h1[np.arange(rows), hlen], idx)
        assert np.array_equal(stop, (idx == int(x32[0].argmax())).astype(np.uint8))


def test_host_argument_checks(gpu):
    d = gpu.DeviceBuffer(1 << 16)
    L, p = gpu.lib.atoma_sample_batch, d.ptr

    def call(logits=p, rows=1, vocab=16, stride=16, dtype=F32, params=p + 1024, u=p + 2048, hist=p + 3072, hstride=8, hlen=p + 4096, append=0,
             eos=p + 5120, num_eos=1, out=p + 6144):
        return L(logits, rows, vocab, stride, dtype, params, u, hist, hstride, hlen, append, eos, num_eos, out, None, None, None)

    d.fill_bytes(0)
    assert call() == 0, gpu.last_error()
    gpu.synchronize()
    assert call(rows=0) == 0
    for kw, word in [(dict(dtype=5), "dtype"), (dict(rows=-1), "shape"), (dict(vocab=0), "shape"), (dict(vocab=(2 << 20) + 1, stride=(2 << 20) + 1), "shape"),
                     (dict(stride=8), "row_stride"), (dict(params=None), "params"), (dict(u=None), "u"), (dict(out=None), "out_idx"),
                     (dict(logits=None), "logits"), (dict(hlen=None), "history_len"), (dict(hist=None), "history"), (dict(hstride=0), "history_stride"),
                     (dict(num_eos=17), "num_eos"), (dict(num_eos=-1), "num_eos"), (dict(eos=None), "eos_ids"), (dict(append=2), "append"),
                     (dict(vocab=262145, stride=262145), "262144")]:
        assert call(**kw) == -1, kw
        assert word in gpu.last_error(), (kw, gpu.last_error())
    assert call(hist=None, hlen=None, hstride=0, eos=None, num_eos=0) == 0, gpu.last_error()       # no history, no EOS list
    gpu.synchronize()

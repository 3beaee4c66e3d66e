"""DecodeStep(sampling=...): the decode step ending in atoma_sample_batch inside its captured graph (tools/decode_step.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import sample_batch_ref as R
from oracle import cache_oracle as CO
from oracle import norm_rope_oracle as NR
from oracle.halfs import BF16, to_f32
from test_sample_batch_gpu import check_rows, mixed_params
from util import rand_half

pytestmark = pytest.mark.gpu


def small_model(rng, B, steps):
    import decode_step as DS
    cfg = DS.Config(layers=2, hidden=512, heads=4, kv_heads=2, head_dim=128, intermediate=1024, vocab=1008, page=16, max_pos=256)
    ctx = rng.integers(1, 100, B)
    blocks = [(int(L) + steps + cfg.page) // cfg.page for L in ctx]
    num_pages = sum(blocks) + 1
    bt = np.zeros((B, max(blocks)), np.int32)
    perm, p0 = rng.permutation(num_pages), 0
    for i, n in enumerate(blocks):
        bt[i, :n] = perm[p0:p0 + n]
        p0 += n
    H, I = cfg.hidden, cfg.inter
    one = lambda: NR.from_f32(1 + 0.1 * rng.standard_normal(H).astype(np.float32), BF16)
    host = dict(emb=rand_half(rng, (cfg.vocab, H), BF16), norm1=[one() for _ in range(cfg.layers)], norm2=[one() for _ in range(cfg.layers)],
                wqkv=[rand_half(rng, (cfg.qkv, H), BF16, H ** -0.5) for _ in range(cfg.layers)],
                wo=[rand_half(rng, (H, cfg.h * cfg.d), BF16, (cfg.h * cfg.d) ** -0.5) for _ in range(cfg.layers)],
                wgu=[rand_half(rng, (2 * I, H), BF16, H ** -0.5) for _ in range(cfg.layers)],
                wdown=[rand_half(rng, (H, I), BF16, I ** -0.5) for _ in range(cfg.layers)], norm_f=one(),
                lm_head=rand_half(rng, (cfg.vocab, H), BF16, 4.0 * H ** -0.5))
    kc0 = [rand_half(rng, (num_pages, cfg.page, cfg.hk, cfg.d), BF16) for _ in range(cfg.layers)]
    vc0 = [rand_half(rng, (num_pages, cfg.page, cfg.hk, cfg.d), BF16) for _ in range(cfg.layers)]
    return DS, cfg, ctx, bt, num_pages, DS.upload_weights(cfg, host), kc0, vc0


def place(step, cfg, bt, ctx, kc0=None, vc0=None, ids=None):
    """metadata of the step that appends position ctx[i] of sequence i"""
    B = len(ctx)
    if kc0 is not None:
        for l in range(cfg.layers):
            step.kc[l].upload(kc0[l])
            step.vc[l].upload(vc0[l])
    slots = np.array([CO.slot_mapping_for(bt[i], int(ctx[i]), int(ctx[i]) + 1, cfg.page)[0] for i in range(B)], np.int64)
    if ids is not None:
        step.set_inputs(ids, ctx, slots, (ctx + 1).astype(np.int32), bt)
    else:                                   # the ids stay on the device: the previous step's next_ids
        step.pos.upload(np.asarray(ctx, np.int64))
        step.slots.upload(slots)
        step.lens.upload((ctx + 1).astype(np.int32))


def test_all_greedy_sampling_step_equals_the_default_step(gpu):
    rng = np.random.default_rng(21)
    B = 24
    DS, cfg, ctx, bt, num_pages, w, kc0, vc0 = small_model(rng, B, 1)
    st = gpu.Stream()
    ids = rng.integers(0, cfg.vocab, B)
    res = []
    for sampling in (None, dict(history_stride=32, eos_ids=[1, 2])):
        step = DS.DecodeStep(cfg, B, num_pages, bt.shape[1], w, st, sampling=sampling)
        place(step, cfg, bt, ctx, kc0, vc0, ids)
        step.run()
        st.synchronize()
        res.append((step.logits.numpy(np.uint16, (B, cfg.vocab)), step.next_ids.numpy(np.int32, (B,)), step.next_val.numpy(np.float32, (B,))))
    assert np.array_equal(res[0][0], res[1][0]), "logits differ"
    assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2].view(np.uint32), res[1][2].view(np.uint32))
    assert np.array_equal(step.ids.numpy(np.int32, (B,)), res[1][1])          # fed back for the next step
    assert np.array_equal(step.history_len.numpy(np.int32, (B,)), np.ones(B, np.int32))
    assert np.array_equal(step.stop.numpy(np.uint8, (B,)), np.isin(res[1][1], [1, 2]).astype(np.uint8))


def test_mixed_sampling_over_four_graph_replays(gpu):
    rng = np.random.default_rng(22)
    B, steps, stride = 32, 4, 24
    DS, cfg, ctx, bt, num_pages, w, kc0, vc0 = small_model(rng, B, steps)
    st = gpu.Stream()
    step = DS.DecodeStep(cfg, B, num_pages, bt.shape[1], w, st, sampling=dict(history_stride=stride, eos_ids=[7]))
    prms = mixed_params(B)
    for p in prms:
        p["repeat_last_n"] = 16
    hist0 = rng.integers(0, cfg.vocab, (B, 12)).astype(np.int32)
    hlen0 = rng.integers(1, 13, B).astype(np.int32)
    ids = rng.integers(0, cfg.vocab, B)
    place(step, cfg, bt, ctx, kc0, vc0, ids)
    step.set_sampling(R.params_array(gpu.SAMPLING_PARAMS_DTYPE, prms), rng.random(B).astype(np.float32), hist0, hlen0)
    step.run()                               # eager once (workspaces), then captured; its effects are overwritten below
    st.synchronize()
    with gpu.Graph.capture(st) as g:
        step.run()
    place(step, cfg, bt, ctx, kc0, vc0, ids)
    hist = np.zeros((B, stride), np.int32)
    hist[:, :12] = hist0
    hlen = hlen0.copy()
    step.set_sampling(history=hist, history_len=hlen)
    fed = np.asarray(ids, np.int32)
    for t in range(steps):
        u = rng.random(B).astype(np.float32)
        step.set_uniforms(u)
        if t:
            place(step, cfg, bt, ctx + t)
        assert np.array_equal(step.ids.numpy(np.int32, (B,)), fed)
        g.launch()
        st.synchronize()
        x32 = to_f32(step.logits.numpy(np.uint16, (B, cfg.vocab)), BF16)
        idx, val = step.next_ids.numpy(np.int32, (B,)), step.next_val.numpy(np.float32, (B,))
        check_rows(x32, prms, u, hist, hlen, idx, val)
        assert np.array_equal(step.stop.numpy(np.uint8, (B,)), (idx == 7).astype(np.uint8))
        hist[np.arange(B), hlen] = idx
        hlen += 1
        fed = idx
    assert np.array_equal(step.history.numpy(np.int32, (B, stride)), hist)
    assert np.array_equal(step.history_len.numpy(np.int32, (B,)), hlen)
    assert np.array_equal(hlen, hlen0 + steps)

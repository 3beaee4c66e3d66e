"""What the GPU tests of the quantised-weight projections (test_linear_fp8w_gpu.py, test_linear_mxfp4_gpu.py) share: the reporting and
comparison helpers, the small model of the decode-step tests, and the op-by-op decode-step check itself, parametrised by the format."""
import numpy as np

from oracle import elementwise_oracle as EO
from oracle import norm_rope_oracle as NR
from oracle import cache_oracle as CO
from oracle.halfs import BF16, to_f32
from util import rand_half


def report(what, got, ref, dtype):
    g, r = to_f32(got, dtype), to_f32(ref, dtype)
    print(f"{what}: max |err| {np.abs(g - r).max() if g.size else 0.0:.3e}, differing {(got != ref).mean() if g.size else 0.0:.5f}")


def unsigned_zero(bits):
    """+0 for -0: the sign of a zero sum is the only thing an exact sum leaves open"""
    bits = np.array(bits, np.uint16)
    bits[bits == 0x8000] = 0
    return bits


def close_linear(got, ref, what):                                # the rule of tests/test_decode_step_gpu.py:28
    g, r = to_f32(got, BF16), to_f32(ref, BF16)
    assert (np.abs(g - r) <= 2.0 ** -7 * np.abs(r) + 3e-5).all(), what


def _step_setup(rng, B):
    import decode_step as DS
    cfg = DS.Config(layers=2, hidden=512, heads=4, kv_heads=2, head_dim=128, intermediate=1024, vocab=1008, page=16, max_pos=256)
    ctx = rng.integers(0, 100, B)
    lens = (ctx + 1).astype(np.int32)
    blocks = [(int(n) + cfg.page - 1) // cfg.page for n in lens]
    num_pages = sum(blocks) + 3
    perm = rng.permutation(num_pages)
    bt = np.zeros((B, max(blocks)), np.int32)
    pos0 = 0
    for i, n in enumerate(blocks):
        bt[i, :n] = perm[pos0:pos0 + n]
        pos0 += n
    H, I = cfg.hidden, cfg.inter
    near1 = lambda: NR.from_f32(1 + to_f32(rand_half(rng, (H,), BF16, 0.1), BF16), BF16)
    host = dict(emb=rand_half(rng, (cfg.vocab, H), BF16), norm1=[near1() for _ in range(cfg.layers)],
                wqkv=[rand_half(rng, (cfg.qkv, H), BF16, H ** -0.5) for _ in range(cfg.layers)],
                wo=[rand_half(rng, (H, cfg.h * cfg.d), BF16, (cfg.h * cfg.d) ** -0.5) for _ in range(cfg.layers)],
                norm2=[near1() for _ in range(cfg.layers)], wgu=[rand_half(rng, (2 * I, H), BF16, H ** -0.5) for _ in range(cfg.layers)],
                wdown=[rand_half(rng, (H, I), BF16, I ** -0.5) for _ in range(cfg.layers)], norm_f=near1(),
                lm_head=rand_half(rng, (cfg.vocab, H), BF16, H ** -0.5))
    kc0 = [rand_half(rng, (num_pages, cfg.page, cfg.hk, cfg.d), BF16) for _ in range(cfg.layers)]
    vc0 = [rand_half(rng, (num_pages, cfg.page, cfg.hk, cfg.d), BF16) for _ in range(cfg.layers)]
    ids = rng.integers(0, cfg.vocab, B)
    slots = np.array([CO.slot_mapping_for(bt[i], int(ctx[i]), int(ctx[i]) + 1, cfg.page)[0] for i in range(B)], np.int64)
    return DS, cfg, host, (ids, ctx, slots, lens, bt), num_pages, kc0, vc0


def check_decode_step_op_by_op(gpu, B, weight_dtype, quantise_ref, linear_ref, w_attr, scale_attr):
    """DecodeStep(weight_dtype=...): every projection's recorded output against the restatement applied to that op's own recorded input,
    residual / SiLU.up results bit-equal to the element-wise oracles on the recorded operands, next_ids = argmax of the step's own logits,
    the stored bytes / scales = the restatement's quantisation of the host weights; then the fused-epilogue run bit-equal to the unfused.
    quantise_ref(w, dtype) -> (bytes, scales), linear_ref(x, bytes, scales, dtype) -> y; w_attr / scale_attr name the step's device copies."""
    rng = np.random.default_rng(40 + B)
    DS, cfg, host, inputs, num_pages, kc0, vc0 = _step_setup(rng, B)
    ids, ctx, slots, lens, bt = inputs
    st = gpu.Stream()
    w = DS.upload_weights(cfg, host)
    H, I, hd, qw = cfg.hidden, cfg.inter, cfg.h * cfg.d, cfg.qkv
    dl = lambda buf, shape: buf.numpy(np.uint16, shape)
    runs = []
    for fused in (False, True):
        step = DS.DecodeStep(cfg, B, num_pages, bt.shape[1], w, st, keep_intermediates=not fused, fused_epilogues=fused, weight_dtype=weight_dtype)
        assert step.fp8w == (weight_dtype == "fp8") and step.mxfp4 == (weight_dtype == "mxfp4") and step.fused == fused
        for l in range(cfg.layers):
            step.kc[l].upload(kc0[l])
            step.vc[l].upload(vc0[l])
        step.set_inputs(*inputs)
        step.run()
        st.synchronize()
        runs.append((dl(step.logits, (B, cfg.vocab)), step.next_ids.numpy(np.int32, (B,)), [dl(step.kc[l], None) for l in range(cfg.layers)],
                     [dl(step.vc[l], None) for l in range(cfg.layers)]))
        if fused:
            continue
        q = {}
        for name in ("wqkv", "wo", "wgu", "wdown"):
            for l in range(cfg.layers):
                ref_w, ref_s = q[name, l] = quantise_ref(host[name][l], BF16)
                assert np.array_equal(getattr(step, w_attr)[name][l].numpy(ref_w.dtype, ref_w.shape), ref_w), f"{name}[{l}] bytes"
                assert np.array_equal(getattr(step, scale_attr)[name][l].numpy(ref_s.dtype, ref_s.shape), ref_s), f"{name}[{l}] scales"
        x_prev = dl(step.trace[0][2]["out"], (B, H))
        assert np.array_equal(x_prev, EO.embedding(ids, host["emb"]))
        for (_, l, t) in step.trace[1:-1]:
            x, xn1, qkv_pre = dl(t["x"], (B, H)), dl(t["xn1"], (B, H)), dl(t["qkv_pre"], (B, qw))
            assert np.array_equal(x, x_prev)
            close_linear(qkv_pre, linear_ref(xn1, *q["wqkv", l], BF16), f"layer {l} qkv projection")
            att, o, x1, xn2 = dl(t["att"], (B, hd)), dl(t["o"], (B, H)), dl(t["x1"], (B, H)), dl(t["xn2"], (B, H))
            close_linear(o, linear_ref(att, *q["wo", l], BF16), f"layer {l} o projection")
            assert np.array_equal(x1, EO.add(x, o, BF16))
            gu, act, dn, x2 = dl(t["gu"], (B, 2 * I)), dl(t["act"], (B, I)), dl(t["dn"], (B, H)), dl(t["x2"], (B, H))
            close_linear(gu, linear_ref(xn2, *q["wgu", l], BF16), f"layer {l} gate/up projection")
            assert np.array_equal(act, EO.silu_mul(np.ascontiguousarray(gu[:, :I]), np.ascontiguousarray(gu[:, I:]), BF16)), f"layer {l} SiLU.up"
            close_linear(dn, linear_ref(act, *q["wdown", l], BF16), f"layer {l} down projection")
            assert np.array_equal(x2, EO.add(x1, dn, BF16))
            x_prev = x2
        assert np.array_equal(runs[0][1], to_f32(runs[0][0], BF16).argmax(1))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    assert all(np.array_equal(a, b) for a, b in zip(runs[0][2] + runs[0][3], runs[1][2] + runs[1][3]))

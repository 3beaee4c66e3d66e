"""MXFP4-weight projections on the device, through the C ABI: the quantiser bit for bit against the tests' restatement (mxfp4_ref), the
products against the exactly accumulated product under the acceptance rule of test_linear_gpu.check, one-hot inputs that pin every nibble
and scale position, integer inputs bit for bit, the epilogues against the separate ops, strides, out-of-range scale bytes, stream order,
and a whole decode step over MXFP4 weights op by op."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from oracle import elementwise_oracle as EO
from oracle.halfs import F16, BF16, to_f32, from_f32
from mxfp4_ref import quantize_blocks, dequantize, linear_mxfp4
from test_linear_gpu import check
from util import rand_half
from wq_cases import report, unsigned_zero, check_decode_step_op_by_op

pytestmark = pytest.mark.gpu

# every slab remainder (K % 512 = 128, 256, 384, 0), one-slab K, and the workgroup widths 1, 2, 4, 8 the plan picks at small N; both regimes
SHAPES = [(1, 128, 16), (3, 384, 48), (4, 640, 272), (2, 2176, 1040), (1, 4096, 4096), (4, 14336, 512), (2, 16384, 32),
          (5, 128, 16), (9, 896, 48), (16, 2176, 1040), (12, 4096, 6144), (16, 14336, 512), (7, 16384, 32)]


def gpu_quantize(gpu, w, dtype, w_stride=None, w4_stride=None, s_stride=None):
    N, K = w.shape
    ws, w4s, ss = w_stride or K, w4_stride or K // 2, s_stride or K // 32
    wide = np.zeros((N, ws), np.uint16)
    wide[:, :K] = w
    wide[:, K:] = 0x7BFF if dtype == F16 else 0x7F7F            # the padding holds the largest finite value: it must not reach amax
    dw, d4, ds = gpu.DeviceBuffer.from_numpy(wide), gpu.DeviceBuffer(N * w4s), gpu.DeviceBuffer(N * ss)
    d4.fill_bytes(0xA5)
    ds.fill_bytes(0x5A)
    assert gpu.lib.atoma_quantize_weight_mxfp4(dw.ptr, N, K, ws, dtype, d4.ptr, w4s, ds.ptr, ss, None) == 0, gpu.last_error()
    gpu.synchronize()
    out4, outs = d4.numpy(np.uint8, (N, w4s)), ds.numpy(np.uint8, (N, ss))
    assert (out4[:, K // 2:] == 0xA5).all() and (outs[:, K // 32:] == 0x5A).all()
    return np.ascontiguousarray(out4[:, :K // 2]), np.ascontiguousarray(outs[:, :K // 32])


def gpu_mxfp4(gpu, x, w4, scale, dtype, stream=None, sync=True):
    B, K, N = x.shape[0], w4.shape[1] * 2, w4.shape[0]
    dx = gpu.DeviceBuffer.from_numpy(x if B else np.zeros((1, K), np.uint16))
    dw, ds = gpu.DeviceBuffer.from_numpy(w4), gpu.DeviceBuffer.from_numpy(scale)
    dy = gpu.DeviceBuffer(max(B, 1) * N * 2)
    dy.fill_bytes(0xFF)
    rc = gpu.lib.atoma_linear_decode_mxfp4(dx.ptr, dw.ptr, ds.ptr, dy.ptr, B, K, N, K, K // 2, K // 32, N, dtype, stream)
    assert rc == 0, gpu.last_error()
    if not sync:
        return dy, (dx, dw, ds)
    gpu.synchronize()
    return dy.numpy(np.uint16, (max(B, 1), N))[:B]


TIES = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_quantize_weight_mxfp4_is_bit_exact(gpu, dtype):
    """bytes and scales == the restatement: 33 blocks per row, default and padded strides of all three tensors (padding untouched on output,
    never part of amax on input), an all-zero block, a dominant outlier, every tie in both signs, the exponent clamp, the largest finite value."""
    rng = np.random.default_rng(5)
    N, K = 48, 1056
    w = rand_half(rng, (N, K), dtype, K ** -0.5)
    w[2, 64:96] = 0                                              # an all-zero block ...
    w[2, 96:128] = 0x8000                                        # ... and one of negative zeros
    w[9, 1000] = 0x7BFF if dtype == F16 else 0x7F7F              # the largest finite value of the dtype
    for r, v in ((11, 30.0), (12, -7.5), (13, 1000.0)):          # one dominant outlier per block
        w[r, int(rng.integers(K))] = from_f32(np.array([v], np.float32), dtype)[0]
    ties = [7.5] + TIES + [-t for t in TIES] + [7.0, -7.0, 5.5, -5.5, 6.0, -6.0, 0.0, -0.0]
    w[20, 32:32 + len(ties)] = from_f32(np.array(ties, np.float32), dtype)   # amax 7.5: e = 0, v is the value itself
    w[20, 32 + len(ties):64] = 0
    w[21, 992:1024] = from_f32((np.array(ties + [0.0] * (32 - len(ties)), np.float32) * 2.0 ** -9), dtype)   # the same block at another exponent
    tiny = 1e-7 if dtype == F16 else 2.0 ** -130
    w[30, 0:32] = from_f32(np.full(32, tiny, np.float32), dtype)            # the exponent clamp: all codes zero
    w[30, 32:64] = from_f32((np.linspace(-6, 6, 32) * (2.0 ** -15 if dtype == F16 else 2.0 ** -127)).astype(np.float32), dtype)   # ... and around it
    ref4, refs = quantize_blocks(w, dtype)
    assert refs[2, 2] == 127 and refs[2, 3] == 127 and (ref4[2, 48:64] == 0x88).all() and refs[20, 1] == 127
    assert refs[30, 0] == (114 if dtype == F16 else 2) and (ref4[30, :16] == 0).all()
    for ws, w4s, ss in ((None, None, None), (K + 24, K // 2 + 48, K // 32 + 7)):
        w4, scale = gpu_quantize(gpu, w, dtype, ws, w4s, ss)
        assert np.array_equal(scale, refs), f"{(scale != refs).sum()} scale bytes differ"
        assert np.array_equal(w4, ref4), f"{(w4 != ref4).sum()} bytes differ"


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("B,K,N", SHAPES + [(0, 4096, 4096)])
def test_linear_decode_mxfp4_projection_shapes(gpu, dtype, B, K, N):
    """both regimes (1..4, 5..16 rows), every slab remainder, weights quantised on the device."""
    rng = np.random.default_rng(B * 7 + K + N)
    x = rand_half(rng, (B, K), dtype)
    w = rand_half(rng, (N, K), dtype, K ** -0.5)
    w4, scale = gpu_quantize(gpu, w, dtype)
    got = gpu_mxfp4(gpu, x, w4, scale, dtype)
    if B == 0:
        assert got.shape == (0, N)
        return
    ref = linear_mxfp4(x, w4, scale, dtype)
    report(f"mxfp4 B={B} K={K} N={N} dtype={dtype}", got, ref, dtype)
    check(got, ref, dtype)


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("B", [4, 16])
@pytest.mark.parametrize("K", [640, 2176])
def test_linear_decode_mxfp4_one_hot_inputs_pick_single_weights(gpu, dtype, B, K):
    """x[b] = e_k(b): y[b][n] is W[n][k(b)] to the bit -- the nibble order, the byte order of a word, the scale of every block and the zeros
    of the partial last slab.  Every code sits at every position of a block (row n holds code (n + i) % 16 at input i)."""
    rng = np.random.default_rng(K + B)
    N = 48
    code = ((np.arange(N)[:, None] + np.arange(K)[None, :]) % 16).astype(np.uint8)
    w4 = (code[:, 0::2] | (code[:, 1::2] << 4)).astype(np.uint8)
    scale = rng.integers(120, 135, (N, K // 32)).astype(np.uint8)
    W = dequantize(w4, scale)
    ks = [0, 1, K // 2 - 1, K // 2 + 37, 7, 8, 15, 16, 30, 31, 32, 33, 63, 64, 127, 128, 255, 256, 383, 384, 510, 511, 512, 513, 543, 544, K - 129, K - 128, K - 97, K - 33, K - 2, K - 1]
    assert len(ks) % B == 0 and max(ks) < K
    one = from_f32(np.array([1.0], np.float32), dtype)[0]
    for i in range(0, len(ks), B):
        x = np.zeros((B, K), np.uint16)
        x[np.arange(B), ks[i:i + B]] = one
        got = gpu_mxfp4(gpu, x, w4, scale, dtype)
        ref = from_f32(W[:, ks[i:i + B]].T.astype(np.float32), dtype)
        assert np.array_equal(to_f32(ref, dtype).astype(np.float64), W[:, ks[i:i + B]].T)      # exact in the dtype
        bad = np.argwhere(unsigned_zero(got) != unsigned_zero(ref))
        assert bad.size == 0, f"k = {ks[i:i + B]}: first mismatch (b, n) = {bad[0]}, got {to_f32(got, dtype)[tuple(bad[0])]}, want {to_f32(ref, dtype)[tuple(bad[0])]}"


@pytest.mark.parametrize("B,K,N", [(1, 2048, 256), (3, 4096, 256), (4, 384, 512), (2, 16384, 32), (9, 2048, 256), (16, 14336, 64), (16, 640, 48), (12, 16384, 32)])
def test_linear_decode_mxfp4_integer_inputs_are_bit_exact(gpu, B, K, N):
    """integer x in [-4, 4], all 16 codes, scale bytes 126..129: every partial sum is a multiple of 0.25 below 2^24 * 0.25, exact in fp32, so
    the result is bit-equal to the restatement whatever the split."""
    rng = np.random.default_rng(B + K + N)
    x = from_f32(rng.integers(-4, 5, (B, K)).astype(np.float32), BF16)
    w4 = rng.integers(0, 256, (N, K // 2)).astype(np.uint8)
    scale = rng.integers(126, 130, (N, K // 32)).astype(np.uint8)
    assert np.abs(dequantize(w4, scale)).max() * 4 * K < 2 ** 24 * 0.25
    got, ref = gpu_mxfp4(gpu, x, w4, scale, BF16), linear_mxfp4(x, w4, scale, BF16)
    assert np.array_equal(unsigned_zero(got), unsigned_zero(ref)), f"{(unsigned_zero(got) != unsigned_zero(ref)).sum()} outputs differ"


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("B", [2, 12])
def test_linear_decode_mxfp4_epilogues_match_the_separate_ops(gpu, dtype, B):
    """_residual and _silu_mul == the plain call followed by atoma_add / atoma_silu_mul on its rounded output, bit for bit."""
    rng = np.random.default_rng(21 + B)
    K, N, I = 1152, 512, 768
    L = gpu.lib
    x, res = rand_half(rng, (B, K), dtype), rand_half(rng, (B, N), dtype)
    w4, sc = quantize_blocks(rand_half(rng, (N, K), dtype, K ** -0.5), dtype)
    g4, gsc = quantize_blocks(rand_half(rng, (2 * I, K), dtype, K ** -0.5), dtype)
    dx, dr, dw, ds, dg, dgs = (gpu.DeviceBuffer.from_numpy(a) for a in (x, res, w4, sc, g4, gsc))
    y, y2, gu, act, act2 = (gpu.DeviceBuffer(n * 2) for n in (B * N, B * N, B * 2 * I, B * I, B * I))
    K2, KS = K // 2, K // 32
    assert L.atoma_linear_decode_mxfp4(dx.ptr, dw.ptr, ds.ptr, y.ptr, B, K, N, K, K2, KS, N, dtype, None) == 0, gpu.last_error()
    gpu.synchronize()
    plain = y.numpy(np.uint16, (B, N))
    check(plain, linear_mxfp4(x, w4, sc, dtype), dtype)
    assert L.atoma_add(y.ptr, dr.ptr, y.ptr, B * N, dtype, None) == 0
    assert L.atoma_linear_decode_mxfp4_residual(dx.ptr, dw.ptr, ds.ptr, dr.ptr, y2.ptr, B, K, N, K, K2, KS, N, N, dtype, None) == 0, gpu.last_error()
    assert L.atoma_linear_decode_mxfp4(dx.ptr, dg.ptr, dgs.ptr, gu.ptr, B, K, 2 * I, K, K2, KS, 2 * I, dtype, None) == 0, gpu.last_error()
    assert L.atoma_silu_mul(gu.ptr, gu.ptr + I * 2, act.ptr, B, I, 2 * I, 2 * I, I, dtype, None) == 0
    assert L.atoma_linear_decode_mxfp4_silu_mul(dx.ptr, dg.ptr, dgs.ptr, act2.ptr, B, K, I, K, K2, KS, I, dtype, None) == 0, gpu.last_error()
    gpu.synchronize()
    assert np.array_equal(y.numpy(np.uint16, (B, N)), y2.numpy(np.uint16, (B, N)))
    assert np.array_equal(y2.numpy(np.uint16, (B, N)), EO.add(plain, res, dtype))
    assert np.array_equal(act.numpy(np.uint16, (B, I)), act2.numpy(np.uint16, (B, I)))


@pytest.mark.parametrize("B", [3, 10])
def test_linear_decode_mxfp4_strides_and_out_of_range_scales(gpu, B):
    """strided x, padded y whose padding stays untouched, w4 and scale rows at padded strides whose padding (0x77 nibbles, 0xFF scales) is
    never read; one 0xFF scale byte leaves every other output column finite and right (nothing is asserted about its own column)."""
    rng = np.random.default_rng(3 + B)
    K, N = 1152, 272
    wide = rand_half(rng, (B, K + 256), BF16)
    x = np.ascontiguousarray(wide[:, 128:128 + K])
    w4, sc = quantize_blocks(rand_half(rng, (N, K), BF16, K ** -0.5), BF16)
    sc[5, 7] = 0xFF
    w4s, ss, ys = K // 2 + 64, K // 32 + 12, N + 64
    w4p, scp = np.full((N, w4s), 0x77, np.uint8), np.full((N, ss), 0xFF, np.uint8)
    w4p[:, :K // 2], scp[:, :K // 32] = w4, sc
    dx, dw, ds = gpu.DeviceBuffer.from_numpy(wide), gpu.DeviceBuffer.from_numpy(w4p), gpu.DeviceBuffer.from_numpy(scp)
    dy = gpu.DeviceBuffer(B * ys * 2)
    dy.fill_bytes(0xAB)
    assert gpu.lib.atoma_linear_decode_mxfp4(dx.ptr + 128 * 2, dw.ptr, ds.ptr, dy.ptr, B, K, N, K + 256, w4s, ss, ys, BF16, None) == 0, gpu.last_error()
    gpu.synchronize()
    out = dy.numpy(np.uint16, (B, ys))
    assert (out[:, N:] == 0xABAB).all()
    ok = np.ones(N, bool)
    ok[5] = False
    assert np.isfinite(to_f32(out[:, :N], BF16)[:, ok]).all()
    check(np.ascontiguousarray(out[:, :N][:, ok]), linear_mxfp4(x, w4[ok], sc[ok], BF16), BF16)


def test_linear_decode_mxfp4_is_stream_ordered(gpu):
    """ten calls back to back on one stream, mixed shapes and regimes, one synchronise at the end."""
    rng = np.random.default_rng(9)
    st = gpu.Stream()
    shapes = [(B, min(K, 4096), min(N, 1040)) for B, K, N in (SHAPES[i] for i in (7, 0, 8, 4, 11, 6, 9, 1, 10, 3))]
    jobs = []
    for B, K, N in shapes:
        x = rand_half(rng, (B, K), BF16)
        w4, sc = quantize_blocks(rand_half(rng, (N, K), BF16, K ** -0.5), BF16)
        jobs.append((x, w4, sc))
    pending = [gpu_mxfp4(gpu, x, w4, sc, BF16, stream=st.s, sync=False) for x, w4, sc in jobs]
    st.synchronize()
    for (x, w4, sc), (dy, _keep) in zip(jobs, pending):
        check(dy.numpy(np.uint16, (x.shape[0], w4.shape[0])), linear_mxfp4(x, w4, sc, BF16), BF16)


def test_linear_decode_mxfp4_rejects_more_than_16_rows_on_the_device(gpu):
    d = gpu.DeviceBuffer(1 << 16)
    assert gpu.lib.atoma_linear_decode_mxfp4(d.ptr, d.ptr, d.ptr, d.ptr, 17, 128, 16, 128, 64, 4, 16, BF16, None) == -1
    assert "16" in gpu.last_error()


@pytest.mark.parametrize("B", [1, 8, 16])
def test_decode_step_over_mxfp4_weights_op_by_op(gpu, B):
    """DecodeStep(weight_dtype="mxfp4") against the restatement, op by op, and fused against unfused (wq_cases.check_decode_step_op_by_op)."""
    check_decode_step_op_by_op(gpu, B, "mxfp4", quantize_blocks, linear_mxfp4, "w4", "w4_scale")


def test_decode_step_over_mxfp4_weights_refuses_more_than_16_rows(gpu):
    import decode_step as DS
    cfg = DS.Config(layers=1, hidden=128, heads=1, kv_heads=1, head_dim=128, intermediate=128, vocab=128, page=16, max_pos=64)
    with pytest.raises(ValueError, match="16"):
        DS.DecodeStep(cfg, 17, 4, 1, {}, gpu.Stream(), weight_dtype="mxfp4")
    with pytest.raises(ValueError, match="tensor-parallel"):
        DS.DecodeStep(cfg, 4, 4, 1, {}, gpu.Stream(), weight_dtype="mxfp4", allreduce=lambda ptr, count: None)

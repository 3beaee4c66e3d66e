"""fp8-weight projections on the device, through the C ABI: the quantiser bit for bit against the tests' restatement (fp8w_ref), the
products against the exactly accumulated product under the acceptance rule of test_linear_gpu.check, one-hot inputs that pin every byte
position, the epilogues against the separate ops, strides, NaN bytes, stream order, and a whole decode step over fp8 weights op by op."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from oracle import elementwise_oracle as EO
from oracle import fp8_oracle as F8
from oracle import linear_oracle as LO
from oracle.halfs import F16, BF16, to_f32, from_f32
from fp8w_ref import quantize_rows, linear_fp8w
from test_linear_gpu import check
from util import rand_half
from wq_cases import report, unsigned_zero, check_decode_step_op_by_op

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4096, 4096), (16, 4096, 6144), (3, 14336, 4096), (7, 128, 16), (16, 2048, 512), (5, 4096, 28672), (2, 8192, 1024), (17, 4096, 4096),
          (32, 2048, 6144), (33, 4096, 1024), (48, 1024, 4112), (64, 4096, 4096), (50, 14336, 512)]   # test_linear_decode_llama_projection_shapes


def gpu_quantize(gpu, w, dtype, w_stride=None, w8_stride=None):
    N, K = w.shape
    ws, w8s = w_stride or K, w8_stride or K
    wide = np.zeros((N, ws), np.uint16)
    wide[:, :K] = w
    wide[:, K:] = 0x7BFF if dtype == F16 else 0x7F7F            # the padding holds the largest finite value: it must not reach amax
    dw, d8, ds = gpu.DeviceBuffer.from_numpy(wide), gpu.DeviceBuffer(N * w8s), gpu.DeviceBuffer(N * 4)
    d8.fill_bytes(0xA5)
    assert gpu.lib.atoma_quantize_weight_fp8(dw.ptr, N, K, ws, dtype, d8.ptr, w8s, ds.ptr, None) == 0, gpu.last_error()
    gpu.synchronize()
    out = d8.numpy(np.uint8, (N, w8s))
    assert (out[:, K:] == 0xA5).all()
    return np.ascontiguousarray(out[:, :K]), ds.numpy(np.float32, (N,))


def gpu_fp8w(gpu, x, w8, scale, dtype, stream=None, sync=True):
    B, K, N = x.shape[0], w8.shape[1], w8.shape[0]
    dx = gpu.DeviceBuffer.from_numpy(x if B else np.zeros((1, K), np.uint16))
    dw, ds = gpu.DeviceBuffer.from_numpy(w8), gpu.DeviceBuffer.from_numpy(np.asarray(scale, np.float32))
    dy = gpu.DeviceBuffer(max(B, 1) * N * 2)
    dy.fill_bytes(0xFF)
    rc = gpu.lib.atoma_linear_decode_fp8w(dx.ptr, dw.ptr, ds.ptr, dy.ptr, B, K, N, K, K, N, dtype, stream)
    assert rc == 0, gpu.last_error()
    if not sync:
        return dy, (dx, dw, ds)
    gpu.synchronize()
    return dy.numpy(np.uint16, (max(B, 1), N))[:B]


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_quantize_weight_fp8_is_bit_exact(gpu, dtype):
    """bytes and scales == the restatement: padded strides, an all-zero row, the dtype's largest finite value, dominant outliers."""
    rng = np.random.default_rng(5)
    N, K = 80, 1056
    w = rand_half(rng, (N, K), dtype, K ** -0.5)
    w[2] = 0
    w[9, 1000] = 0x7BFF if dtype == F16 else 0x7F7F              # the largest finite value of the dtype
    for r, v in ((11, 30.0), (12, -7.5), (13, 1000.0)):          # one dominant outlier per row
        w[r, int(rng.integers(K))] = from_f32(np.array([v], np.float32), dtype)[0]
    ref8, refs = quantize_rows(w, dtype)
    for ws, w8s in ((None, None), (K + 24, K + 48)):
        w8, scale = gpu_quantize(gpu, w, dtype, ws, w8s)
        assert np.array_equal(scale.view(np.uint32), refs.view(np.uint32))
        assert np.array_equal(w8, ref8), f"{(w8 != ref8).sum()} bytes differ"
    assert refs[2] == 1.0 and not ((ref8 & 0x7F) == 0x7F).any()


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("B,K,N", SHAPES + [(0, 4096, 4096)])
def test_linear_decode_fp8w_llama_projection_shapes(gpu, dtype, B, K, N):
    """every regime (1..4, 5..16, 17..64 rows), with and without K split, weights quantised on the device."""
    rng = np.random.default_rng(B * 7 + K + N)
    x = rand_half(rng, (B, K), dtype)
    w = rand_half(rng, (N, K), dtype, K ** -0.5)
    w8, scale = gpu_quantize(gpu, w, dtype)
    got, ref = gpu_fp8w(gpu, x, w8, scale, dtype), linear_fp8w(x, w8, scale, dtype)
    report(f"fp8w B={B} K={K} N={N} dtype={dtype}", got, ref, dtype)
    if B == 0:
        assert got.shape == (0, N)
        return
    check(got, ref, dtype)


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("B", [1, 4, 12, 40, 64])
def test_linear_decode_fp8w_power_of_two_scales_meet_the_16_bit_oracle(gpu, dtype, B):
    """with power-of-two scales the dequantised weights are exact 16-bit numbers: the existing oracle on them is the reference."""
    rng = np.random.default_rng(100 + B)
    K, N = 2176, 1040                                            # K: 8.5 slabs of 256 inputs -- the half slab at the end is live
    w8 = F8.encode((rng.standard_normal((N, K)) * 40).astype(np.float32))
    w8[(w8 & 0x78) == 0] &= 0x80                                 # no fp8 subnormals: times 2^-9 they would leave f16's exact range
    scale = (2.0 ** rng.integers(-9, -4, N)).astype(np.float32)
    dequant = from_f32((F8.decode(w8) * scale[:, None]).astype(np.float32), dtype)
    assert np.array_equal(to_f32(dequant, dtype), F8.decode(w8) * scale[:, None])
    x = rand_half(rng, (B, K), dtype)
    got = gpu_fp8w(gpu, x, w8, scale, dtype)
    report(f"fp8w pow2 B={B} dtype={dtype}", got, LO.linear(x, dequant, dtype), dtype)
    check(got, LO.linear(x, dequant, dtype), dtype)


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("B", [4, 16, 32])
@pytest.mark.parametrize("K", [640, 2432])
def test_linear_decode_fp8w_one_hot_inputs_pick_single_weights(gpu, dtype, B, K):
    """x[b] = e_k(b): y[b][n] is decode(w8[n][k(b)]) * scale[n] to the bit -- the byte order of a load, the lane / piece / slab arithmetic and
    the zeros of the half slab at the end (K = 640: 2.5 slabs in one wavefront; K = 2432: 9.5 slabs over two wavefronts, the half slab the last
    of the second; B = 32: the 17..64-row kernel).  Neighbouring positions hold different codes and every non-NaN code occurs."""
    N = 48
    w8 = ((37 * np.arange(N)[:, None] + np.arange(K)[None, :]) % 256).astype(np.uint8)
    w8[(w8 & 0x7F) == 0x7F] ^= 0x40                              # the two NaN codes -> 0x3F / 0xBF
    assert len(np.unique(w8)) == 254 and (w8[:, 1:] != w8[:, :-1]).all()
    scale = (2.0 ** (np.arange(N) % 5 - 2)).astype(np.float32)   # powers of two in [2^-2, 2^2]
    W = F8.decode(w8).astype(np.float64) * scale[:, None]
    ks = [0, 1, 7, 8, 15, 16, 127, 128, 255, 256, 257, 383, 384, 511, 512, K - 129, K - 128, K - 17, K - 1,
          2, 9, 31, 32, 63, 64, 129, 254, 385, 400, 450, 500, K - 2, K - 16, K - 18, K - 127, K - 200, K - 64]
    ks = list(dict.fromkeys(ks))[:32]                            # 32 distinct positions, the named ones first
    assert len(ks) == 32 and len(ks) % B == 0 and max(ks) < K and {K - 129, K - 128, K - 17, K - 1} <= set(ks)
    one = from_f32(np.array([1.0], np.float32), dtype)[0]
    for i in range(0, len(ks), B):
        x = np.zeros((B, K), np.uint16)
        x[np.arange(B), ks[i:i + B]] = one
        got = gpu_fp8w(gpu, x, w8, scale, dtype)
        ref = from_f32(W[:, ks[i:i + B]].T.astype(np.float32), dtype)
        assert np.array_equal(to_f32(ref, dtype).astype(np.float64), W[:, ks[i:i + B]].T)      # exact in the dtype
        bad = np.argwhere(unsigned_zero(got) != unsigned_zero(ref))
        assert bad.size == 0, f"k = {ks[i:i + B]}: first mismatch (b, n) = {bad[0]}, got {to_f32(got, dtype)[tuple(bad[0])]}, want {to_f32(ref, dtype)[tuple(bad[0])]}"


@pytest.mark.parametrize("B,K,N", [(1, 2048, 2048), (3, 4096, 256), (4, 384, 4096), (9, 2048, 2048), (16, 14336, 512), (16, 640, 48),
                                   (24, 2048, 2048), (64, 8192, 1024), (37, 1152, 4112)])
def test_linear_decode_fp8w_integer_inputs_are_bit_exact(gpu, B, K, N):
    """integer-valued x and w8 with scale 1: every partial sum is exact in fp32, so the result is bit-exact whatever the split."""
    rng = np.random.default_rng(B + K + N)
    x = from_f32(rng.integers(-4, 5, (B, K)).astype(np.float32), BF16)
    w8 = F8.encode(rng.integers(-2, 3, (N, K)).astype(np.float32))
    scale = np.ones(N, np.float32)
    assert np.array_equal(gpu_fp8w(gpu, x, w8, scale, BF16), linear_fp8w(x, w8, scale, BF16))
    assert np.array_equal(linear_fp8w(x, w8, scale, BF16), LO.linear(x, from_f32(F8.decode(w8), BF16), BF16))


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("B", [2, 12, 40])
def test_linear_decode_fp8w_epilogues_match_the_separate_ops(gpu, dtype, B):
    """_residual and _silu_mul == the plain fp8 call followed by atoma_add / atoma_silu_mul on its rounded output, bit for bit."""
    rng = np.random.default_rng(21 + B)
    K, N, I = 1152, 512, 768
    L = gpu.lib
    x, res = rand_half(rng, (B, K), dtype), rand_half(rng, (B, N), dtype)
    w8, sc = quantize_rows(rand_half(rng, (N, K), dtype, K ** -0.5), dtype)
    g8, gsc = quantize_rows(rand_half(rng, (2 * I, K), dtype, K ** -0.5), dtype)
    dx, dr, dw, ds, dg, dgs = (gpu.DeviceBuffer.from_numpy(a) for a in (x, res, w8, sc, g8, gsc))
    y, y2, gu, act, act2 = (gpu.DeviceBuffer(n * 2) for n in (B * N, B * N, B * 2 * I, B * I, B * I))
    assert L.atoma_linear_decode_fp8w(dx.ptr, dw.ptr, ds.ptr, y.ptr, B, K, N, K, K, N, dtype, None) == 0, gpu.last_error()
    gpu.synchronize()
    plain = y.numpy(np.uint16, (B, N))
    check(plain, linear_fp8w(x, w8, sc, dtype), dtype)
    assert L.atoma_add(y.ptr, dr.ptr, y.ptr, B * N, dtype, None) == 0
    assert L.atoma_linear_decode_fp8w_residual(dx.ptr, dw.ptr, ds.ptr, dr.ptr, y2.ptr, B, K, N, K, K, N, N, dtype, None) == 0, gpu.last_error()
    assert L.atoma_linear_decode_fp8w(dx.ptr, dg.ptr, dgs.ptr, gu.ptr, B, K, 2 * I, K, K, 2 * I, dtype, None) == 0, gpu.last_error()
    assert L.atoma_silu_mul(gu.ptr, gu.ptr + I * 2, act.ptr, B, I, 2 * I, 2 * I, I, dtype, None) == 0
    assert L.atoma_linear_decode_fp8w_silu_mul(dx.ptr, dg.ptr, dgs.ptr, act2.ptr, B, K, I, K, K, I, dtype, None) == 0, gpu.last_error()
    gpu.synchronize()
    assert np.array_equal(y.numpy(np.uint16, (B, N)), y2.numpy(np.uint16, (B, N)))
    assert np.array_equal(y2.numpy(np.uint16, (B, N)), EO.add(plain, res, dtype))
    assert np.array_equal(act.numpy(np.uint16, (B, I)), act2.numpy(np.uint16, (B, I)))


@pytest.mark.parametrize("B", [3, 10, 33])
def test_linear_decode_fp8w_strides_and_nan_bytes(gpu, B):
    """strided x, padded y whose padding stays untouched, w8 rows at a padded stride; a NaN byte poisons exactly its output column."""
    rng = np.random.default_rng(3 + B)
    K, N = 1152, 272
    wide = rand_half(rng, (B, K + 256), BF16)
    x = np.ascontiguousarray(wide[:, 128:128 + K])
    w8, sc = quantize_rows(rand_half(rng, (N, K), BF16, K ** -0.5), BF16)
    w8[5, 77], w8[N - 1, K - 1] = 0x7F, 0xFF
    w8s, ys = K + 64, N + 64
    w8p = np.full((N, w8s), 0x7F, np.uint8)                      # NaN bytes in the padding: never read
    w8p[:, :K] = w8
    dx, dw, ds = gpu.DeviceBuffer.from_numpy(wide), gpu.DeviceBuffer.from_numpy(w8p), gpu.DeviceBuffer.from_numpy(sc)
    dy = gpu.DeviceBuffer(B * ys * 2)
    dy.fill_bytes(0xAB)
    assert gpu.lib.atoma_linear_decode_fp8w(dx.ptr + 128 * 2, dw.ptr, ds.ptr, dy.ptr, B, K, N, K + 256, w8s, ys, BF16, None) == 0, gpu.last_error()
    gpu.synchronize()
    out = dy.numpy(np.uint16, (B, ys))
    assert (out[:, N:] == 0xABAB).all()
    got = to_f32(out[:, :N], BF16)
    bad = np.zeros(N, bool)
    bad[[5, N - 1]] = True
    assert np.isnan(got[:, bad]).all() and np.isfinite(got[:, ~bad]).all()
    check(np.ascontiguousarray(out[:, :N][:, ~bad]), linear_fp8w(x, w8[~bad], sc[~bad], BF16), BF16)


def test_linear_decode_fp8w_is_stream_ordered(gpu):
    """20 calls back to back on one stream, different shapes sharing the workspace, one synchronise at the end."""
    rng = np.random.default_rng(9)
    st = gpu.Stream()
    shapes = [SHAPES[i % len(SHAPES)] for i in (7, 0, 8, 4, 11, 6, 9, 1, 10, 3)] * 2
    shapes = [(B, min(K, 4096), min(N, 2048)) for B, K, N in shapes]
    jobs = []
    for i, (B, K, N) in enumerate(shapes):
        x = rand_half(rng, (B, K), BF16)
        w8, sc = quantize_rows(rand_half(rng, (N, K), BF16, K ** -0.5), BF16)
        jobs.append((x, w8, sc))
    pending = [gpu_fp8w(gpu, x, w8, sc, BF16, stream=st.s, sync=False) for x, w8, sc in jobs]
    st.synchronize()
    for (x, w8, sc), (dy, _keep) in zip(jobs, pending):
        check(dy.numpy(np.uint16, (x.shape[0], w8.shape[0])), linear_fp8w(x, w8, sc, BF16), BF16)


def test_linear_decode_fp8w_rejects_more_than_64_rows_on_the_device(gpu):
    d = gpu.DeviceBuffer(1 << 16)
    assert gpu.lib.atoma_linear_decode_fp8w(d.ptr, d.ptr, d.ptr, d.ptr, 65, 128, 16, 128, 128, 16, BF16, None) == -1
    assert "64" in gpu.last_error()


@pytest.mark.parametrize("B", [1, 8, 64])
def test_decode_step_over_fp8_weights_op_by_op(gpu, B):
    """DecodeStep(weight_dtype="fp8") against the restatement, op by op, and fused against unfused (wq_cases.check_decode_step_op_by_op)."""
    check_decode_step_op_by_op(gpu, B, "fp8", quantize_rows, linear_fp8w, "w8", "w8_scale")


def test_decode_step_over_fp8_weights_refuses_more_than_64_rows(gpu):
    import decode_step as DS
    cfg = DS.Config(layers=1, hidden=128, heads=1, kv_heads=1, head_dim=128, intermediate=128, vocab=128, page=16, max_pos=64)
    with pytest.raises(ValueError, match="64"):
        DS.DecodeStep(cfg, 65, 4, 1, {}, gpu.Stream(), weight_dtype="fp8")

"""fp8-weight projections (atoma_linear_decode_fp8w*, atoma_quantize_weight_fp8) without a GPU: the symbols, every argument check
(all fire before any launch), and the tests' own restatement (fp8w_ref) against torch on the CPU."""
import numpy as np
import pytest

import atoma_hip as ah
from atoma_hip import F16, BF16
from oracle import fp8_oracle as F8
from oracle.halfs import from_f32, to_f32
from fp8w_ref import quantize_rows, dequantize_rows, linear_fp8w
from util import rand_half

FAKE = 0x10000  # never dereferenced: every case fails its checks first
NAMES = ("atoma_quantize_weight_fp8", "atoma_linear_decode_fp8w", "atoma_linear_decode_fp8w_residual", "atoma_linear_decode_fp8w_silu_mul")


def test_the_four_entry_points_are_exported_and_bound():
    for name in NAMES:
        f = getattr(ah.lib, name)
        assert f.argtypes is not None, name


def plain(x=FAKE, w8=FAKE, sc=FAKE, y=FAKE, B=1, K=128, N=16, xs=None, ws=None, ys=None, dt=BF16):
    return ah.lib.atoma_linear_decode_fp8w(x, w8, sc, y, B, K, N, xs or K, ws or K, ys or N, dt, None)


def residual(res=FAKE, rs=None, B=1, K=128, N=16):
    return ah.lib.atoma_linear_decode_fp8w_residual(FAKE, FAKE, FAKE, res, FAKE, B, K, N, K, K, rs or N, N, BF16, None)


def silu(B=1, K=128, I=16, ys=None, ws=None):
    return ah.lib.atoma_linear_decode_fp8w_silu_mul(FAKE, FAKE, FAKE, FAKE, B, K, I, K, ws or K, ys or I, BF16, None)


def fails(rc, *words):
    assert rc == -1
    msg = ah.last_error()
    for w in words:
        assert w in msg, msg
    return msg


def test_linear_decode_fp8w_rejects_every_violated_precondition():
    fails(plain(dt=2), "linear_decode_fp8w", "dtype")
    fails(plain(B=65), "batch", "64")
    fails(plain(B=257), "batch", "64")
    fails(plain(B=-1), "batch")
    fails(plain(K=100), "in_features", "128")
    fails(plain(K=0), "in_features")
    fails(plain(N=24), "out_features", "16")
    fails(plain(N=0), "out_features")
    fails(plain(xs=64), "strides must cover")
    fails(plain(ws=64), "strides must cover")
    fails(plain(ys=8), "strides must cover")
    fails(plain(xs=132), "strides")
    fails(plain(ys=18), "strides")
    fails(plain(ws=136), "w8_row_stride", "16")
    fails(plain(x=FAKE + 8), "16-byte aligned")
    fails(plain(w8=FAKE + 8), "16-byte aligned")
    fails(plain(y=FAKE + 4), "8-byte aligned")
    fails(plain(sc=FAKE + 2), "w_scale", "4-byte")
    fails(plain(sc=None), "w_scale")
    assert plain(B=0) == 0                                       # nothing to do: no launch, no device needed
    assert plain(B=0, ws=144) == 0                               # a padded row stride is fine


def test_linear_decode_fp8w_epilogue_entries_check_their_own_arguments():
    fails(residual(res=None), "residual")
    fails(residual(res=FAKE + 4), "residual", "8-byte")
    fails(residual(rs=8), "residual")
    fails(residual(B=65), "batch", "64")
    assert residual(B=0) == 0
    fails(silu(I=24), "silu.up", "32")                          # 2 * 24 = 48: a multiple of 16, not of 32
    fails(silu(I=8), "silu.up", "32")
    fails(silu(B=65), "batch", "64")
    fails(silu(ys=8), "strides must cover")
    fails(silu(I=1 << 20, K=2048, ws=2048), "2 GiB")             # the up rows sit 2 GiB behind the gate rows: beyond a 32-bit buffer offset
    assert silu(B=0) == 0


def test_quantize_weight_fp8_rejects_bad_arguments():
    q = lambda w=FAKE, N=16, K=128, ws=None, dt=BF16, w8=FAKE, w8s=None, sc=FAKE: ah.lib.atoma_quantize_weight_fp8(w, N, K, ws or K, dt, w8, w8s or K, sc, None)
    fails(q(dt=2), "quantize_weight_fp8", "dtype")
    fails(q(N=-1), "out_features")
    fails(q(K=100), "in_features", "16")
    fails(q(ws=64), "strides must cover")
    fails(q(w8s=64), "strides must cover")
    fails(q(ws=132), "w_row_stride")
    fails(q(w8s=136), "w8_row_stride")
    fails(q(w=FAKE + 2), "16-byte aligned")
    fails(q(w8=FAKE + 8), "16-byte aligned")
    fails(q(sc=None), "scale_out")
    fails(q(sc=FAKE + 1), "scale_out")
    assert q(N=0) == 0


def _torch_bits(w, dtype):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(w).view(np.int16))
    return t.view(torch.bfloat16 if dtype == BF16 else torch.float16)


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_quantize_rows_is_the_clamped_torch_cast(dtype):
    """bytes == (w.float() * (1 / scale)).clamp(-448, 448).to(float8_e4m3fn); the clamp is part of the rule (torch's own cast does not
    saturate); decoding gives the same values as torch's."""
    import torch
    rng = np.random.default_rng(11)
    w = rand_half(rng, (48, 512), dtype, 512 ** -0.5)
    w[3] = 0                                                    # an all-zero row: scale 1
    w[5, 17] = from_f32(np.array([60000.0 if dtype == F16 else 3.0e38], np.float32), dtype)[0]   # one dominant outlier
    w[7, :4] = from_f32(np.array([1.0, -1.0, 0.5, 0.031], np.float32), dtype)
    w8, scale = quantize_rows(w, dtype)
    wt = _torch_bits(w, dtype).float()
    amax = wt.abs().amax(dim=1)
    st = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    assert st.dtype == torch.float32 and np.array_equal(st.numpy(), scale)
    assert scale[3] == 1.0 and (w8[3] == 0).all()
    q = (wt * (1.0 / st)[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn)
    assert np.array_equal(q.view(torch.uint8).numpy(), w8)
    assert np.array_equal(q.float().numpy(), F8.decode(w8))
    assert not ((w8 & 0x7F) == 0x7F).any()                      # no NaN byte
    assert (np.abs(F8.decode(w8)).max(axis=1)[[0, 5, 7]] == 448).all()   # the row maximum lands on the largest code
    # saturation, not NaN, beyond the range (what the clamp is for)
    assert np.array_equal(F8.encode(np.array([500.0, -1e9], np.float32)), np.array([0x7E, 0xFE], np.uint8))


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_linear_fp8w_restatement_against_torch(dtype):
    """the product of the restatement == torch's f64 matmul over the dequantised weights, rounded once."""
    import torch
    rng = np.random.default_rng(12)
    x, w = rand_half(rng, (5, 384), dtype), rand_half(rng, (32, 384), dtype, 384 ** -0.5)
    w8, scale = quantize_rows(w, dtype)
    wq = torch.from_numpy(w8).view(torch.float8_e4m3fn).double() * torch.from_numpy(scale).double()[:, None]
    assert np.array_equal(wq.numpy(), dequantize_rows(w8, scale))
    y = (_torch_bits(x, dtype).double() @ torch.from_numpy(w8).view(torch.float8_e4m3fn).double().T) * torch.from_numpy(scale).double()[None, :]
    ref = y.float().to(torch.bfloat16 if dtype == BF16 else torch.float16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(linear_fp8w(x, w8, scale, dtype), ref)

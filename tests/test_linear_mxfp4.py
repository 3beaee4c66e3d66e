"""MXFP4-weight projections (atoma_linear_decode_mxfp4*, atoma_quantize_weight_mxfp4) without a GPU: the symbols, every argument check
(all fire before any launch), and the tests' own restatement (mxfp4_ref) against the OCP tables, torch's e8m0 and its own round trip."""
import numpy as np
import pytest

import atoma_hip as ah
from atoma_hip import F16, BF16
from oracle.halfs import from_f32, to_f32
from mxfp4_ref import MAGNITUDES, quantize_blocks, dequantize, linear_mxfp4
from util import rand_half

FAKE = 0x10000  # never dereferenced: every case fails its checks first
NAMES = ("atoma_quantize_weight_mxfp4", "atoma_linear_decode_mxfp4", "atoma_linear_decode_mxfp4_residual", "atoma_linear_decode_mxfp4_silu_mul")


def test_the_four_entry_points_are_exported_and_bound():
    for name in NAMES:
        f = getattr(ah.lib, name)
        assert f.argtypes is not None, name


def plain(x=FAKE, w4=FAKE, sc=FAKE, y=FAKE, B=1, K=128, N=16, xs=None, ws=None, ss=None, ys=None, dt=BF16):
    return ah.lib.atoma_linear_decode_mxfp4(x, w4, sc, y, B, K, N, xs or K, ws or K // 2, ss or K // 32, ys or N, dt, None)


def residual(res=FAKE, rs=None, B=1, K=128, N=16, ss=None):
    return ah.lib.atoma_linear_decode_mxfp4_residual(FAKE, FAKE, FAKE, res, FAKE, B, K, N, K, K // 2, ss or K // 32, rs or N, N, BF16, None)


def silu(B=1, K=128, I=16, ys=None, ws=None, ss=None):
    return ah.lib.atoma_linear_decode_mxfp4_silu_mul(FAKE, FAKE, FAKE, FAKE, B, K, I, K, ws or K // 2, ss or K // 32, ys or I, BF16, None)


def fails(rc, *words):
    assert rc == -1
    msg = ah.last_error()
    for w in words:
        assert w in msg, msg
    return msg


def test_linear_decode_mxfp4_rejects_every_violated_precondition():
    fails(plain(dt=2), "linear_decode_mxfp4", "dtype")
    fails(plain(B=17), "linear_decode_mxfp4", "batch", "16")
    fails(plain(B=64), "batch", "16")
    fails(plain(B=-1), "batch")
    fails(plain(K=100, ws=64, ss=4), "in_features", "128")
    fails(plain(K=0, ws=64, ss=4), "in_features")
    fails(plain(N=24), "out_features", "16")
    fails(plain(xs=64), "strides must cover")
    fails(plain(ws=48), "strides must cover")                    # 48 bytes hold 96 inputs
    fails(plain(ss=3), "strides must cover", "scale_row_stride")
    fails(plain(K=256, ss=4), "strides must cover", "scale_row_stride")
    fails(plain(ys=8), "strides must cover")
    fails(plain(xs=132), "strides")
    fails(plain(ys=18), "strides")
    fails(plain(ws=72), "w4_row_stride", "16")
    fails(plain(ss=6), "scale_row_stride", "4")
    fails(plain(x=FAKE + 8), "16-byte aligned")
    fails(plain(w4=FAKE + 8), "16-byte aligned")
    fails(plain(y=FAKE + 4), "8-byte aligned")
    fails(plain(sc=FAKE + 2), "w_scale", "4-byte")
    fails(plain(sc=None), "w_scale")
    fails(plain(K=1 << 27, N=16, ws=1 << 26), "2 GiB")           # 32 rows of 64 MiB: beyond a 32-bit buffer offset
    assert plain(B=0) == 0                                       # nothing to do: no launch, no device needed
    assert plain(B=0, ws=80, ss=8) == 0                          # padded row strides are fine
    assert plain(N=0) == 0 and plain(N=0, B=16) == 0             # no output features: nothing to do either
    fails(plain(N=0, B=17), "batch", "16")                       # ... but the entry's own checks still fire
    fails(plain(N=0, ss=6), "scale_row_stride", "4")
    fails(plain(N=-16), "out_features")


def test_linear_decode_mxfp4_epilogue_entries_check_their_own_arguments():
    fails(residual(res=None), "linear_decode_mxfp4", "residual")
    fails(residual(res=FAKE + 4), "residual", "8-byte")
    fails(residual(rs=8), "residual")
    fails(residual(B=17), "batch", "16")
    fails(residual(ss=2), "scale_row_stride")
    assert residual(B=0) == 0 and residual(N=0) == 0
    fails(silu(I=24), "silu.up", "32")                          # 2 * 24 = 48: a multiple of 16, not of 32
    fails(silu(I=8), "silu.up", "32")
    fails(silu(B=17), "batch", "16")
    fails(silu(ys=8), "strides must cover")
    fails(silu(ss=5), "scale_row_stride", "4")
    fails(silu(I=1 << 20, K=4096, ws=2048), "2 GiB")             # the up rows sit 2 GiB behind the gate rows: beyond a 32-bit buffer offset
    assert silu(B=0) == 0 and silu(I=0) == 0


def test_quantize_weight_mxfp4_rejects_bad_arguments():
    def q(w=FAKE, N=16, K=128, ws=None, dt=BF16, w4=FAKE, w4s=None, sc=FAKE, ss=None):
        return ah.lib.atoma_quantize_weight_mxfp4(w, N, K, ws or K, dt, w4, w4s or K // 2, sc, ss or K // 32, None)
    fails(q(dt=2), "quantize_weight_mxfp4", "dtype")
    fails(q(N=-1), "out_features")
    fails(q(K=112, w4s=64, ss=4), "in_features", "32")
    fails(q(K=0, w4s=64, ss=4), "in_features")
    fails(q(ws=64), "strides must cover")
    fails(q(w4s=48), "strides must cover")
    fails(q(ss=3), "strides must cover")
    fails(q(ws=132), "w_row_stride")
    fails(q(w4s=72), "w4_row_stride")
    fails(q(w=FAKE + 2), "16-byte aligned")
    fails(q(w4=FAKE + 8), "16-byte aligned")
    fails(q(sc=None), "scale_out")
    assert q(N=0) == 0
    assert q(N=0, K=1056, ss=33) == 0                            # 33 scale bytes per row: no alignment is asked of the quantiser's scales


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------
# OCP Microscaling Formats (MX) v1.0, table "FP4 E2M1": S 00 0 = 0, S 00 1 = 0.5 (the subnormal), then 2^(E - 1) * (1 + M / 2)
OCP_E2M1 = {0b0000: 0.0, 0b0001: 0.5, 0b0010: 1.0, 0b0011: 1.5, 0b0100: 2.0, 0b0101: 3.0, 0b0110: 4.0, 0b0111: 6.0,
            0b1000: -0.0, 0b1001: -0.5, 0b1010: -1.0, 0b1011: -1.5, 0b1100: -2.0, 0b1101: -3.0, 0b1110: -4.0, 0b1111: -6.0}


def test_dequantize_is_the_ocp_e2m1_table_in_the_documented_nibble_order():
    codes = np.arange(16, dtype=np.uint8)
    w4 = np.zeros((1, 16), np.uint8)
    w4[0, :8] = codes[0::2] | (codes[1::2] << 4)                 # inputs 0..15 = codes 0..15: input 2i in the low nibble of byte i
    w4[0, 8:] = 0x21                                             # inputs 16, 18, ..: code 1 (low nibble); 17, 19, ..: code 2
    for s in (127, 120, 134):
        got = dequantize(w4, np.array([[s]], np.uint8))[0]
        assert np.array_equal(got[:16], np.array([OCP_E2M1[c] for c in range(16)]) * 2.0 ** (s - 127))
        assert np.array_equal(got[16:], np.tile([0.5, 1.0], 8) * 2.0 ** (s - 127))
    assert np.array_equal(MAGNITUDES, [OCP_E2M1[c] for c in range(8)])


def test_scale_bytes_mean_what_torch_e8m0_says():
    import torch
    s = np.arange(1, 255, dtype=np.uint8)                        # 0 (2^-127: a subnormal f32) and 255 (NaN) lie outside the defined range
    ref = torch.from_numpy(s).view(torch.float8_e8m0fnu).float().numpy().astype(np.float64)
    w4 = np.full((len(s), 16), 0x22, np.uint8)                   # every element 1.0: the value is the scale
    assert np.array_equal(dequantize(w4, s[:, None])[:, 0], ref)


def _blocks(dtype, values):
    """one row of whole blocks from f32 values (exact in dtype)"""
    bits = from_f32(np.asarray(values, np.float32), dtype)
    assert np.array_equal(to_f32(bits, dtype), np.asarray(values, np.float32))
    return bits.reshape(1, -1)


TIES = [(0.25, 0), (0.75, 2), (1.25, 2), (1.75, 4), (2.5, 4), (3.5, 6), (5.0, 6)]          # v -> code: ties go to the even code
NEAR = [(0.0, 0), (0.2, 0), (0.3, 1), (0.5, 1), (0.7, 1), (0.8, 2), (1.0, 2), (1.3, 3), (1.5, 3), (1.7, 3), (1.8, 4), (2.0, 4), (2.4, 4), (2.6, 5),
        (3.0, 5), (3.4, 5), (3.6, 6), (4.0, 6), (4.9, 6), (5.1, 7), (6.0, 7), (7.0, 7)]


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_every_tie_and_the_saturation_land_as_the_table_says(dtype):
    """a block with amax 7.5 (e = 0: v is the value itself) holding every tie value, in both signs"""
    vals = [7.5] + [v for v, _ in TIES] + [-v for v, _ in TIES] + [7.0, -7.0, 5.5, -5.5, 6.0, -6.0]
    vals += [0.0] * (32 - len(vals))
    w4, sc = quantize_blocks(_blocks(dtype, vals), dtype)
    assert sc[0, 0] == 127
    code = np.stack([w4[0] & 0xF, w4[0] >> 4], 1).reshape(-1)
    want = [7] + [c for _, c in TIES] + [c | 8 for _, c in TIES] + [7, 15, 7, 15, 7, 15]
    assert list(code[:len(want)]) == want and (code[len(want):] == 0).all()
    # the thresholds are the nearest magnitude, ties to the even code, for any v (brute force)
    from mxfp4_ref import codes_of
    v = np.concatenate([np.linspace(0, 8, 4097), [t for t, _ in TIES]]).astype(np.float32)
    d = np.abs(v[:, None].astype(np.float64) - MAGNITUDES[None, :])
    best = d.min(axis=1, keepdims=True)
    cand = [np.flatnonzero(row == b) for row, b in zip(d, best[:, 0])]
    brute = np.array([c[0] if len(c) == 1 else [x for x in c if x % 2 == 0][0] for c in cand])
    assert np.array_equal(codes_of(v), brute)
    for x, c in NEAR:
        assert codes_of(np.float32(x)) == c, x


def test_the_exponent_clamp_keeps_half_a_scale_normal():
    """an f16 block of 1e-7 (a subnormal: f32 exponent -24): e = -26 is raised to -13, byte 114, v = 2^-10 -> all codes zero"""
    w4, sc = quantize_blocks(from_f32(np.full((1, 32), 1e-7, np.float32), F16), F16)
    assert sc[0, 0] == 114 and (w4 == 0).all()
    w4, sc = quantize_blocks(from_f32(np.full((1, 32), -1e-7, np.float32), F16), F16)
    assert sc[0, 0] == 114 and (w4 == 0x88).all()                # the sign bit is the source's
    w4, sc = quantize_blocks(np.full((1, 32), 0x0001, np.uint16), BF16)   # the smallest bf16 subnormal, 2^-133
    assert sc[0, 0] == 2 and (w4 == 0).all()
    w4, sc = quantize_blocks(np.full((1, 32), 0x0040, np.uint16), BF16)   # 2^-127: v = 2^-127 * 2^125 = 0.25 -> 0; 0x0060 = 1.5 * 2^-127 -> 0.375 -> 1
    assert sc[0, 0] == 2 and (w4 == 0).all()
    assert (quantize_blocks(np.full((1, 32), 0x0060, np.uint16), BF16)[0] == 0x11).all()
    w4, sc = quantize_blocks(np.zeros((1, 32), np.uint16), BF16)
    assert sc[0, 0] == 127 and (w4 == 0).all()


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_dequantised_weights_are_exact_in_the_dtype_and_requantise_to_the_same_bytes(dtype):
    rng = np.random.default_rng(31)
    K = 1056
    w = rand_half(rng, (48, K), dtype, K ** -0.5)
    w[3, 64:96] = 0                                              # an all-zero block
    w[5, 17] = 0x7BFF if dtype == F16 else 0x7F7F                # the dtype's largest finite value
    w[7, 40] = from_f32(np.array([1000.0], np.float32), dtype)[0]            # one dominant outlier
    w4, sc = quantize_blocks(w, dtype)
    assert w4.shape == (48, K // 2) and sc.shape == (48, K // 32) and sc[3, 2] == 127 and (w4[3, 32:48] == 0).all()
    deq = dequantize(w4, sc)
    bits = from_f32(deq.astype(np.float32), dtype)
    assert np.array_equal(to_f32(bits, dtype).astype(np.float64), deq)      # exact in T
    nz = deq[deq != 0]
    tiny = 2.0 ** -126 if dtype == BF16 else 2.0 ** -14
    assert np.isfinite(nz).all() and (np.abs(nz) >= tiny).all()              # ... and finite normal numbers: the defined range
    w4b, scb = quantize_blocks(bits, dtype)
    assert np.array_equal(w4b, w4)
    code = np.stack([w4 & 0xF, w4 >> 4], 2).reshape(48, K // 32, 32)
    live = ((code & 7) != 0).any(axis=2)                         # all-zero-code blocks come back with byte 127
    assert np.array_equal(scb[live], sc[live]) and (scb[~live] == 127).all()
    # relative rms error of round-to-nearest MXFP4 on Gaussian weights: ~11 %
    wf = to_f32(w, dtype).astype(np.float64)
    wf[5, 17] = wf[7, 40] = 0
    deq[5, 17] = deq[7, 40] = 0
    assert 0.05 < np.sqrt(((deq - wf) ** 2).sum() / (wf ** 2).sum()) < 0.2


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_linear_mxfp4_restatement_against_torch(dtype):
    """the product of the restatement == torch's f64 matmul over the dequantised weights, rounded once."""
    import torch
    rng = np.random.default_rng(12)
    x, w = rand_half(rng, (5, 384), dtype), rand_half(rng, (32, 384), dtype, 384 ** -0.5)
    w4, sc = quantize_blocks(w, dtype)
    tdt = torch.bfloat16 if dtype == BF16 else torch.float16
    xt = torch.from_numpy(np.ascontiguousarray(x).view(np.int16)).view(tdt).double()
    y = xt @ torch.from_numpy(dequantize(w4, sc)).T
    ref = y.float().to(tdt).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(linear_mxfp4(x, w4, sc, dtype), ref)

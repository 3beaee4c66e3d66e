"""CPU restatement of the MXFP4-weight ("W4A16") projections for the tests (test infrastructure only): the block quantiser and the product,
in numpy.

The format: w4 ``[N, K / 2]`` bytes, byte i of a row = input 2i in the low nibble, input 2i + 1 in the high nibble; bit 3 of a nibble is the
sign, bits 0..2 index MAGNITUDES.  scale ``[N, K / 32]`` bytes, e8m0: byte s means 2^(s - 127) for inputs 32j .. 32j + 31.

quantize_blocks states atoma_quantize_weight_mxfp4's arithmetic: per row and block amax = max |f32(w)|; scale byte 127 when amax == 0, else
e + 127 with e = (f32 exponent of amax) - 2 raised to at least -125 (bf16) / -13 (f16); per element v = |f32(w)| * 2^-e (exact) and the code
from the threshold table (nearest magnitude, ties to the even code, saturating at 6); the sign bit is the source's sign bit.
linear_mxfp4 is the exactly accumulated product (f64), rounded once to the storage dtype -- what oracle.linear_oracle.linear is for 16-bit
weights; an fp32-accumulating kernel may differ from it by one unit in the last place."""
import numpy as np

from oracle.halfs import BF16, from_f32, to_f32

MAGNITUDES = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def codes_of(v):
    """v >= 0 (f32, already divided by the block scale) -> the code 0..7 of the threshold table."""
    v = np.asarray(v, np.float32)
    code = np.full(v.shape, 7, np.uint8)
    for c, (bound, strict) in reversed(list(enumerate([(0.25, False), (0.75, True), (1.25, False), (1.75, True), (2.5, False), (3.5, True), (5.0, False)]))):
        code[(v < bound) if strict else (v <= bound)] = c
    return code


def quantize_blocks(w, dtype):
    """w ``[N, K]`` storage-form (uint16), K % 32 == 0 -> (w4 ``[N, K / 2]`` uint8, scale ``[N, K / 32]`` uint8)."""
    w = np.asarray(w, np.uint16)
    N, K = w.shape
    assert K % 32 == 0
    wf = np.abs(to_f32(w, dtype).astype(np.float32)).reshape(N, K // 32, 32)
    amax = wf.max(axis=2)
    e = ((amax.view(np.uint32) >> 23) & 0xFF).astype(np.int32) - 127 - 2
    e = np.maximum(e, -125 if dtype == BF16 else -13)       # 0.5 * 2^e stays a normal number of the dtype
    e = np.where(amax > 0, e, 0)
    inv = ((127 - e).astype(np.uint32) << 23).view(np.float32)   # 2^-e
    v = (wf * inv[:, :, None]).astype(np.float32)                # exact: a power of two
    code = codes_of(v).reshape(N, K) | ((w >> 12) & 8).astype(np.uint8)
    w4 = (code[:, 0::2] | (code[:, 1::2] << 4)).astype(np.uint8)
    return w4, (e + 127).astype(np.uint8)


def dequantize(w4, scale):
    """The weights' values e2m1(nibble) * 2^(scale - 127) as float64 ``[N, K]`` (exact)."""
    w4, scale = np.asarray(w4, np.uint8), np.asarray(scale, np.uint8)
    N, half = w4.shape
    code = np.empty((N, 2 * half), np.uint8)
    code[:, 0::2], code[:, 1::2] = w4 & 0xF, w4 >> 4
    val = MAGNITUDES[code & 7] * np.where(code & 8, -1.0, 1.0)
    return val * np.repeat(np.ldexp(1.0, scale.astype(np.int32) - 127), 32, axis=1)


def linear_mxfp4(x, w4, scale, dtype):
    """x ``[B, K]`` storage-form, w4 ``[N, K / 2]``, scale ``[N, K / 32]`` -> y ``[B, N]`` storage-form."""
    y = to_f32(x, dtype).astype(np.float64) @ dequantize(w4, scale).T
    return from_f32(y.astype(np.float32), dtype)

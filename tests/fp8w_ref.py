"""CPU restatement of the fp8-weight ("W8A16") projections for the tests (test infrastructure only): the per-row quantiser and the
product, built from oracle.fp8_oracle.encode / decode, oracle.halfs and numpy f64.

quantize_rows states atoma_quantize_weight_fp8's arithmetic: per output row amax = max |f32(w)|, scale = amax / 448 in f32 (1.0 for an
all-zero row), byte = e4m3fn(clamp(f32(w) * (f32(1) / scale), -448, 448)), round to nearest even, saturating.
linear_fp8w is the exactly accumulated product (f64) times the scale, rounded once to the storage dtype -- what oracle.linear_oracle.linear
is for 16-bit weights; an fp32-accumulating kernel may differ from it by one unit in the last place."""
import numpy as np

from oracle import fp8_oracle as F8
from oracle.halfs import from_f32, to_f32


def quantize_rows(w, dtype):
    """w ``[N, K]`` storage-form (uint16) -> (w8 ``[N, K]`` uint8, scale ``[N]`` float32)."""
    wf = to_f32(w, dtype)
    amax = np.abs(wf).max(axis=1).astype(np.float32)
    scale = np.where(amax > 0, amax / np.float32(448), np.float32(1)).astype(np.float32)
    inv = (np.float32(1) / scale).astype(np.float32)
    return F8.encode((wf * inv[:, None]).astype(np.float32)), scale


def dequantize_rows(w8, scale):
    """The weights' values e4m3(w8[n][k]) * scale[n] as float64 (exact)."""
    return F8.decode(w8).astype(np.float64) * np.asarray(scale, np.float32).astype(np.float64)[:, None]


def linear_fp8w(x, w8, scale, dtype):
    """x ``[B, K]`` storage-form, w8 ``[N, K]`` uint8, scale ``[N]`` f32 -> y ``[B, N]`` storage-form."""
    y = to_f32(x, dtype).astype(np.float64) @ F8.decode(w8).astype(np.float64).T
    y = y * np.asarray(scale, np.float32).astype(np.float64)[None, :]
    return from_f32(y.astype(np.float32), dtype)

"""FP8 (OCP e4m3fn) weight-only quantisation with per-output-row
power-of-two scales: the model-build transform and the encoder / decoder
the fp8 weight packs (ops/hip.py) are made with.

Pure torch on any device.  The torch float8 dtype is not used, so the same
code runs where a device has no cast kernel for it; tests/w8_oracle.py
holds it to an independent decode table.
"""
import torch

FP8_MAX = 448.0


def fp8_row_exponents(w):
    """e[n] = ceil(log2(absmax_n / 448)) as int32, by frexp (a float log2
    is off by one when absmax / 448 is an exact power of two):
    absmax = m * 2^x with m in [0.5, 1) and 448 = 0.875 * 2^9, so the
    ratio is (m / 0.875) * 2^(x - 9) and e = x - 9 + (m > 0.875).
    An all-zero row gets e = 0 (scale 1)."""
    amax = w.float().abs().amax(dim=1)
    m, x = torch.frexp(amax)
    e = x.to(torch.int32) - 9 + (m > 0.875).to(torch.int32)
    return torch.where(amax > 0, e, torch.zeros_like(e))


def e4m3_round(u):
    """Round fp32 |u| <= 448 to the nearest e4m3fn value, ties to even;
    returns fp32.  Normal range (>= 2^-6): round the fp32 mantissa to 3
    bits in integer arithmetic; below it the grid is uniform, 2^-9."""
    bits = u.view(torch.int32)
    rne = (bits + 0x7FFFF + ((bits >> 20) & 1)) & ~0xFFFFF
    normal = rne.view(torch.float32)
    sub = torch.round(u * 512.0) / 512.0          # half to even
    return torch.where(u.abs() < 2.0 ** -6, sub, normal)


def e4m3_encode(v):
    """fp32 values that ARE e4m3fn values -> uint8 codes (sign, 4-bit
    exponent biased 7, 3-bit mantissa); -0.0 keeps its sign."""
    bits = v.view(torch.int32)
    sign = (bits >> 24) & 0x80
    a = v.abs()
    e4 = ((bits >> 23) & 0xFF) - 120               # - 127 + 7
    normal = (e4 << 3) | ((bits >> 20) & 7)
    sub = (a * 512.0).to(torch.int32)              # 0..8; 8 is code 0x08
    return (sign | torch.where(a < 2.0 ** -6, sub, normal)).to(torch.uint8)


def e4m3_decode(codes):
    """uint8 e4m3fn codes -> fp32 (finite codes only)."""
    c = codes.to(torch.int32)
    e4, m3 = (c >> 3) & 15, c & 7
    mag = torch.where(
        e4 == 0, m3.float() * 2.0 ** -9,
        torch.ldexp(1.0 + m3.float() / 8.0, e4 - 7))
    return torch.where((c & 0x80) != 0, -mag, mag)


def quantize_fp8(w):
    """[N, K] -> (codes uint8 [N, K], e int32 [N], dq [N, K] in w.dtype):
    q = e4m3(clamp(w / 2^e, +-448)), dq = q * 2^e.  The scale is a power of
    two and a code has 4 significant bits, so dq is exact in bf16.  The NaN
    codes 0x7f / 0xff are never produced (|q| <= 448 = 0x7e)."""
    e = fp8_row_exponents(w)
    scale = torch.ldexp(torch.ones_like(e, dtype=torch.float32), e)
    u = (w.float() / scale.unsqueeze(1)).clamp(-FP8_MAX, FP8_MAX)
    q = e4m3_round(u)
    dq = (q * scale.unsqueeze(1)).to(w.dtype)
    return e4m3_encode(q), e, dq


def dequantize_fp8_weight(w):
    """The model-build transform: w replaced by its fp8-dequantised values
    (same shape and dtype)."""
    return quantize_fp8(w)[2]

"""Independent yardstick for the FP8 (OCP e4m3fn) weight-only path
(tests/test_w8_oracle_cpu.py proves it and holds ops/quant.py and the fp8
packs to it on the CPU; tests/test_w8_gemm_gpu.py and
tests/test_w8_model_gpu.py apply it to the HIP kernels and the model).

Nothing here uses the project's quantiser.  The decode table is built from
the bit fields of the format; the reference quantiser rounds with torch's
own float8 cast (checked against the table on every finite code) and takes
the row exponent from exact ldexp comparisons.
"""
import math

import torch

import fused_oracle as fo

FP8_MAX = 448.0
NAN_CODES = (0x7F, 0xFF)


def _decode_one(c):
    """e4m3fn: 1 sign, 4 exponent (bias 7), 3 mantissa bits; exponent 0 is
    subnormal (m / 8 * 2^-6); S.1111.111 is NaN, there are no infinities."""
    s, e, m = c >> 7, (c >> 3) & 15, c & 7
    if e == 15 and m == 7:
        return float("nan")
    mag = m / 8.0 * 2.0 ** -6 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 7)
    return -mag if s else mag


# float64 [256]; entries 0x7f and 0xff are NaN
TABLE = torch.tensor([_decode_one(c) for c in range(256)],
                     dtype=torch.float64)
FINITE = [c for c in range(256) if c not in NAN_CODES]


def decode(codes):
    """uint8 codes -> float64 values through the table."""
    return TABLE[codes.long()]


def row_exponent(amax):
    """ceil(log2(amax / 448)) of one row maximum (a Python float), found
    with exact power-of-two comparisons: the smallest e with
    amax <= 448 * 2^e.  An all-zero row gets 0."""
    if amax == 0.0:
        return 0
    e = math.frexp(amax)[1] - 9
    while amax > math.ldexp(FP8_MAX, e):
        e += 1
    while amax <= math.ldexp(FP8_MAX, e - 1):
        e -= 1
    return e


def quantize_ref(w):
    """Reference quantiser of a CPU [N, K] matrix -> (codes uint8 [N, K],
    e int32 [N], dq in w.dtype).  dq is table[codes] * 2^e computed in
    float64 and must survive the cast to w.dtype unchanged."""
    wd = w.detach().cpu().double()
    e = torch.tensor([row_exponent(float(a)) for a in wd.abs().amax(1)],
                     dtype=torch.int32)
    scale = torch.ldexp(torch.ones(len(e), dtype=torch.float64), e)
    u = (wd / scale.unsqueeze(1)).clamp(-FP8_MAX, FP8_MAX)
    codes = u.float().to(torch.float8_e4m3fn).view(torch.uint8)
    dq64 = decode(codes) * scale.unsqueeze(1)
    dq = dq64.to(w.dtype)
    assert torch.equal(dq.double(), dq64), "dq is not exact in w.dtype"
    return codes, e, dq


def scales(e):
    """fp32 2^e."""
    return torch.ldexp(torch.ones(len(e), dtype=torch.float32), e)


# ---------------------------------------------------------------------------
# inputs


def normal(N, K, s=None, seed=0):
    """N(0, s) bf16 weights; s defaults to 1 / sqrt(K)."""
    return fo.rand_bf16(N, K, scale=K ** -0.5 if s is None else s, seed=seed)


def wide_rows(N, K, seed=0):
    """Rows spanning 2^-20 .. 2^20 in magnitude, one all-zero row (row 1)
    and one row (row 2) whose absmax / 448 is an exact power of two."""
    w = torch.randn(N, K, generator=torch.Generator().manual_seed(seed))
    ex = torch.linspace(-20, 20, N).round()
    w = w * torch.ldexp(torch.ones(N), ex.int()).unsqueeze(1)
    w[1] = 0.0
    w[2] = w[2].clamp(-1.0, 1.0) * 2.0 ** -4
    w[2, K // 2] = -448.0 * 2.0 ** -5
    return w.bfloat16()


def all_codes_weight(N=32, K=256):
    """(codes [N, K], e [N], dq bf16): row n holds the 254 finite codes and
    two zeros, rotated by n; row scale 2^(n % 9 - 4)."""
    base = torch.tensor(FINITE + [0, 0], dtype=torch.uint8)
    assert base.numel() == K
    codes = torch.stack([base.roll(n) for n in range(N)])
    e = torch.tensor([n % 9 - 4 for n in range(N)], dtype=torch.int32)
    dq64 = decode(codes) * torch.ldexp(torch.ones(N, dtype=torch.float64),
                                       e).unsqueeze(1)
    dq = dq64.bfloat16()
    assert torch.equal(dq.double(), dq64)
    return codes, e, dq


def ternary_scaled(N, K, seed=0):
    """Ternary W with row n multiplied by 2^(n % 7 - 3): a scale read in
    natural instead of pack order, or gate for up, moves a result by a
    factor of two or more."""
    w = fo.ternary(N, K, seed=seed).float()
    mul = torch.ldexp(torch.ones(N), torch.arange(N, dtype=torch.int32) % 7
                      - 3)
    return (w * mul.unsqueeze(1)).bfloat16()

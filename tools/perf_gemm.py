"""Microbench: weight-streaming packed GEMM vs hipBLASLt on the 8B decode
shapes, with a ksplit x prefetch-depth sweep and a pure-stream arm (same
grid/addressing, loads only) that shows each geometry's load-path ceiling.

Run on a GPU box: python tools/perf_gemm.py [M] [--sweep]
                  python tools/perf_gemm.py [M] --fp8 [--repeat R]

--fp8: the same shapes, cold, with the fp8 (e4m3) pack next to the bf16
pack of the same dequantised weights: the pure-stream ceiling of each
geometry and the kernel through the direct (d1), LDS-staged (xl) and
frag-input (fr, what the fused chain runs) activation paths; R repeats,
printed as median (min..max) microseconds.

COLD-weight protocol: cycles enough weight copies that the 256 MiB L3
never serves a re-read (the serving loop streams weights from HBM once
per step; r01's fragment-direct kernel won warm and lost cold)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
from ollamamq_amd.ops import hip


def bench(fn, args, ncopy, n=50):
    for i in range(5):
        fn(args[i % ncopy])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        fn(args[i % ncopy])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


SHAPES = [("qkv", 6144, 4096), ("o", 4096, 4096),
          ("gate_up", 28672, 4096), ("down", 4096, 14336),
          ("logits", 128256, 4096)]


def _to_frag(x):
    """[M <= 32, K] -> the 32-row frag buffer (common.cuh)."""
    M, K = x.shape
    buf = torch.zeros(32, K, dtype=x.dtype, device=x.device)
    buf[:M] = x
    return buf.reshape(32, K // 64, 4, 2, 8).permute(1, 2, 3, 0, 4) \
              .contiguous().view(-1)


def main_fp8(M, repeat):
    assert M <= 32
    for name, N, K in SHAPES:
        x = torch.randn(M, K).bfloat16().cuda()
        xf = _to_frag(x)
        ncopy = max(2, (600 << 20) // (N * K) + 1)
        p8, p16 = [], []
        for _ in range(ncopy):
            w = (torch.randn(N, K, device="cuda") * K ** -0.5).bfloat16()
            pk = hip.pack_weight_fp8(w)
            p8.append(pk)
            p16.append(hip.pack_weight(hip.unpack_weight_fp8(pk, N, K)))
            del w
        ks = hip._wstream_ksplit(N, K)
        arms = [("pure", lambda p: hip.wstream_pure(p, N, K, ks)),
                ("d1", lambda p: hip.linear_packed(x, p, None, N, ks=ks,
                                                   depth=1, xlds=0)),
                ("xl", lambda p: hip.linear_packed(x, p, None, N, ks=ks,
                                                   depth=1, xlds=1)),
                ("fr", lambda p: hip.linear_packed(xf, p, None, N, ks=ks,
                                                   depth=1, xlds=2, K=K,
                                                   M_frag=M))]
        print(f"{name:8s} N={N:6d} K={K:6d} M={M} ks={ks} "
              f"({ncopy} cold copies)")
        for tag, fn in arms:
            line = f"    {tag:4s}"
            for fmt, packs, nbytes in (("bf16", p16, N * K * 2),
                                       ("fp8", p8, N * K)):
                ts = sorted(bench(fn, packs, ncopy) for _ in range(repeat))
                med = ts[len(ts) // 2]
                line += (f" | {fmt} {med*1e6:7.1f}us ({ts[0]*1e6:.1f}.."
                         f"{ts[-1]*1e6:.1f}) {nbytes/med/1e12:5.2f}TB/s")
            print(line, flush=True)
        del p8, p16
        torch.cuda.empty_cache()


def main():
    hip.require()
    M = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() \
        else 32
    sweep = "--sweep" in sys.argv
    if "--fp8" in sys.argv:
        repeat = int(sys.argv[sys.argv.index("--repeat") + 1]) \
            if "--repeat" in sys.argv else 3
        return main_fp8(M, repeat)
    shapes = SHAPES
    for name, N, K in shapes:
        x = torch.randn(M, K).bfloat16().cuda()
        ncopy = max(2, (600 << 20) // (N * K * 2) + 1)
        ws = [torch.randn(N, K).bfloat16().cuda() for _ in range(ncopy)]
        pks = [hip.pack_weight(w) for w in ws]
        wb = N * K * 2

        t_lib = bench(lambda w: torch.nn.functional.linear(x, w), ws,
                      ncopy)
        print(f"{name:8s} N={N:6d} K={K:6d}: lib {t_lib*1e6:7.1f}us "
              f"{wb/t_lib/1e12:5.2f}TB/s")
        ks_list = ([1, 2, 4, 8] if sweep
                   else [hip._wstream_ksplit(N, K)])
        for ks in ks_list:
            if (K // 64) // (ks * 8) < 1:
                continue
            t_pure = bench(lambda p, k=ks: hip.wstream_pure(p, N, K, k),
                           pks, ncopy)
            line = (f"    ks={ks}: pure {t_pure*1e6:7.1f}us "
                    f"{wb/t_pure/1e12:5.2f}TB/s")
            for tag, kw in (("d1", dict(depth=1, xlds=0)),
                            ("xl", dict(depth=1, xlds=1))):
                t = bench(lambda p, k=ks, kw=kw:
                          hip.linear_packed(x, p, None, N, ks=k, **kw),
                          pks, ncopy)
                line += (f" | {tag} {t*1e6:7.1f}us "
                         f"{wb/t/1e12:5.2f}TB/s")
            print(line, flush=True)
        del ws, pks
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

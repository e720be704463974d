"""Microbench: decode attention old (unsplit) vs flash-decoding path
(two-kernel split and block-split).

Run on a GPU box:  python tools/perf_decode.py [ctx] [batch] [--kv fp8]

--kv fp8 adds the same two paths over an e4m3 KV cache of the same geometry
(ops/quant.py kv_fp8_encode of the bf16 pools), in the same run; TB/s counts
the bytes each format really reads.  Every line is the median of three
repeats with min..max.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from ollamamq_amd.engine.kvcache import PagedKVCache
from ollamamq_amd.ops.interface import AttnMeta
from ollamamq_amd.ops import hip


def main():
    hip.require()
    kv8 = "--kv" in sys.argv and sys.argv[sys.argv.index("--kv") + 1] == "fp8"
    if "--kv" in sys.argv:
        del sys.argv[sys.argv.index("--kv"):sys.argv.index("--kv") + 2]
    ctx = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    Hq_arg = int(sys.argv[3]) if len(sys.argv) > 3 else 32
    KVH_arg = int(sys.argv[4]) if len(sys.argv) > 4 else 8
    # 8 layers cycled per call: the working set (8 × B×KVH×ctx×512B) blows
    # past the 256 MiB L3 like the real 32-layer model does — timing one
    # resident layer would measure L3, not HBM (the perf_gemm.py lesson)
    Hq, KVH, D, L = Hq_arg, KVH_arg, 128, 8
    dev = "cuda"
    n_pages = B * (ctx // 16 + 2)
    cache = PagedKVCache(L, KVH, D, page_size=16, n_pages=n_pages,
                         max_slots=B, max_ctx=ctx + 64, device=dev,
                         dtype=torch.bfloat16)
    for i in range(B):
        s = cache.alloc_slot()
        cache.ensure(s, ctx)
    cache.k_pool.normal_()
    cache.v_pool.normal_()
    q = torch.randn(B, Hq, D, device=dev).bfloat16()
    meta = AttnMeta(
        mode="decode",
        slot_ids=torch.arange(B, dtype=torch.int32, device=dev),
        seq_lens=torch.full((B,), ctx, dtype=torch.int32, device=dev),
        cu_q=torch.arange(B + 1, dtype=torch.int32, device=dev),
        logits_idx=None, max_q=1, max_kv=ctx)

    kv_bytes = B * KVH * ctx * D * 2 * 2

    def bench(fn, label, nbytes=kv_bytes):
        for _ in range(5):
            out = fn(0)
        ts = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 64
            for i in range(n):
                out = fn(i % L)     # cycle layers: cold KV every call
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / n)
        ts.sort()
        print(f"{label}: {ts[1]*1e6:8.1f} us ({ts[0]*1e6:.1f}..{ts[2]*1e6:.1f})"
              f"  {nbytes/ts[1]/1e12:6.2f} TB/s")
        return out

    def path(blk):
        os.environ["OLLAMAMQ_DECODE_BLOCKSPLIT"] = "1" if blk else "0"
        return lambda l: hip.attention_decode(q, cache, l, meta)

    o_new = bench(path(False), "split ")
    G = Hq // KVH
    split = min(max(1, 1024 // (B * KVH)), (ctx + 63) // 64, 32)
    if hip.decode_blocksplit(B, KVH, G, hip._decode_chunk(G), split,
                             {"OLLAMAMQ_DECODE_BLOCKSPLIT": "1"}):
        o_blk = bench(path(True), "block ")
        assert torch.equal(o_blk, o_new), "block path differs from split"
    else:
        print(f"block : not instantiated for G={G} split={split}")
    if kv8:
        from ollamamq_amd.ops.quant import kv_fp8_encode
        c8 = PagedKVCache(L, KVH, D, page_size=16, n_pages=n_pages,
                          max_slots=B, max_ctx=ctx + 64, device=dev,
                          kv_quant="fp8")
        c8.page_table.copy_(cache.page_table)
        for l in range(L):      # per layer: the fp32 temporaries are large
            c8.k_pool[l] = kv_fp8_encode(cache.k_pool[l])
            c8.v_pool[l] = kv_fp8_encode(cache.v_pool[l])
        for blk, label in ((False, "split8"), (True, "block8")):
            os.environ["OLLAMAMQ_DECODE_BLOCKSPLIT"] = "1" if blk else "0"
            bench(lambda l: hip.attention_decode(q, c8, l, meta), label,
                  kv_bytes // 2)
    os.environ["OLLAMAMQ_DECODE_BLOCKSPLIT"] = "0"
    for sp in (1, 2, 4, 8):
        bench(lambda l, sp=sp: hip.decode_pure(cache, l, meta, sp),
              f"pure{sp}")
    o_old = bench(lambda l: hip._attention(q, cache, l, meta, 1), "legacy")
    diff = (o_new.float() - o_old.float()).abs().max().item()
    print("max |new-old| =", diff)
    assert diff < 3e-2, "split path disagrees with legacy"


if __name__ == "__main__":
    main()

"""Split the decode step into GPU time vs host overhead.

Runs the 8B engine to steady state, then times (a) full engine.step()
iterations and (b) bare graph replays of the same captured step — the gap
is Python/host bookkeeping that the GPU waits on.

  python tools/perf_step.py [model] [users] [--penalty]

--penalty measures the same step a second time in the same process with
every row at repeat_penalty 1.1, repeat_last_n 64 (the penalised graph:
the logit-penalty kernel between the forward and the sampling tail) and
prints the difference.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
from ollamamq_amd.models import LlamaModel, PRESETS
from ollamamq_amd.engine import LlamaEngine, PagedKVCache, GenParams


def measure(eng, cfg, users, label, n=30, **pen):
    g = torch.Generator().manual_seed(3)
    for _ in range(users):
        eng.submit(torch.randint(0, cfg.vocab, (512,), generator=g).tolist(),
                   GenParams(max_tokens=10 ** 9, **pen))
    guard = 0
    while eng.waiting and guard < 1000:
        eng.step()
        guard += 1
    for _ in range(5):
        eng.step()
    torch.cuda.synchronize()

    t0 = time.perf_counter()
    for _ in range(n):
        eng.step()
    torch.cuda.synchronize()
    full = (time.perf_counter() - t0) / n

    key = (eng._bucket(users), 0) + ((1,) if pen else ())
    entry = eng._graphs.get(key)
    assert entry is not None and entry["graph"] is not None, \
        (key, sorted(eng._graphs))
    # the bare replays append n more tokens per row: their pages first
    for s in eng.running:
        eng.kv.ensure(s.slot, eng.kv.seq_lens[s.slot] + n + 1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        entry["graph"].replay()
    torch.cuda.synchronize()
    replay = (time.perf_counter() - t0) / n

    # sampler-only cost (argmax + tolist sync); the entry's logits are
    # penalised already where they are penalised at all
    logits = entry["logits"][:users]
    t0 = time.perf_counter()
    for _ in range(n):
        eng._sample(eng.running, logits, penalized=True)
    torch.cuda.synchronize()
    sample = (time.perf_counter() - t0) / n

    print(f"[{label}] full step : {full*1e3:7.3f} ms")
    print(f"[{label}] graph GPU : {replay*1e3:7.3f} ms")
    print(f"[{label}] sample+sync:{sample*1e3:7.3f} ms")
    print(f"[{label}] host gap  : {(full-replay-sample)*1e3:7.3f} ms")
    # the bare replays ran the device ahead of the host: drop the batch
    for s in list(eng.running):
        eng.cancel(s.seq_id)
    eng.step()
    torch.cuda.synchronize()
    return full, replay


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    penalty = "--penalty" in sys.argv[1:]
    model_name = args[0] if args else "llama3-8b"
    users = int(args[1]) if len(args) > 1 else 32
    cfg = PRESETS[model_name]
    dev = "cuda"
    n_pages = (users + 2) * ((512 + 200 + 15) // 16 + 2)
    model = LlamaModel(cfg, device=dev, dtype=torch.bfloat16, seed=1,
                       fast_init=True)
    kv = PagedKVCache.for_model(cfg, n_pages=n_pages, max_slots=users + 2,
                                max_ctx=1024, device=dev,
                                dtype=torch.bfloat16)
    eng = LlamaEngine(model, kv, max_batch=users)
    full, replay = measure(eng, cfg, users, "plain")
    if penalty:
        pfull, preplay = measure(eng, cfg, users, "penalty",
                                 repeat_penalty=1.1, repeat_last_n=64)
        print(f"penalised - plain: full step {(pfull - full)*1e6:+8.1f} us, "
              f"graph GPU {(preplay - replay)*1e6:+8.1f} us")


if __name__ == "__main__":
    main()

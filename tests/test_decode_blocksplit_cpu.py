"""The rule that sends attention_decode down the block-split path
(k_decode_attn_blk: one block per (sequence, kv-head), segments merged
through LDS) is a pure function; no GPU needed."""
from ollamamq_amd.ops.hip import decode_blocksplit, _BLK_INSTANCES

# the benchmark: Llama-3-8B, 32 users -> S 32, KVH 8, G 4, chunk 64, split 4
BENCH = dict(S=32, KVH=8, G=4, chunk=64, split=4)


def _rule(env=None, **kw):
    return decode_blocksplit(**{**BENCH, **kw}, env=env or {})


def test_bench_shape_takes_the_block_path():
    assert _rule()
    assert _rule(S=16)                       # 16 * 8 = 128: the floor itself


def test_few_blocks_keep_the_old_path():
    assert not _rule(S=15)                   # 120 < 128
    assert not _rule(S=32, KVH=2)


def test_split_1_keeps_the_old_path():
    assert not _rule(split=1)


def test_uninstantiated_pairs_keep_the_old_path():
    assert not _rule(G=7, split=4)           # 28 waves
    assert not _rule(G=5, split=4)
    assert not _rule(split=3)
    assert not _rule(split=8)
    assert not _rule(chunk=32)               # G 4 is compiled at chunk 64
    assert not _rule(G=1, chunk=64)          # G 1 at chunk 32
    assert _rule(G=1, chunk=32) and _rule(G=8, split=2) and _rule(G=7, split=2)


def test_instances_are_the_16_wave_set():
    assert _BLK_INSTANCES == {
        (G, 32 if G == 1 else 64, sp)
        for sp in (2, 4) for G in range(1, 9) if sp * G <= 16}
    assert len(_BLK_INSTANCES) == 12


def test_fused_combine_keeps_the_old_path():
    assert not _rule(env={"OLLAMAMQ_FUSED_COMBINE": "1"})
    assert not _rule(env={"OLLAMAMQ_FUSED_COMBINE": "1",
                          "OLLAMAMQ_DECODE_BLOCKSPLIT": "1"})


def test_env_gate():
    assert not _rule(env={"OLLAMAMQ_DECODE_BLOCKSPLIT": "0"})
    # "1" waives the S * KVH floor and nothing else
    assert _rule(S=3, KVH=2, env={"OLLAMAMQ_DECODE_BLOCKSPLIT": "1"})
    assert not _rule(split=1, env={"OLLAMAMQ_DECODE_BLOCKSPLIT": "1"})
    assert not _rule(G=7, env={"OLLAMAMQ_DECODE_BLOCKSPLIT": "1"})


def test_reads_the_process_environment_by_default(monkeypatch):
    monkeypatch.delenv("OLLAMAMQ_FUSED_COMBINE", raising=False)
    monkeypatch.delenv("OLLAMAMQ_DECODE_BLOCKSPLIT", raising=False)
    assert decode_blocksplit(**BENCH)
    monkeypatch.setenv("OLLAMAMQ_DECODE_BLOCKSPLIT", "0")
    assert not decode_blocksplit(**BENCH)

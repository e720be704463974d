"""engine.sampling_rows / penalty_rows: the one place request parameters
become the rows the samplers and the penalty op take."""
from ollamamq_amd.engine import GenParams
from ollamamq_amd.engine.engine import Sequence, penalty_rows, sampling_rows

PARAMS = (
    GenParams(temperature=0.7, top_k=40, top_p=0.9, repeat_penalty=1.3,
              presence_penalty=0.5, frequency_penalty=0.25),
    GenParams(temperature=1.3, top_k=None, top_p=0),
    GenParams(temperature=0.0, top_k=0, top_p=None,
              repeat_penalty=5.0, repeat_last_n=0),       # penalty inactive
    GenParams(temperature=1.0, top_k=5, top_p=1.0, presence_penalty=2.0,
              repeat_last_n=-1),
)
SEEDS = (11, -2 ** 63, 0, 2 ** 63 - 1)


def _seqs():
    return [Sequence(i + 1, [1, 2], p, noise_seed=s)
            for i, (p, s) in enumerate(zip(PARAMS, SEEDS))]


def test_row_helpers():
    seqs = _seqs()
    samp = [(0.7, 40, 0.9, 11), (1.3, 0, 1.0, -2 ** 63), (0.0, 0, 1.0, 0),
            (1.0, 5, 1.0, 2 ** 63 - 1)]
    pen = [(64, 1.3, 0.5, 0.25), (0, 1.0, 0.0, 0.0), (0, 5.0, 0.0, 0.0),
           (-1, 1.0, 2.0, 0.0)]
    assert not PARAMS[2].penalty_active and pen[2][0] == 0
    for pad in (0, 3):
        got_s = list(sampling_rows(seqs, pad))
        got_p = list(penalty_rows(seqs, pad))
        assert got_s == samp + [(0.0, 0, 1.0, 0)] * pad
        assert got_p == pen + [(0, 1.0, 0.0, 0.0)] * pad
        # the types torch.tensor packs them by: ints stay ints
        for rows in (got_s, got_p):
            assert [[type(x) for x in r] for r in rows] \
                == [[type(x) for x in rows[0]]] * len(rows)
    assert list(sampling_rows(seqs)) == samp
    assert list(penalty_rows(seqs)) == pen

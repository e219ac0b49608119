"""Queries of 65 to 256 bytes on the gfx950 fuzzy matcher (the wide tile classes:
a DP column of 2 or 4 u64 words with a carry chain) against the plain DP."""

import random

import numpy as np
import pytest

from move2kube_amd.ops import editdistance, gpu, native

pytestmark = pytest.mark.gpu


def _rand(rng, n, alphabet):
    return "".join(rng.choice(alphabet) for _ in range(n))


@pytest.mark.parametrize("alphabet", ["ab", "".join(chr(c) for c in range(32, 127))], ids=["scaled", "unscaled"])
def test_word_edges_match_the_plain_dp(alphabet):
    rng = random.Random(len(alphabet))
    # every word edge of the wide classes, plus two narrow queries in the same call
    qs = [_rand(rng, n, alphabet) for n in (65, 127, 128, 129, 191, 192, 193, 255, 256, 16, 64)]
    rng.shuffle(qs)
    lens = [0, 1, 16, 63, 64, 65, 127, 128, 129, 200, 256, 257, 300] + [rng.randint(0, 100) for _ in range(11)]
    opts = [_rand(rng, n, alphabet) for n in lens]
    want = [[editdistance.wagner_fischer_py(o, q) for q in qs] for o in opts]
    assert gpu.ed_matrix(opts, qs).tolist() == want


def test_carry_ripples_through_every_word():
    ls, ms = (65, 128, 129, 256), (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300)
    got = gpu.ed_matrix(["a" * m for m in ms], ["a" * n for n in ls])
    assert got.tolist() == [[abs(n - m) for n in ls] for m in ms]


def test_closest_long_queries_with_ties():
    rng = random.Random(13)
    base = [_rand(rng, rng.randint(1, 120), "abcd") for _ in range(40)]
    pick = [rng.randrange(len(base)) for _ in range(1100)]          # > 2 panels, the last one partly padding
    opts = [base[i] for i in pick]
    qs = [_rand(rng, n, "abcd") for n in (65, 66, 100, 128, 129, 130, 191, 192, 193, 222, 255, 256, 0, 9, 33, 64)]
    gi, gd = gpu.ed_closest(opts, qs)
    ci, cd = native.module().closest_batch(opts, qs, 8)
    assert np.array_equal(gd, cd) and np.array_equal(gi, ci)
    for j in (3, 11):
        of_base = [editdistance.wagner_fischer_py(b, qs[j]) for b in base]
        row = [of_base[i] for i in pick]
        assert gd[j] == min(row) and gi[j] == row.index(min(row))   # the first index wins


def test_long_query_reached_from_the_dispatcher(monkeypatch):
    gpu.ed_closest(["warm"], ["up"])
    calls, real = [], gpu.ed_closest
    monkeypatch.setattr(gpu, "ed_closest", lambda o, q: calls.append((len(o), len(q))) or real(o, q))
    rng = random.Random(4)
    opts = [_rand(rng, rng.randint(1, 12), "abcdefgh_-") for _ in range(2048)]
    qs = [_rand(rng, rng.randint(1, 30), "abcdefgh_-") for _ in range(63)] + [_rand(rng, 200, "abcdefgh_-")]
    idx, dist = editdistance.closest_indices(opts, qs)
    assert calls == [(2048, 64)]
    row = [editdistance.wagner_fischer_py(o, qs[63]) for o in opts]
    assert dist[63] == min(row) and idx[63] == row.index(min(row))
    too_long = [qs[63] + "x" * 57]                                   # 257 bytes
    with pytest.raises(gpu.GpuUnsupportedInput):
        gpu.ed_matrix(opts[:8], too_long)
    assert editdistance.matrix(opts[:8], too_long).tolist() == [[editdistance.wagner_fischer_py(o, too_long[0])]
                                                                 for o in opts[:8]]

"""The unit-cost Levenshtein kernels of the gfx950 fuzzy matcher (Myers'
bit-vector recurrence, ``costs=(1, 1, 1)``) against the plain Wagner-Fischer DP."""

import numpy as np
import pytest

from move2kube_amd.ops import editdistance, gpu
from move2kube_amd.ops.editdistance import normalize_alnum_lower as _norm

pytestmark = pytest.mark.gpu

LEV = (1, 1, 1)
LETTERS = "aBc9dEf0gHi1jKl2mNo3pQr4sTu5vWx6yZ7"
# every class edge, nine queries of <= 16 bytes (K16: both halves, a second tile),
# the pair on which the metrics differ, and one-letter runs for the carry chains
QUERIES = ([(LETTERS * 8)[n % 3:n % 3 + n] for n in (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256)]
           + ["abc", "abd", "kitten", "a" * 16, "Bc9dE", "a" * 64, "a" * 100, "a" * 200, "a" * 256])
# short and long options in one panel: a lane freezes while the panel has blocks left
POOL = ([(LETTERS * 9)[n % 5:n % 5 + n] for n in (0, 1, 15, 16, 17, 31, 32, 33, 47, 300)]
        + ["abd", "sitting", "a" * 15, "a" * 48, "a" * 130, "a" * 299])

_DP = {}


def _ref_matrix(opts, qs, norm=None):
    """The plain DP with unit costs, once per distinct pair."""
    out = np.empty((len(opts), len(qs)), dtype=np.int32)
    for i, o in enumerate(opts):
        for j, q in enumerate(qs):
            key = (norm(o), norm(q)) if norm else (o, q)
            if key not in _DP:
                _DP[key] = editdistance.wagner_fischer_py(key[0], key[1], *LEV)
            out[i, j] = _DP[key]
    return out


@pytest.mark.parametrize("na", [1, 512, 513])
def test_matrix_matches_plain_dp(na):
    opts = [POOL[(i * 7 + 3) % len(POOL)] for i in range(na)]
    got = editdistance.matrix(opts, QUERIES, device="gpu", costs=LEV)
    assert got.shape == (na, len(QUERIES))
    assert np.array_equal(got, _ref_matrix(opts, QUERIES))


def test_the_metrics_differ():
    assert editdistance.matrix(["abc"], ["abd"], device="gpu", costs=LEV).tolist() == [[1]]
    assert editdistance.matrix(["abc"], ["abd"], device="gpu").tolist() == [[2]]


def test_more_than_63_byte_values():
    """Unscaled codes: the other instantiation of every class."""
    opts = [bytes(range(1, 1 + n)) for n in (0, 5, 17, 70, 100, 130)] + [bytes(range(120, 20, -1))]
    qs = [bytes(range(5, 5 + n)) for n in (2, 16, 30, 60, 100, 140)] + [b"", bytes(range(90, 60, -1))]
    assert len(set(b"".join(opts + qs))) > 63
    assert np.array_equal(gpu.ed_matrix(opts, qs, metric=gpu.LEVENSHTEIN), _ref_matrix(opts, qs))


def test_closest_is_the_first_minimum_of_the_matrix():
    opts = POOL * 200                                   # every minimum is tied 200 times
    d = editdistance.matrix(opts, QUERIES, device="gpu", costs=LEV)
    idx, dist = editdistance.closest_indices(opts, QUERIES, device="gpu", costs=LEV)
    assert idx.tolist() == d.argmin(axis=0).tolist() and dist.tolist() == d.min(axis=0).tolist()
    assert idx.max() < len(POOL) and np.array_equal(d[:len(POOL)], _ref_matrix(POOL, QUERIES))


def test_normalising_mode():
    opts = ["--" + o[:9] + "_. " + o[9:] + "-é" for o in POOL] * 40
    qs = ["Ab_cD-eF.gH iJ/kL:mN;oP", "- -", "a-B-c", "".join(c + "-" for c in (LETTERS * 8)[:256]), "A" * 70 + "é" + "a" * 30]
    want = _ref_matrix(opts, qs, _norm)
    assert np.array_equal(editdistance.matrix(opts, qs, device="gpu", normalize="alnum_lower", costs=LEV), want)
    idx, dist = editdistance.closest_indices(opts, qs, device="gpu", normalize="alnum_lower", costs=LEV)
    assert idx.tolist() == want.argmin(axis=0).tolist() and dist.tolist() == want.min(axis=0).tolist()


def test_query_limit():
    gpu.ed_closest(["warm"], ["up"])                    # a warm runtime uses the small-batch threshold
    opts, qs = ["abc", "x" * 250, "abd"] * 3000, ["x" * 257, "abd"]
    with pytest.raises(gpu.GpuUnsupportedInput):
        editdistance.closest_indices(opts, qs, device="gpu", costs=LEV)
    idx, dist = editdistance.closest_indices(opts, qs, costs=LEV)      # auto: the CPU answers
    assert (idx.tolist(), dist.tolist()) == ([1, 2], [7, 0])

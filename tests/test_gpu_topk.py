"""The top-k kernels of the gfx950 fuzzy matcher (the k closest options of every
query in one pass) against the plain Wagner-Fischer DP."""

import numpy as np
import pytest

from move2kube_amd.ops import editdistance, gpu
from move2kube_amd.ops.editdistance import normalize_alnum_lower as _norm

pytestmark = pytest.mark.gpu

COSTS = [(1, 1, 2), (1, 1, 1)]
LETTERS = "aBc9dEf0gHi1jKl2mNo3pQr4sTu5vWx6yZ7"
# every tile class edge (all five classes launch, each with its own part plan) and nine
# queries of <= 16 bytes: a second K16 tile, both halves of a word
QUERIES = ([(LETTERS * 8)[n % 3:n % 3 + n] for n in (0, 1, 16, 17, 32, 33, 64, 65, 128, 129, 256)]
           + ["abc", "abd", "kitten", "a" * 16, "Bc9dE", "sittin", "a" * 9, "dEf0", "9"])
# 16 distinct options of 0..300 bytes: every distance is tied many times, so the index order inside ties counts
POOL = ([(LETTERS * 9)[n % 5:n % 5 + n] for n in (0, 1, 15, 16, 17, 31, 32, 33, 47, 300)]
        + ["abd", "sitting", "a" * 15, "a" * 48, "a" * 130, "a" * 299])

_DP = {}


def _want(opts, qs, k, costs, norm=None):
    """The first k of every column of the plain DP, stably sorted; one DP per distinct pair."""
    ref = np.empty((len(opts), len(qs)), dtype=np.int32)
    for i, o in enumerate(opts):
        for j, q in enumerate(qs):
            key = (norm(o), norm(q), costs) if norm else (o, q, costs)
            if key not in _DP:
                _DP[key] = editdistance.wagner_fischer_py(key[0], key[1], *costs)
            ref[i, j] = _DP[key]
    order = np.argsort(ref, axis=0, kind="stable")[:k]
    idx = np.full((len(qs), k), -1, dtype=np.int32)
    dist = idx.copy()
    idx[:, :len(order)] = order.T
    dist[:, :len(order)] = np.take_along_axis(ref, order, axis=0).T
    return idx, dist


# one option, fewer options than k (padding), one full panel, one option into a second panel,
# 9 panels on 8 workgroups (a workgroup walks two panels, the merge sees 32 parts per query)
@pytest.mark.parametrize("costs", COSTS)
@pytest.mark.parametrize("k", [1, 2, 7, 64])
@pytest.mark.parametrize("na", [1, 3, 512, 513, 4608])
def test_first_k_of_every_column(na, k, costs):
    opts = [POOL[(i * 7 + 3) % len(POOL)] for i in range(na)]
    idx, dist = editdistance.closest_k(opts, QUERIES, k, device="gpu", costs=costs)
    want = _want(opts, QUERIES, k, costs)
    assert idx.dtype == dist.dtype == np.int32 and idx.shape == dist.shape == (len(QUERIES), k)
    assert np.array_equal(dist, want[1]) and np.array_equal(idx, want[0])
    if k == 1:
        one = editdistance.closest_indices(opts, QUERIES, device="gpu", costs=costs)
        assert np.array_equal(idx[:, 0], one[0]) and np.array_equal(dist[:, 0], one[1])


@pytest.mark.parametrize("metric, costs", [(gpu.INDEL2, (1, 1, 2)), (gpu.LEVENSHTEIN, (1, 1, 1))])
def test_more_than_63_byte_values(metric, costs):
    """Unscaled codes: the other instantiation of every class."""
    opts = [bytes(range(1, 1 + n)) for n in (0, 5, 17, 70, 100, 130)] + [bytes(range(120, 20, -1))]
    qs = [bytes(range(5, 5 + n)) for n in (2, 16, 30, 60, 100, 140)] + [b"", bytes(range(90, 60, -1))]
    assert len(set(b"".join(opts + qs))) > 63
    idx, dist = gpu.ed_closest_k(opts, qs, 5, metric=metric)
    want = _want(opts, qs, 5, costs)
    assert np.array_equal(dist, want[1]) and np.array_equal(idx, want[0])


@pytest.mark.parametrize("costs", COSTS)
def test_normalising_mode(costs):
    opts = ["--" + o[:9] + "_. " + o[9:] + "-é" for o in POOL] * 40
    qs = ["Ab_cD-eF.gH iJ/kL:mN;oP", "- -", "a-B-c", "".join(c + "-" for c in (LETTERS * 8)[:256]), "A" * 70 + "é" + "a" * 30]
    idx, dist = editdistance.closest_k(opts, qs, 50, device="gpu", normalize="alnum_lower", costs=costs)
    want = _want(opts, qs, 50, costs, _norm)
    assert np.array_equal(dist, want[1]) and np.array_equal(idx, want[0])


def test_k_limit():
    gpu.ed_closest(["warm"], ["up"])                    # a warm runtime uses the small-batch threshold
    opts, qs = ["abc", "x" * 250, "abd"] * 3000, ["x" * 250, "abd"]
    with pytest.raises(gpu.GpuUnsupportedInput):
        editdistance.closest_k(opts, qs, gpu.MAX_K + 1, device="gpu")
    idx, dist = editdistance.closest_k(opts, qs, gpu.MAX_K + 1)        # auto: the CPU answers
    want = _want(opts, qs, gpu.MAX_K + 1, (1, 1, 2))
    assert np.array_equal(dist, want[1]) and np.array_equal(idx, want[0])

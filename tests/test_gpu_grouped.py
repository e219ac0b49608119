"""The grouped closest kernels of the gfx950 fuzzy matcher (the closest option
of every group in one pass) against the plain Wagner-Fischer DP."""

import numpy as np
import pytest

from move2kube_amd.ops import editdistance, gpu
from move2kube_amd.ops.editdistance import normalize_alnum_lower as _norm

pytestmark = pytest.mark.gpu

COSTS = [(1, 1, 2), (1, 1, 1)]
LETTERS = "aBc9dEf0gHi1jKl2mNo3pQr4sTu5vWx6yZ7"
# every tile class edge, nine queries of <= 16 bytes (a second K16 tile), one-letter runs for the carry chains
QUERIES = ([(LETTERS * 8)[n % 3:n % 3 + n] for n in (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256)]
           + ["abc", "abd", "kitten", "a" * 16, "Bc9dE", "a" * 100, "a" * 256])
# 16 distinct options, so every minimum is tied many times and the first index has to win
POOL = ([(LETTERS * 9)[n % 5:n % 5 + n] for n in (0, 1, 15, 16, 17, 31, 32, 33, 47, 300)]
        + ["abd", "sitting", "a" * 15, "a" * 48, "a" * 130, "a" * 299])

_DP = {}


def _want(groups, qs, costs, norm=None):
    """First minimum of the plain DP within every group, one DP per distinct pair."""
    idx = np.full((len(qs), len(groups)), -1, dtype=np.int32)
    dist = idx.copy()
    for g, options in enumerate(groups):
        for j, q in enumerate(qs):
            bi = bd = -1
            for i, o in enumerate(options):
                key = (norm(o), norm(q), costs) if norm else (o, q, costs)
                if key not in _DP:
                    _DP[key] = editdistance.wagner_fischer_py(key[0], key[1], *costs)
                if bi < 0 or _DP[key] < bd:
                    bi, bd = i, _DP[key]
            idx[j, g], dist[j, g] = bi, bd
    return idx, dist


def _split(options, sizes):
    ends = np.cumsum(sizes)
    return [options[e - n:e] for n, e in zip(sizes, ends)]


# the smallest shape for each path of the reduction: one live lane and an empty
# group; every wave mixed (per-lane atomics); every wave uniform in another
# group (flushes); a boundary inside a wave; a panel with one live lane in a new
# group; 15 panels on 8 workgroups (a workgroup walks two panels) holding one
# group, and changing group between its panels
@pytest.mark.parametrize("costs", COSTS)
@pytest.mark.parametrize("sizes", [[1], [5, 0, 3], [40] * 10, [64] * 8, [300, 300], [512, 1], [7200], [3700, 3500]],
                         ids=lambda s: "x".join(map(str, s)) if len(set(s)) > 1 else "%dx%d" % (len(s), s[0]))
def test_first_closest_option_of_every_group(sizes, costs):
    groups = _split([POOL[(i * 7 + 3) % len(POOL)] for i in range(sum(sizes))], sizes)
    idx, dist = editdistance.closest_in_groups(groups, QUERIES, device="gpu", costs=costs)
    want = _want(groups, QUERIES, costs)
    assert idx.dtype == dist.dtype == np.int32 and idx.shape == dist.shape == (len(QUERIES), len(sizes))
    assert np.array_equal(dist, want[1]) and np.array_equal(idx, want[0])


@pytest.mark.parametrize("metric, costs", [(gpu.INDEL2, (1, 1, 2)), (gpu.LEVENSHTEIN, (1, 1, 1))])
def test_more_than_63_byte_values(metric, costs):
    """Unscaled codes: the other instantiation of every class."""
    opts = [bytes(range(1, 1 + n)) for n in (0, 5, 17, 70, 100, 130)] + [bytes(range(120, 20, -1))]
    qs = [bytes(range(5, 5 + n)) for n in (2, 16, 30, 60, 100, 140)] + [b"", bytes(range(90, 60, -1))]
    assert len(set(b"".join(opts + qs))) > 63
    group_of = [2, 0, 2, 0, 3, 2, 0]                         # not sorted; group 1 is empty
    idx, dist = gpu.ed_closest_grouped(opts, group_of, 4, qs, metric=metric)
    members = [[i for i, g in enumerate(group_of) if g == k] for k in range(4)]
    want = _want([[opts[i] for i in m] for m in members], qs, costs)
    assert np.array_equal(dist, want[1])
    assert idx.tolist() == [[m[i] if i >= 0 else -1 for m, i in zip(members, row)] for row in want[0].tolist()]


@pytest.mark.parametrize("costs", COSTS)
def test_normalising_mode(costs):
    groups = _split(["--" + o[:9] + "_. " + o[9:] + "-é" for o in POOL] * 40, [100, 0, 300, 240])
    qs = ["Ab_cD-eF.gH iJ/kL:mN;oP", "- -", "a-B-c", "".join(c + "-" for c in (LETTERS * 8)[:256]), "A" * 70 + "é" + "a" * 30]
    idx, dist = editdistance.closest_in_groups(groups, qs, device="gpu", normalize="alnum_lower", costs=costs)
    want = _want(groups, qs, costs, _norm)
    assert np.array_equal(dist, want[1]) and np.array_equal(idx, want[0])


@pytest.mark.parametrize("costs", COSTS)
def test_one_group_is_closest_indices(costs):
    opts = POOL * 100
    idx, dist = editdistance.closest_in_groups([opts], QUERIES, device="gpu", costs=costs)
    one = editdistance.closest_indices(opts, QUERIES, device="gpu", costs=costs)
    assert np.array_equal(idx[:, 0], one[0]) and np.array_equal(dist[:, 0], one[1])


def test_query_limit():
    gpu.ed_closest(["warm"], ["up"])                    # a warm runtime uses the small-batch threshold
    groups, qs = [["abc", "x" * 250, "abd"] * 3000, ["abd"]], ["x" * 257, "abd"]
    with pytest.raises(gpu.GpuUnsupportedInput):
        editdistance.closest_in_groups(groups, qs, device="gpu")
    idx, dist = editdistance.closest_in_groups(groups, qs)            # auto: the CPU answers
    assert (idx.tolist(), dist.tolist()) == ([[1, 0], [2, 0]], [[7, 257 + 3], [0, 0]])


@pytest.mark.parametrize("group_of, n_groups", [([0, 2], 2), ([-1, 0], 2), ([0, 0], 0)])
def test_group_id_out_of_range(group_of, n_groups):
    with pytest.raises(ValueError):
        gpu.ed_closest_grouped(["a", "b"], group_of, n_groups, ["a"])

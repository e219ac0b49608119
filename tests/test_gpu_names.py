"""The names-in-lanes kernels of the gfx950 fuzzy matcher (``gpu.ed_closest_names``:
a few options in LDS, many names of any length in the lanes) against the plain
Wagner-Fischer DP."""

import numpy as np
import pytest

from move2kube_amd.ops import editdistance, gpu
from move2kube_amd.ops.editdistance import normalize_alnum_lower as _norm

pytestmark = pytest.mark.gpu

METRICS = [(gpu.INDEL2, (1, 1, 2)), (gpu.LEVENSHTEIN, (1, 1, 1))]
ALPHABETS = {"scaled": b"aBc9dEf0gHi1jKl2mNo3pQr4sTu5vWx6yZ7", "unscaled": bytes(range(33, 123))}   # 35 / 90 symbols
EDGES = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256)
NAME_LENGTHS = (0, 1, 15, 16, 17, 47, 300)


def _strings(alphabet):
    """Distinct options (every class edge, one-letter runs for the carry chains)
    and distinct names (300 bytes: longer than any query the other families take)."""
    cut = lambda n, k: (alphabet * 12)[n % k:n % k + n]   # noqa: E731
    options = [cut(n, 3) for n in EDGES] + [alphabet[:1] * n for n in (64, 128, 256)]
    names = [cut(n, 5) for n in NAME_LENGTHS] + [alphabet[:1] * 300, cut(16, 3), cut(129, 3)]
    return options, names


_DP = {}


def _table(alphabet, costs):
    """dist[name, option] over the distinct strings, computed once per alphabet and metric."""
    if (alphabet, costs) not in _DP:
        options, names = _strings(ALPHABETS[alphabet])
        _DP[alphabet, costs] = np.array([[editdistance.wagner_fischer_py(o, n, *costs) for o in options]
                                         for n in names], dtype=np.int32)
    return _DP[alphabet, costs]


def _first_minimum(d, members):
    """(idx, dist) of the first minimum of every row of ``d`` over the columns ``members``."""
    if len(members) == 0:
        return np.full(len(d), -1, dtype=np.int32), np.full(len(d), -1, dtype=np.int32)
    at = d[:, members].argmin(axis=1)
    return members[at].astype(np.int32), d[np.arange(len(d)), members[at]]


# 340 options: each of the 19 distinct ones 17 or 18 times (ties go to the
# lowest index), so every class has 54 to 72 of them: more tiles than one LDS
# chunk holds (8, the wide classes 4), with one group and with three.  Grouped:
# groups 0..2 span every class (their keys are committed by five launches),
# group 3 is empty, group 4 is option 0 alone.  Names: 1 / 512 / 513 / 1100 are
# the panel edges; sorted by length, 47- and 300-byte names share the last panel.
@pytest.mark.parametrize("n_names", [1, 512, 513, 1100])
@pytest.mark.parametrize("grouped", [False, True], ids=["one_group", "groups"])
@pytest.mark.parametrize("alphabet", list(ALPHABETS))
@pytest.mark.parametrize("metric, costs", METRICS, ids=["indel2", "levenshtein"])
def test_first_closest_option_of_every_name(metric, costs, alphabet, grouped, n_names):
    options, names = _strings(ALPHABETS[alphabet])
    assert (len(set(b"".join(options + names))) > 63) == (alphabet == "unscaled")
    opt_at = np.array([(i * 7 + 3) % len(options) for i in range(340)])
    name_at = np.array([(i * 3 + 6) % len(names) for i in range(n_names)])
    d = _table(alphabet, costs)[name_at][:, opt_at]
    opts, nms = [options[i] for i in opt_at], [names[i] for i in name_at]
    if grouped:
        group_of = np.array([4] + [i % 3 for i in range(1, len(opts))], dtype=np.int32)
        idx, dist = gpu.ed_closest_names(opts, nms, group_of, 5, metric=metric)
        assert idx.shape == dist.shape == (n_names, 5)
        want = [_first_minimum(d, np.flatnonzero(group_of == g)) for g in range(5)]
        want = np.stack([w[0] for w in want], axis=1), np.stack([w[1] for w in want], axis=1)
    else:
        idx, dist = gpu.ed_closest_names(opts, nms, metric=metric)
        assert idx.shape == dist.shape == (n_names,)
        want = _first_minimum(d, np.arange(len(opts)))
    assert idx.dtype == dist.dtype == np.int32
    assert np.array_equal(dist, want[1]) and np.array_equal(idx, want[0])


@pytest.mark.parametrize("metric, costs", METRICS, ids=["indel2", "levenshtein"])
def test_same_answers_as_the_other_families(metric, costs):
    options, names = _strings(ALPHABETS["scaled"])
    opts = [options[(i * 5 + 1) % len(options)] for i in range(90)]
    nms = [n for n in names if len(n) <= gpu.MAX_QUERY_BYTES] * 150
    group_of = [i % 4 for i in range(len(opts))]
    one, other = gpu.ed_closest_names(opts, nms, metric=metric), gpu.ed_closest(opts, nms, metric=metric)
    assert np.array_equal(one[0], other[0]) and np.array_equal(one[1], other[1])
    one = gpu.ed_closest_names(opts, nms, group_of, 4, metric=metric)
    other = gpu.ed_closest_grouped(opts, group_of, 4, nms, metric=metric)
    assert np.array_equal(one[0], other[0]) and np.array_equal(one[1], other[1])


@pytest.mark.parametrize("metric, costs", METRICS, ids=["indel2", "levenshtein"])
def test_normalising_mode(metric, costs):
    opts = ["NodeJS_Buildpack", "java-buildpack", "Paketo Buildpacks/NodeJS", "--", "Go", "x-" * 256, "Java_Buildpack"]
    names = ["nodejs", "https://github.com/CloudFoundry/Java-Buildpack.git#v4.2", "é-É", "", "G_o",
             "Https://Git.Example.com/" + "Team-Build_Packs/" * 20 + "nodejs-buildpack.git", "x" * 300]
    assert len(names[5]) > 256 and len(_norm(names[5])) > 256
    idx, dist = gpu.ed_closest_names(opts, names * 90, mode=gpu.ALNUM_LOWER, metric=metric)
    d = np.array([[editdistance.wagner_fischer_py(_norm(o), _norm(n), *costs) for o in opts] for n in names])
    want = _first_minimum(d, np.arange(len(opts)))
    assert np.array_equal(dist, np.tile(want[1], 90)) and np.array_equal(idx, np.tile(want[0], 90))


def test_refusals():
    with pytest.raises(gpu.GpuUnsupportedInput):
        gpu.ed_closest_names(["abc", "x" * 257], ["abc"])
    with pytest.raises(gpu.GpuUnsupportedInput):
        gpu.ed_closest_names(["abc", "x-" * 257], ["abc"], mode=gpu.ALNUM_LOWER)
    with pytest.raises(ValueError):
        gpu.ed_closest_names(["a", "b"], ["a"], [0, 2], 2)

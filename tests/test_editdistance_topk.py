"""``editdistance.closest_k`` on the CPU route: the first k entries of every
matrix column in (distance, option index) order, against the plain DP."""

import numpy as np
import pytest

from move2kube_amd.ops import editdistance, gpu
from move2kube_amd.utils import common

OPTS = ["kitten", "sitting", "", "mitten", "kitten", "abc", "sittin", "Kit-Ten", "abd", "kitchen", "mitten"]
QUERIES = ["kitten", "abd", "", "sitting!"]


def _want(opts, qs, k, costs):
    ref = np.array([[editdistance.wagner_fischer_py(o, q, *costs) for q in qs] for o in opts], dtype=np.int32)
    order = np.argsort(ref, axis=0, kind="stable")[:k]
    idx = np.full((len(qs), k), -1, dtype=np.int32)
    dist = idx.copy()
    idx[:, :len(order)] = order.T
    dist[:, :len(order)] = np.take_along_axis(ref, order, axis=0).T
    return idx, dist


@pytest.mark.parametrize("costs", [(1, 1, 2), (1, 1, 1), (2, 3, 4)])
@pytest.mark.parametrize("k", [1, 3, len(OPTS), len(OPTS) + 4])
def test_cpu_route_against_the_dp(k, costs):
    idx, dist = editdistance.closest_k(OPTS, QUERIES, k, device="cpu", costs=costs)
    want = _want(OPTS, QUERIES, k, costs)
    assert idx.dtype == dist.dtype == np.int32 and idx.shape == dist.shape == (len(QUERIES), k)
    assert np.array_equal(dist, want[1]) and np.array_equal(idx, want[0])
    if k == 1:
        one = editdistance.closest_indices(OPTS, QUERIES, device="cpu", costs=costs)
        assert np.array_equal(idx[:, 0], one[0]) and np.array_equal(dist[:, 0], one[1])


@pytest.mark.parametrize("opts, qs", [([], ["a", "b"]), (["a"], []), ([], [])])
def test_nothing_to_rank(opts, qs):
    idx, dist = editdistance.closest_k(opts, qs, 3, device="cpu")
    assert idx.shape == dist.shape == (len(qs), 3) and (idx == -1).all() and (dist == -1).all()


def test_bad_requests():
    with pytest.raises(ValueError):
        editdistance.closest_k(OPTS, QUERIES, 0, device="cpu")
    with pytest.raises(ValueError):
        gpu.ed_closest_k(OPTS, QUERIES, 0)
    with pytest.raises(gpu.GpuUnsupportedInput):
        editdistance.closest_k(OPTS, QUERIES, 2, device="gpu", costs=(2, 3, 4))


def test_k_closest_matching_strings():
    opts = ["java_buildpack", "Node.js-Buildpack", "nodejs_buildpack", "go", "nodejs"]
    got = common.get_k_closest_matching_strings(opts, ["NodeJS buildpack", "g"], 3)
    assert got == [["Node.js-Buildpack", "nodejs_buildpack", "java_buildpack"], ["go", "nodejs", "java_buildpack"]]
    assert common.get_k_closest_matching_strings(opts[:2], ["go"], 3) == [["java_buildpack", "Node.js-Buildpack"]]
    assert common.get_k_closest_matching_strings([], ["go"], 3) == [[]]
    assert common.get_k_closest_matching_strings(opts, [], 3) == []

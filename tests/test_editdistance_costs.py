"""``costs=`` of the edit-distance front end on the CPU route, against the Python DP."""

import pytest

from move2kube_amd.ops import editdistance as ed

OPTS = ["abc", "abd", "", "kitten", "sitting", "java_buildpack", "a" * 70, "abd"]
QS = ["abd", "sitten", "", "javabuildpak", "a" * 66 + "b"]


def _dp(costs):
    return [[ed.wagner_fischer_py(o, q, *costs) for q in QS] for o in OPTS]


@pytest.mark.parametrize("costs", [(1, 1, 1), (2, 3, 4)])
def test_costs_on_the_cpu_match_the_dp(costs):
    want = _dp(costs)
    assert ed.matrix(OPTS, QS, device="cpu", costs=costs).tolist() == want
    first = [min(range(len(OPTS)), key=lambda i: want[i][j]) for j in range(len(QS))]   # lowest index on ties
    best = [want[i][j] for j, i in enumerate(first)]
    idx, dist = ed.closest_indices(OPTS, QS, device="cpu", costs=costs)
    assert (idx.tolist(), dist.tolist()) == (first, best)
    assert ed.closest_index_list(OPTS, QS, device="cpu", costs=costs) == (first, best)


def test_the_default_is_still_one_one_two():
    assert ed.matrix(OPTS, QS, device="cpu").tolist() == _dp((1, 1, 2)) != _dp((1, 1, 1))
    assert ed.matrix(OPTS, QS, device="cpu", costs=(1, 1, 2)).tolist() == _dp((1, 1, 2))
    assert ed.closest_index_list(OPTS, ["abd"], device="cpu")[0] == [1]


def test_normalize_combines_with_costs():
    assert ed.matrix(["A-b_C"], ["abd"], device="cpu", normalize="alnum_lower", costs=(1, 1, 1)).tolist() == [[1]]


def test_the_gpu_refuses_other_costs():
    from move2kube_amd.ops import gpu
    with pytest.raises(gpu.GpuUnsupportedInput):
        ed.matrix(OPTS, QS, device="gpu", costs=(2, 3, 4))
    with pytest.raises(ValueError):
        ed.matrix(OPTS, QS, costs=(1, 1))

"""Routing of ``closest_indices`` / ``closest_in_groups`` to the names kernels
(``gpu.ed_closest_names``), with a stand-in for ``ops/gpu.py``."""

import sys

import numpy as np
import pytest

from move2kube_amd.ops import editdistance as ed


def test_rule_at_its_bounds():
    most, per = ed.NAMES_ROUTE_MAX_OPTIONS, ed.NAMES_ROUTE_MIN_QUERIES_PER_OPTION
    assert most >= 1 and per >= 1
    assert ed.names_route(1, per) and ed.names_route(most, per * most)
    assert not ed.names_route(most + 1, per * (most + 1))
    assert not ed.names_route(most, per * most - 1) and not ed.names_route(1, per - 1)
    assert not ed.names_route(0, 10 ** 6)


class _Gpu:
    MAX_QUERY_BYTES, NO_MODE, ALNUM_LOWER, LEVENSHTEIN = 256, 0, 1, 1

    class GpuUnsupportedInput(RuntimeError):
        pass

    def __init__(self):
        self.calls = []

    def ed_closest(self, options, queries):
        self.calls.append("closest")
        return np.zeros(len(queries), dtype=np.int32), np.zeros(len(queries), dtype=np.int32)

    def ed_closest_normalized(self, options, queries):
        self.calls.append("normalized")
        raise self.GpuUnsupportedInput("the kernel library's own check of the normalised queries")

    def ed_closest_grouped(self, options, group_of, n_groups, queries, mode=0):
        self.calls.append("grouped")
        return (np.zeros((len(queries), n_groups), dtype=np.int32),) * 2


class _GpuWithNames(_Gpu):
    def ed_closest_names(self, options, names, group_of=None, n_groups=1, mode=0):
        self.calls.append("names")
        shape = (len(names), n_groups) if group_of is not None else (len(names),)
        return np.zeros(shape, dtype=np.int32), np.zeros(shape, dtype=np.int32)


@pytest.mark.parametrize("cls, option, want", [(_Gpu, "go", ["closest", "grouped"]),
                                               (_GpuWithNames, "go", ["names", "names"]),
                                               (_GpuWithNames, "x" * 257, ["closest", "grouped"])],
                         ids=["module_without_the_entry", "routed", "option_over_the_limit"])
def test_route_taken(monkeypatch, cls, option, want):
    g = cls()
    monkeypatch.setattr(ed, "_gpu", lambda: g)
    monkeypatch.setitem(sys.modules, "move2kube_amd.ops.gpu", g)
    names = ["n%d" % i for i in range(2 * ed.NAMES_ROUTE_MIN_QUERIES_PER_OPTION)]
    assert ed.closest_indices([option, "java"], names, device="gpu")[0].shape == (len(names),)
    assert ed.closest_in_groups([[option], ["java"]], names, device="gpu")[0].shape == (len(names), 2)
    assert g.calls == want
    with pytest.raises(g.GpuUnsupportedInput):   # the query limit is checked before any routing
        ed.closest_indices([option, "java"], names + ["x" * 257], device="gpu")


def test_normalised_query_over_the_limit_keeps_todays_route(monkeypatch):
    g = _GpuWithNames()
    monkeypatch.setattr(ed, "_gpu", lambda: g)
    monkeypatch.setitem(sys.modules, "move2kube_amd.ops.gpu", g)
    names = ["n%d" % i for i in range(2 * ed.NAMES_ROUTE_MIN_QUERIES_PER_OPTION)]
    # 300 bytes raw, nothing left after normalisation: within the limit, routed
    ed.closest_indices(["go", "java"], names + ["-" * 300], device="gpu", normalize="alnum_lower")
    assert g.calls == ["names"]
    with pytest.raises(g.GpuUnsupportedInput):   # 257 bytes after normalisation: refused as before
        ed.closest_indices(["go", "java"], names + ["x-" * 257], device="gpu", normalize="alnum_lower")
    assert g.calls == ["names", "normalized"]

"""The dispatcher takes the longest GPU query from the kernel library
(``gpu.MAX_QUERY_BYTES``), observed on the CPU with a stand-in module."""

import sys

import numpy
import pytest

from move2kube_amd.ops import editdistance as ed

OPTS = ["nodejs_buildpack", "java_buildpack", "go_buildpack", "python_buildpack"]


class _FakeGpu:
    MAX_QUERY_BYTES = 256
    GpuUnavailable = GpuUnsupportedInput = RuntimeError
    calls = 0
    gpu_host = warm = staticmethod(lambda: True)

    def ed_matrix(self, options, queries):
        self.calls += 1
        return numpy.zeros((len(options), len(queries)), dtype=numpy.int32)


def test_limit_comes_from_the_gpu_module(monkeypatch):
    g = _FakeGpu()
    monkeypatch.setattr(ed, "_gpu", lambda: g)
    monkeypatch.setitem(sys.modules, "move2kube_amd.ops.gpu", g)
    monkeypatch.setattr(ed, "GPU_MIN_PAIRS", 4)
    assert ed.matrix(OPTS, ["x" * 65]).tolist() == [[0]] * 4 and g.calls == 1     # auto: the stand-in answered
    q = "nodejs" * 42 + "abcde"                                                      # 257 bytes
    want = [[ed.wagner_fischer_py(o, q)] for o in OPTS]
    assert ed.matrix(OPTS, [q]).tolist() == want and g.calls == 1                  # stays on the CPU
    with pytest.raises(g.GpuUnavailable, match="longer than 256 bytes"):
        ed.matrix(OPTS, [q], device="gpu")

"""The normalising mode of the gfx950 fuzzy matcher (raw names in, the options
stripped to [a-zA-Z0-9] and lower-cased by the fill kernel as it writes their
panels) against Python normalisation followed by the plain Wagner-Fischer DP."""

import re

import numpy as np
import pytest

from move2kube_amd.ops import editdistance, gpu, native

pytestmark = pytest.mark.gpu

LETTERS = "aBc9dEf0gHi1jKl2mNo3pQr4sTu5vWx6yZ7"


def _norm(s):
    if isinstance(s, bytes):
        s = s.decode("utf-8", "surrogateescape")
    return re.sub("[^a-zA-Z0-9]+", "", s).lower()


_DP = {}


def _ref_matrix(opts, qs):
    """The plain DP on the normalised strings, once per distinct pair."""
    out = np.empty((len(opts), len(qs)), dtype=np.int32)
    no, nq = [_norm(o) for o in opts], [_norm(q) for q in qs]
    for i, o in enumerate(no):
        for j, q in enumerate(nq):
            if (o, q) not in _DP:
                _DP[(o, q)] = editdistance.wagner_fischer_py(o, q)
            out[i, j] = _DP[(o, q)]
    return out


def _pool():
    """24 option shapes: normalised lengths around the 16-byte block edges, the
    separators at the head, at the tail and in runs in the middle."""
    pool = []
    for n in (0, 1, 15, 16, 17, 31, 32, 33):
        s = (LETTERS * 2)[n % 5:n % 5 + n]
        pool += ["--_ " + s, s + "..  -", s[:n // 2] + "-é--" + s[n // 2:n // 2 + 3] + "___" + s[n // 2 + 3:]]
    pool[7] = pool[7].encode() + b"\xff"            # a bytes option with a byte that is no UTF-8
    assert sorted({len(_norm(o)) for o in pool}) == [0, 1, 15, 16, 17, 31, 32, 33] and _norm(pool[2]) == ""
    return pool


def _queries():
    long = "".join(c + "-" for c in (LETTERS * 8)[:256])       # 512 raw bytes, 256 after normalisation
    qs = ["- -", "Ab_cD-eF.gH iJ/kL:mN;oP", (LETTERS * 2)[3:20] + "é", "." + (LETTERS * 2)[:64],
          (LETTERS * 2)[1:33] + "__" + (LETTERS * 2)[2:35], long]
    assert [len(_norm(q)) for q in qs] == [0, 16, 17, 64, 65, 256]
    return qs


@pytest.mark.parametrize("na", [1, 512, 513])
def test_matrix_matches_plain_dp(na):
    pool, qs = _pool(), _queries()
    opts = [pool[(i * 7 + 3) % len(pool)] for i in range(na)]
    got = gpu.ed_matrix_normalized(opts, qs)
    assert got.shape == (na, len(qs))
    assert np.array_equal(got, _ref_matrix(opts, qs))


def test_stale_arena_is_cleared():
    """The second request's panels are planned on raw lengths (3 blocks) but
    hold 3 codes per option: everything behind them must be zero blocks, not
    the first request's 40-byte options."""
    qs = ["abc", LETTERS, "b-c"]
    first = [(LETTERS + "abcde")[:40]] * 600
    assert np.array_equal(gpu.ed_matrix_normalized(first, qs), _ref_matrix(first, qs))
    second = ["a" + "-" * 37 + "bc"] * 600 + ["A-b-C", "_____", "abcde"]
    assert np.array_equal(gpu.ed_matrix_normalized(second, qs), _ref_matrix(second, qs))


def test_one_long_option_among_short_ones():
    long = ("Ab-" * 1667)[:5000]
    opts = ["opt_%d" % i for i in range(10)] + [long] + ["Name.%d" % i for i in range(10)]
    qs = ["opt3", "name 7", "ab" * 100, ""]
    want = _ref_matrix(opts, qs)
    assert np.array_equal(gpu.ed_matrix_normalized(opts, qs), want)
    idx, dist = gpu.ed_closest_normalized(opts, qs)
    assert dist.tolist() == want.min(axis=0).tolist() and idx.tolist() == want.argmin(axis=0).tolist()


def test_ties_go_to_the_first_option():
    opts = ["Java_Buildpack", "java-buildpack", "JAVABUILDPACK"] * 200
    idx, dist = gpu.ed_closest_normalized(opts, ["java buildpack"])
    assert (idx.tolist(), dist.tolist()) == ([0], [0])


def test_query_limit_applies_after_normalisation():
    opts = ["Node-JS", "java_buildpack", "GO"] * 3000
    qs = ["x-" * 257, "go"]                        # 257 bytes after normalisation
    with pytest.raises(gpu.GpuUnsupportedInput):
        gpu.ed_closest_normalized(opts, qs)
    idx, dist = editdistance.closest_indices(opts, qs, normalize="alnum_lower")
    ci, cd = native.module().closest_batch([_norm(o) for o in opts], [_norm(q) for q in qs], 8)
    assert np.array_equal(idx, ci) and np.array_equal(dist, cd) and idx[1] == 2


def test_closest_matching_strings_sends_raw_names(monkeypatch):
    from move2kube_amd.utils import common
    gpu.ed_closest(["warm"], ["up"])  # a warm runtime uses the small-batch threshold
    calls = []
    real = gpu.ed_closest_normalized

    def spy(o, q):
        calls.append((o, q))
        return real(o, q)

    monkeypatch.setattr(gpu, "ed_closest_normalized", spy)
    opts = ["NodeJS_Buildpack", "java-buildpack", "Python.Buildpack", "go_buildpack", "RUBY buildpack"] * 1000
    names = ["Node", "java_a", "Pythn", "GoLang", "ruby-y"] * 20
    got = common.get_closest_matching_strings(opts, names)
    assert calls == [(opts, names)]
    assert got == opts[:5] * 20
    idx, _ = editdistance.closest_index_list(opts, names, device="cpu", normalize="alnum_lower")
    assert got == [opts[i] for i in idx]

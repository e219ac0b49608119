"""ctypes binding for the MI355X batched fuzzy-matching kernel (``ed_kernel.hip``).

The HIP library is built in-tree for gfx950 (``libm2k_ed_hip.so``).  On a
machine that exposes an AMD GPU (``/dev/kfd``) a missing library is an error
(``GpuUnavailable``) rather than a silent CPU fallback; on CPU-only hosts the
callers use the native CPU path.
"""

import _thread
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libm2k_ed_hip.so")

_lib = None
_state = None  # None=untried, True=ok, False=unavailable
_lock = _thread.RLock()


class GpuUnavailable(RuntimeError):
    pass


# Longest query the kernels take (the widest tile class holds one DP column of
# 4 x 64 bits); the dispatcher reads the limit from here.
MAX_QUERY_BYTES = 256


# Longest ranked list of the top-k kernels: a wave keeps one rank per lane.
MAX_K = 64


class GpuUnsupportedInput(GpuUnavailable):
    """The kernel cannot take this input (query > MAX_QUERY_BYTES, all 256 byte values used, k > MAX_K)."""


_RC_UNSUPPORTED = (-2, -8)


def gpu_host():
    """True on a host exposing an AMD GPU to this process."""
    if os.environ.get("M2K_FORCE_CPU"):
        return False
    return os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK | os.W_OK)


def _load():
    if _state is not None:
        return _lib
    with _lock:   # one thread loads; the others wait for it
        return _load_locked()


def _load_locked():
    """Load the library (under ``_lock``).  ``_lib`` is set before ``_state``
    and ``_state`` only when the outcome is known, so the lock-free check in
    :func:`_load` never hands a thread a provisional None while another
    thread is still loading (the round-4 race of ``ops/native.py``)."""
    global _state
    if _state is not None:
        return _lib
    ok = False
    try:
        ok = _open_library()
    finally:
        _state = ok
    return _lib


def _open_library():
    global _lib
    if not os.path.exists(LIB_PATH):
        if gpu_host():
            raise GpuUnavailable("HIP library %s not built (run __graft_entry__.build())" % LIB_PATH)
        return False
    lib = ctypes.CDLL(LIB_PATH)
    i64p = ctypes.POINTER(ctypes.c_int64)
    i32p = ctypes.POINTER(ctypes.c_int32)
    for fn in (lib.m2k_ed_matrix, lib.m2k_ed_closest):
        fn.restype = ctypes.c_int
    lib.m2k_ed_matrix.argtypes = [ctypes.c_char_p, i64p, ctypes.c_int, ctypes.c_char_p, i64p, ctypes.c_int, i32p]
    lib.m2k_ed_closest.argtypes = [ctypes.c_char_p, i64p, ctypes.c_int, ctypes.c_char_p, i64p, ctypes.c_int, i32p,
                                   i32p]
    if hasattr(lib, "m2k_ed_closest_norm"):   # absent from an earlier build named by the benchmark's --lib
        lib.m2k_ed_matrix_norm.restype = lib.m2k_ed_closest_norm.restype = ctypes.c_int
        lib.m2k_ed_matrix_norm.argtypes = [ctypes.c_char_p, i64p, ctypes.c_int, ctypes.c_char_p, i64p, ctypes.c_int,
                                           ctypes.c_int, i32p]
        lib.m2k_ed_closest_norm.argtypes = [ctypes.c_char_p, i64p, ctypes.c_int, ctypes.c_char_p, i64p, ctypes.c_int,
                                            ctypes.c_int, i32p, i32p]
        lib.m2k_ed_last_fill_ms.restype = ctypes.c_double
        lib.m2k_ed_last_fill_ms.argtypes = []
    if hasattr(lib, "m2k_ed_closest_metric"):   # likewise: the metric entry points
        lib.m2k_ed_matrix_metric.restype = lib.m2k_ed_closest_metric.restype = ctypes.c_int
        lib.m2k_ed_matrix_metric.argtypes = [ctypes.c_char_p, i64p, ctypes.c_int, ctypes.c_char_p, i64p, ctypes.c_int,
                                             ctypes.c_int, ctypes.c_int, i32p]
        lib.m2k_ed_closest_metric.argtypes = [ctypes.c_char_p, i64p, ctypes.c_int, ctypes.c_char_p, i64p,
                                              ctypes.c_int, ctypes.c_int, ctypes.c_int, i32p, i32p]
    if hasattr(lib, "m2k_ed_closest_grouped"):   # likewise: the closest option per group
        lib.m2k_ed_closest_grouped.restype = ctypes.c_int
        lib.m2k_ed_closest_grouped.argtypes = [ctypes.c_char_p, i64p, ctypes.c_int, i32p, ctypes.c_int,
                                               ctypes.c_char_p, i64p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               i32p, i32p]
    if hasattr(lib, "m2k_ed_closest_k"):   # likewise: the k closest options
        lib.m2k_ed_closest_k.restype = ctypes.c_int
        lib.m2k_ed_closest_k.argtypes = [ctypes.c_char_p, i64p, ctypes.c_int, ctypes.c_char_p, i64p, ctypes.c_int,
                                         ctypes.c_int, ctypes.c_int, ctypes.c_int, i32p, i32p]
    if hasattr(lib, "m2k_ed_closest_names"):   # likewise: many names against a few options
        lib.m2k_ed_closest_names.restype = ctypes.c_int
        lib.m2k_ed_closest_names.argtypes = [ctypes.c_char_p, i64p, ctypes.c_int, i32p, ctypes.c_int,
                                             ctypes.c_char_p, i64p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             i32p, i32p]
    lib.m2k_ed_last_timings.restype = None
    lib.m2k_ed_last_timings.argtypes = [ctypes.POINTER(ctypes.c_double)]
    lib.m2k_gpu_device_count.restype = ctypes.c_int
    lib.m2k_gpu_arch.restype = ctypes.c_char_p
    _lib = lib
    return True


def available():
    try:
        lib = _load()
    except OSError:
        return False
    return lib is not None and lib.m2k_gpu_device_count() > 0


def has_entry(name):
    """Whether the loaded kernel library exports ``name`` (an earlier build named
    by the benchmark's ``--lib`` lacks the late entry points)."""
    lib = _load()
    return lib is not None and hasattr(lib, name)


_warm = False


def warm():
    """A kernel call has completed in this process (HIP runtime initialised)."""
    return _warm


def last_timings():
    """{prep, h2d, kernel, d2h, fill} milliseconds of the last kernel call.
    ``kernel_ms`` is the matcher kernels; ``fill_ms`` is the device panel fill
    of the ``*_normalized`` calls (0 for the others, whose fill is in ``prep_ms``)."""
    lib = _lib_or_raise()
    buf = (ctypes.c_double * 4)()
    lib.m2k_ed_last_timings(buf)
    out = dict(zip(("prep_ms", "h2d_ms", "kernel_ms", "d2h_ms"), (round(x, 3) for x in buf)))
    out["fill_ms"] = round(lib.m2k_ed_last_fill_ms(), 3) if hasattr(lib, "m2k_ed_last_fill_ms") else 0.0
    return out


def device_arch():
    lib = _load()
    return lib.m2k_gpu_arch().decode() if lib is not None else ""


def _pack(strings):
    """(packed bytes, int64 offsets[n+1], max length)."""
    from . import native
    m = native.module()
    if m is not None and isinstance(strings, list):
        data, off, maxlen = m.pack_strings(strings)
        return data, off, int(maxlen)
    bs = [s.encode("utf-8", "surrogateescape") if isinstance(s, str) else bytes(s) for s in strings]
    lens = np.fromiter((len(b) for b in bs), dtype=np.int64, count=len(bs))
    off = np.zeros(len(bs) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    return b"".join(bs), off, int(lens.max()) if len(bs) else 0


def _ptr(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def _lib_or_raise():
    lib = _load()
    if lib is None:
        raise GpuUnavailable("HIP library not available")
    return lib


# Metrics of the kernel library (``run()`` in ``ed_kernel.hip``): INDEL2 is
# ins = del = 1, sub = 2 (the LCS kernels), LEVENSHTEIN is ins = del = sub = 1
# (the Myers kernels).  Normalising modes: NO_MODE matches the strings as they are.
INDEL2 = 0
LEVENSHTEIN = 1
NO_MODE = 0
ALNUM_LOWER = 1


def _metric_fn(lib, name, metric):
    if metric not in (INDEL2, LEVENSHTEIN):
        raise ValueError("unknown metric %r" % (metric,))
    if not hasattr(lib, name):
        raise GpuUnavailable("this build of the HIP library has no %s (rebuild it for metric %d)" % (name, metric))
    return getattr(lib, name)


def ed_matrix(options, queries, metric=INDEL2):
    """Distance matrix, shape [len(options), len(queries)] (int32 numpy view of a
    query-major device result).  Every query must be <= MAX_QUERY_BYTES.
    ``metric``: INDEL2 (the default) or LEVENSHTEIN."""
    lib = _lib_or_raise()
    na, nb = len(options), len(queries)
    if na == 0 or nb == 0:
        return np.zeros((na, nb), dtype=np.int32)
    a, offa, _ = _pack(options)
    q, offb, qmax = _pack(queries)
    if qmax > MAX_QUERY_BYTES:
        raise GpuUnsupportedInput("queries longer than %d bytes are not supported on the GPU path" % MAX_QUERY_BYTES)
    outT = np.empty((nb, na), dtype=np.int32)
    if metric == INDEL2:
        rc = lib.m2k_ed_matrix(a, _ptr(offa, ctypes.c_int64), na, q, _ptr(offb, ctypes.c_int64), nb,
                               _ptr(outT, ctypes.c_int32))
    else:
        rc = _metric_fn(lib, "m2k_ed_matrix_metric", metric)(
            a, _ptr(offa, ctypes.c_int64), na, q, _ptr(offb, ctypes.c_int64), nb, NO_MODE, metric,
            _ptr(outT, ctypes.c_int32))
    if rc in _RC_UNSUPPORTED:
        raise GpuUnsupportedInput("m2k_ed_matrix cannot take this input (code %d)" % rc)
    if rc != 0:
        raise GpuUnavailable("m2k_ed_matrix failed with code %d" % rc)
    global _warm
    _warm = True
    return outT.T


def ed_closest(options, queries, metric=INDEL2):
    """(index, distance) int32 arrays: for every query the first option with the
    minimum distance (-1, -1 when there are no options).  ``metric`` as in
    :func:`ed_matrix`."""
    lib = _lib_or_raise()
    na, nb = len(options), len(queries)
    idx = np.full(nb, -1, dtype=np.int32)
    dist = np.full(nb, -1, dtype=np.int32)
    if nb == 0 or na == 0:
        return idx, dist
    a, offa, _ = _pack(options)
    q, offb, qmax = _pack(queries)
    if qmax > MAX_QUERY_BYTES:
        raise GpuUnsupportedInput("queries longer than %d bytes are not supported on the GPU path" % MAX_QUERY_BYTES)
    if metric == INDEL2:
        rc = lib.m2k_ed_closest(a, _ptr(offa, ctypes.c_int64), na, q, _ptr(offb, ctypes.c_int64), nb,
                                _ptr(idx, ctypes.c_int32), _ptr(dist, ctypes.c_int32))
    else:
        rc = _metric_fn(lib, "m2k_ed_closest_metric", metric)(
            a, _ptr(offa, ctypes.c_int64), na, q, _ptr(offb, ctypes.c_int64), nb, NO_MODE, metric,
            _ptr(idx, ctypes.c_int32), _ptr(dist, ctypes.c_int32))
    if rc in _RC_UNSUPPORTED:
        raise GpuUnsupportedInput("m2k_ed_closest cannot take this input (code %d)" % rc)
    if rc != 0:
        raise GpuUnavailable("m2k_ed_closest failed with code %d" % rc)
    global _warm
    _warm = True
    return idx, dist


def ed_matrix_normalized(options, queries, mode=ALNUM_LOWER, metric=INDEL2):
    """:func:`ed_matrix` of the normalised strings, from the raw ones: keep
    ``0-9 a-z A-Z``, fold to lower case, drop every other byte.  The options are
    normalised on the device as their panels are filled; MAX_QUERY_BYTES applies
    to the normalised queries."""
    lib = _lib_or_raise()
    na, nb = len(options), len(queries)
    if na == 0 or nb == 0:
        return np.zeros((na, nb), dtype=np.int32)
    a, offa, _ = _pack(options)
    q, offb, _ = _pack(queries)
    outT = np.empty((nb, na), dtype=np.int32)
    if metric == INDEL2:
        rc = lib.m2k_ed_matrix_norm(a, _ptr(offa, ctypes.c_int64), na, q, _ptr(offb, ctypes.c_int64), nb, mode,
                                    _ptr(outT, ctypes.c_int32))
    else:
        rc = _metric_fn(lib, "m2k_ed_matrix_metric", metric)(
            a, _ptr(offa, ctypes.c_int64), na, q, _ptr(offb, ctypes.c_int64), nb, mode, metric,
            _ptr(outT, ctypes.c_int32))
    _check_norm_rc("m2k_ed_matrix_norm", rc)
    return outT.T


def ed_closest_normalized(options, queries, mode=ALNUM_LOWER, metric=INDEL2):
    """:func:`ed_closest` of the normalised strings, from the raw ones (see
    :func:`ed_matrix_normalized`)."""
    lib = _lib_or_raise()
    na, nb = len(options), len(queries)
    idx = np.full(nb, -1, dtype=np.int32)
    dist = np.full(nb, -1, dtype=np.int32)
    if nb == 0 or na == 0:
        return idx, dist
    a, offa, _ = _pack(options)
    q, offb, _ = _pack(queries)
    if metric == INDEL2:
        rc = lib.m2k_ed_closest_norm(a, _ptr(offa, ctypes.c_int64), na, q, _ptr(offb, ctypes.c_int64), nb, mode,
                                     _ptr(idx, ctypes.c_int32), _ptr(dist, ctypes.c_int32))
    else:
        rc = _metric_fn(lib, "m2k_ed_closest_metric", metric)(
            a, _ptr(offa, ctypes.c_int64), na, q, _ptr(offb, ctypes.c_int64), nb, mode, metric,
            _ptr(idx, ctypes.c_int32), _ptr(dist, ctypes.c_int32))
    _check_norm_rc("m2k_ed_closest_norm", rc)
    return idx, dist


def ed_closest_grouped(options, group_of, n_groups, queries, mode=NO_MODE, metric=INDEL2):
    """The closest option of every group: ``group_of[i]`` in ``[0, n_groups)`` is
    the group of ``options[i]``.  Returns (index, distance) int32 arrays of shape
    ``[len(queries), n_groups]``; ``index`` is into the flat ``options`` (the
    first of the group's closest ones), -1 / -1 for a group without options.
    One pass over the options serves every group.  ``mode``: NO_MODE or
    ALNUM_LOWER (see :func:`ed_matrix_normalized`); ``metric`` as in :func:`ed_matrix`."""
    lib = _lib_or_raise()
    fn = _metric_fn(lib, "m2k_ed_closest_grouped", metric)
    groups = np.ascontiguousarray(group_of, dtype=np.int32)
    na, nb = len(options), len(queries)
    if groups.shape != (na,):
        raise ValueError("group_of needs one group id per option")
    if n_groups < 1:
        raise ValueError("n_groups must be >= 1")
    idx = np.full((nb, n_groups), -1, dtype=np.int32)
    dist = np.full((nb, n_groups), -1, dtype=np.int32)
    if nb == 0 or na == 0:
        return idx, dist
    a, offa, _ = _pack(options)
    q, offb, qmax = _pack(queries)
    if mode == NO_MODE and qmax > MAX_QUERY_BYTES:
        raise GpuUnsupportedInput("queries longer than %d bytes are not supported on the GPU path" % MAX_QUERY_BYTES)
    rc = fn(a, _ptr(offa, ctypes.c_int64), na, _ptr(groups, ctypes.c_int32), n_groups, q,
            _ptr(offb, ctypes.c_int64), nb, mode, metric, _ptr(idx, ctypes.c_int32), _ptr(dist, ctypes.c_int32))
    if rc == -11:
        raise ValueError("m2k_ed_closest_grouped: group ids must lie in [0, n_groups)")
    _check_norm_rc("m2k_ed_closest_grouped", rc)
    return idx, dist


def ed_closest_k(options, queries, k, mode=NO_MODE, metric=INDEL2):
    """The ``k`` closest options of every query: (index, distance) int32 arrays of
    shape ``[len(queries), k]``, row ``j`` in (distance, option index) order, so
    column 0 is :func:`ed_closest`'s answer; -1 / -1 behind the last option.
    ``k`` is at most MAX_K.  The selection runs on the device (one sorted list
    per wave, then a merge): only ``k`` pairs per query come back.  ``mode`` and
    ``metric`` as in :func:`ed_closest_grouped`."""
    if k < 1:
        raise ValueError("k must be >= 1")
    if k > MAX_K:
        raise GpuUnsupportedInput("the GPU path ranks at most %d options per query" % MAX_K)
    fn = _metric_fn(_lib_or_raise(), "m2k_ed_closest_k", metric)
    na, nb = len(options), len(queries)
    idx = np.full((nb, k), -1, dtype=np.int32)
    dist = np.full((nb, k), -1, dtype=np.int32)
    if nb == 0 or na == 0:
        return idx, dist
    a, offa, _ = _pack(options)
    q, offb, qmax = _pack(queries)
    if mode == NO_MODE and qmax > MAX_QUERY_BYTES:
        raise GpuUnsupportedInput("queries longer than %d bytes are not supported on the GPU path" % MAX_QUERY_BYTES)
    rc = fn(a, _ptr(offa, ctypes.c_int64), na, q, _ptr(offb, ctypes.c_int64), nb, k, mode, metric,
            _ptr(idx, ctypes.c_int32), _ptr(dist, ctypes.c_int32))
    _check_norm_rc("m2k_ed_closest_k", rc)
    return idx, dist


def ed_closest_names(options, names, group_of=None, n_groups=1, mode=NO_MODE, metric=INDEL2):
    """:func:`ed_closest` / :func:`ed_closest_grouped` for a few options against
    very many names, with the sides' roles swapped on the device: the names fill
    the lanes and the options' tables sit in LDS.  Returns (index, distance)
    int32 arrays of shape ``[len(names)]``, or ``[len(names), n_groups]`` with
    ``group_of`` (one group id in ``[0, n_groups)`` per option); ``index`` is into
    the flat ``options``, the first of the closest ones, -1 / -1 for a group
    without options.  Here MAX_QUERY_BYTES limits the *options* (after
    normalisation under ``mode``); the names may be of any length.  ``mode`` and
    ``metric`` as in :func:`ed_closest_grouped`."""
    fn = _metric_fn(_lib_or_raise(), "m2k_ed_closest_names", metric)
    na, nb = len(options), len(names)
    groups = None
    if group_of is not None:
        groups = np.ascontiguousarray(group_of, dtype=np.int32)
        if groups.shape != (na,):
            raise ValueError("group_of needs one group id per option")
        if n_groups < 1:
            raise ValueError("n_groups must be >= 1")
    shape = (nb, n_groups) if groups is not None else (nb,)
    idx = np.full(shape, -1, dtype=np.int32)
    dist = np.full(shape, -1, dtype=np.int32)
    if nb == 0 or na == 0:
        return idx, dist
    a, offa, amax = _pack(options)
    q, offb, _ = _pack(names)
    if mode == NO_MODE and amax > MAX_QUERY_BYTES:
        raise GpuUnsupportedInput("options longer than %d bytes are not supported on the names route"
                                  % MAX_QUERY_BYTES)
    rc = fn(a, _ptr(offa, ctypes.c_int64), na, _ptr(groups, ctypes.c_int32) if groups is not None else None,
            n_groups, q, _ptr(offb, ctypes.c_int64), nb, mode, metric, _ptr(idx, ctypes.c_int32),
            _ptr(dist, ctypes.c_int32))
    if rc == -11:
        raise ValueError("m2k_ed_closest_names: group ids must lie in [0, n_groups)")
    _check_norm_rc("m2k_ed_closest_names", rc)
    return idx, dist


def _check_norm_rc(name, rc):
    global _warm
    if rc in _RC_UNSUPPORTED:
        raise GpuUnsupportedInput("%s cannot take this input (code %d; queries normalise to <= %d bytes)"
                                  % (name, rc, MAX_QUERY_BYTES))
    if rc != 0:
        raise GpuUnavailable("%s failed with code %d" % (name, rc))
    _warm = True

"""Weighted edit distance (smetrics.WagnerFischer(a, b, 1, 1, 2)) with dispatch.

Small problems (the common case: a handful of options) run on the CPU; large
all-pairs batches (CF foundation exports: thousands of app buildpack names x
builder buildpack lists) are offloaded to the MI355X kernel in
``ed_kernel.hip`` when a GPU is present.
"""

import os
import sys

from . import native
from ..utils.lazyre import lazy as _lazy_re

# numpy and the HIP wrapper (which needs numpy) are imported on first use:
# importing numpy costs more than the handful of matches a CLI run makes
# (``closest_index_list``).


def _np():
    import numpy
    return numpy


def _gpu():
    from . import gpu
    return gpu

# Crossover measured on MI355X (profiles/r01_ed_crossover.log): once the HIP
# runtime is up, the GPU wins from ~8k pairs (0.09 ms vs 0.09-0.22 ms on 16
# threads); the first HIP call of a process costs ~280 ms, which the CPU path
# only exceeds around 10^8 pairs.
GPU_MIN_PAIRS = int(os.environ.get("M2K_GPU_MIN_PAIRS", "8192"))
GPU_MIN_PAIRS_COLD = int(os.environ.get("M2K_GPU_MIN_PAIRS_COLD", "100000000"))


def _gpu_warm():
    """True when this process already paid the HIP start-up (our library ran,
    or torch initialised the device)."""
    if "move2kube_amd.ops.gpu" in sys.modules and _gpu().warm():
        return True
    torch = sys.modules.get("torch")
    try:
        return bool(torch is not None and torch.cuda.is_initialized())
    except Exception:  # noqa: BLE001
        return False


def wagner_fischer_py(a, b, icost=1, dcost=1, scost=2):
    if isinstance(a, str):
        a = a.encode("utf-8", "surrogateescape")
    if isinstance(b, str):
        b = b.encode("utf-8", "surrogateescape")
    row1 = [j * icost for j in range(len(b) + 1)]
    for i in range(1, len(a) + 1):
        row2 = [i * dcost] + [0] * len(b)
        ai = a[i - 1]
        for j in range(1, len(b) + 1):
            if ai == b[j - 1]:
                row2[j] = row1[j - 1]
            else:
                ins = row2[j - 1] + icost
                dele = row1[j] + dcost
                sub = row1[j - 1] + scost
                if ins < dele and ins < sub:
                    row2[j] = ins
                elif dele < sub:
                    row2[j] = dele
                else:
                    row2[j] = sub
        row1 = row2
    return row1[len(b)]


# ``normalize="alnum_lower"``: the distances are those of the strings with every
# character outside [a-zA-Z0-9] removed and the rest lower-cased, which is what
# the reference's GetClosestMatchingString compares (utils.go:377-401).  What
# is left is ASCII, so ``str.lower`` is Go's ``strings.ToLower`` here.  The GPU
# path takes the raw strings and normalises on the device.
_NON_ALNUM_RE = _lazy_re(r"[^a-zA-Z0-9]+")


def _check_normalize(normalize):
    if normalize not in (None, "alnum_lower"):
        raise ValueError("normalize must be None or 'alnum_lower', not %r" % (normalize,))


def normalize_alnum_lower(s):
    if not isinstance(s, str):
        s = bytes(s).decode("utf-8", "surrogateescape")
    return _NON_ALNUM_RE.sub("", s).lower()


def _normalized(strings, normalize):
    return [normalize_alnum_lower(s) for s in strings] if normalize else strings


def _use_gpu(pairs, device, queries, normalize=None):
    if device == "cpu":
        return False
    if device != "gpu" and pairs < GPU_MIN_PAIRS:
        return False
    gpu = _gpu()
    if normalize:   # the limit applies after normalisation: the kernel library checks it
        if device == "gpu":
            return True
        return gpu.gpu_host() and (pairs >= GPU_MIN_PAIRS_COLD or _gpu_warm())
    # the limit belongs to the kernel library; one that states none has the single-word kernels' 64
    limit = getattr(gpu, "MAX_QUERY_BYTES", 64)
    fits = all(len(q.encode("utf-8", "surrogateescape") if isinstance(q, str) else q) <= limit for q in queries)
    if device == "gpu":
        if not fits:
            raise gpu.GpuUnsupportedInput("queries longer than %d bytes are not supported on the GPU path" % limit)
        return True
    if not fits or pairs < GPU_MIN_PAIRS or not gpu.gpu_host():
        return False
    return pairs >= GPU_MIN_PAIRS_COLD or _gpu_warm()


# The names route (``gpu.ed_closest_names``): a few options against very many
# queries run with the sides' roles swapped on the device.  It is taken only
# after ``_use_gpu`` has chosen the GPU, so limits, fallbacks and exceptions are
# those of the functions below (``_names_fn`` keeps a request that today's route
# would refuse on today's route), and the answers are the same by construction.
# Constants from the sweeps on MI355X (docs/history.md, "Many names against a
# few options"): at 16, 64 and 256 options the route's end-to-end range lay
# wholly below today's from 64 queries per option on, grouped or not, and at 16
# per option it did not; 1024 and 4096 options were measured at 1M names only,
# so the bound on the options stays at the largest count swept over both.
# The sweep over the name count was made with ``normalize="alnum_lower"`` (the
# device fills the panels) and costs (1, 1, 2); costs (1, 1, 1) were measured
# at the rule's edge and at 1M names only: wholly below at 64 queries per option
# and at 1M, not at every option count at 16 per option.  ``normalize=None`` (the host fills the panels) is routed by the
# same rule and was not measured.
NAMES_ROUTE_MAX_OPTIONS = 256
NAMES_ROUTE_MIN_QUERIES_PER_OPTION = 64


def names_route(na, nb):
    """Whether ``na`` options against ``nb`` queries go to the names kernels."""
    return 0 < na <= NAMES_ROUTE_MAX_OPTIONS and nb >= NAMES_ROUTE_MIN_QUERIES_PER_OPTION * na


def _names_fn(gpu, options, queries, normalize):
    """``gpu.ed_closest_names`` when the request is of the names route's shape
    and the kernel library (or a stand-in module) has it, else None.  An option
    over the kernels' limit keeps today's route, which has no limit on them.  So
    does a query over it: the names kernels would take it, but today's route
    refuses it, and these functions' exceptions and fallbacks stay as they were.
    Without ``normalize`` ``_use_gpu`` has checked the queries already; with it
    the kernel library checks them after normalisation, which only drops
    characters, so only a query that is over the limit raw is normalised here."""
    fn = getattr(gpu, "ed_closest_names", None)
    if fn is None or not names_route(len(options), len(queries)):
        return None
    has = getattr(gpu, "has_entry", None)
    if has is not None and not has("m2k_ed_closest_names"):
        return None
    limit = getattr(gpu, "MAX_QUERY_BYTES", 64)
    if any(len(o.encode("utf-8", "surrogateescape") if isinstance(o, str) else o) > limit for o in options):
        return None
    if normalize and max(map(len, queries)) > limit and any(
            len(q) > limit and len(normalize_alnum_lower(q)) > limit for q in queries):
        return None
    return fn


# costs = (insertion, deletion, substitution).  The GPU kernels serve two
# triples: the default (1, 1, 2), whose path is untouched by the argument, and
# (1, 1, 1), plain Levenshtein distance, under the same dispatch rules.  Every
# other triple is the CPU's scalar DP.
DEFAULT_COSTS = (1, 1, 2)
LEVENSHTEIN_COSTS = (1, 1, 1)


def _check_costs(costs, device):
    costs = tuple(costs)
    if len(costs) != 3 or any(not isinstance(c, int) or c < 0 for c in costs):
        raise ValueError("costs must be three non-negative integers (insert, delete, substitute), not %r" % (costs,))
    if costs not in (DEFAULT_COSTS, LEVENSHTEIN_COSTS):
        if device == "gpu":
            raise _gpu().GpuUnsupportedInput("the GPU kernels take costs (1, 1, 2) and (1, 1, 1), not %r" % (costs,))
        device = "cpu"
    return costs, device


def _gpu_kwargs(costs):
    """Nothing for the default costs: their calls stay as they were."""
    return {} if costs == DEFAULT_COSTS else {"metric": _gpu().LEVENSHTEIN}


def _cpu_matrix(options, queries, costs):
    na, nb = len(options), len(queries)
    m = native.module()
    if m is not None:
        return m.edit_distance_batch(list(options), list(queries), costs[0], costs[1], costs[2], _threads())
    np = _np()
    return np.array([[wagner_fischer_py(o, q, *costs) for q in queries] for o in options],
                    dtype=np.int32).reshape(na, nb)


def _cpu_closest(options, queries, costs):
    """Other costs than the default: the first minimum of every matrix column."""
    np = _np()
    d = _cpu_matrix(options, queries, costs)
    idx = d.argmin(axis=0).astype(np.int32)
    return idx, d[idx, np.arange(len(queries))].astype(np.int32)


def _threads():
    from ..utils.constants import host_threads
    return host_threads(16)


def matrix(options, queries, device="auto", normalize=None, costs=DEFAULT_COSTS):
    """Distance matrix, int32 array of shape [len(options), len(queries)].

    device: "auto" | "cpu" | "gpu"; normalize: None | "alnum_lower";
    costs: (insert, delete, substitute)."""
    _check_normalize(normalize)
    costs, device = _check_costs(costs, device)
    na, nb = len(options), len(queries)
    if _use_gpu(na * nb, device, queries, normalize):
        gpu = _gpu()
        try:
            kw = _gpu_kwargs(costs)
            return (gpu.ed_matrix_normalized(options, queries, **kw) if normalize
                    else gpu.ed_matrix(options, queries, **kw))
        except gpu.GpuUnsupportedInput:
            if device == "gpu":
                raise
    options, queries = _normalized(options, normalize), _normalized(queries, normalize)
    return _cpu_matrix(options, queries, costs)


def closest_indices(options, queries, device="auto", normalize=None, costs=DEFAULT_COSTS):
    """For every query the index of the first option with the minimum distance
    and that distance (int32 arrays; -1 when there are no options).  The argmin
    is fused into the distance computation (GPU kernel or native CPU; for costs
    other than the default the CPU takes it from the matrix)."""
    _check_normalize(normalize)
    costs, device = _check_costs(costs, device)
    na, nb = len(options), len(queries)
    np = _np()
    if na == 0 or nb == 0:
        return np.full(nb, -1, dtype=np.int32), np.full(nb, -1, dtype=np.int32)
    if _use_gpu(na * nb, device, queries, normalize):
        gpu = _gpu()
        try:
            kw = _gpu_kwargs(costs)
            names_fn = _names_fn(gpu, options, queries, normalize)
            if names_fn is not None:
                return names_fn(options, queries, mode=gpu.ALNUM_LOWER if normalize else gpu.NO_MODE, **kw)
            return (gpu.ed_closest_normalized(options, queries, **kw) if normalize
                    else gpu.ed_closest(options, queries, **kw))
        except gpu.GpuUnsupportedInput:
            if device == "gpu":
                raise
    options, queries = _normalized(options, normalize), _normalized(queries, normalize)
    if costs != DEFAULT_COSTS:
        return _cpu_closest(options, queries, costs)
    m = native.module()
    if m is not None:
        return m.closest_batch(list(options), list(queries), _threads())
    idx, dist = _closest_py(options, queries)
    return np.array(idx, dtype=np.int32), np.array(dist, dtype=np.int32)


def closest_in_groups(groups, queries, device="auto", normalize=None, costs=DEFAULT_COSTS):
    """:func:`closest_indices` within every group of options at once.

    ``groups`` is a sequence of option lists.  Returns (idx, dist), int32 arrays
    of shape [len(queries), len(groups)]: ``idx[j, g]`` is the position within
    ``groups[g]`` of its first option closest to ``queries[j]``, ``dist[j, g]``
    the distance, -1 / -1 for an empty group.  On the GPU it is one pass over
    all options (the grouped kernels); on the CPU one call per group."""
    _check_normalize(normalize)
    costs, device = _check_costs(costs, device)
    np = _np()
    groups = [list(g) for g in groups]
    nb, ng = len(queries), len(groups)
    sizes = [len(g) for g in groups]
    idx = np.full((nb, ng), -1, dtype=np.int32)
    dist = np.full((nb, ng), -1, dtype=np.int32)
    if nb == 0 or sum(sizes) == 0:
        return idx, dist
    if _use_gpu(sum(sizes) * nb, device, queries, normalize):
        gpu = _gpu()
        try:
            first = np.cumsum([0] + sizes[:-1]).astype(np.int32)
            flat_options, group_of = [o for g in groups for o in g], np.repeat(np.arange(ng, dtype=np.int32), sizes)
            mode = gpu.ALNUM_LOWER if normalize else gpu.NO_MODE
            names_fn = _names_fn(gpu, flat_options, queries, normalize)
            if names_fn is not None:
                flat, dist = names_fn(flat_options, queries, group_of, ng, mode=mode, **_gpu_kwargs(costs))
            else:
                flat, dist = gpu.ed_closest_grouped(flat_options, group_of, ng, queries, mode=mode,
                                                    **_gpu_kwargs(costs))
            return np.where(flat < 0, flat, flat - first[None, :]).astype(np.int32), dist
        except gpu.GpuUnsupportedInput:
            if device == "gpu":
                raise
    for g, options in enumerate(groups):
        idx[:, g], dist[:, g] = closest_indices(options, queries, "cpu", normalize, costs)
    return idx, dist


def closest_k(options, queries, k, device="auto", normalize=None, costs=DEFAULT_COSTS):
    """The ``k`` closest options of every query, closest first.

    Returns (idx, dist), int32 arrays of shape [len(queries), k]: row ``j`` is
    the first ``k`` entries of query ``j``'s matrix column in (distance, option
    index) order, so column 0 is :func:`closest_indices`; -1 / -1 where the
    options run out.  On the GPU the selection is fused into the distance pass
    (the top-k kernels, ``k`` up to ``gpu.MAX_K``); the CPU sorts the matrix."""
    _check_normalize(normalize)
    costs, device = _check_costs(costs, device)
    if k < 1:
        raise ValueError("k must be >= 1, not %r" % (k,))
    np = _np()
    na, nb = len(options), len(queries)
    idx = np.full((nb, k), -1, dtype=np.int32)
    dist = np.full((nb, k), -1, dtype=np.int32)
    if na == 0 or nb == 0:
        return idx, dist
    if k > _gpu().MAX_K:
        if device == "gpu":
            raise _gpu().GpuUnsupportedInput("the GPU path ranks at most %d options per query" % _gpu().MAX_K)
        device = "cpu"
    if _use_gpu(na * nb, device, queries, normalize):
        gpu = _gpu()
        try:
            return gpu.ed_closest_k(options, queries, k, mode=gpu.ALNUM_LOWER if normalize else gpu.NO_MODE,
                                    **_gpu_kwargs(costs))
        except gpu.GpuUnsupportedInput:
            if device == "gpu":
                raise
    d = _cpu_matrix(_normalized(options, normalize), _normalized(queries, normalize), costs)
    order = np.argsort(d, axis=0, kind="stable")[:k]
    idx[:, :len(order)] = order.T
    dist[:, :len(order)] = np.take_along_axis(d, order, axis=0).T
    return idx, dist


def _closest_py(options, queries):
    idx, dist = [], []
    for q in queries:
        bi, bd = -1, -1
        for i, o in enumerate(options):
            d = wagner_fischer_py(o, q)
            if bi < 0 or d < bd:
                bi, bd = i, d
        idx.append(bi)
        dist.append(bd)
    return idx, dist


def closest_index_list(options, queries, device="auto", normalize=None, costs=DEFAULT_COSTS):
    """:func:`closest_indices` as two Python lists.  Below the GPU threshold
    this path never imports numpy with the default costs (the native
    ``closest_list``)."""
    _check_normalize(normalize)
    costs, device = _check_costs(costs, device)
    na, nb = len(options), len(queries)
    if na == 0 or nb == 0:
        return [-1] * nb, [-1] * nb
    if _use_gpu(na * nb, device, queries, normalize):
        idx, dist = closest_indices(options, queries, device, normalize, costs)
        return [int(i) for i in idx], [int(d) for d in dist]
    options, queries = _normalized(options, normalize), _normalized(queries, normalize)
    if costs != DEFAULT_COSTS:
        idx, dist = _cpu_closest(options, queries, costs)
        return [int(i) for i in idx], [int(d) for d in dist]
    m = native.module()
    if m is not None:
        return m.closest_list(list(options), list(queries), _threads())
    return _closest_py(options, queries)


def distances(options, search):
    """Distances of each option to one search string."""
    return [int(x) for x in matrix(options, [search])[:, 0]] if options else []


def closest(options, search):
    if not options:
        return ""
    idx, _ = closest_index_list(options, [search])
    return options[idx[0]]

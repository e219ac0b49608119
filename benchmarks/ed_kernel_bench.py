#!/usr/bin/env python3
"""Micro-benchmark of the batched fuzzy-matching path: gfx950 kernel vs the
native multi-threaded CPU implementation, on a synthetic "CF foundation"
(N app/buildpack names x M builder buildpack ids).  Prints one JSON line.

``--qmin L --qmax L`` makes every query L bytes, which runs one tile class
alone (64, 128, 256: K64, K128, K256); ``--lib`` times another build of the
kernel library, e.g. an earlier commit's, one process per library;
``--groups G`` times the closest option per group (see ``bench_groups``);
``--topk K`` times the K closest options per query (see ``bench_topk``);
``--names-route on`` times a few options against very many names (see
``bench_names``)."""

import argparse
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from move2kube_amd.ops import gpu, native  # noqa: E402


def words(rng, n, lo, hi, alpha="abcdefghijklmnopqrstuvwxyz_-0123456789"):
    return ["".join(rng.choice(alpha) for _ in range(rng.randint(lo, hi))) for _ in range(n)]


def raw_names(rng, names):
    """Names as a caller has them: first letter upper case and about one
    separator per 8 characters."""
    out = []
    for s in names:
        cs = list(s[:1].upper() + s[1:])
        for at in sorted((rng.randrange(len(cs) + 1) for _ in range((len(cs) + 7) // 8)), reverse=True):
            cs.insert(at, rng.choice("-_. /"))
        out.append("".join(cs))
    return out


def panel_blocks(names):
    """16-byte blocks the panels of these options take: 512 options per panel in
    length order, every slot as long as the panel's longest."""
    lens = sorted(len(s) for s in names)
    return sum((lens[min(len(lens), at + 512) - 1] + 15) // 16 * 512 for at in range(0, len(lens), 512))


def bench_raw(a, res):
    """Two routes from raw names to the closest option, in one process:
    (a) normalise in Python, then ``ed_closest``; (b) ``ed_closest_normalized``."""
    from move2kube_amd.ops.editdistance import normalize_alnum_lower
    rng = random.Random(0)
    alnum = "abcdefghijklmnopqrstuvwxyz0123456789"
    opts = raw_names(rng, words(rng, a.options, 4, 40, alnum))
    qs = raw_names(rng, words(rng, a.queries, min(a.qmin, a.qmax), a.qmax, alnum))
    res.update(raw=True, queries=len(qs), option_bytes=sum(len(o) for o in opts))
    gpu.ed_closest(opts[:1024], [normalize_alnum_lower(q) for q in qs[:8]])  # warm-up / context creation
    gpu.ed_closest_normalized(opts[:1024], qs[:8])
    ta, tn, tb, ka, kb = [], [], [], [], []
    for _ in range(a.reps):   # the routes alternate
        t0 = time.perf_counter()
        no, nq = [normalize_alnum_lower(o) for o in opts], [normalize_alnum_lower(q) for q in qs]
        t1 = time.perf_counter()
        ra = gpu.ed_closest(no, nq)
        t2 = time.perf_counter()
        ka.append(gpu.last_timings())
        t3 = time.perf_counter()
        rb = gpu.ed_closest_normalized(opts, qs)
        t4 = time.perf_counter()
        kb.append(gpu.last_timings())
        tn.append(t1 - t0)
        ta.append(t2 - t1)
        tb.append(t4 - t3)
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    res["routes_agree"] = bool((ra[0] == rb[0]).all() and (ra[1] == rb[1]).all())
    res["a_python_normalise_s"] = med(tn)
    res["a_gpu_closest_s"] = med(ta)
    res["a_end_to_end_s"] = med([x + y for x, y in zip(tn, ta)])
    res["b_end_to_end_s"] = med(tb)
    for key in ("prep_ms", "h2d_ms", "fill_ms", "kernel_ms", "d2h_ms"):
        res["a_" + key] = med([k[key] for k in ka])
        res["b_" + key] = med([k[key] for k in kb])
    res["panel_blocks_raw"] = panel_blocks(opts)
    res["panel_blocks_normalised"] = panel_blocks(no)
    res["arch"] = gpu.device_arch()
    if not res["routes_agree"]:
        raise SystemExit("the two routes disagree: " + json.dumps(res))


def bench_groups(a, split):
    """The closest option per group, two routes from raw names in one process:
    (a) one ``ed_closest_grouped`` call; (b) one ``ed_closest_normalized`` call
    per group, which is what a caller without the grouped kernels makes.  The
    routes alternate after both are warm and their answers are compared.
    ``split``: "equal" group sizes or "skewed" (sizes ~ 1 / rank)."""
    import numpy as np
    rng = random.Random(0)
    alnum = "abcdefghijklmnopqrstuvwxyz0123456789"
    opts = raw_names(rng, words(rng, a.options, 4, 40, alnum))
    qs = raw_names(rng, words(rng, a.queries, min(a.qmin, a.qmax), a.qmax, alnum))
    G = a.groups
    weight = np.ones(G) if split == "equal" else 1.0 / np.arange(1, G + 1)
    ends = np.round(np.cumsum(weight) / weight.sum() * len(opts)).astype(np.int64)
    sizes = np.diff(np.concatenate(([0], ends)))
    group_of = np.repeat(np.arange(G, dtype=np.int32), sizes)
    groups = [opts[e - n:e] for n, e in zip(sizes, ends)]
    metric = gpu.LEVENSHTEIN if a.costs == "1,1,1" else gpu.INDEL2
    res = {"groups": G, "split": split, "options": len(opts), "queries": len(qs), "qmin": min(a.qmin, a.qmax),
           "qmax": a.qmax, "reps": a.reps, "costs": a.costs, "largest_group": int(sizes.max()),
           "smallest_group": int(sizes.min())}

    def per_group():
        idx = np.full((len(qs), G), -1, dtype=np.int32)
        dist = idx.copy()
        kernel = 0.0
        for g, (options, first) in enumerate(zip(groups, ends - sizes)):
            if options:
                i, dist[:, g] = gpu.ed_closest_normalized(options, qs, metric=metric)
                idx[:, g] = i + first
                kernel += gpu.last_timings()["kernel_ms"]
        return idx, dist, kernel

    gpu.ed_closest_grouped(opts[:1024], group_of[:1024], G, qs[:8], mode=gpu.ALNUM_LOWER, metric=metric)
    gpu.ed_closest_normalized(opts[:1024], qs[:8], metric=metric)
    gpu.ed_closest_grouped(opts, group_of, G, qs, mode=gpu.ALNUM_LOWER, metric=metric)   # arena at full size
    ta, tb, ka, kb, fixed = [], [], [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        ra = gpu.ed_closest_grouped(opts, group_of, G, qs, mode=gpu.ALNUM_LOWER, metric=metric)
        t1 = time.perf_counter()
        lt = gpu.last_timings()
        ka.append(lt["kernel_ms"])
        fixed.append(round((t1 - t0) * 1e3 - lt["kernel_ms"], 3))
        t2 = time.perf_counter()
        rb = per_group()
        t3 = time.perf_counter()
        kb.append(round(rb[2], 3))
        ta.append(round((t1 - t0) * 1e3, 3))
        tb.append(round((t3 - t2) * 1e3, 3))
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    res["routes_agree"] = bool((ra[0] == rb[0]).all() and (ra[1] == rb[1]).all())
    res.update(grouped_ms=ta, per_group_ms=tb, grouped_kernel_ms=ka, per_group_kernel_ms=kb,
               grouped_outside_kernel_ms=fixed, grouped_median_ms=med(ta), per_group_median_ms=med(tb),
               speedup_end_to_end=round(med(tb) / med(ta), 3), kernel_ratio=round(med(ka) / med(kb), 4),
               arch=gpu.device_arch())
    print(json.dumps(res), flush=True)
    if not res["routes_agree"]:
        raise SystemExit("the two routes disagree")


def host_topk(d, k):
    """The first ``k`` of every column of ``d`` in (distance, index) order: a
    partition per column, ties at the k-th distance taken in index order."""
    import numpy as np
    idx = np.full((d.shape[1], k), -1, dtype=np.int32)
    for j in range(d.shape[1]):
        col = d[:, j]
        kth = np.partition(col, k - 1)[k - 1]
        below = np.flatnonzero(col < kth)
        cand = np.concatenate((below, np.flatnonzero(col == kth)[:k - len(below)]))
        idx[j] = cand[np.lexsort((cand, col[cand]))]
    return idx, np.take_along_axis(d, idx.T, axis=0).T


def bench_topk(a):
    """A ranked list of ``--topk`` options per query, from raw names, three
    calls alternating in one process after all are warm, every one ending in a
    stream synchronise: (a) ``ed_closest_k``; (b) ``ed_closest_normalized`` at
    the same shape (what the selection costs over the plain argmin: compare the
    kernel times at K = 1); (c) ``ed_matrix_normalized`` plus a partition and
    sort of every column on the host, the only route to a ranked list without
    the top-k kernels.  (a) and (c) are checked against each other."""
    rng = random.Random(0)
    alnum = "abcdefghijklmnopqrstuvwxyz0123456789"
    opts = raw_names(rng, words(rng, a.options, 4, 40, alnum))
    qs = raw_names(rng, words(rng, a.queries, min(a.qmin, a.qmax), a.qmax, alnum))
    metric = gpu.LEVENSHTEIN if a.costs == "1,1,1" else gpu.INDEL2
    k = a.topk
    res = {"topk": k, "options": len(opts), "queries": len(qs), "qmin": min(a.qmin, a.qmax), "qmax": a.qmax,
           "reps": a.reps, "costs": a.costs}
    for n in (1024, len(opts)):   # warm, then the arena at full size
        gpu.ed_closest_k(opts[:n], qs, k, mode=gpu.ALNUM_LOWER, metric=metric)
        gpu.ed_closest_normalized(opts[:n], qs, metric=metric)
    host_topk(gpu.ed_matrix_normalized(opts, qs[:8], metric=metric), k)
    t = {"topk": [], "closest": [], "matrix_host": []}
    kern = {"topk": [], "closest": [], "matrix_host": []}
    select, last = [], {}

    def timed(name, fn):
        t0 = time.perf_counter()
        r = fn()
        t1 = time.perf_counter()
        last[name] = gpu.last_timings()
        kern[name].append(last[name]["kernel_ms"])
        return r, t0, t1

    for _ in range(a.reps):
        ra, t0, t1 = timed("topk", lambda: gpu.ed_closest_k(opts, qs, k, mode=gpu.ALNUM_LOWER, metric=metric))
        t["topk"].append(round((t1 - t0) * 1e3, 3))
        rb, t0, t1 = timed("closest", lambda: gpu.ed_closest_normalized(opts, qs, metric=metric))
        t["closest"].append(round((t1 - t0) * 1e3, 3))
        if not a.no_matrix:
            d, t0, t1 = timed("matrix_host", lambda: gpu.ed_matrix_normalized(opts, qs, metric=metric))
            rc = host_topk(d, k)
            t2 = time.perf_counter()
            del d
            t["matrix_host"].append(round((t2 - t0) * 1e3, 3))
            select.append(round((t2 - t1) * 1e3, 3))
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    res["first_rank_is_closest"] = bool((ra[0][:, 0] == rb[0]).all() and (ra[1][:, 0] == rb[1]).all())
    res.update(topk_ms=t["topk"], closest_ms=t["closest"], topk_kernel_ms=kern["topk"],
               closest_kernel_ms=kern["closest"], topk_breakdown=last["topk"], closest_breakdown=last["closest"],
               kernel_ratio_topk_over_closest=round(med(kern["topk"]) / med(kern["closest"]), 4))
    if not a.no_matrix:
        res["routes_agree"] = bool((ra[0] == rc[0]).all() and (ra[1] == rc[1]).all())
        res.update(matrix_host_ms=t["matrix_host"], matrix_kernel_ms=kern["matrix_host"], host_select_ms=select,
                   speedup_end_to_end=round(med(t["matrix_host"]) / med(t["topk"]), 3))
    res["arch"] = gpu.device_arch()
    print(json.dumps(res), flush=True)
    if not res["first_rank_is_closest"] or not res.get("routes_agree", True):
        raise SystemExit("the routes disagree")


def bench_names(a):
    """Few options against very many raw names (``--options`` small, ``--queries``
    large), two routes alternating in one process after both are warm:
    (a) ``ed_closest_names``, the names in the lanes; (b) today's route on the
    same inputs, ``ed_closest_grouped`` with ``--groups`` > 0 and
    ``ed_closest_normalized`` without; and (c) the public function on them,
    ``editdistance.closest_in_groups`` / ``closest_indices`` with ``device="gpu"``,
    which adds its checks of the input and takes whichever route its rule names
    (``public_takes_names_route``).  ``--names-route off`` times (b) alone.
    Every repetition's answers are compared.  The names are drawn from 50k
    distinct ones, as a foundation export repeats its buildpack names."""
    import numpy as np
    from move2kube_amd.ops import editdistance as ed
    rng = random.Random(0)
    alnum = "abcdefghijklmnopqrstuvwxyz0123456789"
    opts = raw_names(rng, words(rng, a.options, 4, 40, alnum))
    distinct = raw_names(rng, words(rng, min(a.queries, 50000), min(a.qmin, a.qmax), a.qmax, alnum))
    qs = rng.choices(distinct, k=a.queries)
    G = a.groups
    group_of = [i * G // len(opts) for i in range(len(opts))] if G > 0 else None
    metric = gpu.LEVENSHTEIN if a.costs == "1,1,1" else gpu.INDEL2
    on = a.names_route == "on"
    res = {"names_route": a.names_route, "options": len(opts), "groups": G, "queries": len(qs),
           "qmin": min(a.qmin, a.qmax), "qmax": a.qmax, "reps": a.reps, "costs": a.costs}

    def names():
        return gpu.ed_closest_names(opts, qs, group_of, max(G, 1), mode=gpu.ALNUM_LOWER, metric=metric)

    def existing():
        if G > 0:
            return gpu.ed_closest_grouped(opts, group_of, G, qs, mode=gpu.ALNUM_LOWER, metric=metric)
        return gpu.ed_closest_normalized(opts, qs, metric=metric)

    costs = tuple(int(c) for c in a.costs.split(","))
    groups = [[o for o, g in zip(opts, group_of) if g == at] for at in range(G)] if G > 0 else None
    first = np.cumsum([0] + [len(g) for g in groups[:-1]]).astype(np.int32) if G > 0 else None

    def public():
        if G > 0:
            return ed.closest_in_groups(groups, qs, device="gpu", normalize="alnum_lower", costs=costs)
        return ed.closest_indices(opts, qs, device="gpu", normalize="alnum_lower", costs=costs)

    routes = ([("names", names)] if on else []) + [("existing", existing)] + ([("public", public)] if on else [])
    for _, fn in routes:   # warm: context, then the arena at full size
        fn()
    t = {name: [] for name, _ in routes}
    kern = {name: [] for name, _ in routes}
    last, agree = {}, True
    for _ in range(a.reps):
        got = {}
        for name, fn in routes:
            t0 = time.perf_counter()
            got[name] = fn()
            t[name].append(round((time.perf_counter() - t0) * 1e3, 3))
            last[name] = gpu.last_timings()
            kern[name].append(last[name]["kernel_ms"])
        if on:
            if G > 0:   # positions within the groups to indices into the flat options
                got["public"] = (np.where(got["public"][0] < 0, -1, got["public"][0] + first), got["public"][1])
            agree = agree and all((x == y).all() and (x == z).all()
                                  for x, y, z in zip(got["names"], got["existing"], got["public"]))
    for name, _ in routes:
        res[name + "_ms"], res[name + "_kernel_ms"], res[name + "_breakdown"] = t[name], kern[name], last[name]
    if on:
        res["routes_agree"] = bool(agree)
        res["names_wholly_below_existing"] = max(t["names"]) < min(t["existing"])
        res["public_takes_names_route"] = ed.names_route(len(opts), len(qs))
    res["arch"] = gpu.device_arch()
    print(json.dumps(res), flush=True)
    if not agree:
        raise SystemExit("the routes disagree")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--options", type=int, default=200000)
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu", action="store_true", help="also time the native CPU path")
    ap.add_argument("--qmax", type=int, default=64, help="longest query (buildpack names are mostly <= 32)")
    ap.add_argument("--qmin", type=int, default=4, help="shortest query")
    ap.add_argument("--lib", default=None, help="kernel library to load instead of the in-tree one")
    ap.add_argument("--raw", action="store_true",
                    help="names with separators and mixed case: Python normalisation + ed_closest against "
                         "ed_closest_normalized (medians over --reps, the routes checked against each other)")
    ap.add_argument("--costs", default="1,1,2",
                    help="insert,delete,substitute: 1,1,2 (the LCS kernels) or 1,1,1 (the Levenshtein kernels); "
                         "--cpu then times the native scalar DP and takes the first minimum per query")
    ap.add_argument("--groups", type=int, default=0,
                    help="split the options into G groups and time one grouped call against G closest calls, from "
                         "raw names: one JSON line for equal group sizes and one for skewed ones (G = 1: the "
                         "grouped kernels against the plain closest kernels on the same data)")
    ap.add_argument("--topk", type=int, default=0,
                    help="time the K closest options per query (ed_closest_k) against ed_closest and against "
                         "ed_matrix plus a host selection, from raw names, alternating (K in 1..64)")
    ap.add_argument("--no-matrix", action="store_true", help="with --topk: leave the matrix route out")
    ap.add_argument("--names-route", choices=("off", "on"), default=None,
                    help="few options against many raw names (small --options, large --queries; --groups G for the "
                         "grouped request): on = ed_closest_names alternating with today's route, off = today's "
                         "route alone (see bench_names)")
    a = ap.parse_args()
    costs = tuple(int(c) for c in a.costs.split(","))
    if costs not in ((1, 1, 2), (1, 1, 1)):
        raise SystemExit("--costs is 1,1,2 or 1,1,1")
    if a.names_route:
        if a.lib:
            gpu.LIB_PATH = os.path.abspath(a.lib)
        if not gpu.available():
            raise SystemExit("--names-route needs the GPU")
        bench_names(a)
        return
    if a.topk > 0:
        if a.lib:
            gpu.LIB_PATH = os.path.abspath(a.lib)
        if not gpu.available():
            raise SystemExit("--topk needs the GPU")
        bench_topk(a)
        return
    if a.groups > 0:
        if a.lib:
            gpu.LIB_PATH = os.path.abspath(a.lib)
        if not gpu.available():
            raise SystemExit("--groups needs the GPU")
        for split in ("equal", "skewed") if a.groups > 1 else ("equal",):
            bench_groups(a, split)
        return
    kw = {"metric": gpu.LEVENSHTEIN} if costs == (1, 1, 1) else {}
    if a.lib:
        gpu.LIB_PATH = os.path.abspath(a.lib)
    if a.raw:
        if not gpu.available():
            raise SystemExit("--raw needs the GPU")
        res = {"options": a.options, "qmin": min(a.qmin, a.qmax), "qmax": a.qmax, "reps": a.reps}
        bench_raw(a, res)
        print(json.dumps(res), flush=True)
        return
    rng = random.Random(0)
    opts = words(rng, a.options, 4, 40)
    qs = words(rng, a.queries, min(a.qmin, a.qmax), a.qmax)
    res = {"options": a.options, "queries": a.queries, "qmin": min(a.qmin, a.qmax), "qmax": a.qmax,
           "pairs": a.options * a.queries, "option_bytes": sum(len(o) for o in opts), "lib": os.path.basename(a.lib) if a.lib else "in-tree",
           "costs": list(costs)}
    cells = sum(len(o) for o in opts) * a.queries  # option bytes x queries = bit-parallel steps
    if gpu.available():
        gpu.ed_closest(opts[:1024], qs[:8])  # warm-up / context creation
        for name, fn in (("closest", gpu.ed_closest), ("matrix", gpu.ed_matrix)):
            t, k = [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                r = fn(opts, qs, **kw)
                t.append(time.perf_counter() - t0)
                k.append(gpu.last_timings()["kernel_ms"])
            res["gpu_%s_s" % name] = min(t)
            res["gpu_%s_kernel_ms" % name] = k
            res["gpu_%s_breakdown" % name] = gpu.last_timings()
            res["gpu_%s_gsteps_per_s" % name] = cells / min(t) / 1e9
        res["arch"] = gpu.device_arch()
        gi, gd = gpu.ed_closest(opts, qs, **kw)
    if a.cpu and native.available():
        th = min(16, os.cpu_count() or 1)
        t0 = time.perf_counter()
        if kw:   # no fused argmin for these costs on the CPU: the matrix, then its first minimum per query
            d = native.module().edit_distance_batch(opts, qs, costs[0], costs[1], costs[2], th)
            ci = d.argmin(axis=0)
            cd = d.min(axis=0)
        else:
            ci, cd = native.module().closest_batch(opts, qs, th)
        res["cpu_native_closest_s"] = time.perf_counter() - t0
        res["cpu_threads"] = th
        if gpu.available():
            res["gpu_cpu_agree"] = bool((gi == ci).all() and (gd == cd).all())
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

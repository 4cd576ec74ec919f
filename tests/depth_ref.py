"""The reference of `screen --depth` and of dd_exact_depth, a computation of its own in plain Python: a collections.Counter
over pyref.kmers of a sample's text, restricted to the universe's {key: mask} dictionary, binned and summed by the rules of
include/dandd_hip.h; the statistics of a histogram from a sort of the expanded depths; and the two CSVs of the command as
rows of strings, from the files' text alone.  Integers only in the arrays: every comparison against them is ==."""
import collections

import pyref

CLASSES = ("core", "private", "signature")
COLS = {
    "depth": ["sample", "k", "target", "class", "kmers", "covered", "breadth", "mean_depth", "mean_covered", "median_depth", "median_covered",
              "clipped"],
    "depth_hist": ["sample", "k", "target", "class", "depth", "kmers"],
}


def matches(m, a, b):
    return m & a == a and m & b == 0


def depths(text, k, canonical, masks):
    """{key: the positions of `text` at which it ends} for the keys of the universe"""
    c = collections.Counter(pyref.kmers(text, k, canonical))
    return {x: v for x, v in c.items() if x in masks}


def answer(text, k, canonical, masks, n, queries, bins):
    """-> (hist [n+nq][bins], total [n+nq]) of one sample: row i < n the keys whose mask has bit i, row n + q those that match
    query q; bin d < bins - 1 the keys of the row that stand d times in the text (0: not at all), the last bin those that
    stand bins - 1 times or more; total the sum of the times, unclipped"""
    c = depths(text, k, canonical, masks)
    rows = [lambda m, i=i: m >> i & 1 for i in range(n)] + [lambda m, a=int(a), b=int(b): matches(m, a, b) for a, b in queries]
    hist, total = [[0] * bins for _ in rows], [0] * len(rows)
    # (the keys with the same mask and depth go together: a few hundred classes instead of every key times every row)
    for (m, d), keys in collections.Counter((m, c.get(x, 0)) for x, m in masks.items()).items():
        for r, holds in enumerate(rows):
            if holds(m):
                hist[r][min(d, bins - 1)] += keys
                total[r] += d * keys
    return hist, total


def lower_median(values):
    """the lower median of a list: element (len - 1) // 2 of its sort; None of an empty one"""
    s = sorted(values)
    return s[(len(s) - 1) // 2] if s else None


def stats(hist, total):
    """one histogram -> (kmers, covered, breadth, mean, mean_covered, median, median_covered, clipped) from the expanded depths:
    a clipped depth stands as the last bin; None where a number has nothing to stand on"""
    last = len(hist) - 1
    all_d = [d for d, v in enumerate(hist) for _ in range(v)]
    cov_d = [d for d in all_d if d >= 1]
    kmers, covered = len(all_d), len(cov_d)
    med, med_cov = lower_median(all_d), lower_median(cov_d)
    return (kmers, covered, covered / kmers if kmers else None, total / kmers if kmers else None, total / covered if covered else None,
            med, med_cov, med == last or med_cov == last)


def cell(v):
    return "" if v is None else str(v)


def query_list(n, groups):
    """the queries of DeltaTree.depth_tables: (0, 0), (full, 0), every genome's private pair, then core / private / signature
    of every group (members: indices)"""
    full = (1 << n) - 1
    qs = [(0, 0), (full, 0)] + [(1 << i, full ^ (1 << i)) for i in range(n)]
    for _, members in groups or []:
        M = sum(1 << i for i in members)
        qs += [(M, 0), (0, full ^ M), (M, full ^ M)]
    return qs


def tables(universe, samples, ks, groups, bins=64, canonical=True):
    """The files of `screen --depth --depth-hist` as lists of rows of strings.
    universe: [(name as the CSV shows it, FASTA bytes)], samples: [(name, text)], groups: [(label, members)] or None."""
    import test_core as cpuc
    n = len(universe)
    qs = query_list(n, groups)
    targets = [(name, cls, row) for i, (name, _) in enumerate(universe) for cls, row in (("all", i), ("private", n + 2 + i))]
    targets += [("pan", "all", n), ("core", "all", n + 1)]
    targets += [(label, cls, 2 * n + 2 + 3 * gi + c) for gi, (label, _) in enumerate(groups or []) for c, cls in enumerate(CLASSES)]
    depth, dhist = [], []
    for sname, text in samples:
        for k in ks:
            masks = cpuc.masks_of([fa for _, fa in universe], k, canonical)
            hist, total = answer(text, k, canonical, masks, n, qs, bins)
            for target, cls, row in targets:
                depth.append([sname, k, target, cls, *stats(hist[row], total[row])])
                for d, v in enumerate(hist[row]):
                    if v:
                        dhist.append([sname, k, target, cls, f">={d}" if d == bins - 1 else d, v])
    out = {"depth": depth, "depth_hist": dhist}
    return {name: [[cell(v) for v in r] for r in body] for name, body in out.items()}

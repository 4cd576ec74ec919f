"""The reference of `screen --gather` and of dd_exact_gather, a computation of its own in plain Python: depth_ref.depths (a
collections.Counter over pyref.kmers of a sample's text, restricted to the universe's {key: mask} dictionary), then the loop
of include/dandd_hip.h word for word -- count, per input, the held keys whose mask meets the picks so far nowhere; take the
largest count, the lowest input on a tie; stop below min_hits or behind `steps` picks --; and the two CSVs of the command as
rows of strings, from the files' text alone.  Integers only in the arrays: every comparison against them is ==."""
import pyref
from depth_ref import depths

COLS = {
    "gather": ["sample", "k", "rank", "fasta", "genome_kmers", "shared", "unique", "f_sample_unique", "f_genome_shared", "f_genome_unique",
               "unique_depth", "mean_depth", "f_depth", "remaining"],
    "gather_summary": ["sample", "k", "sample_kmers", "in_pan", "novel", "genomes", "explained", "unexplained", "top_fasta"],
}


def walk(held, n, min_hits=1, steps=None):
    """held: the (mask, depth) pairs of the keys a sample holds, depth > 0 -> (pick [steps], unique [steps], depth [steps],
    shared [n], total [2]); behind the stop pick = -1, unique = depth = 0"""
    steps = n if steps is None else steps
    # (the keys with the same mask go together: a few hundred classes [keys, sum of depths] instead of every key times every input)
    cls = {}
    for m, d in held:
        assert int(d) > 0 and int(m) > 0
        c = cls.setdefault(int(m), [0, 0])
        c[0] += 1
        c[1] += int(d)
    pick, unique, depth = [-1] * steps, [0] * steps, [0] * steps
    shared = [sum(c[0] for m, c in cls.items() if m >> b & 1) for b in range(n)]
    total = [sum(c[0] for c in cls.values()), sum(c[1] for c in cls.values())]
    taken = 0
    for t in range(steps):
        U = [sum(c[0] for m, c in cls.items() if not m & taken and m >> b & 1) for b in range(n)]
        best = max(range(n), key=lambda b: (U[b], -b))
        if U[best] < min_hits:
            break
        pick[t], unique[t] = best, U[best]
        depth[t] = sum(c[1] for m, c in cls.items() if not m & taken and m >> best & 1)
        taken |= 1 << best
    return pick, unique, depth, shared, total


def answer(text, k, canonical, masks, n, min_hits=1, steps=None):
    """-> walk(...) of one sample's text against the universe's {key: mask}"""
    return walk([(masks[x], d) for x, d in depths(text, k, canonical, masks).items()], n, min_hits, steps)


def cell(v):
    return "" if v is None else str(v)


def ratio(a, b):
    return a / b if b else None


def tables(universe, samples, ks, min_hits=1, steps=None, canonical=True):
    """The files of `screen --gather` as lists of rows of strings.
    universe: [(name as the CSV shows it, FASTA bytes)], samples: [(name, text)]."""
    import test_core as cpuc
    n = len(universe)
    picks, summary = [], []
    for sname, text in samples:
        for k in ks:
            masks = cpuc.masks_of([fa for _, fa in universe], k, canonical)
            size = [sum(1 for m in masks.values() if m >> i & 1) for i in range(n)]
            q = len(set(pyref.kmers(text, k, canonical)))
            pick, unique, depth, shared, (in_pan, deep) = answer(text, k, canonical, masks, n, min_hits, steps)
            explained, chosen = 0, []
            for t, i in enumerate(pick):
                if i < 0:
                    break
                explained += unique[t]
                chosen.append(universe[i][0])
                picks.append([sname, k, t + 1, universe[i][0], size[i], shared[i], unique[t], ratio(unique[t], q), ratio(shared[i], size[i]),
                              ratio(unique[t], size[i]), depth[t], ratio(depth[t], unique[t]), ratio(depth[t], deep), in_pan - explained])
            summary.append([sname, k, q, in_pan, q - in_pan, len(chosen), explained, in_pan - explained, chosen[0] if chosen else None])
    out = {"gather": picks, "gather_summary": summary}
    return {name: [[cell(v) for v in r] for r in body] for name, body in out.items()}

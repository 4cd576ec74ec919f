"""The reference of `screen --cover` and of dd_exact_cover, a computation of its own in plain Python: a target genome's k-mer
ends (test_core_regions.ends_of: {end token: key}), the sample's depth of every key (depth_ref.depths: a collections.Counter
over pyref.kmers of the sample's text, restricted to the universe's {key: mask} dictionary), binned by token // window into
the six columns of include/dandd_hip.h; the states and runs of the windows; and the three CSVs of the command as rows of
strings, from the files' text alone.  Integers only in the arrays: every comparison against them is ==."""
import depth_ref
import paint_ref
import test_core_regions as cpur

COLS = {
    "cover": ["sample", "k", "fasta", "window", "record", "start", "end", "records", "valid", "covered", "depth", "private", "private_covered",
              "private_depth"],
    "cover_regions": ["sample", "k", "fasta", "state", "first_window", "windows", "record", "start", "end_record", "end", "valid", "covered",
                      "depth"],
    "cover_summary": ["sample", "k", "fasta", "windows", "valid", "covered", "breadth", "depth", "mean_covered_depth", "private", "private_covered",
                      "private_breadth", "private_mean_covered_depth", "present_windows", "absent_windows", "empty_windows",
                      "longest_absent_windows"],
}
STATES = ("empty", "present", "absent")


def rows(ends, g, ntok, depth, masks, window, clip):
    """[[valid, covered, depth, private, private_covered, private_depth]] per window of `window` tokens of target g's token
    stream of ntok tokens.  ends: {end token: key} of the target, depth: {key: the positions of the sample at which it
    stands}, masks: {key: membership mask} of the universe.  A k-mer counts in the window that holds its END token."""
    out = [[0] * 6 for _ in range(-(-ntok // window))]
    for t, x in ends.items():
        c = depth.get(x, 0)
        row = out[t // window]
        row[0] += 1
        row[1] += 1 if c >= 1 else 0
        row[2] += min(c, clip)
        if masks[x] == 1 << g:
            row[3] += 1
            row[4] += 1 if c >= 1 else 0
            row[5] += min(c, clip)
    return out


def fixture_rows(g, text, k, canonical, window, clip):
    """rows of target g of test_core_regions.genomes() for the sample `text`"""
    ends, masks = cpur.reference(k, canonical)
    return rows(ends[g], g, cpur.index_of(cpur.genomes()[g])[2], depth_ref.depths(text, k, canonical, masks), masks, window, clip)


def states(body, min_percent):
    """-> ([state per window], [(state, first window, windows)] the maximal runs of equal state): 0 empty (valid == 0), 1
    present (100 * covered >= min_percent * valid), 2 absent"""
    st = [0 if r[0] == 0 else 1 if 100 * r[1] >= min_percent * r[0] else 2 for r in body]
    runs = []
    for w, s in enumerate(st):
        if runs and runs[-1][0] == s:
            runs[-1][2] += 1
        else:
            runs.append([s, w, 1])
    return st, [tuple(r) for r in runs]


def cell(v):
    return "" if v is None else str(v)


def ratio(a, b):
    return a / b if b else None


def tables(universe, samples, ks, window, targets=None, clip=255, min_percent=50, canonical=True):
    """The files of `screen --cover W --cover-clip C --cover-min P` as lists of rows of strings.  universe: [(name as the CSV
    shows it, FASTA bytes)], samples: [(name, text)], targets: indices of the universe (None: all)."""
    import test_core as cpuc
    targets = list(range(len(universe))) if targets is None else list(targets)
    cover, regions, summary = [], [], []
    for sname, text in samples:
        for k in ks:
            masks = cpuc.masks_of([fa for _, fa in universe], k, canonical)
            depth = depth_ref.depths(text, k, canonical, masks)
            for g in targets:
                fname, fa = universe[g]
                where = paint_ref.places(fa, window)
                body = rows(cpur.ends_of(fa, k, canonical), g, cpur.index_of(fa)[2], depth, masks, window, clip)
                for w, row in enumerate(body):
                    cover.append([sname, k, fname, w, *where[w], *row])
                st, runs = states(body, min_percent)
                for state, first, length in runs:
                    last = first + length - 1
                    regions.append([sname, k, fname, STATES[state], first, length, where[first][0], where[first][1], where[last][0], where[last][2],
                                    *(sum(r[c] for r in body[first:last + 1]) for c in range(3))])
                tot = [sum(r[c] for r in body) for c in range(6)]
                summary.append([sname, k, fname, len(body), tot[0], tot[1], ratio(tot[1], tot[0]), tot[2], ratio(tot[2], tot[1]), tot[3], tot[4],
                                ratio(tot[4], tot[3]), ratio(tot[5], tot[4]), st.count(1), st.count(2), st.count(0),
                                max((length for state, _, length in runs if state == 2), default=0)])
    out = {"cover": cover, "cover_regions": regions, "cover_summary": summary}
    return {name: [[cell(v) for v in r] for r in body] for name, body in out.items()}

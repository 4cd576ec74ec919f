"""The reference of `screen --reads` and of dd_exact_reads, a computation of its own in plain Python: a sample's k-mer ends
from test_core_regions.ends_of, the universe's {key: mask} dictionary, the rows binned by bisect over the borders, the vote
and the class from the rules of include/dandd_hip.h; and the two CSVs of the command as rows of strings, from the files'
text alone.  Integers only: every comparison against it is ==."""
import bisect

import test_core_regions as cpur

NONE = 0xFFFFFFFF
CLASS_NAMES = ("ambiguous", "unclassified", "no_kmer")
COLS = {
    "reads_summary": ["sample", "k", "target", "reads", "fraction"],
    "reads": ["sample", "k", "record", "name", "length", "valid", "in_pan", "class", "best_fasta", "best_shared", "second_fasta", "second_shared",
              "ties", "consistent"],
}


def counts(text, k, canonical, masks, n, borders, ends=None):
    """[[valid, in_pan, shared with genome 0, .., n-1]] per row: row r covers the tokens borders[r] .. borders[r+1]-1, the
    last row runs to the end; a k-mer counts in the row that holds its END token, once per position; a token in front of
    the first border counts nowhere.  ends: test_core_regions.ends_of(text, k, canonical) where the caller has it already"""
    borders = [int(b) for b in borders]
    out = [[0] * (n + 2) for _ in borders]
    for t, x in (cpur.ends_of(text, k, canonical) if ends is None else ends).items():
        r = bisect.bisect_right(borders, t) - 1
        if r < 0:
            continue
        row = out[r]
        row[0] += 1
        m = masks.get(x, 0)
        if m:
            row[1] += 1
            for i in range(n):
                row[2 + i] += m >> i & 1
    return out


def vote(row, n, min_hits):
    """one row of counts -> (call [valid, hit, best, best_count, second, second_count], [ties, full], class): the class is the
    best genome's index where the call is unique, n ambiguous, n + 1 unclassified, n + 2 without a valid k-mer"""
    valid, hit, cols = row[0], row[1], row[2:]
    best = second = None
    if hit != 0:
        for i in range(n):                                    # the largest column; a tie stays with the earlier genome
            if best is None or cols[i] > cols[best]:
                best = i
        for i in range(n):                                    # the largest non-zero column among the others
            if i != best and cols[i] != 0 and (second is None or cols[i] > cols[second]):
                second = i
    best_count = 0 if best is None else cols[best]
    ties = sum(1 << i for i in range(n) if cols[i] == best_count) if best_count != 0 else 0
    full = sum(1 << i for i in range(n) if cols[i] == hit) if hit != 0 else 0
    if valid == 0:
        cls = n + 2
    elif best_count < min_hits:
        cls = n + 1
    elif bin(ties).count("1") == 1:
        cls = best
    else:
        cls = n
    call = [valid, hit, NONE if best is None else best, best_count, NONE if second is None else second, 0 if second is None else cols[second]]
    return call, [ties, full], cls


def answer(text, k, canonical, masks, n, borders, min_hits, ends=None):
    """-> (counts, calls, sets, classes, tally [n+3]) of one sample"""
    cnt = counts(text, k, canonical, masks, n, borders, ends)
    calls, sets, classes, tally = [], [], [], [0] * (n + 3)
    for row in cnt:
        c, s, cls = vote(row, n, min_hits)
        calls.append(c), sets.append(s), classes.append(cls)
        tally[cls] += 1
    return cnt, calls, sets, classes, tally


def cell(v):
    return "" if v is None else str(v)


def tables(universe, samples, ks, min_hits=1, canonical=True):
    """The files of `screen --reads --reads-calls` as lists of rows of strings: the rows are the samples' records.
    universe: [(name as the CSV shows it, FASTA bytes)], samples: [(name, text)]."""
    import test_core as cpuc
    n = len(universe)
    summary, reads = [], []
    for sname, text in samples:
        lens, starts, _ = cpur.index_of(text)
        names = cpur.header_names(text)
        for k in ks:
            masks = cpuc.masks_of([fa for _, fa in universe], k, canonical)
            _, calls, sets, classes, tally = answer(text, k, canonical, masks, n, starts, min_hits)
            for target, count in zip([name for name, _ in universe] + list(CLASS_NAMES), tally):
                summary.append([sname, k, target, count, count / len(starts) if starts else None])
            for r, (c, s, cls) in enumerate(zip(calls, sets, classes)):
                valid, hit, best, best_count, second, second_count = c
                reads.append([sname, k, r, names[r], lens[r], valid, hit, "unique" if cls < n else CLASS_NAMES[cls - n],
                              None if best == NONE else universe[best][0], None if best == NONE else best_count,
                              None if second == NONE else universe[second][0], None if second == NONE else second_count,
                              bin(s[0]).count("1"), bin(s[1]).count("1")])
    out = {"reads_summary": summary, "reads": reads}
    return {name: [[cell(v) for v in r] for r in body] for name, body in out.items()}

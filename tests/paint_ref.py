"""The reference of `screen --paint`, a computation of its own: a sample's k-mer ends from test_core_regions.ends_of, the
universe's {key: mask} dictionary, binned into windows in plain Python; and the three CSVs of the command as rows of
strings, from the files' text alone.  Integers only: every comparison against it is ==."""
import test_core_regions as cpur

COLS = {
    "paint": ["sample", "k", "window", "tok_start", "tok_end", "record", "start", "end", "records", "valid", "in_pan", "novel", "best_fasta",
              "best_shared", "second_fasta", "second_shared"],
    "paint_segments": ["sample", "k", "first_window", "last_window", "tok_start", "tok_end", "best_fasta", "valid", "in_pan", "best_shared"],
}


def rows(text, k, canonical, masks, n, window, ends=None):
    """[[valid, in_pan, shared with genome 0, .., n-1]] per window of `window` tokens of the token stream of `text` (one
    BREAK in front of every record's bases): a k-mer counts in the window that holds its END token, once per position.
    ends: test_core_regions.ends_of(text, k, canonical) where the caller has it already"""
    ntok = cpur.index_of(text)[2]
    out = [[0] * (n + 2) for _ in range(-(-ntok // window))]
    for t, x in (cpur.ends_of(text, k, canonical) if ends is None else ends).items():
        row = out[t // window]
        row[0] += 1
        m = masks.get(x, 0)
        if m:
            row[1] += 1
            for i in range(n):
                row[2 + i] += m >> i & 1
    return out


def places(text, window):
    """per window (record name or None, start, end, records): the record that holds the window's first base, the half-open
    interval of its bases inside the window, the records with a base in the window -- token by token"""
    names = cpur.header_names(text)
    lens, starts, ntok = cpur.index_of(text)
    where = [None] * ntok                                     # token -> (record, base) where the token is a base
    for r, (s, n) in enumerate(zip(starts, lens)):
        for b in range(n):
            where[s + b] = (r, b)
    out = []
    for lo in range(0, ntok, window):
        inside = [w for w in where[lo:lo + window] if w is not None]
        if not inside:
            out.append((None, 0, 0, 0))
            continue
        r = inside[0][0]
        mine = [b for rr, b in inside if rr == r]
        out.append((names[r], mine[0], mine[-1] + 1, len({rr for rr, _ in inside})))
    return out


def cell(v):
    return "" if v is None else str(v)


def tables(universe, samples, ks, window, canonical=True):
    """The files of `screen --paint W --paint-matrix` as lists of rows of strings.  universe: [(name as the CSV shows it, FASTA
    bytes)], samples: [(name, text)]."""
    import test_core as cpuc
    n = len(universe)
    paint, segments, matrix = [], [], []
    for sname, text in samples:
        ntok = cpur.index_of(text)[2]
        where = places(text, window)
        for k in ks:
            masks = cpuc.masks_of([fa for _, fa in universe], k, canonical)
            run = None
            for w, row in enumerate(rows(text, k, canonical, masks, n, window)):
                valid, in_pan, cols = row[0], row[1], row[2:]
                best = second = None
                if in_pan:
                    for i in range(n):                        # the largest column; a tie stays with the earlier genome
                        if best is None or cols[i] > cols[best]:
                            best = i
                    for i in range(n):
                        if i != best and cols[i] and (second is None or cols[i] > cols[second]):
                            second = i
                lo, hi = w * window, min((w + 1) * window, ntok)
                paint.append([sname, k, w, lo, hi, *where[w], valid, in_pan, valid - in_pan,
                              None if best is None else universe[best][0], None if best is None else cols[best],
                              None if second is None else universe[second][0], None if second is None else cols[second]])
                matrix.append([sname, k, w, *cols])
                if run is None or run["best"] != best:
                    run = dict(best=best, first=w, lo=lo, valid=0, in_pan=0, shared=0)
                    segments.append([sname, k, run])
                run["last"], run["hi"] = w, hi
                run["valid"] += valid
                run["in_pan"] += in_pan
                run["shared"] += 0 if best is None else cols[best]
    segs = [[s, k, r["first"], r["last"], r["lo"], r["hi"], None if r["best"] is None else universe[r["best"]][0], r["valid"], r["in_pan"],
             None if r["best"] is None else r["shared"]] for s, k, r in segments]
    out = {"paint": paint, "paint_segments": segs, "paint_matrix": matrix}
    return {name: [[cell(v) for v in r] for r in body] for name, body in out.items()}

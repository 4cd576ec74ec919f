"""`dandd tree | progressive | kij | deltadelta | abba | greedy | core | screen | patterns | neighbors` on the MI355X engine: same sub-commands, flags,
defaults and output files as /root/reference/lib/dandd_cmd.py (flags :141-286, handlers :43-132); only the
sketching backend differs.  (deltadelta, abba, greedy, core, screen, patterns and neighbors are this package's own: the reference has none of them.)  Run as  python -m dandd_amd.host.cli <subcommand> ...
`neighbors` places new samples in a tree of SKETCHES (any number of genomes): each sample's genomes by K-independent Jaccard
(<prefix>.neighbors.csv), its two closest and what it would add to the collection's delta (<prefix>.neighbors_summary.csv), and
with `--jaccard` every k's cardinalities (<prefix>.neighbors_j.csv); the tree's own files stay as they are.
`kij`, `progressive` and `deltadelta` on a `tree --exact` of up to 255 genomes take ONE sort of the leaves' k-mers per k for
all their unions (up to 64 genomes: a 64-bit membership mask per k-mer; 65 to 255: a row of up to four such words); beyond
255 genomes, under --safe and under DD_NO_PREFETCH every union is counted on its own.
`screen --paint W` adds where along each sample the collection's k-mers lie: one row per window of W bases.
`screen --reads` adds which genome each record of a sample -- a read, a contig -- belongs to and how many records go to each
genome (<prefix>.reads_summary.csv); `--reads-calls` writes the call of every record too (<prefix>.reads.csv), and
`--reads-min-hits H` asks H positions of a genome for a call.
`screen --depth` adds how many times a sample holds the k-mers of each genome, of its private k-mers, of the pan-genome and of
the core: breadth, mean and median depth per row (<prefix>.depth.csv); `--depth-bins B` sets the bins of the histogram
behind them (2..256, default 64: depths from B-1 on share the last bin) and `--depth-hist` writes its non-zero bins too
(<prefix>.depth_hist.csv).
`screen --cover W` adds where along each GENOME of the collection a sample lies, and how deep: one row per sample, genome and
window of W bases of the genome (<prefix>.cover.csv), the runs of windows that are present, absent or empty
(<prefix>.cover_regions.csv: the absent runs are the deleted or missing stretches) and one row per sample and genome
(<prefix>.cover_summary.csv).  `--cover-fastas LIST` lays the samples along the genomes LIST names (one per line; default:
the whole universe), `--cover-clip C` counts a position's depth as at most C (1..1023, default 255), `--cover-min P` calls a
window present where the sample holds at least P per cent of its positions (1..100, default 50).
`screen --gather` adds which genomes of the collection EXPLAIN a sample, one by one: the genome that holds most of the sample's
k-mers, then the one that holds most of what is left, and so on -- a close relative of a pick adds almost nothing --, one row
per sample, k and pick with the k-mers it adds and how deep the sample holds them (<prefix>.gather.csv), and one row per
sample and k (<prefix>.gather_summary.csv).  `--gather-min H` stops at a pick that adds fewer than H k-mers (default 1),
`--gather-steps N` behind N picks (default: as many as the universe has genomes).
"""
import argparse
import os
import pickle
import sys

from . import deltatree
from .deltatree import write_listdict_to_csv


def tree_command(args):
    if not (args.genomedir or args.flist_loc):
        print("ERROR: You must provide either a datadirectory or a fasta file list!")
        sys.exit(1)
    if not args.sketchdir:
        args.sketchdir = os.path.join(args.outdir, "sketchdb")
        os.makedirs(args.sketchdir, exist_ok=True)
    tool = "dashing"
    if args.exact:  # exact distinct k-mer counts on the GPU (the reference's KMC branch, :51-53)
        tool = "kmc"
        args.registers = 20
    ksweep = (int(args.mink), int(args.maxk)) if args.ksweep else None
    os.makedirs(args.outdir, exist_ok=True)
    # a sketch directory with nothing in it: this run will sketch, so the GPU context is brought up beside the
    # digests and directory walks instead of after them (a fully cached run never touches the GPU and starts none)
    try:
        cold = not any(e.is_dir() and any(os.scandir(e.path)) for e in os.scandir(args.sketchdir))
    except OSError:
        cold = True
    if cold:
        deltatree.prewarm_backend({"registers": int(args.registers), "canonicalize": args.canonicalize, "tool": tool})
    try:
        tree = deltatree.create_delta_tree(
            tag=args.tag, genomedir=args.genomedir, sketchdir=args.sketchdir, kstart=args.kstart,
            nchildren=args.nchildren, registers=int(args.registers), flist_loc=args.flist_loc,
            canonicalize=args.canonicalize, tool=tool, debug=args.debug, nthreads=int(args.nthreads),
            safety=args.safety, fast=args.fast, verbose=args.verbose, ksweep=ksweep, lowmem=args.lowmem)
    except deltatree.WorkerDone:  # rank > 0 of a multi-GPU run: its leaf sketches are on disk
        return
    prefix = tree.make_prefix(outdir=args.outdir, tag=args.tag, label=args.label)
    tree.save(fileprefix=prefix, fast=args.fast)


def _load_tree(path):
    """A tree pickle written by this package or by the reference itself (dandd_amd/host/compat.py)."""
    from .compat import load_tree
    return load_tree(path)


def progressive_command(args):
    tree = _load_tree(args.delta_tree)
    if not args.tag:
        args.tag = tree.speciesinfo.tag
    outfile = tree.make_prefix(tag=args.tag, label=f"progu{args.norderings}", outdir=args.outdir)
    exp = tree.experiment
    exp.update(debug=args.debug, safety=args.safety, fast=args.fast, verbose=args.verbose, lowmem=args.lowmem,
               baseset=set(), ksweep=(int(args.mink), int(args.maxk)) if args.ksweep else None)
    tree.speciesinfo.update(tool=exp["tool"])
    if deltatree.dist_ranks()[0] != 0:
        # rank > 0 of a multi-GPU run: its share of the leaf sketches the sweep needs, then done.  The spider
        # over the run's FASTAs is the one rank 0 builds inside progressive_union; both meet at its barrier.
        try:
            deltatree.DeltaSpider(fasta_files=tree.progressive_fastas(args.flist_loc), speciesinfo=tree.speciesinfo,
                                  experiment=exp)
        except deltatree.WorkerDone:
            pass
        return
    results, summary = tree.progressive_wrapper(flist_loc=args.flist_loc, count=args.norderings,
                                                ordering_file=args.ordering_file, step=args.step)
    write_listdict_to_csv(outfile + ".csv", results)
    write_listdict_to_csv(outfile + "summary.csv", summary)
    tree.save(fileprefix=outfile)


def kij_command(args):
    tree = _load_tree(args.delta_tree)
    tree.speciesinfo.update(tool=tree.experiment["tool"])
    if not args.tag:
        args.tag = tree.speciesinfo.tag
    outfile = tree.make_prefix(tag=args.tag, label=args.label, outdir=args.outdir)
    if args.flist_loc:
        with open(args.flist_loc) as f:
            wanted = {line.strip() for line in f}
        sub = [n for n in tree.leaf_nodes() if n.fastas[0] in wanted or os.path.basename(n.fastas[0]) in wanted]
    else:
        sub = []
    if args.ksweep:
        tree.experiment["ksweep"] = (int(args.mink), int(args.maxk))
    if deltatree.dist_ranks()[1] > 1:
        # every rank sketches its share of the leaves for the whole range; rank 0 finishes alone
        rank = deltatree.dist_ranks()[0]
        tree.presketch_range(int(args.mink), int(args.maxk))   # (ends at the barrier, which switches sharding off)
        if rank != 0:
            return
    tree.ksweep(mink=int(args.mink), maxk=int(args.maxk))
    kij_rows, j_rows = tree.pairwise_spiders(sublist=sub, mink=args.mink, maxk=args.maxk, jaccard=args.jaccard)
    write_listdict_to_csv(outfile + ".kij.csv", kij_rows)
    if args.jaccard:
        write_listdict_to_csv(outfile + ".j.csv", j_rows)
    tree.speciesinfo.save_cardkey(tree.experiment["tool"])
    tree.speciesinfo.save_references(fast=False)
    if args.afproject:
        with open(outfile + "_AFtuples.pickle", "wb") as f:
            pickle.dump(tree.prepare_AFproject(kij_rows, j_rows), f)


def _leaf_lookup(tree, cmd, tree_path):
    """-> leaf_of(name): the tree's leaf FASTA a name means -- its path, its absolute path or its basename when that is unique
    -- or an exit with a `<cmd>: ...` message"""
    leaves = tree.leaf_nodes()
    by_name = {}
    for leaf in leaves:
        f = leaf.fastas[0]
        for key in {f, os.path.abspath(f)}:
            by_name[key] = f
    base_count = {}
    for leaf in leaves:
        b = os.path.basename(leaf.fastas[0])
        base_count[b] = base_count.get(b, 0) + 1
    for leaf in leaves:
        b = os.path.basename(leaf.fastas[0])
        if base_count[b] == 1:
            by_name.setdefault(b, leaf.fastas[0])

    def leaf_of(name):
        f = by_name.get(name) or by_name.get(os.path.abspath(name))
        if f is None:
            sys.exit(f"{cmd}: {name} is not a leaf of the tree {tree_path}")
        return f
    return leaf_of


def _lines(path):
    with open(path) as fh:
        return [line.rstrip("\n") for line in fh if line.strip()]


def _read_groups(cmd, path, leaf_of):
    """-> (groups as lists of leaf FASTAs, their labels in order of first appearance) from 'fasta<TAB>group' lines"""
    groups, labels = [], []
    for n, line in enumerate(_lines(path), 1):
        parts = line.split("\t")
        if len(parts) != 2 or not parts[0].strip() or not parts[1].strip():
            sys.exit(f"{cmd}: {path}:{n}: expected 'fasta<TAB>group', found {line!r}")
        f, label = leaf_of(parts[0].strip()), parts[1].strip()
        if label not in labels:
            labels.append(label)
            groups.append([])
        groups[labels.index(label)].append(f)
    return groups, labels


def _deltadelta_groups(tree, args):
    """-> (groups as lists of leaf FASTAs, their labels) from -f / -g, or every leaf on its own in tree order"""
    leaves = tree.leaf_nodes()
    leaf_of = _leaf_lookup(tree, "deltadelta", args.delta_tree)
    if args.flist_loc and args.groups_loc:
        sys.exit("deltadelta: -f/--fastas and -g/--groups are mutually exclusive")
    if args.groups_loc:
        return _read_groups("deltadelta", args.groups_loc, leaf_of)
    if args.flist_loc:
        seen, groups = set(), []
        for name in _lines(args.flist_loc):
            f = leaf_of(name.strip())
            if f not in seen:
                seen.add(f)
                groups.append([f])
    else:
        groups = [[leaf.fastas[0]] for leaf in leaves]
    title = {leaf.fastas[0]: leaf.node_title for leaf in leaves}
    return groups, [title[g[0]] for g in groups]


# ---- what the analyses over a loaded tree (deltadelta, abba, greedy, core, screen, patterns) share ------------------------------------
def _open_tree(cmd, args, exact=False, safe=False):
    """-> (the tree of -d, the prefix of the command's output files).  exact: the command sums over membership masks, so a
    tree of sketches is an exit; safe: the command has an object path, which --safe asks for through the experiment."""
    tree = _load_tree(args.delta_tree)
    tree.speciesinfo.update(tool=tree.experiment["tool"])
    if exact and tree.experiment["tool"] != "kmc":
        sys.exit(f"{cmd}: {args.delta_tree} is a tree of sketches: build it with `tree --exact` -- intersections are sums over exact "
                 "membership masks, and inclusion-exclusion over HyperLogLog union estimates amplifies their error")
    if not args.tag:
        args.tag = tree.speciesinfo.tag
    if safe and args.safety:
        tree.experiment["safety"] = True
    return tree, tree.make_prefix(tag=args.tag, label=args.label, outdir=args.outdir)


def _window_or_exit(cmd, args, tree, why=""):
    """-> the k window (lo, hi) of --ksweep, else the tree's own; `why` says what a hill-climb would make of the command"""
    if args.ksweep:
        return (int(args.mink), int(args.maxk))
    if tree.experiment.get("ksweep") is not None:
        return tuple(int(v) for v in tree.experiment["ksweep"])
    sys.exit(f"{cmd}: a k window is needed: give --ksweep --mink --maxk, or a tree built with --ksweep" + (f" ({why})" if why else ""))


def _universe_or_exit(cmd, tree, args, least, most=None, most_why=""):
    """-> the FASTAs of -f (default: every leaf), in the order `progressive -f` takes them: `least` to `most` of them"""
    fastas = tree.progressive_fastas(args.flist_loc)
    n = len(fastas)
    if n < least:
        sys.exit(f"{cmd}: {n} genome(s) in the universe: at least 2 are needed" if least == 2 else
                 f"{cmd}: {n} genomes in the universe: at least {least} is needed")
    if most is not None and n > most:
        sys.exit(f"{cmd}: {n} genomes in the universe: at most {most} ({most_why}); choose them with -f/--fastas")
    return fastas


MASK_BITS = "a membership mask has one bit per genome"    # why `core`, `screen` and `patterns` take at most 64 genomes


def _groups_in_universe(cmd, args, leaf_of, fastas):
    """-> (groups, labels) of -g, every member in the universe; ([], []) without -g"""
    if not args.groups_loc:
        return [], []
    groups, labels = _read_groups(cmd, args.groups_loc, leaf_of)
    for g in groups:
        for f in g:
            if f not in fastas:
                sys.exit(f"{cmd}: {f} (-g) is not in the universe of this run (-f)")
    return groups, labels


def _rank0_after_presketch(tree, window):
    """A multi-GPU run: every rank sketches its share of the leaves for the window; -> True on the rank that finishes alone"""
    rank, world = deltatree.dist_ranks()
    if world > 1:
        tree.presketch_range(*window)      # (ends at the barrier, which switches sharding off: the rank is asked for before it)
    return rank == 0


def _finish(tree):
    tree.speciesinfo.save_cardkey(tree.experiment["tool"])
    tree.speciesinfo.save_references(fast=False)


def deltadelta_command(args):
    """How much each genome (or group of genomes) adds to the collection's delta: delta(all) - delta(all but it), the quantity
    of the reference's DeltaTree.find_delta_delta (lib/huffman_dandd.py:559-566), for every group in one command."""
    tree, outfile = _open_tree("deltadelta", args)
    groups, labels = _deltadelta_groups(tree, args)
    os.makedirs(args.outdir, exist_ok=True)
    window = (int(args.mink), int(args.maxk)) if args.ksweep else (None, None)
    try:
        rows, summary = tree.leave_out_deltas(groups, *window, labels=labels)
    except ValueError as e:
        sys.exit(f"deltadelta: {e}")
    write_listdict_to_csv(outfile + ".deltadelta.csv", rows)
    if summary:
        write_listdict_to_csv(outfile + "_deltadeltasummary.csv", summary)
    _finish(tree)


def _write_csv(path, cols, rows):
    """rows (lists) under the header `cols`, in that order; None is an empty cell"""
    import csv
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(cols)
        w.writerows(rows)


def abba_command(args):
    """Exact order effects over ALL n! orderings of n <= 16 genomes, from the unions of all 2^n subsets: the growth curve,
    each genome's mean / min / max contribution, and "A before B, B before A" -- b's mean increment at each of its
    positions over the orderings with a before it and over those with a after it.  The reference planned this sub-command
    (lib/dandd_cmd.py:248-258, commented out) and sampled orderings with `progressive` in its place."""
    tree, outfile = _open_tree("abba", args, safe=True)
    window = _window_or_exit("abba", args, tree, why="hill-climb deltas per subset would depend on the order of the climbs")
    leaf_of = _leaf_lookup(tree, "abba", args.delta_tree)
    fastas = _universe_or_exit("abba", tree, args, least=2, most=16, most_why="2^n subset unions")
    n = len(fastas)
    if (args.fastaA is None) != (args.fastaB is None):
        sys.exit("abba: -A/--fastaA and -B/--fastaB go together")
    pairs = [(a, b) for a in range(n) for b in range(n) if a != b]
    if args.fastaA is not None:
        fa, fb = leaf_of(args.fastaA), leaf_of(args.fastaB)
        if fa == fb:
            sys.exit(f"abba: -A and -B name the same genome {fa}")
        for f in (fa, fb):
            if f not in fastas:
                sys.exit(f"abba: {f} is not in the universe of this run (-f)")
        ia, ib = fastas.index(fa), fastas.index(fb)
        pairs = [(ia, ib), (ib, ia)]
    if not _rank0_after_presketch(tree, window):
        return
    os.makedirs(args.outdir, exist_ok=True)
    ex = tree.ordering_expectations(fastas, *window)
    delta, kval, growth, contrib = ex["delta"], ex["kval"], ex["growth"], ex["contrib"]
    from math import factorial
    half, per = factorial(n) // 2, factorial(n - 2)
    rows = []
    for a, b in pairs:
        for s in range(1, n + 1):
            nb, na = (s - 1) * per, (n - s) * per
            mb = float(ex["before"][a, b, s - 1]) if nb else None
            ma = float(ex["after"][a, b, s - 1]) if na else None
            rows.append([fastas[a], fastas[b], s, nb, mb, na, ma, mb - ma if nb and na else None])
        mb, ma = float(ex["before_all"][a, b]), float(ex["after_all"][a, b])
        rows.append([fastas[a], fastas[b], "all", half, mb, half, ma, mb - ma])
    _write_csv(outfile + ".abba.csv", ["a", "b", "step", "orderings_a_before", "mean_a_before", "orderings_a_after",
                                       "mean_a_after", "abba"], rows)
    full = (1 << n) - 1
    rows = [[f, float(delta[1 << g]), int(kval[1 << g]), float(contrib[g, 0]), float(contrib[g, 1]), float(contrib[g, 2]),
             float(delta[full] - delta[full ^ (1 << g)])] for g, f in enumerate(fastas)]
    _write_csv(outfile + ".abba_contrib.csv", ["fasta", "delta_alone", "k_alone", "mean_contrib", "min_contrib", "max_contrib",
                                               "delta_last"], rows)
    rows = [[ng, int(growth[ng - 1, 0]), float(growth[ng - 1, 1]), float(growth[ng - 1, 2]), float(growth[ng - 1, 3]),
             float(growth[ng - 1, 4])] for ng in range(1, n + 1)]
    _write_csv(outfile + ".abba_growth.csv", ["ngen", "nsubsets", "mean", "sd", "min", "max"], rows)
    if args.subsets:
        size = ex["size"]
        rows = [[mask, int(size[mask]), float(delta[mask]), int(kval[mask]),
                 "|".join(fastas[i] for i in range(n) if mask >> i & 1)] for mask in range(1, full + 1)]
        _write_csv(outfile + ".abba_subsets.csv", ["mask", "ngen", "delta", "kval", "fastas"], rows)
    _finish(tree)


def greedy_command(args):
    """The steepest and the flattest growth ordering: add at each step the genome that raises delta the most (--mode max) or
    the least (min) -- the envelope `progressive`'s sampled orderings are read against, and the answer to "which genome
    next".  Each step depends on the union so far, so the orderings cannot be listed in advance."""
    tree, outfile = _open_tree("greedy", args, safe=True)
    window = _window_or_exit("greedy", args, tree, why="hill-climb deltas per candidate would depend on the order of the climbs")
    leaf_of = _leaf_lookup(tree, "greedy", args.delta_tree)
    fastas = _universe_or_exit("greedy", tree, args, least=2)
    n = len(fastas)
    base = []
    if args.base_loc:
        with open(args.base_loc) as fh:
            names = [line.strip() for line in fh if line.strip()]
        for name in names:
            f = leaf_of(name)
            if f not in fastas:
                sys.exit(f"greedy: {f} (-b) is not in the universe of this run (-f)")
            if f in base:
                sys.exit(f"greedy: {f} is listed twice in {args.base_loc}")
            base.append(f)
    steps = n if args.steps is None else int(args.steps)
    if steps < 1 or steps > n:
        sys.exit(f"greedy: --steps {steps} outside 1..{n}, the genomes in the universe")
    if steps < len(base):
        sys.exit(f"greedy: --steps {steps} is fewer than the {len(base)} genomes of -b/--base, which start every ordering")
    modes = ["max", "min"] if args.mode == "both" else [args.mode]
    if not _rank0_after_presketch(tree, window):
        return
    os.makedirs(args.outdir, exist_ok=True)
    res = tree.greedy_orderings(fastas, *window, modes, base=base, steps=steps)
    rows, summary = [], []
    for mode in modes:
        r = res[mode]
        prev = 0.0
        for j, f in enumerate(r["order"]):
            delta = float(r["delta"][j])
            rows.append([mode, j + 1, f, delta, int(r["kval"][j]), delta - prev, "|".join(r["order"][:j + 1])])
            prev = delta
            for k, c in zip(res["ks"], r["cards"][j]):
                summary.append([mode, j + 1, int(k), float(c), float(c) / k])
        with open(f"{outfile}.greedy_{mode}.txt", "w") as fh:
            fh.write("".join(f + "\n" for f in r["order"]))
    _write_csv(outfile + ".greedy.csv", ["mode", "ngen", "fasta", "delta", "kval", "gain", "fastas"], rows)
    _write_csv(outfile + ".greedysummary.csv", ["mode", "ngen", "kval", "card", "delta_pos"], summary)
    _finish(tree)


def core_command(args):
    """The intersection side of a pan-genome study, exact: how many k-mers 1, 2, ... n genomes hold (the spectrum), the core
    of every prefix of an ordering next to its union (the second curve of a pan/core plot), and per group of genomes its
    core, its private k-mers and its signature (in every member, in nobody else).  All of it sums over the membership
    masks of an exact tree; sketches have no such sums (inclusion-exclusion over 2^n union estimates amplifies their error)."""
    tree, outfile = _open_tree("core", args, exact=True, safe=True)
    window = _window_or_exit("core", args, tree)
    leaf_of = _leaf_lookup(tree, "core", args.delta_tree)
    fastas = _universe_or_exit("core", tree, args, least=1, most=64, most_why=MASK_BITS)
    n = len(fastas)
    orderings = [tuple(range(n))]
    if args.ordering_file or args.norderings:
        try:
            fastas, orderings = tree.orderings_list(ordering_file=args.ordering_file, flist_loc=args.flist_loc, count=args.norderings)
        except ValueError as e:
            sys.exit(f"core: {e}")
    for o in orderings:
        if sorted(o) != list(range(n)):
            sys.exit(f"core: an ordering of {len(o)} entries does not order the {n} genomes of the universe")
    groups, labels = _groups_in_universe("core", args, leaf_of, fastas)

    def in_window_or_exit(flag, ks):
        for k in ks or []:
            if not max(1, window[0]) <= k <= window[1]:
                sys.exit(f"core: {flag} {k} is outside the k window {max(1, window[0])}..{window[1]}")
    if not args.kmers and (args.kmers_k or args.kmers_max is not None):
        sys.exit("core: --kmers-k and --kmers-max go with --kmers")
    kmers_max = 1_000_000 if args.kmers_max is None else int(args.kmers_max)
    if args.kmers:
        in_window_or_exit("--kmers-k", args.kmers_k)
        if kmers_max < 0:
            sys.exit(f"core: --kmers-max {kmers_max}: a number of k-mers")
    if not args.regions and args.regions_k:
        sys.exit("core: --regions-k goes with --regions")
    if args.regions:
        in_window_or_exit("--regions-k", args.regions_k)
    if (args.kmers or args.regions) and not groups:                  # the whole universe: its core is the core genome
        groups, labels = [list(fastas)], ["all"]
    os.makedirs(args.outdir, exist_ok=True)
    try:
        res = tree.core_tables(fastas, *window, orderings, groups)
    except ValueError as e:
        sys.exit(f"core: {e}")
    lists = []
    if args.kmers:
        try:
            lists = tree.core_kmers(fastas, groups, args.kmers, ks=sorted(set(args.kmers_k or [])) or None, limit=kmers_max,
                                    window=window, counts=res["groups"])
        except ValueError as e:
            sys.exit(f"core: {e} (--kmers-max {kmers_max}: raise it, or narrow the class)" if "more than the limit" in str(e) else f"core: {e}")
    regions = []
    if args.regions:
        try:
            regions = tree.core_regions(fastas, groups, args.regions, ks=sorted(set(args.regions_k or [])) or None, window=window,
                                        counts=res["groups"])
        except ValueError as e:
            sys.exit(f"core: {e}")
    ks = res["ks"]
    delta_of = deltatree._window_delta
    spec = res["spectrum"]
    _write_csv(outfile + ".core_spectrum.csv", ["k", "ngen", "kmers"],
               [[k, j, int(spec[j, kk])] for kk, k in enumerate(ks) for j in range(1, n + 1)])
    rows, summary = [], []
    for o, order in enumerate(orderings):
        for j, g in enumerate(order):
            pan, core = [int(v) for v in res["pan"][o, j]], [int(v) for v in res["core"][o, j]]
            rows.extend([o + 1, j + 1, fastas[g], k, p, c] for k, p, c in zip(ks, pan, core))
            summary.append([o + 1, j + 1, fastas[g], *delta_of(pan, ks), *delta_of(core, ks)])
    _write_csv(outfile + ".core_growth.csv", ["ordering", "step", "fasta", "k", "pan", "core"], rows)
    _write_csv(outfile + ".core_growthsummary.csv", ["ordering", "step", "fasta", "pan_delta", "pan_k", "core_delta", "core_k"], summary)
    if groups:
        rows, summary = [], []
        for gi, (label, g) in enumerate(zip(labels, groups)):
            cols = [[int(v) for v in res["groups"][gi, c]] for c in range(3)]
            rows.extend([label, len(set(g)), k, *(col[kk] for col in cols)] for kk, k in enumerate(ks))
            summary.append([label, len(set(g)), *(v for col in cols for v in delta_of(col, ks))])
        _write_csv(outfile + ".core_groups.csv", ["group", "ngen", "k", "core", "private", "signature"], rows)
        _write_csv(outfile + ".core_groupsummary.csv", ["group", "ngen", "core_delta", "core_k", "private_delta", "private_k",
                                                        "signature_delta", "signature_k"], summary)
    if args.kmers:
        from ..engine import kmer_text
        index = []
        for cell in lists:                                           # (nothing is written before every list is there)
            gi, cls, k = cell["group"], cell["cls"], cell["k"]
            path = f"{outfile}.core_kmers.g{gi + 1}.{cls}.k{k}.fasta"
            with open(path, "w") as fh:
                for j, (text, m) in enumerate(zip(kmer_text(cell["kmers"], k), cell["masks"]), 1):
                    fh.write(f">{labels[gi]}.{cls}.k{k}.{j} ngen={bin(int(m)).count('1')}\n{text}\n")
            index.append([labels[gi], cls, k, len(cell["masks"]), os.path.basename(path)])
        _write_csv(outfile + ".core_kmers.csv", ["group", "class", "k", "kmers", "file"], index)
    if args.regions:
        index = []
        for cell in regions:                                         # (nothing is written before every cell is there)
            gi, cls, k = cell["group"], cell["cls"], cell["k"]
            path = f"{outfile}.core_regions.g{gi + 1}.{cls}.k{k}.bed"
            with open(path, "w") as fh:
                for fasta, rows in cell["genomes"]:
                    base = os.path.basename(fasta)
                    fh.write("".join(f"{name}\t{start}\t{end}\t{base}\n" for name, start, end in rows))
                    index.append([labels[gi], cls, k, base, len(rows), sum(end - start for _, start, end in rows), os.path.basename(path)])
        _write_csv(outfile + ".core_regions.csv", ["group", "class", "k", "fasta", "regions", "bases", "file"], index)
    _finish(tree)


def screen_command(args):
    """New samples -- assemblies or read sets that are no leaves -- against the genomes of an exact tree: how much of each
    genome a sample contains and the other way round, which genome it is closest to, how much of it is in the pan-genome and
    the core, and with -g which group's core, private k-mers and signature it carries.  Counts are over distinct k-mers;
    the samples enter no sort and change none of the collection's numbers.  --paint W adds the positional answer: every
    sample in windows of W bases, counted over positions (_paint_rows).  --reads adds the answer for a read set or a draft
    assembly: every record called to the genome that holds most of its k-mer positions, and the sample's abundance profile
    over the genomes, voted and tallied on the device (_reads_rows).  --depth adds how many times the sample holds the k-mers
    of every genome and class: a histogram of depths per row, counted and binned on the device (_depth_rows).  --cover W turns
    the view round: every genome of the collection in windows of W bases, and per sample how much of each window it holds and
    how deep (_cover_rows).  --gather explains every sample by the genomes one by one, a greedy set cover walked on the
    device (_gather_rows)."""
    tree, outfile = _open_tree("screen", args, exact=True)
    ks = sorted(set(int(k) for k in args.ks)) if args.ks else [int(tree.root_k())]
    for k in ks:
        if not 1 <= k <= 64:
            sys.exit(f"screen: -k {k} is outside 1..64")
    if args.paint is not None and (args.paint < 64 or args.paint % 64 or args.paint > 1 << 22):
        sys.exit(f"screen: --paint {args.paint}: a window is a multiple of 64 bases in 64..{1 << 22}")
    if args.paint_matrix and args.paint is None:
        sys.exit("screen: --paint-matrix goes with --paint")
    if args.reads_calls and not args.reads:
        sys.exit("screen: --reads-calls goes with --reads")
    if args.reads_min_hits < 1:
        sys.exit(f"screen: --reads-min-hits {args.reads_min_hits}: a call needs at least one position (H >= 1)")
    if (args.depth_bins is not None or args.depth_hist) and not args.depth:
        sys.exit(f"screen: {'--depth-bins' if args.depth_bins is not None else '--depth-hist'} goes with --depth")
    bins = 64 if args.depth_bins is None else args.depth_bins
    if not 2 <= bins <= 256:
        sys.exit(f"screen: --depth-bins {bins}: bin 0, then at least the clipped bin, 256 bins at the most (B in 2..256)")
    if args.cover is not None and (args.cover < 64 or args.cover % 64 or args.cover > 1 << 22):
        sys.exit(f"screen: --cover {args.cover}: a window is a multiple of 64 bases in 64..{1 << 22}")
    for flag, value in (("--cover-fastas", args.cover_fastas), ("--cover-clip", args.cover_clip), ("--cover-min", args.cover_min)):
        if value is not None and args.cover is None:
            sys.exit(f"screen: {flag} goes with --cover")
    clip = 255 if args.cover_clip is None else args.cover_clip
    if not 1 <= clip <= 1023:
        sys.exit(f"screen: --cover-clip {clip}: a position's depth counts as at most C, C in 1..1023")
    cover_min = 50 if args.cover_min is None else args.cover_min
    if not 1 <= cover_min <= 100:
        sys.exit(f"screen: --cover-min {cover_min}: the per cent of a window's positions a sample must hold, P in 1..100")
    for flag, value in (("--gather-min", args.gather_min), ("--gather-steps", args.gather_steps)):
        if value is not None and not args.gather:
            sys.exit(f"screen: {flag} goes with --gather")
    gather_min = 1 if args.gather_min is None else args.gather_min
    if not 1 <= gather_min < 1 << 32:
        sys.exit(f"screen: --gather-min {gather_min}: a pick adds at least one k-mer, and the count is 32 bits wide (H in 1..{(1 << 32) - 1})")
    if args.gather_steps is not None and args.gather_steps < 1:
        sys.exit(f"screen: --gather-steps {args.gather_steps}: at least one pick (N >= 1)")
    if args.cover_fastas is not None and not os.path.isfile(args.cover_fastas):
        sys.exit(f"screen: {args.cover_fastas} (--cover-fastas) not found")
    names = list(args.samples)
    if args.query_loc:
        if not os.path.isfile(args.query_loc):
            sys.exit(f"screen: {args.query_loc} (-q) not found")
        names.extend(line.strip() for line in _lines(args.query_loc))
    samples = []
    for f in names:
        if f not in samples:
            samples.append(f)
    if not samples:
        sys.exit("screen: no sample: give files, or -q with one path per line")
    for f in samples:
        if not os.path.isfile(f):
            sys.exit(f"screen: {f} not found")
    leaf_of = _leaf_lookup(tree, "screen", args.delta_tree)
    fastas = _universe_or_exit("screen", tree, args, least=1, most=64, most_why=MASK_BITS)
    ns = len(samples)
    if args.gather_steps is not None and args.gather_steps > len(fastas):
        sys.exit(f"screen: --gather-steps {args.gather_steps}: the universe of this run has {len(fastas)} genomes (N in 1..{len(fastas)})")
    groups, labels = _groups_in_universe("screen", args, leaf_of, fastas)
    cover_targets = None                                                 # --cover-fastas: the genomes the samples are laid along
    if args.cover_fastas is not None:
        cover_targets = []
        for name in _lines(args.cover_fastas):
            f = leaf_of(name.strip())
            if f not in fastas:
                sys.exit(f"screen: {f} (--cover-fastas) is not in the universe of this run (-f)")
            if f in cover_targets:
                sys.exit(f"screen: {f} stands twice in {args.cover_fastas} (--cover-fastas)")
            cover_targets.append(f)
        if not cover_targets:
            sys.exit(f"screen: {args.cover_fastas} (--cover-fastas) names no genome")
    try:
        res = tree.screen_tables(fastas, samples, ks, groups)
        painted = tree.paint_tables(fastas, samples, ks, args.paint) if args.paint is not None else None
        called = tree.reads_tables(fastas, samples, ks, args.reads_min_hits, args.reads_calls) if args.reads else None
        depths = tree.depth_tables(fastas, samples, ks, groups, bins) if args.depth else None
        covered = tree.cover_tables(fastas, samples, ks, args.cover, cover_targets, clip) if args.cover is not None else None
        gathered = tree.gather_tables(fastas, samples, ks, gather_min, args.gather_steps) if args.gather else None
    except (ValueError, OSError) as e:
        sys.exit("screen: " + " ".join(str(e).split()))

    def ratio(a, b):
        return a / b if b else None
    rows, summary, marks = [], [], []
    for s, sample in enumerate(samples):                                 # (nothing is written before every table is there)
        for kk, k in enumerate(ks):
            q = int(res["sample_kmers"][kk, s])
            best = None
            for i, fasta in enumerate(fastas):
                g, sh = int(res["shared"][kk, ns, i]), int(res["shared"][kk, s, i])
                jac = ratio(sh, g + q - sh)
                rows.append([sample, k, fasta, g, q, sh, ratio(sh, g), ratio(sh, q), jac])
                if sh and (best is None or jac > best[1]):               # (ties: the earlier genome of the universe)
                    best = (fasta, jac, ratio(sh, g))
            in_pan, in_core = int(res["match"][kk, s, 0]), int(res["match"][kk, s, 1])
            summary.append([sample, k, q, in_pan, q - in_pan, in_core, *(best or (None, None, None))])
            for gi, label in enumerate(labels):
                for c, cls in enumerate(tree.KMER_CLASSES):
                    total, hits = int(res["match"][kk, ns, 2 + 3 * gi + c]), int(res["match"][kk, s, 2 + 3 * gi + c])
                    marks.append([sample, k, label, cls, total, hits, ratio(hits, total)])
    os.makedirs(args.outdir, exist_ok=True)
    _write_csv(outfile + ".screen.csv", ["sample", "k", "fasta", "genome_kmers", "sample_kmers", "shared", "genome_containment",
                                         "sample_containment", "jaccard"], rows)
    _write_csv(outfile + ".screen_summary.csv", ["sample", "k", "sample_kmers", "in_pan", "novel", "in_core", "best_fasta", "best_jaccard",
                                                 "best_genome_containment"], summary)
    if groups:
        _write_csv(outfile + ".screen_groups.csv", ["sample", "k", "group", "class", "marker_kmers", "hits", "fraction"], marks)
    if painted is not None:
        windows, segments, matrix = _paint_rows(samples, fastas, painted)
        _write_csv(outfile + ".paint.csv", ["sample", "k", "window", "tok_start", "tok_end", "record", "start", "end", "records", "valid", "in_pan",
                                            "novel", "best_fasta", "best_shared", "second_fasta", "second_shared"], windows)
        _write_csv(outfile + ".paint_segments.csv", ["sample", "k", "first_window", "last_window", "tok_start", "tok_end", "best_fasta", "valid",
                                                     "in_pan", "best_shared"], segments)
        if args.paint_matrix:
            _write_csv(outfile + ".paint_matrix.csv", ["sample", "k", "window", *fastas], matrix)
    if called is not None:
        profile, records = _reads_rows(samples, fastas, called)
        _write_csv(outfile + ".reads_summary.csv", ["sample", "k", "target", "reads", "fraction"], profile)
        if args.reads_calls:
            _write_csv(outfile + ".reads.csv", ["sample", "k", "record", "name", "length", "valid", "in_pan", "class", "best_fasta", "best_shared",
                                                "second_fasta", "second_shared", "ties", "consistent"], records)
    if depths is not None:
        stats, hists = _depth_rows(samples, fastas, labels, tree.KMER_CLASSES, depths)
        _write_csv(outfile + ".depth.csv", DEPTH_COLUMNS, stats)
        if args.depth_hist:
            _write_csv(outfile + ".depth_hist.csv", ["sample", "k", "target", "class", "depth", "kmers"], hists)
    if covered is not None:
        for name, rows in zip(COVER_COLUMNS, _cover_rows(samples, covered, cover_min)):
            _write_csv(f"{outfile}.{name}.csv", COVER_COLUMNS[name], rows)
    if gathered is not None:
        for name, rows in zip(GATHER_COLUMNS, _gather_rows(samples, fastas, res, gathered)):
            _write_csv(f"{outfile}.{name}.csv", GATHER_COLUMNS[name], rows)
    _finish(tree)


GATHER_COLUMNS = {
    "gather": ["sample", "k", "rank", "fasta", "genome_kmers", "shared", "unique", "f_sample_unique", "f_genome_shared", "f_genome_unique",
               "unique_depth", "mean_depth", "f_depth", "remaining"],
    "gather_summary": ["sample", "k", "sample_kmers", "in_pan", "novel", "genomes", "explained", "unexplained", "top_fasta"],
}


def _gather_rows(samples, fastas, res, gathered):
    """gather_tables' walk, with screen_tables' sizes -> the rows of <prefix>.gather.csv (one per sample, k and pick, rank 1
    first: the genome, its k-mers, those the sample shares with it, those of them no earlier pick holds -- `unique` --, unique
    over the sample's k-mers, shared and unique over the genome's, the times the sample holds the unique ones -- summed, per
    k-mer, and over the depth of all the sample holds of the pan-genome --, and the sample's k-mers in the pan-genome that are
    still unexplained behind this pick) and of .gather_summary.csv (one per sample and k: the sample's k-mers, those in the
    pan-genome, the others, the picks, the k-mers they explain together, those they leave, the first pick; an empty cell
    where a ratio has nothing to stand on or nothing is picked)."""
    ns = len(samples)
    ratio = lambda a, b: a / b if b else None
    picks, summary = [], []
    for s, sample in enumerate(samples):
        for kk, k in enumerate(gathered["ks"]):
            q, in_pan = int(res["sample_kmers"][kk, s]), int(res["match"][kk, s, 0])
            deep = int(gathered["total"][kk, s, 1])
            explained, chosen = 0, []
            for t, i in enumerate(gathered["pick"][kk, s].tolist()):
                if i < 0:
                    break
                g, sh = int(res["shared"][kk, ns, i]), int(gathered["shared"][kk, s, i])
                uq, ud = int(gathered["unique"][kk, s, t]), int(gathered["depth"][kk, s, t])
                explained += uq
                chosen.append(fastas[i])
                picks.append([sample, k, t + 1, fastas[i], g, sh, uq, ratio(uq, q), ratio(sh, g), ratio(uq, g), ud, ratio(ud, uq), ratio(ud, deep),
                              in_pan - explained])
            summary.append([sample, k, q, in_pan, q - in_pan, len(chosen), explained, in_pan - explained, chosen[0] if chosen else None])
    return picks, summary


COVER_COLUMNS = {
    "cover": ["sample", "k", "fasta", "window", "record", "start", "end", "records", "valid", "covered", "depth", "private", "private_covered",
              "private_depth"],
    "cover_regions": ["sample", "k", "fasta", "state", "first_window", "windows", "record", "start", "end_record", "end", "valid", "covered",
                      "depth"],
    "cover_summary": ["sample", "k", "fasta", "windows", "valid", "covered", "breadth", "depth", "mean_covered_depth", "private", "private_covered",
                      "private_breadth", "private_mean_covered_depth", "present_windows", "absent_windows", "empty_windows",
                      "longest_absent_windows"],
}
COVER_STATES = ("empty", "present", "absent")     # engine.cover_states' states, as the files name them


def _cover_rows(samples, covered, min_percent):
    """cover_tables' counters -> the rows of <prefix>.cover.csv (one per sample, k, genome and window of the genome: where the
    window lies in the genome's records -- engine.paint_windows -- and its six counts), of .cover_regions.csv (the runs of
    consecutive windows with the same state -- engine.cover_states: present, absent, empty --: the record and base the run
    starts at, the record and base its last window ends at, the sums of its windows) and of .cover_summary.csv (one per sample,
    k and genome: the sums over its windows, breadth = covered / valid, the mean depth of the covered positions, the same of
    the private positions, the windows of each state and the longest absent run; an empty cell where a ratio has nothing to
    stand on)."""
    from ..engine import COVER_ABSENT, cover_states, paint_windows
    W = covered["window"]
    ratio = lambda a, b: a / b if b else None
    windows, regions, summary = [], [], []
    for s, sample in enumerate(samples):
        for kk, k in enumerate(covered["ks"]):
            for t, fasta in enumerate(covered["targets"]):
                names, seq_len, tok_start, _ = covered["index"][t]
                rows = covered["counts"][kk][t][s]
                record, start, end, records = paint_windows(len(rows), W, tok_start, seq_len)
                name_of = lambda w: names[record[w]] if record[w] >= 0 else None
                body = rows.astype("int64").tolist()
                for w, row in enumerate(body):
                    windows.append([sample, k, fasta, w, name_of(w), int(start[w]), int(end[w]), int(records[w]), *row])
                states, runs = cover_states(rows, min_percent)
                for state, first, length in runs.tolist():
                    last = first + length - 1
                    valid, cov, depth = (sum(r[c] for r in body[first:last + 1]) for c in range(3))
                    regions.append([sample, k, fasta, COVER_STATES[state], first, length, name_of(first), int(start[first]), name_of(last),
                                    int(end[last]), valid, cov, depth])
                tot = [sum(r[c] for r in body) for c in range(6)]
                per = [int((states == st).sum()) for st in range(3)]
                longest = max((length for state, _, length in runs.tolist() if state == COVER_ABSENT), default=0)
                summary.append([sample, k, fasta, len(body), tot[0], tot[1], ratio(tot[1], tot[0]), tot[2], ratio(tot[2], tot[1]), tot[3], tot[4],
                                ratio(tot[4], tot[3]), ratio(tot[5], tot[4]), per[1], per[2], per[0], longest])
    return windows, regions, summary


DEPTH_COLUMNS = ["sample", "k", "target", "class", "kmers", "covered", "breadth", "mean_depth", "mean_covered", "median_depth", "median_covered",
                 "clipped"]


def _depth_rows(samples, fastas, labels, classes, depths):
    """depth_tables' answer -> the rows of <prefix>.depth.csv (per sample and k: every genome's k-mers (`all`) and its
    private ones, the pan-genome, the core, and every group's classes; engine.depth_stats' columns, an empty cell where a
    number has nothing to stand on -- a row without a k-mer, the covered columns of a row the sample holds nothing of) and
    of .depth_hist.csv (the non-zero bins of the same rows, the last bin's depth written as >=B-1)."""
    from ..engine import depth_stats
    n, B = len(fastas), int(depths["bins"])
    targets = [(fasta, cls, row) for i, fasta in enumerate(fastas) for cls, row in (("all", i), ("private", n + 2 + i))]   # rows: n genomes | pan | core | n private | groups
    targets += [("pan", "all", n), ("core", "all", n + 1)]
    targets += [(label, cls, 2 * n + 2 + len(classes) * gi + c) for gi, label in enumerate(labels) for c, cls in enumerate(classes)]
    st = depth_stats(depths["hist"], depths["total"])
    cell = lambda v, as_int=False: None if v != v else int(v) if as_int else float(v)   # (NaN: an empty cell)
    stats, hists = [], []
    for s, sample in enumerate(samples):
        for kk, k in enumerate(depths["ks"]):
            for target, cls, row in targets:
                at = (kk, s, row)
                stats.append([sample, k, target, cls, int(st["kmers"][at]), int(st["covered"][at]), cell(st["breadth"][at]), cell(st["mean"][at]),
                              cell(st["mean_covered"][at]), cell(st["median"][at], True), cell(st["median_covered"][at], True),
                              bool(st["clipped"][at])])
                for d, v in enumerate(depths["hist"][at].tolist()):
                    if v:
                        hists.append([sample, k, target, cls, f">={d}" if d == B - 1 else d, v])
    return stats, hists


def _paint_rows(samples, fastas, painted):
    """paint_tables' counters -> the rows of <prefix>.paint.csv (one per sample, k and window: where the window lies, and
    the two genomes that share most positions with it -- ties: the earlier genome of the universe; empty cells where nothing
    is shared), of .paint_segments.csv (runs of consecutive windows of a sample and k with the same best genome; the windows
    the universe holds nothing of form runs of their own, with an empty best_fasta: the novel stretches) and of
    .paint_matrix.csv (the genomes' columns as they are)."""
    from ..engine import paint_windows
    W = painted["window"]
    windows, segments, matrix = [], [], []
    for s, sample in enumerate(samples):
        names, seq_len, tok_start, ntok = painted["index"][s]
        for kk, k in enumerate(painted["ks"]):
            rows = painted["counts"][kk][s]
            record, start, end, records = paint_windows(len(rows), W, tok_start, seq_len)
            seg = seg_best = None                                        # the row of the segments in the making, and its best genome
            for w, row in enumerate(rows):
                valid, in_pan, cols = int(row[0]), int(row[1]), [int(v) for v in row[2:]]
                order = sorted(range(len(cols)), key=lambda i: (-cols[i], i))
                best = order[0] if in_pan else None
                second = order[1] if in_pan and len(order) > 1 and cols[order[1]] else None
                windows.append([sample, k, w, w * W, min((w + 1) * W, int(ntok)), names[record[w]] if record[w] >= 0 else None,
                                int(start[w]), int(end[w]), int(records[w]), valid, in_pan, valid - in_pan,
                                None if best is None else fastas[best], None if best is None else cols[best],
                                None if second is None else fastas[second], None if second is None else cols[second]])
                matrix.append([sample, k, w, *cols])
                if seg is None or seg_best != best:
                    seg, seg_best = [sample, k, w, w, w * W, 0, None if best is None else fastas[best], 0, 0, None if best is None else 0], best
                    segments.append(seg)
                seg[3], seg[5], seg[7], seg[8] = w, windows[-1][4], seg[7] + valid, seg[8] + in_pan
                if best is not None:
                    seg[9] += cols[best]
    return windows, segments, matrix


READ_CLASSES = ("ambiguous", "unclassified", "no_kmer")    # the tally's bins behind the genomes', and a record's class beside "unique"


def _reads_rows(samples, fastas, called):
    """reads_tables' answer -> the rows of <prefix>.reads_summary.csv (per sample and k: the records uniquely called to each
    genome, then the ambiguous, the unclassified and those without a valid k-mer, each with its share of the sample's
    records; an empty cell for a sample without a record) and of .reads.csv (one per sample, k and record: its name and
    length, the positions with a valid k-mer and those the collection holds, its class, the two genomes that share most
    positions with it -- ties: the earlier genome of the universe; empty cells where nothing is shared --, how many genomes
    tie for the best count and how many hold every shared position; no row without the calls)."""
    from ..engine import NO_GENOME, read_classes
    n = len(fastas)
    profile, records = [], []
    for s, sample in enumerate(samples):
        names, seq_len, _, _ = called["index"][s]
        for kk, k in enumerate(called["ks"]):
            tally = [int(v) for v in called["tally"][kk][s]]
            total = sum(tally)
            for target, reads in zip([*fastas, *READ_CLASSES], tally):
                profile.append([sample, k, target, reads, reads / total if total else None])
            if called["calls"][kk][s] is None:
                continue
            calls, sets = called["calls"][kk][s]
            classes, _ = read_classes(calls, sets, called["min_hits"], n)
            for r, (row, (ties, full), cls) in enumerate(zip(calls.tolist(), sets.tolist(), classes.tolist())):
                valid, hit, best, best_count, second, second_count = row
                records.append([sample, k, r, names[r], int(seq_len[r]), valid, hit, "unique" if cls < n else READ_CLASSES[cls - n],
                                None if best == NO_GENOME else fastas[best], None if best == NO_GENOME else best_count,
                                None if second == NO_GENOME else fastas[second], None if second == NO_GENOME else second_count,
                                bin(ties).count("1"), bin(full).count("1")])
    return profile, records


NEIGHBORS_COLUMNS = {
    "neighbors": ["sample", "fasta", "sample_delta", "sample_k", "genome_delta", "genome_k", "union_delta", "union_k", "KIJ", "rank"],
    "neighbors_summary": ["sample", "sample_delta", "sample_k", "best_fasta", "best_KIJ", "second_fasta", "second_KIJ", "collection_delta",
                          "with_sample_delta", "delta_added"],
    "neighbors_j": ["sample", "fasta", "kval", "Scard", "Gcard", "SGcard", "jaccard"],
}


def _neighbor_rows(samples, fastas, res, top=None):
    """neighbor_tables' cards -> the rows of <prefix>.neighbors.csv (per sample the genomes by KIJ = (delta_S + delta_G -
    delta_SG) / delta_SG descending, ties in the universe's order, rank 1 first, the first `top` of them), of
    .neighbors_summary.csv (one per sample: its two closest genomes, the collection's delta, the delta of the collection with
    the sample, and their difference -- the sample's deltadelta as a newcomer) and of .neighbors_j.csv (kij's .j.csv for
    the rectangle: per sample, genome and k the three cardinalities and their Jaccard)"""
    rows, summary, jrows = [], [], []
    for s, sample in enumerate(samples):
        ds, ks_ = float(res["sample_delta"][s]), int(res["sample_k"][s])
        kij = []
        for j in range(len(fastas)):
            dsg = float(res["pair_delta"][s, j])
            kij.append((ds + float(res["genome_delta"][j]) - dsg) / dsg if dsg else 0.0)       # (an empty sample against an empty genome)
        order = sorted(range(len(fastas)), key=lambda j: -kij[j])       # (stable: ties keep the universe's order)
        for rank, j in enumerate(order[:top], 1):
            rows.append([sample, fastas[j], ds, ks_, float(res["genome_delta"][j]), int(res["genome_k"][j]), float(res["pair_delta"][s, j]),
                         int(res["pair_k"][s, j]), kij[j], rank])
        second = (fastas[order[1]], kij[order[1]]) if len(order) > 1 else (None, None)
        whole, joined = float(res["whole_delta"]), float(res["with_delta"][s])
        summary.append([sample, ds, ks_, fastas[order[0]], kij[order[0]], *second, whole, joined, joined - whole])
        for j, fasta in enumerate(fastas):
            for kk, k in enumerate(res["ks"]):
                a, b, ab = float(res["sample"][s, kk]), float(res["genome"][j, kk]), float(res["pair"][s, j, kk])
                jrows.append([sample, fasta, int(k), a, b, ab, (a + b - ab) / ab if ab else None])
    return rows, summary, jrows


def neighbors_command(args):
    """New samples against a tree of SKETCHES, the tree DandD builds by default and the one without a limit on its genomes:
    which genomes of the collection each sample is closest to by DandD's own K-independent Jaccard, and what the sample
    would add to the collection's delta.  One rectangle of unions -- samples x leaves x k -- over the leaf slab; the samples
    are sketched in memory and the tree's sketch directory, cardinality cache and pickle stay as they are."""
    tree, outfile = _open_tree("neighbors", args)
    if tree.experiment["tool"] == "kmc":
        sys.exit(f"neighbors: {args.delta_tree} is an exact tree: `screen` places samples in it by exact containment; "
                 "neighbors works on the unions of sketches")
    window = _window_or_exit("neighbors", args, tree, why="KIJ compares deltas taken over one window")
    if args.top is not None and args.top < 1:
        sys.exit(f"neighbors: --top {args.top}: at least one genome per sample (N >= 1)")
    names = list(args.samples)
    if args.query_loc:
        if not os.path.isfile(args.query_loc):
            sys.exit(f"neighbors: {args.query_loc} (-q) not found")
        names.extend(line.strip() for line in _lines(args.query_loc))
    samples = []
    for f in names:
        if f not in samples:
            samples.append(f)
    if not samples:
        sys.exit("neighbors: no sample: give files, or -q with one path per line")
    for f in samples:
        if not os.path.isfile(f):
            sys.exit(f"neighbors: {f} not found")
    fastas = _universe_or_exit("neighbors", tree, args, least=1)
    if not _rank0_after_presketch(tree, window):
        return
    try:
        res = tree.neighbor_tables(fastas, samples, *window)
    except (ValueError, OSError) as e:
        sys.exit("neighbors: " + " ".join(str(e).split()))
    rows, summary, jrows = _neighbor_rows(samples, fastas, res, args.top)
    os.makedirs(args.outdir, exist_ok=True)
    _write_csv(outfile + ".neighbors.csv", NEIGHBORS_COLUMNS["neighbors"], rows)
    _write_csv(outfile + ".neighbors_summary.csv", NEIGHBORS_COLUMNS["neighbors_summary"], summary)
    if args.jaccard:
        _write_csv(outfile + ".neighbors_j.csv", NEIGHBORS_COLUMNS["neighbors_j"], jrows)


def patterns_command(args):
    """Which sets of genomes share k-mers, and how many: the distinct membership masks of the universe with the distinct
    k-mers that carry exactly each -- the table behind an UpSet plot, and what tells which groups `core -g` and `screen -g`
    are worth asking about.  --splits reads the table as bipartitions of the universe and gives each its support."""
    tree, outfile = _open_tree("patterns", args, exact=True)
    ks = sorted(set(int(k) for k in args.ks)) if args.ks else [int(tree.root_k())]
    window = tree.experiment.get("ksweep")
    for k in ks:
        if not 1 <= k <= 64:
            sys.exit(f"patterns: -k {k} is outside 1..64")
        if window is not None and not max(1, int(window[0])) <= k <= int(window[1]):
            sys.exit(f"patterns: -k {k} is outside the k window {max(1, int(window[0]))}..{int(window[1])} of the tree")
    top, most = int(args.top), int(args.max_patterns)
    if top < 0 or most < 0:
        sys.exit("patterns: --top and --max-patterns are numbers of rows")
    fastas = _universe_or_exit("patterns", tree, args, least=1, most=64, most_why=MASK_BITS)
    n = len(fastas)
    full = (1 << n) - 1
    whole = args.splits or top == 0 or top > most        # (--splits needs every row)
    try:
        res = tree.pattern_tables(fastas, ks, top=most + 1)               # (one row more than allowed: too many shows)
    except (ValueError, OSError) as e:
        sys.exit("patterns: " + " ".join(str(e).split()))
    for k in ks:
        if whole and res[k]["found"] > most:
            sys.exit(f"patterns: {res[k]['found']} patterns at k={k}, more than --max-patterns {most}; give --top N for the largest N, "
                     "or raise --max-patterns")

    def members(mask):
        return ";".join(f for i, f in enumerate(fastas) if mask >> i & 1)
    rows, summary, splits = [], [], []
    for k in ks:                                                          # (nothing is written before every table is there)
        t = res[k]
        table = list(zip(t["masks"], t["counts"]))
        shown = table if top == 0 else table[:top]
        for rank, (mask, count) in enumerate(shown, 1):
            rows.append([k, rank, count, count / t["distinct"] if t["distinct"] else None, bin(mask).count("1"), f"{mask:x}", members(mask)])
        # core and singletons are sums over the whole table: empty cells when it has more than --max-patterns rows
        known = t["found"] <= most
        summary.append([k, t["distinct"], t["found"], len(shown), sum(c for _, c in shown),
                        sum(c for m, c in table if m == full) if known else None,
                        sum(c for m, c in table if m & (m - 1) == 0) if known else None, members(shown[0][0]) if shown else None])
        if args.splits:
            count_of = dict(table)
            sides = sorted({min(m, full ^ m) for m in count_of if 2 <= bin(m).count("1") <= n - 2})
            found = [(count_of.get(a, 0) + count_of.get(full ^ a, 0), a) for a in sides]
            for support, a in sorted(found, key=lambda r: (-r[0], r[1])):
                splits.append([k, members(a), members(full ^ a), support])
    os.makedirs(args.outdir, exist_ok=True)
    _write_csv(outfile + ".patterns.csv", ["k", "rank", "kmers", "fraction", "ngenomes", "mask", "members"], rows)
    _write_csv(outfile + ".patterns_summary.csv", ["k", "distinct_kmers", "patterns", "rows_written", "kmers_in_rows", "core", "singletons",
                                                   "top_members"], summary)
    if args.splits:
        _write_csv(outfile + ".splits.csv", ["k", "side_a", "side_b", "support"], splits)
    _finish(tree)


def serve_command(args):
    """A resident `dandd`: commands arrive over a unix socket (dandd_amd.host.client), run one at a time in THIS process --
    whose backends (deltatree._backends: GPU context, kernel modules, pinned buffers, job-table cache) outlive them -- with the
    client's working directory and DANDD_* / DD_* environment, and their stdout / stderr / exit status go back.  The code that
    runs is main() below, the one-shot CLI's: same files, byte for byte."""
    import contextlib
    import io
    import socket
    import time
    from .client import ENV_PREFIXES, recv_msg, send_msg
    path = args.socket
    try:
        os.unlink(path)
    except FileNotFoundError:
        pass
    srv = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
    old_mask = os.umask(0o177)   # the socket runs commands as this user: nobody else may connect, from the moment it exists
    try:
        srv.bind(path)
    finally:
        os.umask(old_mask)
    srv.listen(8)
    if args.warm:              # bring a backend up before the first command arrives: "<registers>[,nc]"
        for spec in args.warm:
            regs, _, flag = spec.partition(",")
            deltatree.backend_for({"registers": int(regs), "canonicalize": flag != "nc", "tool": "dashing"})
    deltatree.RESIDENT = True
    print(f"dandd serve: listening on {path}", flush=True)
    served, home = 0, os.getcwd()

    def handle(conn):
        """one connection = one request; -> True when the server is asked to leave"""
        nonlocal served
        conn.settimeout(10.0)      # a client that connects and then says nothing (or never reads its reply) holds the single line ten seconds, not for ever
        req = recv_msg(conn)
        if not isinstance(req, dict):
            return False
        if req.get("op") == "ping":
            send_msg(conn, {"rc": 0, "served": served, "pid": os.getpid()})
            return False
        if req.get("op") == "shutdown":
            send_msg(conn, {"rc": 0, "served": served})
            return True
        out, err = io.StringIO(), io.StringIO()
        saved = {k: v for k, v in os.environ.items() if k.startswith(ENV_PREFIXES)}
        t0 = time.perf_counter()
        rc = 1
        try:
            for k in saved:
                del os.environ[k]
            os.environ.update({k: str(v) for k, v in (req.get("env") or {}).items() if k.startswith(ENV_PREFIXES)})
            deltatree.new_command()
            with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
                try:
                    os.chdir(req.get("cwd") or home)      # (a directory that is gone: the client gets the message, like any failed command)
                    argv = list(req.get("argv") or [])
                    if argv[:1] == ["serve"]:
                        raise SystemExit("dandd serve: a server does not start servers")
                    rc = main(argv) or 0
                except SystemExit as e:
                    rc = e.code if isinstance(e.code, int) else (0 if e.code is None else 1)
                    if isinstance(e.code, str):
                        print(e.code, file=sys.stderr)
                except BaseException:
                    import traceback
                    traceback.print_exc()
                    rc = 1
        finally:
            for k in [k for k in os.environ if k.startswith(ENV_PREFIXES)]:
                del os.environ[k]
            os.environ.update(saved)
            os.chdir(home)
        served += 1
        send_msg(conn, {"rc": rc, "stdout": out.getvalue(), "stderr": err.getvalue(), "seconds": time.perf_counter() - t0})
        return False

    try:
        while True:
            srv.settimeout(args.idle_exit if args.idle_exit > 0 else None)
            try:
                conn, _ = srv.accept()
            except socket.timeout:
                break
            with conn:
                # a client that hangs up mid-command (Ctrl-C, a timeout) or sends something that is not a request costs its own
                # connection, never the server: the warm GPU context is what this process exists to keep
                try:
                    if handle(conn):
                        break
                except (OSError, ValueError) as e:   # (BrokenPipeError, ConnectionResetError; JSONDecodeError, UnicodeDecodeError)
                    print(f"dandd serve: connection dropped: {type(e).__name__}: {e}", file=sys.stderr, flush=True)
    finally:
        srv.close()
        try:
            os.unlink(path)
        except OSError:
            pass
    return 0


def build_parser():
    common = argparse.ArgumentParser(add_help=False)
    common.add_argument("--version", action="version", version="%(prog)s 1.0.0 (dandd_amd / MI355X)")
    common.add_argument("--verbose", "-v", action="store_true", default=False)
    common.add_argument("--debug", action="store_true", default=False)
    common.add_argument("--lowmem", action="store_true", default=False)
    common.add_argument("--safe", action="store_true", default=False, dest="safety")
    common.add_argument("--fast", action="store_true", default=False)
    sweep = argparse.ArgumentParser(add_help=False)
    sweep.add_argument("--ksweep", dest="ksweep", default=None, action="store_true")
    sweep.add_argument("--mink", dest="mink", default=2, type=int)
    sweep.add_argument("--maxk", dest="maxk", default=32, type=int)

    parser = argparse.ArgumentParser(prog="DandD", parents=[common],
                                     description="delta values for a set of fasta files (MI355X sketching engine)")
    subs = parser.add_subparsers(title="subcommands")
    subs.required = True

    t = subs.add_parser("tree", parents=[common, sweep])
    t.add_argument("-s", "--tag", dest="tag", type=str, default="dandd")
    t.add_argument("-x", "--exact", dest="exact", default=False, action="store_true")
    t.add_argument("-d", "--datadir", dest="genomedir", default=None, type=str)
    t.add_argument("-o", "--out", dest="outdir", default=os.getcwd(), type=str)
    t.add_argument("-c", "--sketchdir", dest="sketchdir", default=None, type=str)
    t.add_argument("-k", "--kstart", dest="kstart", default=12, type=int)
    t.add_argument("-f", "--fastas", dest="flist_loc", type=str, default=None)
    t.add_argument("-l", "--label", dest="label", default="")
    t.add_argument("-n", "--nchildren", dest="nchildren", type=int, default=None)
    t.add_argument("-r", "--registers", dest="registers", default=20)
    t.add_argument("-e", "--nthreads", dest="nthreads", type=int, default=0)
    t.add_argument("-C", "--no-canon", action="store_false", default=True, dest="canonicalize")
    t.set_defaults(func=tree_command)

    p = subs.add_parser("progressive", parents=[common, sweep],
                        description="the growth of delta along orderings of the genomes"
                                    " -- on a `tree --exact` of up to 255 genomes every union of a k comes from one sort of the leaves' k-mers (beyond that: one count per union)")
    p.add_argument("-d", "--dtree", dest="delta_tree", required=True)
    p.add_argument("-s", "--tag", dest="tag", type=str)
    p.add_argument("-r", "--orderings", dest="ordering_file", type=str, default=None)
    p.add_argument("-f", "--fastas", dest="flist_loc", default=None, type=str)
    p.add_argument("-n", "--norderings", dest="norderings", default=0, type=int)
    p.add_argument("-o", "--outdir", dest="outdir", default=os.getcwd(), type=str)
    p.add_argument("-l", "--label", dest="label", default="")
    p.add_argument("--step", dest="step", default=1, type=int)
    p.set_defaults(func=progressive_command)

    k = subs.add_parser("kij", parents=[common, sweep],
                        description="delta of every pair of genomes, and with --jaccard their Jaccard coefficients"
                                    " -- on a `tree --exact` of up to 255 genomes every union of a k comes from one sort of the leaves' k-mers (beyond that: one count per union)")
    k.add_argument("-d", "--dtree", dest="delta_tree", required=True)
    k.add_argument("-s", "--tag", dest="tag", type=str)
    k.add_argument("-f", "--fastas", dest="flist_loc", default=None, type=str)
    k.add_argument("-o", "--outdir", dest="outdir", default=os.getcwd(), type=str)
    k.add_argument("-l", "--label", dest="label", default="")
    k.add_argument("--afproject", dest="afproject", default=False, action="store_true")
    k.add_argument("--jaccard", dest="jaccard", default=False, action="store_true")
    k.set_defaults(func=kij_command)

    dd = subs.add_parser("deltadelta", parents=[common, sweep],
                         description="delta(all) - delta(all but a genome or group): each one's contribution"
                                     " -- on a `tree --exact` of up to 255 genomes every union of a k comes from one sort of the leaves' k-mers (beyond that: one count per union)")
    dd.add_argument("-d", "--dtree", dest="delta_tree", required=True)
    dd.add_argument("-s", "--tag", dest="tag", type=str)
    dd.add_argument("-f", "--fastas", dest="flist_loc", default=None, type=str,
                    help="leave each listed FASTA out on its own (default: every leaf); the others stay in every union")
    dd.add_argument("-g", "--groups", dest="groups_loc", default=None, type=str,
                    help="'fasta<TAB>group' lines: each group left out as a whole; unlisted leaves stay in every union")
    dd.add_argument("-o", "--outdir", dest="outdir", default=os.getcwd(), type=str)
    dd.add_argument("-l", "--label", dest="label", default="")
    dd.set_defaults(func=deltadelta_command)

    ab = subs.add_parser("abba", parents=[common, sweep],
                         description="exact order effects over all n! orderings of n <= 16 genomes, from all 2^n subset unions")
    ab.add_argument("-d", "--dtree", dest="delta_tree", required=True)
    ab.add_argument("-s", "--tag", dest="tag", type=str)
    ab.add_argument("-f", "--fastas", dest="flist_loc", default=None, type=str,
                    help="the genomes to order (default: every leaf), in the order `progressive -f` takes them")
    ab.add_argument("-A", "--fastaA", dest="fastaA", default=None, type=str, help="report only the pairs (A, B) and (B, A)")
    ab.add_argument("-B", "--fastaB", dest="fastaB", default=None, type=str)
    ab.add_argument("--subsets", dest="subsets", default=False, action="store_true",
                    help="also write every subset's delta (<prefix>.abba_subsets.csv)")
    ab.add_argument("-o", "--outdir", dest="outdir", default=os.getcwd(), type=str)
    ab.add_argument("-l", "--label", dest="label", default="")
    ab.set_defaults(func=abba_command)

    gr = subs.add_parser("greedy", parents=[common, sweep],
                         description="the steepest and the flattest growth ordering: at each step the genome that raises delta the most / the least")
    gr.add_argument("-d", "--dtree", dest="delta_tree", required=True)
    gr.add_argument("-s", "--tag", dest="tag", type=str)
    gr.add_argument("-f", "--fastas", dest="flist_loc", default=None, type=str,
                    help="the genomes to order (default: every leaf), in the order `progressive -f` takes them; ties go to the earlier one")
    gr.add_argument("--mode", dest="mode", choices=["max", "min", "both"], default="both")
    gr.add_argument("-b", "--base", dest="base_loc", default=None, type=str,
                    help="FASTAs that start every ordering, in the file's order, each in the universe")
    gr.add_argument("--steps", dest="steps", default=None, type=int,
                    help="stop after this many genomes in all, the --base ones included (default: all)")
    gr.add_argument("-o", "--outdir", dest="outdir", default=os.getcwd(), type=str)
    gr.add_argument("-l", "--label", dest="label", default="")
    gr.set_defaults(func=greedy_command)

    co = subs.add_parser("core", parents=[common, sweep],
                         description="exact core genome, k-mer frequency spectrum and group markers of up to 64 genomes of a `tree --exact`")
    co.add_argument("-d", "--dtree", dest="delta_tree", required=True)
    co.add_argument("-s", "--tag", dest="tag", type=str)
    co.add_argument("-f", "--fastas", dest="flist_loc", default=None, type=str,
                    help="the genomes of the universe (default: every leaf), in the order `progressive -f` takes them")
    co.add_argument("-r", "--orderings", dest="ordering_file", type=str, default=None)
    co.add_argument("-n", "--norderings", dest="norderings", default=0, type=int,
                    help="with neither -r nor -n: one ordering, the genomes as listed")
    co.add_argument("-g", "--groups", dest="groups_loc", default=None, type=str,
                    help="'fasta<TAB>group' lines: per group its core, its private k-mers and its signature")
    co.add_argument("--kmers", dest="kmers", action="append", choices=["core", "private", "signature"], default=None, metavar="CLASS",
                    help="also write the k-mers of this class (core, private, signature; repeatable) of every group as FASTA, at the k "
                         "the group summary reports for it; without -g: of one group `all`, the whole universe")
    co.add_argument("--kmers-k", dest="kmers_k", action="append", type=int, default=None, metavar="K",
                    help="write the k-mers at this k of the window (repeatable) instead of each class's own")
    co.add_argument("--kmers-max", dest="kmers_max", type=int, default=None, metavar="N",
                    help="most k-mers of one group, class and k (default 1000000): more ends the command before anything is written")
    co.add_argument("--regions", dest="regions", action="append", choices=["core", "private", "signature"], default=None, metavar="CLASS",
                    help="also write where the k-mers of this class (core, private, signature; repeatable) lie in every genome of the "
                         "group, as BED (record, start, end, fasta), at the k the group summary reports for it; without -g: of one "
                         "group `all`, the whole universe")
    co.add_argument("--regions-k", dest="regions_k", action="append", type=int, default=None, metavar="K",
                    help="write the regions at this k of the window (repeatable) instead of each class's own")
    co.add_argument("-o", "--outdir", dest="outdir", default=os.getcwd(), type=str)
    co.add_argument("-l", "--label", dest="label", default="")
    co.set_defaults(func=core_command)

    sc = subs.add_parser("screen", parents=[common],
                         description="exact containment of new samples (assemblies, read sets) in up to 64 genomes of a `tree --exact`")
    sc.add_argument("-d", "--dtree", dest="delta_tree", required=True)
    sc.add_argument("-s", "--tag", dest="tag", type=str)
    sc.add_argument("-f", "--fastas", dest="flist_loc", default=None, type=str,
                    help="the genomes of the universe (default: every leaf), in the order `progressive -f` takes them")
    sc.add_argument("-g", "--groups", dest="groups_loc", default=None, type=str,
                    help="'fasta<TAB>group' lines: per group the share of its core, private and signature k-mers each sample holds")
    sc.add_argument("-q", "--queries", dest="query_loc", default=None, type=str, help="a file of sample paths, one per line")
    sc.add_argument("-k", dest="ks", action="append", type=int, default=None, metavar="K",
                    help="screen at this k (1..64, repeatable; default: the k of the tree's root)")
    sc.add_argument("--paint", dest="paint", type=int, default=None, metavar="W",
                    help="also paint every sample in windows of W bases (a multiple of 64): per window the positions whose k-mer the "
                         "collection holds, the two genomes that share most of them (<prefix>.paint.csv) and the runs of windows with "
                         "the same best genome, novel stretches among them (<prefix>.paint_segments.csv)")
    sc.add_argument("--paint-matrix", dest="paint_matrix", default=False, action="store_true",
                    help="with --paint: also write every genome's shared positions per window (<prefix>.paint_matrix.csv)")
    sc.add_argument("--reads", dest="reads", default=False, action="store_true",
                    help="also call every record of every sample -- a read, a contig -- to the genome that holds most of its k-mer "
                         "positions and write how many records go to each genome, how many are ambiguous (several genomes tie), "
                         "unclassified or without a k-mer (<prefix>.reads_summary.csv)")
    sc.add_argument("--reads-calls", dest="reads_calls", default=False, action="store_true",
                    help="with --reads: also write every record's call, its best and second genome and how many genomes tie "
                         "(<prefix>.reads.csv)")
    sc.add_argument("--reads-min-hits", dest="reads_min_hits", type=int, default=1, metavar="H",
                    help="with --reads: call a record only where its best genome holds at least H of its positions (default 1)")
    sc.add_argument("--depth", dest="depth", default=False, action="store_true",
                    help="also count how many times every sample holds each k-mer of the collection and write, per genome, per "
                         "genome's private k-mers, for the pan-genome, the core and with -g every group's classes, breadth, mean and "
                         "median depth (<prefix>.depth.csv)")
    sc.add_argument("--depth-bins", dest="depth_bins", type=int, default=None, metavar="B",
                    help="with --depth: the bins of the depth histogram, 2..256 (default 64); depths from B-1 on share the last bin, "
                         "a median that lies there is marked clipped")
    sc.add_argument("--depth-hist", dest="depth_hist", default=False, action="store_true",
                    help="with --depth: also write the non-zero bins of every histogram (<prefix>.depth_hist.csv)")
    sc.add_argument("--cover", dest="cover", type=int, default=None, metavar="W",
                    help="also lay every sample along every genome of the collection in windows of W bases of the genome (a multiple "
                         "of 64): per window the positions whose k-mer the sample holds, their depth, and the same for the k-mers no "
                         "other genome holds (<prefix>.cover.csv), the runs of present, absent and empty windows "
                         "(<prefix>.cover_regions.csv) and a row per sample and genome (<prefix>.cover_summary.csv)")
    sc.add_argument("--cover-fastas", dest="cover_fastas", type=str, default=None, metavar="LIST",
                    help="with --cover: a file of genomes of the universe, one per line, to lay the samples along (default: all of it)")
    sc.add_argument("--cover-clip", dest="cover_clip", type=int, default=None, metavar="C",
                    help="with --cover: a position's depth counts as at most C, 1..1023 (default 255), so that one repeat does not "
                         "carry a window's mean")
    sc.add_argument("--cover-min", dest="cover_min", type=int, default=None, metavar="P",
                    help="with --cover: a window is present where the sample holds at least P per cent of its positions, 1..100 "
                         "(default 50)")
    sc.add_argument("--gather", dest="gather", default=False, action="store_true",
                    help="also explain every sample by the genomes of the collection one by one: the genome that holds most of its "
                         "k-mers, then the one that holds most of what is left, ... with the k-mers each pick adds and their depth "
                         "(<prefix>.gather.csv) and a row per sample (<prefix>.gather_summary.csv)")
    sc.add_argument("--gather-min", dest="gather_min", type=int, default=None, metavar="H",
                    help="with --gather: stop at a pick that adds fewer than H k-mers of the sample (default 1)")
    sc.add_argument("--gather-steps", dest="gather_steps", type=int, default=None, metavar="N",
                    help="with --gather: N picks at the most, 1..the genomes of the universe (default: all of them)")
    sc.add_argument("samples", nargs="*", metavar="SAMPLE", help="FASTA / FASTQ files, plain or gzip, that are no leaves of the tree")
    sc.add_argument("-o", "--outdir", dest="outdir", default=os.getcwd(), type=str)
    sc.add_argument("-l", "--label", dest="label", default="")
    sc.set_defaults(func=screen_command)

    nb = subs.add_parser("neighbors", parents=[common, sweep],
                         description="new samples (assemblies, read sets) against a tree of sketches: the closest genomes of the collection "
                                     "by the K-independent Jaccard, and what each sample would add to the collection's delta")
    nb.add_argument("-d", "--dtree", dest="delta_tree", required=True)
    nb.add_argument("-s", "--tag", dest="tag", type=str)
    nb.add_argument("-f", "--fastas", dest="flist_loc", default=None, type=str,
                    help="the genomes of the universe (default: every leaf), in the order `progressive -f` takes them")
    nb.add_argument("-q", "--queries", dest="query_loc", default=None, type=str, help="a file of sample paths, one per line")
    nb.add_argument("--top", dest="top", type=int, default=None, metavar="N", help="write each sample's N closest genomes (default: all)")
    nb.add_argument("--jaccard", dest="jaccard", default=False, action="store_true",
                    help="also write the cardinalities and the Jaccard of every sample and genome at every k (<prefix>.neighbors_j.csv)")
    nb.add_argument("samples", nargs="*", metavar="SAMPLE", help="FASTA / FASTQ files, plain or gzip; a leaf of the tree is allowed")
    nb.add_argument("-o", "--outdir", dest="outdir", default=os.getcwd(), type=str)
    nb.add_argument("-l", "--label", dest="label", default="")
    nb.set_defaults(func=neighbors_command)

    pa = subs.add_parser("patterns", parents=[common],
                         description="which sets of up to 64 genomes of a `tree --exact` share k-mers, and how many: the distinct membership "
                                     "patterns with their k-mer counts")
    pa.add_argument("-d", "--dtree", dest="delta_tree", required=True)
    pa.add_argument("-s", "--tag", dest="tag", type=str)
    pa.add_argument("-f", "--fastas", dest="flist_loc", default=None, type=str,
                    help="the genomes of the universe (default: every leaf), in the order `progressive -f` takes them")
    pa.add_argument("-k", dest="ks", action="append", type=int, default=None, metavar="K",
                    help="the patterns at this k (1..64, repeatable; default: the k of the tree's root)")
    pa.add_argument("--top", dest="top", type=int, default=1000, metavar="N", help="write the N largest patterns (default 1000; 0: all)")
    pa.add_argument("--max-patterns", dest="max_patterns", type=int, default=1_000_000, metavar="N",
                    help="most patterns of one k a whole table may have (--top 0, --splits; default 1000000): more ends the command "
                         "before anything is written")
    pa.add_argument("--splits", dest="splits", default=False, action="store_true",
                    help="also write every bipartition {mask, rest} with 2 <= genomes <= n - 2 on a side and its support "
                         "(<prefix>.splits.csv)")
    pa.add_argument("-o", "--outdir", dest="outdir", default=os.getcwd(), type=str)
    pa.add_argument("-l", "--label", dest="label", default="")
    pa.set_defaults(func=patterns_command)

    # (not in the reference: its every command is a fresh process that shells out to fresh `dashing` processes)
    sv = subs.add_parser("serve", description="keep the GPU context alive and run the commands dandd_amd.host.client forwards")
    sv.add_argument("--socket", required=True, help="path of the unix socket to listen on (clients: DANDD_SERVER=<path>)")
    sv.add_argument("--idle-exit", type=float, default=0.0, help="leave after this many seconds without a command (0: never)")
    sv.add_argument("--warm", action="append", default=[], metavar="REGISTERS[,nc]", help="create this backend before listening, e.g. --warm 20")
    sv.set_defaults(func=serve_command)
    return parser


def main(argv=None):
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    dist = None
    if world > 1:
        # one process per GPU (torch.distributed.run): every sub-command shards the leaf sketches it needs
        # over the ranks and hands them over through the shared sketch directory; the process group is only
        # a barrier
        import torch.distributed as dist
        if not dist.is_initialized():
            dist.init_process_group("gloo", rank=rank, world_size=world)
        deltatree.set_dist_active(True)
    elif "torch" not in sys.modules:  # stand-alone process: no torch anywhere on this path (engine.load_library)
        os.environ.setdefault("DANDD_NO_TORCH", "1")
    try:
        args = build_parser().parse_args(sys.argv[1:] if argv is None else argv)
        args.func(args)
        if dist is not None:
            dist.barrier()
    except BaseException as e:
        if dist is not None and not (isinstance(e, SystemExit) and not e.code):
            # a rank that fails must not leave its peers waiting in a barrier it will never reach: leave at once with
            # a non-zero status and let the launcher (torch.distributed.run) end the others
            import traceback
            traceback.print_exc()
            sys.stderr.flush()
            sys.stdout.flush()
            os._exit(1)
        raise
    finally:
        deltatree.set_dist_active(False)
        if dist is not None:
            dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""DandD's experiment layer (delta trees, progressive unions, K-independent Jaccard) on top of the
MI355X sketching engine.

Behavioural mirror of /root/reference/lib/huffman_dandd.py and the SketchObj lifecycle of
/root/reference/lib/sketch_classes.py:124-373 -- same class and attribute names (the CLI pickles
these objects), same argmax-k hill-climb (ties move on, `kstart` is mutated as the climb proceeds,
lib/huffman_dandd.py:106-146), same tree shapes, same CSV rows -- with every `subprocess` call
replaced by a backend object (dandd_amd.host.backend.HipBackend: the GPU).  The goldens in
tests/golden/ref_*.json were produced by running the reference itself; tests/test_host_golden.py
replays them against this module.

Differences that are deliberate:
  * a leaf k-batch is ONE fused GPU pass over the FASTA instead of `parallel` over k;
  * `Sketch.cmd` holds a descriptive string instead of a shell line;
  * k < 1 is never sketched (the reference would create a k=-1 placeholder when a climb reaches k=0).
"""
import csv
import os
import weakref
import pickle
import sys
from collections import namedtuple
from functools import cached_property
from itertools import permutations
from math import factorial
from random import sample, shuffle

import numpy as np

from .store import Catalog, SketchPath, ensure_dir, forget_sketch, sketch_exists

# ---------------------------------------------------------------------------------------------
# backend plumbing: objects of this module are pickled, the GPU context is not
# ---------------------------------------------------------------------------------------------
_backend_factory = None
_backends = {}
RESIDENT = False    # `dandd serve` sets it: backends outlive commands, so what a command leaves on the device is worth keeping
_SWEPT = weakref.WeakKeyDictionary()   # DeltaTreeNode -> the ks its subtree has been brought up to date for, in this command


def new_command():
    """Forget what an earlier command of this process learned about the sketch directory (dandd serve calls it per command)."""
    _SWEPT.clear()
    from . import store
    store.new_command()
    for be in _backends.values():          # (registers of sketch files kept in memory: trusted only while size and mtime stand, but a
        forget = getattr(be, "new_command", None)   # command boundary is a good place to stop trusting altogether)
        if forget:
            forget()
_leaf_batch = None  # set while a tree solves its leaves: sketches missing ks for all of them at once


def set_backend_factory(factory):
    """factory(registers:int, canonicalize:bool) -> backend.  None restores the GPU default."""
    global _backend_factory
    _backend_factory = factory
    _backends.clear()


def _backend_key(experiment):
    exact = experiment.get("tool") == "kmc"
    return (int(experiment["registers"]), bool(experiment["canonicalize"]), exact)


def _make_backend(key):
    # both fail loudly without libdandd_hip.so / a gfx950 GPU; under torch.distributed.run every rank drives its own GPU
    from .backend import HipBackend, HipExactBackend
    cls = HipExactBackend if key[2] else HipBackend
    return cls(log2m=key[0], canonical=key[1], device=int(os.environ.get("LOCAL_RANK", "0")))


_prewarm = {}   # key -> (thread, result box)


def prewarm_backend(experiment, first_launches=True):
    """Start creating the GPU backend of `experiment` on a thread of its own: loading libdandd_hip.so, HIP's first
    use of the device and the first launch of every kernel module cost 0.25-0.35 s in a fresh process, during which a
    one-shot `dandd` command has blake2b digests, directory walks and imports of its own to do (ctypes calls release
    the GIL).  backend_for() picks the result up -- or the exception, which it re-raises.  (Measured on `tree` over
    10 x 50 Mbp, four alternating runs: 0.68 s with / 0.66 s without at log2m 14, 0.82 / 0.85 at log2m 20 -- within the
    box's noise; in `progressive` and `kij`, whose host-side set-up is short, it cost 0.05-0.1 s and is not used.)"""
    import threading
    key = _backend_key(experiment)
    if _backend_factory is not None or key in _backends or key in _prewarm or os.environ.get("DANDD_NO_PREWARM") == "1":
        return
    box = []

    def work():
        try:
            be = _make_backend(key)
            if first_launches and hasattr(be.engine, "warmup"):   # (the sketching kernels: a command that will sketch)
                be.engine.warmup()
            box.append(be)
        except BaseException as e:  # handed to the thread that asks for the backend
            box.append(e)

    t = threading.Thread(target=work, name="dandd-backend-prewarm")
    _prewarm[key] = (t, box)
    t.start()


def backend_for(experiment):
    key = _backend_key(experiment)
    if key in _prewarm:
        t, box = _prewarm.pop(key)
        t.join()
        if isinstance(box[0], BaseException):
            raise box[0]
        _backends[key] = box[0]
    if key not in _backends:
        _backends[key] = _backend_factory(key[0], key[1]) if _backend_factory is not None else _make_backend(key)
    if RESIDENT and hasattr(_backends[key], "resident"):
        _backends[key].resident = True
    return _backends[key]


# ---- one process per GPU (python -m torch.distributed.run ... -m dandd_amd.host.cli <subcommand> ...) ---
# Leaf sketching -- the only heavy step -- is sharded over the ranks by file size; the sketches travel
# the way they always do in DandD, as files in the shared sketch directory; after a barrier rank 0
# carries on alone with every leaf sketch cached and the other ranks are done.  The sharding is switched
# on by the CLI (set_dist_active) for the commands in which EVERY rank takes part, never by the mere
# presence of WORLD_SIZE in the environment: a barrier needs all its parties.
class WorkerDone(Exception):
    """Raised on ranks > 0 once their share of the leaf sketches is on disk."""


_dist_active = False


def set_dist_active(on):
    global _dist_active
    _dist_active = bool(on)


def dist_ranks():
    if not _dist_active:
        return 0, 1
    return int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))


def dist_barrier():
    """The ONE meeting point of a multi-rank command: every rank's share of the leaf sketches is on disk.  Behind
    it rank 0 finishes alone, so the sharding is switched off here: from now on `_batch_leaf_sketch` batches ALL
    leaves again and the hill-climb's batch hook is back (a rank 0 that kept seeing world > 1 would batch only its
    own shard and sketch the other leaves one genome at a time)."""
    if not _dist_active:
        return
    try:
        import torch.distributed as dist
    except ImportError:
        return
    if dist.is_available() and dist.is_initialized():
        dist.barrier()
    set_dist_active(False)


class RowTable:
    """Rows of ONE shape held as columns: what a list of dicts holds, for tables of tens of thousands of rows that are made
    column-wise anyway (`kij --jaccard` over 64 genomes: 62 496 rows of 9 cells).  Iterating or indexing gives the dicts;
    write_listdict_to_csv writes the columns without ever making them."""

    def __init__(self, names):
        self.cols = {n: [] for n in names}

    def __len__(self):
        return len(next(iter(self.cols.values()))) if self.cols else 0

    def __iter__(self):
        names = list(self.cols)
        for values in zip(*self.cols.values()):
            yield dict(zip(names, values))

    def __getitem__(self, i):
        if isinstance(i, slice):
            return list(self)[i]
        return {n: c[i] for n, c in self.cols.items()}


def write_listdict_to_csv(outfile, listdict, suffix="", last_col=None):
    """Rows as CSV, union of keys as header, `fastas`/`files` last (they may contain commas)."""
    names = sorted(listdict.cols) if isinstance(listdict, RowTable) else sorted({k for row in listdict for k in row})
    for special in ("fastas", "files"):
        if special in names:
            last_col = special
    if last_col in names:
        names.remove(last_col)
        names.append(last_col)
    out = sys.stdout if outfile in (None, "-") else open(outfile + suffix, "w", newline="")
    try:
        if isinstance(listdict, RowTable):
            # The csv module's "excel" dialect written by hand, a COLUMN at a time: a cell is str(value); it is quoted (quotes
            # doubled) iff it holds a comma, a quote or a line break; rows end in \r\n.  A column of few distinct values -- the
            # two paths and titles of a pair stand in each of its rows, a leaf's cardinality at k in every pair's row -- is
            # formatted once per value.  62 496 rows of 9 cells: 0.12 s through csv.writer, 0.03 s this way; same bytes
            # (tests/test_store.py::test_rowtable_csv_is_the_csv_modules).
            import re
            needs_quote = re.compile('[,"\r\n]').search

            def cell(v):
                t = v if isinstance(v, str) else ("" if v is None else str(v))
                return '"' + t.replace('"', '""') + '"' if needs_quote(t) else t
            text_cols = []
            for n in names:
                col = listdict.cols[n]
                kinds = set(map(type, col))
                # (by OBJECT, not by value: 0.0 == -0.0 == 0 and nan != nan; the repeats are the same objects)
                repeats = len(col) > 256 and 4 * len(set(map(id, col[:256]))) < 256    # (judged on the first 256 cells)
                if repeats:
                    memo = {i: cell(v) for i, v in {id(v): v for v in col}.items()}
                    text_cols.append(list(map(memo.__getitem__, map(id, col))))
                elif kinds <= {float, int}:
                    text_cols.append(list(map(str, col)))       # (numbers never need quoting)
                else:
                    text_cols.append([cell(v) for v in col])
            out.write(",".join(cell(n) for n in names) + "\r\n")
            if text_cols and text_cols[0]:
                out.write("\r\n".join(map(",".join, zip(*text_cols))) + "\r\n")
        elif len(names) > 1 and all(len(row) == len(names) for row in listdict):
            # every row has every column: the same bytes as DictWriter's, from C all the way (a `kij --jaccard` over 64
            # genomes writes 62 496 rows of 10 cells)
            from operator import itemgetter
            w = csv.writer(out)
            w.writerow(names)
            w.writerows(map(itemgetter(*names), listdict))
        else:
            w = csv.DictWriter(out, fieldnames=names)
            w.writeheader()
            w.writerows(listdict)
    finally:
        if out is not sys.stdout:
            out.close()


def permute(length, norder, preexist=frozenset(), exhaust=False, verbose=False):
    """`norder` distinct orderings of range(length), extending `preexist`
    (lib/huffman_dandd.py:36-60: shuffled full enumeration below 7!+1, rejection sampling above)."""
    total = factorial(length)
    result = set(preexist)
    norder = min(norder, total)
    if total < 5041 or norder == total or exhaust:
        pool = list(permutations(range(length)))
        shuffle(pool)
    else:
        pool = []
        while len(pool) < norder:
            pool.extend(tuple(sample(range(length), length)) for _ in range(norder))
            pool = list(set(pool))
    for cand in pool:
        if len(result) >= norder:
            break
        result.add(cand)
    return result


# ---------------------------------------------------------------------------------------------
class Sketch:
    """One (set of FASTAs, k) sketch: file on disk + cached cardinality (the reference's SketchObj)."""

    def __init__(self, kval, sfp, speciesinfo, experiment, presketches=()):
        self.kval = kval
        self.sfp = sfp
        self.sketch = None
        self.cmd = None
        self.card = 0
        self.delta_pos = 0
        self.speciesinfo = speciesinfo
        self.experiment = experiment
        self._presketches = list(presketches)
        experiment["baseset"].add(sfp.base)
        if kval > 0:
            self.create_sketch()
            self.card = self.check_cardinality()
            self.delta_pos = self.card / kval

    def __lt__(self, other):
        return self.delta_pos < other.delta_pos

    def __gt__(self, other):
        return self.delta_pos > other.delta_pos

    def __repr__(self):
        return f"['sketch loc: {self.sketch}', k: {self.kval}, pos delta: {self.delta_pos}, cardinality: {self.card}, command: {self.cmd}  ]"

    def sketch_check(self, path=None):
        return sketch_exists(path or self.sfp.full)

    def _build(self):
        be = backend_for(self.experiment)
        if self.sfp.ngen == 1:
            be.leaf(self.sfp.ffiles[0], [self.kval], [self.sfp.full])
        else:
            be.union(self._presketches, self.sfp.full)

    def create_sketch(self, just_do_it=False):
        if self.sfp.ngen < 1:
            raise RuntimeError("For some reason you are trying to sketch an empty list of files. Don't do that.")
        be = backend_for(self.experiment)
        op = "sketch" if self.sfp.ngen == 1 else "union"
        self.cmd = be.describe(op, k=self.kval, out=os.path.basename(self.sfp.full)) if hasattr(be, "describe") else op
        # a union whose cardinality was already computed by a batched GPU schedule
        # (prefetch_union_cards) is not materialised as a file, exactly like --lowmem; the
        # cardinality cache is asked before the file system
        trusted = self.experiment["lowmem"] or (self.sfp.ngen > 1 and self.experiment.get("prefetched"))
        if just_do_it:
            self._build()
        elif trusted and self.check_cardinality() > 0:
            pass
        elif not self.sketch_check():
            self._build()
        self.sketch = self.sfp.full
        return self.sketch

    def individual_card(self):
        if self.kval == 0:
            return
        be = backend_for(self.experiment)
        try:
            value = be.card(self.sfp.full)
        except Exception:
            print(f"Recreating sketch {self.sfp.full}")
            self.create_sketch(just_do_it=True)
            value = be.card(self.sfp.full)
        self.speciesinfo.cardkey[self.sfp.full] = float(value)

    def check_cardinality(self):
        key, cards = self.sfp.full, self.speciesinfo.cardkey
        if key not in cards and self.experiment["lowmem"]:
            return 0
        if key not in cards or cards[key] is None or float(cards[key]) == 0:
            if not self.sketch_check():
                return 0
            self.individual_card()
        self.card = float(cards[key])
        self.delta_pos = self.card / int(self.kval)
        return float(self.card)

    def remove_sketch(self):
        import glob
        pattern = self.sfp.full.replace("{}", "*") if self.kval == 0 else self.sfp.full
        for f in glob.glob(pattern):
            try:
                os.remove(f)
            except FileNotFoundError:
                pass
            forget_sketch(f)


class DashSketchObj(Sketch):
    """HyperLogLog sketch (the reference's class of this name, lib/sketch_classes.py:302)."""


class KMCSketchObj(Sketch):
    """Exact k-mer database (`--exact`; the reference's class of this name, lib/sketch_classes.py:377)."""


def sketch_class(experiment):
    return KMCSketchObj if experiment.get("tool") == "kmc" else DashSketchObj


# ---------------------------------------------------------------------------------------------
class _Climber:
    """The argmax-k local search of a union (lib/huffman_dandd.py:106-146) and its per-k summary rows, shared by DeltaTreeNode
    (sketch objects) and _FlatUnion (a row of a union table).  A subclass gives _climb_step(k) -- bring k-1..k+1 up to date,
    -> card / k at k -- and _summary_cells(k) -> (card, delta_pos, command)."""

    def find_delta_helper(self, kval, direction=1):
        while True:
            if self.experiment["tool"] == "dashing" and kval > 32 and not self.experiment.get("allow_k64"):
                raise ValueError("Exploratory k value is too high for dashing. Either something is amiss "
                                 "with your data or you need to be using --exact mode")
            if kval < 1:
                return
            candidate = self._climb_step(kval)
            if direction < 0:
                self.mink = kval
            else:
                self.maxk = kval
            if not self.delta <= candidate:  # ties keep climbing
                return
            self.speciesinfo.kstart = kval
            self.bestk = kval
            self.delta = candidate
            kval += direction

    def find_delta(self, kval):
        self.find_delta_helper(kval, 1)
        self.find_delta_helper(kval, -1)

    def summarize(self, mink=0, maxk=0, ordering_number=0):
        rows = []
        for k in range(mink, maxk + 1):
            card, delta_pos, command = self._summary_cells(k)
            rows.append({"ngen": self.ngen, "kval": k, "card": card, "delta_pos": delta_pos,
                         "title": self.node_title, "command": command, "ordering": ordering_number})
        return rows


class DeltaTreeNode(_Climber):
    def __init__(self, node_title, children, speciesinfo, experiment, progeny=None):
        self.experiment = experiment
        self.speciesinfo = speciesinfo
        self.children = children
        self.mink = self.maxk = 0
        if experiment["ksweep"] is not None:
            self.mink, self.maxk = experiment["ksweep"]
        self.bestk = 0
        self.delta = 0
        self.ksketches = [None] * max(100, self.maxk + 2)
        if progeny:
            self.node_title = node_title
            self.progeny = list(progeny)
        else:  # a leaf is its own progeny; its title is the file name without the last extension
            self.progeny = [self]
            self.fastas = [node_title]
            self.node_title = os.path.splitext(os.path.basename(node_title))[0]
        self.fastas = [leaf.fastas[0] for leaf in self.progeny]
        self.ngen = len(self.progeny)

    def __repr__(self):
        return f"{self.__class__.__name__}['{self.node_title}', k: {self.bestk}, delta: {self.delta}, ngen: {self.ngen}, children: {self.children!r} ]"

    def __lt__(self, other):
        return self.ngen < other.ngen

    def _grow(self, k):
        if k >= len(self.ksketches):
            self.ksketches.extend([None] * (k - len(self.ksketches) + 2))

    def _template(self):
        """k-placeholder SketchPath of this node's file set (the set never changes)."""
        t = self.__dict__.get("_tmpl")
        if t is None:
            t = self._tmpl = SketchPath(self.fastas, 0, self.speciesinfo, self.experiment)
        return t

    # ---- sketch files for a k range (the reference's `parallel` batch, lib/huffman_dandd.py:148-239)
    def ksweep_update_node(self, mink, maxk):
        mink, maxk = int(mink), int(maxk)
        self._grow(maxk)
        template = self._template()
        if self.ksketches[0] is None:
            self.ksketches[0] = sketch_class(self.experiment)(0, template, self.speciesinfo, self.experiment)
        # ks this node (and therefore its whole subtree) was already brought up to date for, in this
        # process: leaves are shared by hundreds of spiders and would otherwise be re-checked every time
        # (kept BESIDE the node, not in it: a memo inside the object went into the tree pickle -- with this process's pid in
        # it, so no two runs wrote the same bytes -- and a resident `dandd serve`, whose pid never changes, would have believed a
        # pickle's memo about sketch files of another day; new_command() forgets everything between commands)
        swept = _SWEPT.get(self)
        if swept is None:
            swept = _SWEPT[self] = set()
        ks = [k for k in range(max(1, mink), maxk + 1) if k not in swept]
        if not ks:
            return
        for k in ks:
            ensure_dir(template.dir.replace("{}", str(k)))
            self.experiment["baseset"].add(template.base.replace("{}", str(k)))
        for child in (self.children if self.ngen > 1 else []):
            child.ksweep_update_node(mink, maxk)
        cards = self.speciesinfo.cardkey
        todo = []
        for k in ks:
            path = template.with_k(k)
            # (dictionary first: a prefetched union has a cardinality and no file, and asking the
            # file system about every such path dominated `progressive`)
            if (self.experiment["lowmem"] or self.experiment.get("prefetched")) and self.ngen > 1 \
                    and float(cards.get(path) or 0) > 0:
                continue
            if sketch_exists(path):
                continue
            todo.append(k)
        if todo and self.ngen == 1 and _leaf_batch is not None:
            _leaf_batch(todo)  # the same ks (and a margin) for every leaf of the tree in one batch
            todo = [k for k in todo if not sketch_exists(template.with_k(k))]
        if todo:
            be = backend_for(self.experiment)
            if self.ngen == 1:
                be.leaf(self.fastas[0], todo, [template.with_k(k) for k in todo])  # one fused GPU pass
            else:
                for k in todo:
                    ins = [c.ksketches[0].sfp.with_k(k) for c in self.children]
                    be.union(ins, template.with_k(k))
        swept.update(ks)

    def update_node(self, kval):
        """Sketch object (file + cardinality) for k at this node and, first, at every descendant."""
        window = self.experiment["ksweep"]
        if window is not None and not (window[0] <= kval <= window[1]):
            print(f"k={kval} is outside of ksweep range ", window)
            return
        self._grow(kval)
        if self.ksketches[kval]:
            return
        sfp = self._template().at_k(kval, self.speciesinfo, self.experiment)
        inputs = []
        if self.ngen > 1:
            for child in self.children:
                child.update_node(kval)
                inputs.append(child.ksketches[kval].sketch)
        self.ksketches[kval] = sketch_class(self.experiment)(kval, sfp, self.speciesinfo, self.experiment, presketches=inputs)

    def node_ksweep(self, mink, maxk):
        self.ksweep_update_node(mink, maxk)
        for k in range(max(1, mink), maxk + 1):
            if self.ksketches[k] is None:
                self.update_node(k)
        self.mink, self.maxk = mink, maxk

    # ---- argmax-k local search (_Climber) ----------------------------------------------------------
    def _climb_step(self, kval):
        self._grow(kval + 1)
        self.node_ksweep(mink=kval - 1, maxk=kval + 1)
        self.update_node(kval)
        return self.ksketches[kval].delta_pos

    def find_delta(self, kval):
        super().find_delta(kval)
        self.card = self.ksketches[self.bestk].card

    def _summary_cells(self, k):
        s = self.ksketches[k]
        return s.card, s.delta_pos, s.cmd


# ---------------------------------------------------------------------------------------------
# Cardinalities of a whole union schedule from one GPU launch, k in [lo, hi] along the last axis: table[i, j] for the pair of
# leaves i, j (`kij`), table[o, j] for the first j+1 leaves of ordering o (`progressive`), table[g] for every leaf outside group g
# (`deltadelta`).  index: id(leaf) -> its number in the table; orders: ordering as a tuple of leaf numbers -> o.
UnionTable = namedtuple("UnionTable", "table lo hi index orders", defaults=(None, None))


def _cache_row(cards, tmpl, row, lo):
    """A table row stored in the cardinality cache under the names the union's sketch files of each k would have."""
    for kk, card in enumerate(row):
        cards[tmpl.with_k(lo + kk)] = float(card)


class _FlatUnion(_Climber):
    """The body node of a SubSpider as NUMBERS.  When a whole union schedule has come back from the GPU as one table of
    cardinalities (UnionTable: every pair x k of `kij`, every prefix x k of `progressive`, every complement x k of `deltadelta`),
    a SubSpider per pair or prefix -- a DeltaTreeNode, a Sketch object and a SketchPath per (set, k), 76 608 of them for 64
    genomes -- computes nothing: it walks dictionaries.  This class goes through the same steps on one row of the table --
    _Climber's find_delta with its `<=` ties and the kstart it moves, node_ksweep's k-1..k+1 window (lib/huffman_dandd.py:117),
    fill_tree's update_node of every bestk (:451-457), summarize (:289-301) -- and leaves the same traces a tree save reads: the
    base names in the experiment's base set, their sketchinfo entries, the row's cardinalities in the cache under the union's
    sketch names.  A one-leaf union uses the leaf's own files, not the row.  A k outside the table goes through the file-based
    backend (leaf sketches, union, card) as the object path does."""

    def __init__(self, tree, kids, experiment, table, row):
        sp = tree.speciesinfo
        self.speciesinfo, self.experiment, self.kids = sp, experiment, list(kids)
        self.lo, self.hi = int(table.lo), int(table.hi)
        self.fastas = [leaf.fastas[0] for c in self.kids for leaf in c.progeny]
        self.ngen = len(self.fastas)
        self.node_title = "_".join(os.path.basename(c.node_title) for c in self.kids)
        self.tmpl = SketchPath(self.fastas, 0, sp, experiment)   # (the '{}' form: registers its base as the node's placeholder sketch does)
        experiment["baseset"].add(self.tmpl.base)
        self.delta, self.bestk, self.mink, self.maxk = 0, 0, 0, 0
        self._touched = set()
        self._be = backend_for(experiment)
        self._base = self.tmpl.base.split("{}")       # the base name around its k
        self.row = row if self.ngen > 1 else None
        if self.row is not None:
            _cache_row(sp.cardkey, self.tmpl, row, self.lo)

    def touch(self, k):
        """what update_node(k) leaves behind besides the Sketch object: the base name in the experiment's base set and its
        sketchinfo entry (a tree save lists them: <prefix>_sketchdb.txt).  NOT the ngen<N>/k<K> directory the reference makes
        for every k it looks at (lib/huffman_dandd.py:171-174): no file of this union is written unless card() has to build
        one, which makes the directory then -- 2 046 empty directories were 0.1 s of a 64-genome `progressive`."""
        if k in self._touched:
            return
        self._touched.add(k)
        base = str(k).join(self._base)
        self.experiment["baseset"].add(base)
        if base not in self.speciesinfo.sketchinfo:
            self.speciesinfo.sketchinfo[base] = {"sketchbase": base, "files": self.tmpl.files, "ngen": self.ngen, "kval": k,
                                        "registers": self.experiment["registers"]}

    def card(self, k):
        if self.row is not None and self.lo <= k <= self.hi:
            return float(self.row[k - self.lo])
        path = self.tmpl.with_k(k)
        cards = self.speciesinfo.cardkey
        if float(cards.get(path) or 0) > 0:
            return float(cards[path])
        # outside the table: the files, as DeltaTreeNode.ksweep_update_node + Sketch would (a hill-climb that leaves the window)
        for c in self.kids:
            c.ksweep_update_node(k, k)
        if self.ngen > 1 and not sketch_exists(path):
            ensure_dir(self.tmpl.dir.replace("{}", str(k)))
            self._be.union([c.ksketches[0].sfp.with_k(k) for c in self.kids], path)
        cards[path] = float(self._be.card(path))
        return cards[path]

    def node_ksweep(self, mink, maxk):
        lo = max(1, mink)
        if maxk - lo >= 4:
            # a whole window at once (every pair of `kij --jaccard`, every prefix of a k-sweep `progressive`): the same traces as
            # touch(k) for each k, without a call per k
            pre, post = self._base
            seen = self._touched
            ks = [k for k in range(lo, maxk + 1) if k not in seen]
            bases = [pre + str(k) + post for k in ks]
            self._touched.update(ks)
            self.experiment["baseset"].update(bases)
            info, files, ngen, regs = self.speciesinfo.sketchinfo, self.tmpl.files, self.ngen, self.experiment["registers"]
            for k, base in zip(ks, bases):
                if base not in info:
                    info[base] = {"sketchbase": base, "files": files, "ngen": ngen, "kval": k, "registers": regs}
        else:
            for k in range(lo, maxk + 1):
                self.touch(k)
        self.mink, self.maxk = mink, maxk

    def _climb_step(self, kval):
        self.node_ksweep(kval - 1, kval + 1)
        return self.card(kval) / kval

    def fill(self):
        """SubSpider.fill_tree in a hill-climb run: the root brought up to date at every node's argmax-k"""
        for k in sorted({c.bestk for c in self.kids} | {self.bestk}):
            if k > 0:
                self.touch(k)

    def _summary_cells(self, k):
        if k == 0:   # the placeholder sketch (a hill-climb run's summary is made of these: SURVEY.md section 9)
            return 0, 0, None
        c = self.card(k)
        op = "sketch" if self.ngen == 1 else "union"
        command = self._be.describe(op, k=k, out=os.path.basename(self.tmpl.with_k(k))) if hasattr(self._be, "describe") else op
        return c, c / k, command


# ---------------------------------------------------------------------------------------------
DEFAULT_EXPERIMENT = {"tool": "dashing", "registers": 20, "canonicalize": True, "debug": False, "nthreads": 0,
                      "baseset": set(), "safety": False, "fast": False, "verbose": False, "ksweep": None,
                      "lowmem": False}


def _batched(experiment):
    """May an analysis take a backend's whole table in one call?  Not under --safe, not under DD_NO_PREFETCH."""
    return not experiment.get("safety") and not os.environ.get("DD_NO_PREFETCH")


def _cards_or_wide(be, method, *args):
    """A backend's union table (`method`: pairwise_cards / progressive_cards / leave_out_cards) and, where that is None --
    more leaves than its membership mask has bits -- the table of its wide_ method of the same name, for a backend that has
    one (exact trees of up to 255 leaves: still one sort per k).  None: the caller takes the object path."""
    table = getattr(be, method)(*args)
    if table is None and hasattr(be, "wide_" + method):
        table = getattr(be, "wide_" + method)(*args)
    return table


# The k-mer classes of a group of genomes: membership queries (all of, none of) over the masks of a universe, from the
# group's mask G and the universe's mask `full`.  Their order is the order of every table and CSV column that holds them.
KMER_QUERIES = {"core": lambda G, full: (G, 0), "private": lambda G, full: (0, full ^ G), "signature": lambda G, full: (G, full ^ G)}


def group_queries(gmasks, full):
    """-> (alls, nones): the KMER_QUERIES of every group mask, group after group, as a backend's select entry points take them"""
    pairs = [query(G, full) for G in gmasks for query in KMER_QUERIES.values()]
    return [a for a, _ in pairs], [b for _, b in pairs]


class _Universe:
    """The leaf FASTAs one analysis call works over (bit i of a membership mask is fastas[i]) and its k window
    [max(1, lo), hi]: the experiment and backend of that window, the leaves' files (made on first use: the object paths
    never ask), the backend's two ways to fail, and the object path for one union.  A local of the call -- trees are
    pickled, so it is never stored on one, nor on a node or an experiment."""

    def __init__(self, tree, fastas, lo, hi):
        by_fasta = {leaf.fastas[0]: leaf for leaf in tree.leaf_nodes()}
        self.tree, self.fastas = tree, fastas
        self.nodes = [by_fasta[f] for f in fastas]
        self.n = len(self.nodes)
        self.index = {f: i for i, f in enumerate(fastas)}
        self.full = (1 << self.n) - 1
        self.lo, self.hi = max(1, int(lo)), int(hi)
        if self.hi < self.lo:
            raise ValueError(f"empty k window {self.lo}..{self.hi}")
        self.ks = list(range(self.lo, self.hi + 1))
        self.exp = dict(tree.experiment, ksweep=(self.lo, self.hi))
        self.batched = _batched(self.exp)

    @cached_property
    def be(self):
        return backend_for(self.exp)

    @cached_property
    def paths(self):
        return self.tree._leaf_files(self.nodes, self.lo, self.hi)

    def masks(self, groups):
        """groups (lists of FASTAs of the universe) -> their membership masks"""
        return [sum(1 << self.index[f] for f in set(g)) for g in groups]

    def need(self, *entries, why):
        for entry in entries:
            if not hasattr(self.be, entry):
                raise ValueError(f"the backend {getattr(self.be, 'name', type(self.be).__name__)} has no {entry}: {why} exact membership masks")

    def table(self, got, shape=None):
        """what a mask entry point gave -- None: no table for these leaves -- as unsigned integers of `shape` (None: as it is)"""
        if got is None:
            raise ValueError(f"the backend has no membership masks for {self.n} genomes")
        return got if shape is None else np.asarray(got).astype(np.uint64).reshape(shape)

    def union_cards(self, node_indices):
        """The object path for one union: a SubSpider over these genomes of the universe, swept over the window -> cards [K]"""
        sub = SubSpider([self.nodes[i] for i in node_indices], self.tree.speciesinfo, self.exp)
        sub.root.node_ksweep(self.lo, self.hi)
        return [sub.root.ksketches[k].card for k in self.ks]


class DeltaTree:
    def __init__(self, fasta_files, speciesinfo, nchildren=2, leafnodes=(), experiment=None, padding=True):
        self.experiment = experiment if experiment is not None else dict(DEFAULT_EXPERIMENT, baseset=set())
        self.mink = self.maxk = 0
        if self.experiment["ksweep"] is not None:
            self.mink, self.maxk = self.experiment["ksweep"]
        self.kstart = speciesinfo.kstart
        self.speciesinfo = speciesinfo
        if self.experiment["verbose"]:
            print("Now making tree for fastas: " + ", ".join(fasta_files))
        self._build_tree(fasta_files, nchildren)
        self.fill_tree(padding=padding)
        self.ngen = len(fasta_files)
        self.root = self._dt[-1]
        self.delta = self.root_delta()
        self.fastas = fasta_files
        if self.experiment["ksweep"] is None:
            speciesinfo.kstart = self.root_k()
        speciesinfo.save_references(fast=self.experiment["fast"])
        speciesinfo.save_cardkey(tool=self.experiment["tool"])

    def __sub__(self, other):
        print("Larger Tree Delta: ", self.delta)
        print("Subtree Delta: ", other.delta)
        print("Subtraction Result: ", self.delta - other.delta)
        return self.delta - other.delta

    def __repr__(self):
        return f"{self.__class__.__name__}(FASTAS: {self.fastas}, NODES: {self._dt[-1]!r})"

    def root_delta(self):
        return self._dt[-1].delta

    def root_k(self):
        return self._dt[-1].bestk

    def _solve(self, node):
        if self.experiment["ksweep"] is None:
            node.find_delta(self.speciesinfo.kstart)
        else:
            node.node_ksweep(mink=self.mink, maxk=self.maxk)

    def _predigest(self, leaves):
        """blake2b of every leaf file not yet in the catalog, hashed on a few threads (hashlib releases
        the GIL) instead of one file at a time inside SketchPath: 0.5 s -> 0.1 s for 10 x 50 MB."""
        from concurrent.futures import ThreadPoolExecutor
        from .store import file_digest
        missing = [leaf.fastas[0] for leaf in leaves
                   if os.path.basename(leaf.fastas[0]) not in self.speciesinfo.fastahex]
        if len(missing) < 2:
            return
        with ThreadPoolExecutor(max_workers=min(8, len(missing))) as pool:
            for path, digest in zip(missing, pool.map(file_digest, missing)):
                self.speciesinfo.fastahex[os.path.basename(path)] = digest

    def _batch_leaf_sketch(self, leaves, lo, hi):
        """Sketch files of k in [lo, hi] for every leaf that lacks any of them, by ONE pipelined batch
        (files are read/inflated ahead while the GPU sketches); sharded over the ranks when several."""
        be = backend_for(self.experiment)
        lo = max(int(lo), 1)
        # (a hill-climb never asks Dashing for k > 32, lib/huffman_dandd.py:109; an explicit --ksweep range is taken
        # as given, there as here -- the per-leaf path sketches those ks too, one genome at a time)
        if self.experiment["tool"] == "dashing" and not self.experiment.get("allow_k64") and self.experiment["ksweep"] is None:
            hi = min(int(hi), 32)
        if hi < lo or not hasattr(be, "leaf_many"):
            return 0
        rank, world = dist_ranks()
        if world > 1:
            # the plan covers ALL leaves and depends on nothing a rank could see differently (file sizes,
            # not which sketches happen to exist at the moment a rank looks): every rank computes the same
            # shards, then skips what is already on disk within its own
            from ..dist import shard_by_weight
            mine = set(shard_by_weight([os.path.getsize(leaf.fastas[0]) for leaf in leaves], world)[rank])
        todo, templates = [], []
        for i, leaf in enumerate(leaves):
            if world > 1 and i not in mine:
                continue
            tmpl = leaf._template() if hasattr(leaf, "_template") else SketchPath(leaf.fastas, 0, self.speciesinfo, self.experiment)
            if any(not sketch_exists(tmpl.with_k(k)) for k in range(lo, hi + 1)):
                for k in range(lo, hi + 1):
                    ensure_dir(tmpl.dir.replace("{}", str(k)))
                todo.append(leaf.fastas[0])
                templates.append(tmpl)
        if todo and (world > 1 or len(todo) > 1):
            cards = be.leaf_many(todo, lo, hi, lambda i, k: templates[i].with_k(k))
            # (the product backend estimates every sketch of the batch in one launch: its answers go where
            # individual_card would have put them one file at a time; an empty sketch's 0 is left for that path)
            if cards:
                self.speciesinfo.cardkey.update({p: c for p, c in cards.items() if c > 0})
        return len(todo)

    def presketch_range(self, lo, hi):
        """Sketch files of k in [lo, hi] for every leaf of this tree in one batch -- sharded over the ranks
        of a multi-GPU run, which meet at a barrier afterwards (every rank must call this)."""
        leaves = self.leaf_nodes()
        self._predigest(leaves)
        n = self._batch_leaf_sketch(leaves, lo, hi)
        dist_barrier()
        return n

    def _presketch_leaves(self, leaves, radius=3):
        """Leaf sketches for the ks the per-leaf searches are about to ask for -- the whole ksweep
        range, or kstart +- radius for the hill-climb -- made for ALL leaves by one pipelined batch
        instead of genome by genome (the reference's loop, lib/huffman_dandd.py:402-407, is strictly
        sequential).  Purely a cache warm-up: see _leaf_batch_hook for searches that leave the window."""
        be = backend_for(self.experiment)
        if not hasattr(be, "leaf_many") or len(leaves) < 2 or os.environ.get("DD_NO_PREFETCH"):
            return
        self._predigest(leaves)
        if self.experiment["ksweep"] is not None:
            lo, hi = (int(v) for v in self.experiment["ksweep"])
        else:
            lo, hi = max(1, int(self.speciesinfo.kstart) - radius), int(self.speciesinfo.kstart) + radius
        self._batch_leaf_sketch(leaves, lo, hi)

    def _leaf_batch_hook(self, leaves, margin=2):
        """While the leaves are being solved: a hill-climb that asks one leaf for ks outside what is on
        disk gets them -- and `margin` more on either side -- sketched for EVERY
        leaf in one batch, because the other leaves' searches are about to walk the same way.  One pass
        over all files per window extension instead of one file read per (leaf, step)."""
        if len(leaves) < 2 or os.environ.get("DD_NO_PREFETCH") or dist_ranks()[1] > 1:
            return None

        def hook(ks):
            return self._batch_leaf_sketch(leaves, min(ks) - margin, max(ks) + margin)
        return hook

    def _build_tree(self, symbol, nchildren, leafnodes=()):
        """Leaves first (in the order given; the sort by ngen is stable), then unions of `nchildren`
        consecutive nodes, each new union inserted behind the nodes that are not larger than it
        (lib/huffman_dandd.py:377-438, including its end-of-list widening of the last union)."""
        nodes = list(leafnodes) or [DeltaTreeNode(s, [], self.speciesinfo, self.experiment) for s in symbol]
        nodes.sort()
        self._presketch_leaves(nodes)
        if not leafnodes and dist_ranks()[1] > 1:  # a tree built from FASTA names in a multi-rank run
            rank = dist_ranks()[0]
            dist_barrier()
            if rank != 0:
                raise WorkerDone()
        global _leaf_batch
        _leaf_batch = self._leaf_batch_hook(nodes) if self.experiment["ksweep"] is None else None
        try:
            for leaf in nodes:
                self._solve(leaf)
        finally:
            _leaf_batch = None
        self._dt = nodes
        insert_at = 0
        current = 0
        while current != len(self._dt) - 1:
            step = nchildren - 1
            kids = self._dt[current:current + nchildren]
            union = DeltaTreeNode("_".join(k.node_title for k in kids), kids, self.speciesinfo, self.experiment,
                                  progeny=[leaf for k in kids for leaf in k.progeny])
            self._solve(union)
            while insert_at < len(self._dt) - step and self._dt[insert_at + step].ngen <= union.ngen:
                insert_at += step
            cut = insert_at + step
            self._dt = self._dt[:cut] + [union] + self._dt[cut:]
            current += nchildren
            if cut > len(self._dt) - 1:
                nchildren = len(self._dt) - current

    def print_list(self):
        print(" -> ".join(f"'{n.node_title}'({n.ngen}'({' '.join(p.node_title for p in n.progeny)})" for n in self._dt))

    def fill_tree(self, padding=False):
        root = self._dt[-1]
        if self.experiment["ksweep"] is None:
            for k in sorted({n.bestk for n in self._dt} - {0}):
                root.update_node(k)
        else:
            self.ksweep(*self.experiment["ksweep"])

    def leaf_nodes(self):
        return [n for n in self._dt if n.ngen == 1]

    def delete_sketches(self):
        for node in self._dt[:-1]:
            if node.ngen > 1:
                for s in node.ksketches:
                    if s is not None:
                        s.remove_sketch()

    def make_prefix(self, tag, label="", outdir=None):
        outdir = outdir or os.getcwd()
        label = "_" + label if label else ""
        return os.path.join(outdir, f"{tag}{label}_{self.ngen}_{self.experiment['tool']}")

    def save(self, fileprefix, fast=False):
        filepath = fileprefix + "_dtree.pickle"
        if not fast:
            from .compat import dump_tree
            with open(filepath, "wb") as f:
                dump_tree(self, f)  # under the reference's GLOBAL names: its own progressive/kij can load it
            print("Tree Pickle saved to: " + filepath)
            mapping = fileprefix + "_sketchdb.txt"
            write_listdict_to_csv(mapping, [self.speciesinfo.sketchinfo[b] for b in self.experiment["baseset"]])
            print(f"Output Sketch/DB mapping saved to {mapping}.")
        deltapath = fileprefix + "_deltas.csv"
        write_listdict_to_csv(deltapath, self.report_deltas())
        print("Deltas saved to: " + deltapath)
        return filepath

    def report_deltas(self):
        rows = []

        def visit(node):
            best = node.ksketches[node.bestk]
            rows.append({"delta": node.delta, "k": node.bestk, "title": node.node_title, "ngen": node.ngen,
                         "sketchloc": best.sketch, "card": best.card, "fastas": "|".join(node.fastas)})
            for child in node.children or []:
                visit(child)

        visit(self._dt[-1])
        return rows

    def nodes_from_fastas(self, fasta_list):
        return [n for n in self.leaf_nodes() if n.fastas[0] in fasta_list]

    def find_delta_delta(self, fasta_subset):
        rest = [f for f in self.fastas if f not in fasta_subset]
        small = SubSpider(self.nodes_from_fastas(rest), self.speciesinfo, self.experiment)
        print("Full Tree Delta: ", self.delta)
        print("Subtree Delta: ", small.delta)
        return self - small

    def ksweep(self, mink, maxk):
        for node in self._dt:
            node.node_ksweep(mink=mink, maxk=maxk)

    # ---- relative contributions: delta(all) - delta(all but a group) (lib/huffman_dandd.py:559-566) ---------------------
    def leave_out_deltas(self, groups, mink=None, maxk=None, labels=None):
        """One row per group of leaf FASTAs (`groups`, in order): delta_all - delta_rest, where `rest` is every leaf of the tree
        outside the group (leaves in no group are in every `rest`).
          * Hill-climb (no window: neither mink/maxk nor the tree's --ksweep): exactly what find_delta_delta(group) would give,
            called group after group -- the same climb from speciesinfo.kstart, which each climb moves for the next --, with
            delta_all the tree's own root delta.
          * A window [mink, maxk] (given, or the tree's --ksweep): the reference has no delta for a union there (SubSpider.delta
            stays None), so delta here is max over k in the window of card / k, ties going to the larger k (the climb's `<=`),
            for the rest and, by the same rule, for the union of all leaves.  Per-k rows come back too.
        With a backend that has leave_out_cards (the GPU) every complement at every k of a window comes from ONE launch over the
        leaf slab (exact trees: one sort of the leaves' k-mers per k) and the climbs walk that table (_FlatUnion), falling back to
        files where a climb leaves it; otherwise (--safe, DD_NO_PREFETCH, a backend without a table for these leaves, the CPU
        checkers) each group goes through SubSpider / find_delta_delta on the object path.
        -> (rows, per-k rows)"""
        leaves = self.leaf_nodes()
        by_fasta = {leaf.fastas[0]: leaf for leaf in leaves}
        groups = [list(g) for g in groups]
        owner = {}
        for gi, g in enumerate(groups):
            if not g:
                raise ValueError(f"group {gi + 1} is empty")
            for f in g:
                if f not in by_fasta:
                    raise ValueError(f"{f} is not a leaf of this tree")
                if owner.setdefault(f, gi) != gi:
                    raise ValueError(f"{f} is in more than one group")
            if len(set(g)) == len(leaves):
                raise ValueError(f"group {gi + 1} holds every leaf of the tree: there is nothing left to compare with")
        labels = list(labels) if labels is not None else [str(i + 1) for i in range(len(groups))]
        if mink is None or maxk is None:
            window = self.experiment["ksweep"]
        else:
            window = (int(mink), int(maxk))
        exp = dict(self.experiment, ksweep=tuple(int(v) for v in window) if window is not None else None)
        be = backend_for(exp)
        sched = None
        if hasattr(be, "leave_out_cards") and _batched(exp):
            lo, hi = self._table_window(exp)
            lo = max(1, lo)
            if hi >= lo:
                group_of = [owner.get(leaf.fastas[0], -1) for leaf in leaves]
                table = _cards_or_wide(be, "leave_out_cards", self._leaf_files(leaves, lo, hi), group_of)
                if table is not None:       # (None: the backend has no schedule for this many leaves)
                    sched = UnionTable(table, lo, hi)
        rows, summary = [], []
        full = None
        for gi, g in enumerate(groups):
            out = set(g)
            kids = [leaf for leaf in leaves if leaf.fastas[0] not in out]     # tree order, as nodes_from_fastas gives them
            row = {"group": labels[gi], "fastas": "|".join(f for f in self.fastas if f in out),
                   "nout": len(out), "ngen_rest": len(kids)}
            sub = _FlatUnion(self, kids, exp, sched, sched.table[gi]) if sched is not None else None
            if window is None:
                if sub is None:
                    # find_delta_delta's own steps, keeping the spider it builds (its result is `self - small`)
                    small = SubSpider(self.nodes_from_fastas([f for f in self.fastas if f not in out]), self.speciesinfo, exp)
                    k_rest = small.root_k()
                else:
                    sub.find_delta(self.speciesinfo.kstart)       # SubSpider.__init__ ...
                    sub.fill()                                    # ... and its fill_tree
                    small, k_rest = sub, sub.bestk
                print("Full Tree Delta: ", self.delta)
                print("Subtree Delta: ", small.delta)
                row["deltadelta"] = self - small
                row["delta_rest"], row["k_rest"] = small.delta, k_rest
                row["delta_all"], row["k_all"] = self.delta, self.root_k()
            else:
                lo, hi = exp["ksweep"]
                ks = list(range(max(1, lo), hi + 1))
                if sub is None:
                    if full is None:
                        full_tree = SubSpider(leaves, self.speciesinfo, exp)
                        full = [full_tree.root.ksketches[k].card for k in ks]
                    small = SubSpider(kids, self.speciesinfo, exp)
                    rest = [small.root.ksketches[k].card for k in ks]
                else:
                    if full is None:
                        full = [float(v) for v in sched.table[len(groups)]]
                    sub.node_ksweep(lo, hi)
                    rest = [sub.card(k) for k in ks]
                row["delta_all"], row["k_all"] = _window_delta(full, ks)
                row["delta_rest"], row["k_rest"] = _window_delta(rest, ks)
                row["deltadelta"] = row["delta_all"] - row["delta_rest"]
                for k, a, r in zip(ks, full, rest):
                    summary.append({"group": labels[gi], "kval": k, "card_all": a, "card_rest": r, "delta_pos_rest": r / k})
            rows.append(row)
        return rows, summary

    # ---- exact order effects over all n! orderings, from the 2^n subset unions (`dandd abba`) ---------------------------
    def ordering_expectations(self, fastas, lo, hi):
        """Window delta of the union of every subset of `fastas` (n <= 16 leaf FASTAs, the universe U) over k in
        [max(1, lo), hi] -- the largest card / k, ties going to the larger k; 0 for the empty set -- and what they give over
        all n! orderings of U (abba_expectations).  Bit i of a mask is fastas[i].
          * Schedule path (a backend with subset_cards): the leaves' window sketches, then every subset at every k of the
            window from ONE launch over the leaf slab.  Subset unions are neither written nor cached (65 536 at n = 16).
          * Object path (--safe, DD_NO_PREFETCH, a backend without a table for these leaves, the CPU checkers): one SubSpider
            per non-empty subset.
        -> dict: ks, cards [2^n][K], delta [2^n], kval [2^n] and the abba_expectations entries"""
        u = self._universe(fastas, lo, hi)
        n, ks = u.n, np.array(u.ks)
        cards = None
        if hasattr(u.be, "subset_cards") and u.batched:
            cards = u.be.subset_cards(u.paths)
        if cards is not None:
            cards = np.asarray(cards, dtype=np.float64).reshape(1 << n, len(ks))
        else:
            cards = np.zeros((1 << n, len(ks)))
            for mask in range(1, 1 << n):
                cards[mask] = u.union_cards([i for i in range(n) if mask >> i & 1])
        ratio = cards / ks
        last = len(ks) - 1 - np.argmax(ratio[:, ::-1], axis=1)        # (ties: the larger k, as _window_delta)
        delta = ratio[np.arange(1 << n), last]
        kval = ks[last]
        delta[0], kval[0] = 0.0, 0
        out = dict(ks=ks, cards=cards, delta=delta, kval=kval)
        out.update(abba_expectations(delta))
        return out

    # ---- steepest and flattest growth orderings (`dandd greedy`) --------------------------------------------------------
    def greedy_orderings(self, fastas, lo, hi, modes, base=(), steps=None):
        """For each mode ("max", "min") the ordering of `fastas` (leaf FASTAs, the universe) that starts with `base` (in its
        order) and then adds at each step the genome whose union with the chosen ones has the largest (smallest) window delta
        over k in [max(1, lo), hi], until `steps` genomes stand (default: all).  The rule is _greedy_pick's -- the largest
        card / k, ties between k to the larger k, ties between genomes to the earlier one of `fastas` -- on every path:
          * Schedule path (a backend with greedy_cards, the GPU): one call per mode -- over the leaf slab, or, on exact trees
            of 17..64 genomes, over the membership masks of one sort per k.
          * n <= 16 and a backend with subset_cards (exact trees on the GPU): a walk over that one table.
          * Object path (--safe, DD_NO_PREFETCH, a backend with neither, the CPU checkers, exact trees of more than 64
            genomes or whose masks do not fit their store): one SubSpider per (step, candidate), through the cardinality
            cache.
        -> dict: ks, and per mode dict(order: FASTAs [steps], cards [steps][K], delta [steps], kval [steps])"""
        base = list(base)
        given = set(base)
        seq = base + [f for f in fastas if f not in given]          # candidates in tie-break order behind the given start
        n, nfixed = len(seq), len(base)
        steps = n if steps is None else int(steps)
        if not 1 <= steps <= n or steps < nfixed:
            raise ValueError(f"{steps} steps: between {max(1, nfixed)} and {n}")
        u = self._universe(seq, lo, hi)
        be, ks = u.be, u.ks
        out = {"ks": ks}
        table = None
        for mode in modes:
            order = cards = None
            if u.batched and hasattr(be, "greedy_cards"):
                got = be.greedy_cards(u.paths, mode, nfixed, steps, u.lo)
                if got is not None:
                    order = [int(i) for i in got[0]]
                    cards = np.asarray(got[1], dtype=np.float64).reshape(steps, len(ks))
            if order is None:
                if table is None and u.batched and n <= 16 and hasattr(be, "subset_cards"):
                    table = be.subset_cards(u.paths)
                    if table is not None:
                        table = np.asarray(table, dtype=np.float64).reshape(1 << n, len(ks))
                if table is not None:
                    def card_of(chosen, c, table=table):
                        return table[sum(1 << i for i in chosen) | 1 << c]
                else:
                    def card_of(chosen, c):
                        return u.union_cards([*chosen, c])
                order, cards = _greedy_walk(card_of, n, nfixed, steps, mode, ks)
            picked = [_window_delta([float(c) for c in row], ks) for row in cards]
            out[mode] = dict(order=[seq[i] for i in order], cards=np.asarray(cards, dtype=np.float64),
                             delta=[d for d, _ in picked], kval=[k for _, k in picked])
        return out

    # ---- core genome, k-mer spectrum and group markers (`dandd core`) -----------------------------------------------------
    def core_tables(self, fastas, lo, hi, orderings, groups=None):
        """What the exact membership masks of `fastas` (1..64 leaf FASTAs of an exact tree, the universe; bit i is fastas[i])
        say over k in [max(1, lo), hi], each table from ONE backend call:
          spectrum [n+1][K]   k-mers held by exactly j genomes (spectrum_counts)
          core [o][n][K]      k-mers held by every one of the first j+1 genomes of each ordering (core_progressive_counts)
          pan [o][n][K]       the union of the same prefixes: progressive_cards where the backend has that table, else one
                              SubSpider per prefix (the object path of `progressive`)
          groups [g][3][K]    with `groups` (lists of FASTAs): core, private and signature k-mers (KMER_QUERIES) of
                              every group, three queries each in one select_counts call
        There is no object path behind the three new tables: a backend without them, or without a table for these leaves,
        is a ValueError.  -> dict: ks and the tables as integer arrays"""
        u = self._universe(fastas, lo, hi)
        u.need("spectrum_counts", "core_progressive_counts", "select_counts", why="intersections need")
        be, paths, n, ks = u.be, u.paths, u.n, u.ks
        orderings = [[int(i) for i in o] for o in orderings]
        out = {"ks": ks}
        out["spectrum"] = u.table(be.spectrum_counts(paths), (n + 1, len(ks)))
        out["core"] = u.table(be.core_progressive_counts(paths, orderings), (len(orderings), n, len(ks)))
        pan = None
        if hasattr(be, "progressive_cards") and u.batched:
            pan = _cards_or_wide(be, "progressive_cards", paths, orderings)
        if pan is None:
            pan = np.zeros((len(orderings), n, len(ks)))
            seen = {}
            for o, order in enumerate(orderings):
                for j in range(n):
                    key = frozenset(order[:j + 1])
                    if key not in seen:
                        seen[key] = u.union_cards(sorted(key))
                    pan[o, j] = seen[key]
        out["pan"] = np.rint(np.asarray(pan, dtype=np.float64)).astype(np.uint64).reshape(len(orderings), n, len(ks))
        if groups:
            out["groups"] = u.table(be.select_counts(paths, *group_queries(u.masks(groups), u.full)), (len(groups), 3, len(ks)))
        return out

    KMER_CLASSES = tuple(KMER_QUERIES)                    # the columns of core_tables' groups, in that order

    def _core_cells(self, fastas, groups, wanted, ks, window, counts, entry):
        """What core_kmers and core_regions share: the universe over the window, whose backend must have select_counts and
        `entry`, and one cell per group, class of `wanted` and k -- the class's argmax of count / k over the window
        (_window_delta's rule: the *_k of the group summary), or every k of `ks`.
        -> (universe, members [g] (indices into fastas), cells [(group, class, k, all, none, count)])"""
        wanted = [c for c in self.KMER_CLASSES if c in set(wanted)]
        if window is None:
            window = self.experiment.get("ksweep")
        if window is None:
            raise ValueError("a k window is needed")
        u = self._universe(fastas, *window)
        for k in ks or []:
            if int(k) not in u.ks:
                raise ValueError(f"k={k} is outside the window {u.lo}..{u.hi}")
        u.need("select_counts", entry, why="intersections need")
        paths = u.paths
        members = [sorted({u.index[f] for f in g}) for g in groups]
        gmasks = u.masks(groups)
        if counts is None:
            counts = u.be.select_counts(paths, *group_queries(gmasks, u.full))
        counts = u.table(counts, (len(groups), 3, len(u.ks)))
        cells = []
        for gi, G in enumerate(gmasks):
            for cls in wanted:
                col = [int(v) for v in counts[gi, self.KMER_CLASSES.index(cls)]]
                for k in ([int(k) for k in ks] if ks else [_window_delta(col, u.ks)[1]]):
                    cells.append((gi, cls, k, *KMER_QUERIES[cls](G, u.full), col[k - u.lo]))
        return u, members, cells

    def core_kmers(self, fastas, groups, wanted, ks=None, limit=1_000_000, window=None, counts=None):
        """The k-mers behind the cells of core_tables' `groups`: for every group (lists of FASTAs of the universe `fastas`) and
        every class of `wanted` (core, private, signature: KMER_QUERIES) the k-mers themselves at the k
        where count / k is largest over the window (_window_delta's rule: the *_k of the group summary), or at every k of
        `ks`.  window: (lo, hi), default the tree's --ksweep; counts: core_tables(...)["groups"] of the same window where the
        caller has it, else one select_counts call.  ONE select_kmers call per distinct k carries every query of that k; the
        records come back once each, ascending, and go to their queries by their masks, here.  A cell of more than `limit`
        k-mers is a ValueError that names it, before any k-mer is asked for.
        -> list of dict(group, cls, k, kmers uint64 [m][2] (lo, hi), masks uint64 [m]) in (group, class as KMER_CLASSES, k) order"""
        u, _, cells = self._core_cells(fastas, groups, wanted, ks, window, counts, "select_kmers")
        for gi, cls, k, _, _, count in cells:
            if count > limit:
                raise ValueError(f"group {gi + 1}, {cls}, k={k}: {count} k-mers, more than the limit of {limit}")
        got = {}
        for k in sorted({cell[2] for cell in cells}):
            mine = sorted({(a, b) for _, _, kk, a, b, _ in cells if kk == k})
            room = sum(count for _, _, kk, _, _, count in cells if kk == k)     # (the union of the queries holds no more)
            res = u.table(u.be.select_kmers(u.paths, k, [a for a, _ in mine], [b for _, b in mine], room))
            got[k] = (np.asarray(res[0], dtype=np.uint64).reshape(-1, 2), np.asarray(res[1], dtype=np.uint64).reshape(-1))
        out = []
        for gi, cls, k, a, b, count in cells:
            kmers, masks = got[k]
            keep = ((masks & np.uint64(a)) == np.uint64(a)) & ((masks & np.uint64(b)) == np.uint64(0))
            if int(keep.sum()) != count:
                raise ValueError(f"group {gi + 1}, {cls}, k={k}: {int(keep.sum())} k-mers came back, {count} were counted")
            out.append(dict(group=gi, cls=cls, k=k, kmers=kmers[keep], masks=masks[keep]))
        return out

    def core_regions(self, fastas, groups, wanted, ks=None, window=None, counts=None):
        """Where the k-mers of core_kmers' cells lie in the genomes: for every group, every class of `wanted` and the k of
        core_kmers' rule (the class's argmax of count / k over the window, or every k of `ks`), the query is painted onto every
        genome OF ITS GROUP and the hit positions become 0-based half-open base intervals per record -- the union of the
        k-mers' spans, overlapping and abutting ones merged (engine.regions_from_hits).  ONE locate_hits call per distinct k
        carries every job of that k.  window, counts: as for core_kmers.
        -> list of dict(group, cls, k, genomes [(fasta, [(record name, start, end)])]) in (group, class as KMER_CLASSES, k)
        order; a cell's genomes in the universe's order, a genome's rows by record, then start"""
        from ..engine import regions_from_hits
        u, members, cells = self._core_cells(fastas, groups, wanted, ks, window, counts, "locate_hits")
        got = {}                                                       # (k, all, none, genome) -> intervals per record
        names = {}                                                     # genome -> its records' names
        for k in sorted({cell[2] for cell in cells}):
            jobs = sorted({(a, b, g) for gi, _, kk, a, b, _ in cells if kk == k for g in members[gi]})
            recs, hits = u.table(u.be.locate_hits(u.paths, k, jobs))
            for (a, b, g), words in zip(jobs, hits):
                rec_names, seq_len, tok_start, _ = recs[g]
                names[g] = list(rec_names)
                got[(k, a, b, g)] = regions_from_hits(words, k, tok_start, seq_len)
        out = []
        for gi, cls, k, a, b, _ in cells:
            per = [(fastas[g], [(name, int(s), int(e)) for name, spans in zip(names[g], got[(k, a, b, g)]) for s, e in spans])
                   for g in members[gi]]
            out.append(dict(group=gi, cls=cls, k=k, genomes=per))
        return out

    # ---- samples that are no leaves (`dandd screen`) ---------------------------------------------------------------------
    SCREEN_BATCH_FILES, SCREEN_BATCH_BYTES = 64, 4 << 30    # samples of one screen_counts call: files, bytes of their files

    def screen_tables(self, fastas, samples, ks, groups=None):
        """Exact containment of `samples` (files that are no leaves: FASTA / FASTQ, plain or gzip) in the universe `fastas`
        (1..64 leaf FASTAs of an exact tree; bit i is fastas[i]) at every k of `ks`.  The queries are (0, 0) -- in the
        pan-genome at all --, (full, 0) -- in the core --, then the core, private and signature k-mers
        (KMER_QUERIES, in that order) of every group of `groups` (lists of FASTAs).  The samples go to the backend's
        screen_counts in batches of at most SCREEN_BATCH_FILES files or SCREEN_BATCH_BYTES bytes, whichever comes first; each
        batch sorts the universe again, which is cheap next to reading the samples.  A sample's own distinct k-mers are a
        leaf database of its own, made in a temporary directory and counted by the backend's card.  There is no object path:
        a backend without screen_counts, or without a table for these leaves, is a ValueError.
        -> dict: ks, shared [K][ns+1][n], match [K][ns+1][nq] (row ns: the universe itself), sample_kmers [K][ns]"""
        import tempfile
        n, ns, nq = len(fastas), len(samples), 2 + len(self.KMER_CLASSES) * len(groups or [])
        ks = self._ks(ks)
        out = {"ks": ks, "shared": np.zeros((len(ks), ns + 1, n), dtype=np.uint64), "match": np.zeros((len(ks), ns + 1, nq), dtype=np.uint64),
               "sample_kmers": np.zeros((len(ks), ns), dtype=np.uint64)}
        be = {}      # the backend of every k's universe
        for kk, k, u, batch, files in self._sample_calls(fastas, samples, ks, "screen_counts", "containment needs"):
            be[k] = u.be
            alls, nones = group_queries(u.masks(groups or []), u.full)
            got = u.table(u.be.screen_counts(u.paths, k, files, [0, u.full] + alls, [0, 0] + nones))
            shared, match = u.table(got[0], (len(batch) + 1, n)), u.table(got[1], (len(batch) + 1, nq))
            out["shared"][kk, batch] = shared[:-1]
            out["match"][kk, batch] = match[:-1]
            out["shared"][kk, ns], out["match"][kk, ns] = shared[-1], match[-1]      # (the same in every batch)
        with tempfile.TemporaryDirectory(prefix="dandd_screen_") as tmp:
            for kk, k in enumerate(ks):
                for j, f in enumerate(samples):
                    db = os.path.join(tmp, f"s{j}.k{k}")
                    be[k].leaf(f, [k], [db])
                    out["sample_kmers"][kk, j] = int(be[k].card(db))
        return out

    @staticmethod
    def _ks(ks):
        """`ks` as a list of ints, each a k of the engine"""
        ks = [int(k) for k in ks]
        for k in ks:
            if not 1 <= k <= 64:
                raise ValueError(f"k={k} is outside 1..64")
        return ks

    @staticmethod
    def _window(window):
        """a window of tokens (paint: of a sample's stream; cover: of a target's): whole 64-token segments"""
        window = int(window)
        if window < 64 or window % 64 or window > 1 << 22:
            raise ValueError(f"a window of {window} tokens: a multiple of 64 in 64..{1 << 22} is needed")
        return window

    def _sample_calls(self, fastas, samples, ks, entry, why):
        """The backend calls of a table over samples that are no leaves, one per k of `ks` (checked: _ks) and batch of
        `samples` (_sample_batches): (kk, k, the universe at that k -- whose backend has `entry` --, the batch's indices, its files)"""
        batches = self._sample_batches(samples)
        for kk, k in enumerate(ks):
            u = self._universe(fastas, k, k)
            u.need(entry, why=why)
            for batch in batches:
                yield kk, k, u, batch, [samples[j] for j in batch]

    def _sample_batches(self, samples):
        """indices of `samples` in batches of at most SCREEN_BATCH_FILES files or SCREEN_BATCH_BYTES bytes, whichever comes first"""
        batches, size = [[]], 0
        for j, f in enumerate(samples):
            b = os.path.getsize(f)
            if batches[-1] and (len(batches[-1]) >= self.SCREEN_BATCH_FILES or size + b > self.SCREEN_BATCH_BYTES):
                batches.append([])
                size = 0
            batches[-1].append(j)
            size += b
        return batches

    def paint_tables(self, fastas, samples, ks, window):
        """Where along each of `samples` (files that are no leaves: FASTA / FASTQ, plain or gzip) the k-mers of the universe
        `fastas` (1..64 leaf FASTAs of an exact tree; bit i is fastas[i]) lie, at every k of `ks`: the sample's token stream
        (one BREAK in front of every record's bases) in windows of `window` tokens, a multiple of 64, and per window the
        positions where a valid k-mer ends, where the universe holds it, and where fastas[i] holds it -- positions, not
        distinct k-mers.  The samples go to the backend's paint_counts in screen_tables' batches.  There is no object path:
        a backend without paint_counts, or without a table for these leaves, is a ValueError.
        -> dict: ks, window, index [ns] of (names, seq_len, tok_start, ntok), counts [K][ns] of uint32 [nwin_s][n+2]"""
        n, ns, ks, window = len(fastas), len(samples), self._ks(ks), self._window(window)
        out = {"ks": ks, "window": window, "index": [None] * ns, "counts": [[None] * ns for _ in ks]}
        for kk, k, u, batch, files in self._sample_calls(fastas, samples, ks, "paint_counts", "painting needs"):
            index, counts = u.table(u.be.paint_counts(u.paths, k, files, window))
            for j, ix, rows in zip(batch, index, counts):
                nwin = -(-int(ix[3]) // window)
                out["index"][j] = ix
                out["counts"][kk][j] = u.table(rows, (nwin, n + 2)).astype(np.uint32)
        return out

    def reads_tables(self, fastas, samples, ks, min_hits=1, want_calls=False):
        """Which genome of the universe `fastas` (1..64 leaf FASTAs of an exact tree; bit i is fastas[i]) each record of each
        of `samples` (files that are no leaves: a read set, a draft assembly; FASTA / FASTQ, plain or gzip) belongs to, at
        every k of `ks`, and how many records of a sample go to each genome.  A record is called to the genome that holds
        most of its k-mer positions where those are at least `min_hits`; several genomes with that count make it ambiguous.
        The samples go to the backend's read_calls in screen_tables' batches.  There is no object path: a backend without
        read_calls, or without a table for these leaves, is a ValueError.
        -> dict: ks, min_hits, index [ns] of (names, seq_len, tok_start, ntok), tally [K] of uint64 [ns][n+3] (unique to
        genome i | ambiguous | unclassified | no valid k-mer), calls [K][ns] of (calls uint32 [r][6], sets uint64 [r][2]),
        None without want_calls"""
        n, ns, ks, min_hits = len(fastas), len(samples), self._ks(ks), int(min_hits)
        if min_hits < 1:
            raise ValueError(f"min_hits={min_hits}: a call needs at least one position")
        out = {"ks": ks, "min_hits": min_hits, "index": [None] * ns, "tally": [np.zeros((ns, n + 3), dtype=np.uint64) for _ in ks],
               "calls": [[None] * ns for _ in ks]}
        for kk, k, u, batch, files in self._sample_calls(fastas, samples, ks, "read_calls", "calling records needs"):
            index, per, tally = u.table(u.be.read_calls(u.paths, k, files, min_hits, bool(want_calls)))
            out["tally"][kk][batch] = u.table(tally, (len(batch), n + 3))
            for j, ix, got in zip(batch, index, per):
                out["index"][j] = ix
                if want_calls:
                    r = len(ix[2])
                    out["calls"][kk][j] = (u.table(got[0], (r, 6)).astype(np.uint32), u.table(got[1], (r, 2)).astype(np.uint64))
        return out

    def depth_tables(self, fastas, samples, ks, groups=None, bins=64):
        """How many times each of `samples` (files that are no leaves: a read set, an assembly; FASTA / FASTQ, plain or gzip)
        holds the k-mers of the universe `fastas` (1..64 leaf FASTAs of an exact tree; bit i is fastas[i]), at every k of
        `ks`: per row of k-mers a histogram of `bins` depths (positions of the sample per distinct k-mer; bin 0: k-mers the
        sample lacks, the last bin: depth >= bins - 1) and the sum of the depths.  The rows are the n genomes, then the queries
        (0, 0) -- the pan-genome --, (full, 0) -- the core --, every genome's private k-mers (1 << i, full ^ (1 << i)), then
        the core, private and signature k-mers (KMER_QUERIES, in that order) of every group of `groups` (lists of FASTAs).
        The samples go to the backend's depth_hists in screen_tables' batches.  There is no object path: a backend without
        depth_hists, or without a table for these leaves, is a ValueError.
        -> dict: ks, bins, hist [K][ns][n+nq][bins], total [K][ns][n+nq] (engine.depth_stats turns them into breadth, mean
        and median); nq = 2 + n + 3 * len(groups)"""
        n, ns, ks, bins = len(fastas), len(samples), self._ks(ks), int(bins)
        nq = 2 + n + len(self.KMER_CLASSES) * len(groups or [])
        if not 2 <= bins <= 256:
            raise ValueError(f"bins={bins} is outside 2..256")
        out = {"ks": ks, "bins": bins, "hist": np.zeros((len(ks), ns, n + nq, bins), dtype=np.uint64),
               "total": np.zeros((len(ks), ns, n + nq), dtype=np.uint64)}
        for kk, k, u, batch, files in self._sample_calls(fastas, samples, ks, "depth_hists", "depth needs"):
            alls, nones = group_queries(u.masks(groups or []), u.full)
            alls = [0, u.full] + [1 << i for i in range(n)] + alls
            nones = [0, 0] + [u.full ^ (1 << i) for i in range(n)] + nones
            got = u.table(u.be.depth_hists(u.paths, k, files, alls, nones, bins))
            out["hist"][kk, batch] = u.table(got[0], (len(batch), n + nq, bins))
            out["total"][kk, batch] = u.table(got[1], (len(batch), n + nq))
        return out

    def cover_tables(self, fastas, samples, ks, window, targets=None, clip=255):
        """Where along the genomes `targets` (FASTAs of the universe; None: all of it) each of `samples` (files that are no
        leaves: a read set, an assembly; FASTA / FASTQ, plain or gzip) lies, and how deep, at every k of `ks`; the universe
        `fastas` is 1..64 leaf FASTAs of an exact tree.  The TARGET's token stream (one BREAK in front of every record's bases)
        goes in windows of `window` tokens, a multiple of 64, and per sample and window six counts over the positions where
        a valid k-mer ends: valid, covered (the sample holds the k-mer), depth (the times it holds it, at most `clip` a
        position, summed), and private, private_covered, private_depth -- the same over the positions whose k-mer no other
        genome of the universe holds.  The samples go to the backend's cover_counts in screen_tables' batches.  There is no
        object path: a backend without cover_counts, or without a table for these leaves, is a ValueError.
        -> dict: ks, window, clip, targets (FASTAs), index [nt] of (names, seq_len, tok_start, ntok), counts [K][nt] of uint32
        [ns][nwin_t][6]"""
        n, ns, ks, window, clip = len(fastas), len(samples), self._ks(ks), self._window(window), int(clip)
        if not 1 <= clip <= 1023:
            raise ValueError(f"clip={clip} is outside 1..1023")
        targets = list(fastas) if targets is None else list(targets)
        for f in targets:
            if f not in fastas:
                raise ValueError(f"{f} is not in the universe")
        if not targets or len(set(targets)) != len(targets):
            raise ValueError("the targets are genomes of the universe, each once, at least one")
        at = [fastas.index(f) for f in targets]
        out = {"ks": ks, "window": window, "clip": clip, "targets": targets, "index": [None] * len(at), "counts": [[None] * len(at) for _ in ks]}
        for kk, k, u, batch, files in self._sample_calls(fastas, samples, ks, "cover_counts", "coverage needs"):
            index, counts = u.table(u.be.cover_counts(u.paths, k, files, window, at, clip))
            for t, (ix, rows) in enumerate(zip(index, counts)):
                nwin = -(-int(ix[3]) // window)
                out["index"][t] = ix
                if out["counts"][kk][t] is None:
                    out["counts"][kk][t] = np.zeros((ns, nwin, 6), dtype=np.uint32)
                out["counts"][kk][t][batch] = u.table(rows, (len(batch), nwin, 6))
        return out

    def gather_tables(self, fastas, samples, ks, min_hits=1, steps=None):
        """Which genomes of the universe `fastas` (1..64 leaf FASTAs of an exact tree; bit i is fastas[i]) explain each of
        `samples` (files that are no leaves: a metagenome, a contaminated assembly; FASTA / FASTQ, plain or gzip), one by
        one, at every k of `ks`: the greedy set cover of the sample's distinct k-mers.  Step t picks the genome that holds
        most of the sample's k-mers that no earlier pick holds -- ties: the earlier genome of the universe -- and the walk
        stops at a pick with fewer than `min_hits` such k-mers or behind `steps` picks (None: as many as there are genomes).
        The samples go to the backend's gather_picks in screen_tables' batches.  There is no object path: a backend without
        gather_picks, or without a table for these leaves, is a ValueError.
        -> dict: ks, min_hits, steps, pick int32 [K][ns][steps] (-1 behind the stop), unique [K][ns][steps] (the k-mers a
        pick adds), depth [K][ns][steps] (the times the sample holds them, summed), shared [K][ns][n] (screen_tables'
        shared), total [K][ns][2] (the sample's distinct k-mers in the universe, the sum of their depths)"""
        n, ns, ks, min_hits = len(fastas), len(samples), self._ks(ks), int(min_hits)
        steps = n if steps is None else int(steps)
        if not 1 <= min_hits < 1 << 32:
            raise ValueError(f"min_hits={min_hits}: a pick needs at least one k-mer, and the count is 32 bits wide")
        if not 1 <= steps <= n:
            raise ValueError(f"steps={steps} is outside 1..{n}, the genomes of the universe")
        out = {"ks": ks, "min_hits": min_hits, "steps": steps, "pick": np.full((len(ks), ns, steps), -1, dtype=np.int32),
               "unique": np.zeros((len(ks), ns, steps), dtype=np.uint64), "depth": np.zeros((len(ks), ns, steps), dtype=np.uint64),
               "shared": np.zeros((len(ks), ns, n), dtype=np.uint64), "total": np.zeros((len(ks), ns, 2), dtype=np.uint64)}
        for kk, k, u, batch, files in self._sample_calls(fastas, samples, ks, "gather_picks", "gathering needs"):
            got = u.table(u.be.gather_picks(u.paths, k, files, min_hits, steps))
            out["pick"][kk, batch] = np.asarray(got[0]).astype(np.int32).reshape(len(batch), steps)     # (signed: -1 behind the stop)
            for name, arr, cols in zip(("unique", "depth", "shared", "total"), got[1:], (steps, steps, n, 2)):
                out[name][kk, batch] = u.table(arr, (len(batch), cols))
        return out

    # ---- which sets of genomes share k-mers (`dandd patterns`) --------------------------------------------------------------
    def pattern_tables(self, fastas, ks, top=None):
        """The membership patterns of the universe `fastas` (1..64 leaf FASTAs of an exact tree; bit i is fastas[i]) at every
        k of `ks`: the distinct masks and the distinct k-mers that carry exactly each, count descending, ties by mask
        ascending -- the first `top` of them (None: all).  One pattern_counts call of the backend per k.  There is no object
        path: a backend without pattern_counts, or without a table for these leaves, is a ValueError.
        -> dict: ks, and per k of it dict(masks [int], counts [int], found: the number of distinct masks, distinct: the distinct
        k-mers of the universe)"""
        ks = self._ks(ks)
        out = {"ks": ks}
        for k in ks:
            u = self._universe(fastas, k, k)
            u.need("pattern_counts", why="the pattern table is a count over")
            masks, counts, found, distinct = u.table(u.be.pattern_counts(u.paths, k, None if top is None else int(top)))
            out[k] = dict(masks=[int(m) for m in masks], counts=[int(v) for v in counts], found=int(found), distinct=int(distinct))
        return out

    # ---- new samples against a tree of sketches (`dandd neighbors`) ---------------------------------------------------------
    def neighbor_tables(self, fastas, samples, mink, maxk):
        """The union cardinalities that place each of `samples` (files that are no leaves; FASTA / FASTQ, plain or gzip) among
        the universe `fastas` (leaf FASTAs of a tree of sketches, any number of them) over k in [max(1, mink), maxk]: every
        sample against every genome -- the rectangle --, and against the union of them all.
          * The leaves are brought up to date over the window as `kij` brings them; the samples are sketched by the backend
            (sample_sketches) and kept in memory only: no sketch file, no cardinality cache entry, nothing in the pickle.
          * |S| from sample_cards; |S U G| from ONE cross_cards call of the samples against the leaf slab; |S U all| from a
            second one against ONE row per k, the union of the universe's leaves -- the root's sketches when the universe is
            every leaf, else the leaves merged by the backend.
          * A sample of empty registers rides behind the samples in both calls: max(0, g) = g, so its row holds |G| of every
            genome and |all|, from the histograms and the estimator every other cell comes from.  A sample that is a copy of
            a leaf therefore has |S U G| == |G| == |S| to the last bit, and KIJ 1.0.
          * deltas over the window: _window_delta (ties to the larger k).
        A backend without cross_cards is a ValueError.
        -> dict: ks, sample [ns][K], genome [n][K], pair [ns][n][K], whole [K] (the universe), with [ns][K] (the universe
        and the sample), and per name of (sample, genome, pair, whole, with) `<name>_delta` and `<name>_k` of that shape less K"""
        u = self._universe(fastas, mink, maxk)
        for entry in ("cross_cards", "sample_sketches", "sample_cards"):
            if not hasattr(u.be, entry):
                raise ValueError(f"the backend {getattr(u.be, 'name', type(u.be).__name__)} has no {entry}: "
                                 "the samples are placed by one rectangle of unions over the leaf slab")
        ns, n, K = len(samples), u.n, len(u.ks)
        paths = u.paths
        regs = np.asarray(u.be.sample_sketches(list(samples), u.lo, u.hi), dtype=np.uint8).reshape(ns, K, -1)
        rows = np.concatenate([regs, np.zeros((1,) + regs.shape[1:], dtype=np.uint8)])
        pair = np.asarray(u.be.cross_cards(rows, paths), dtype=np.float64).reshape(ns + 1, n, K)
        merged = paths
        if set(fastas) == {leaf.fastas[0] for leaf in self.leaf_nodes()} and self.root.ngen > 1:
            self.root.ksweep_update_node(u.lo, u.hi)
            root = [self.root.ksketches[0].sfp.with_k(k) for k in u.ks]
            if all(sketch_exists(p) for p in root):
                merged = [root]
        whole = np.asarray(u.be.cross_cards(rows, merged, merged=True), dtype=np.float64).reshape(ns + 1, K)
        out = {"ks": u.ks, "sample": np.asarray(u.be.sample_cards(regs.reshape(ns * K, -1)), dtype=np.float64).reshape(ns, K),
               "genome": pair[ns], "pair": pair[:ns], "whole": whole[ns], "with": whole[:ns]}
        for name in ("sample", "genome", "pair", "whole", "with"):
            cards = out[name]
            flat = [_window_delta(c, u.ks) for c in cards.reshape(-1, K)]
            out[name + "_delta"] = np.array([d for d, _ in flat], dtype=np.float64).reshape(cards.shape[:-1])
            out[name + "_k"] = np.array([k for _, k in flat], dtype=np.int64).reshape(cards.shape[:-1])
        return out

    # ---- batched GPU union schedules ------------------------------------------------------------------
    def _table_window(self, experiment):
        """[lo, hi] of a union table for climbs over this tree's leaves: the --ksweep window, or a hill-climb's guess -- the
        climbs stay within a few k of the leaves' and the root's argmax (capped at 32 for dashing, allow_k64 or not; at the
        engine's 64 for exact trees)."""
        if experiment["ksweep"] is not None:
            lo, hi = experiment["ksweep"]
        else:
            lo = max(1, min(leaf.bestk for leaf in self.leaf_nodes()) - 2)
            hi = self.root_k() + 3
            if experiment["tool"] == "dashing":
                hi = min(hi, 32)
            else:
                hi = min(hi, 64)      # (exact trees: the engine's k <= 64)
        return int(lo), int(hi)

    def _universe(self, fastas, lo, hi):
        """What every analysis over a set of this tree's leaf FASTAs and a k window starts from (_Universe)"""
        return _Universe(self, fastas, lo, hi)

    def _leaf_files(self, leaves, lo, hi):
        """Make sure every leaf has its sketch file for k in [lo, hi] (one fused GPU pass per leaf)
        and return the paths as [leaf][k]."""
        rows = []
        for leaf in leaves:
            before = set(leaf.experiment["baseset"])
            leaf.ksweep_update_node(lo, hi)
            # ksweep_update_node notes every k of the range in the experiment's base set, as the reference's does
            # (lib/huffman_dandd.py:174) -- there every such k is then visited (node_ksweep) and registered.  This
            # window is a prefetch of OURS: a k the search never visits must not reach `save`, whose sketch/DB table
            # (lib/huffman_dandd.py:503) looks every base up and would die on it (hill-climb `progressive` did).
            # In a hill-climb run the reference never calls it at all: nothing of the window stays on the record.
            fresh = leaf.experiment["baseset"] - before
            if leaf.experiment.get("ksweep") is not None:
                fresh = {b for b in fresh if b not in self.speciesinfo.sketchinfo}
            leaf.experiment["baseset"].difference_update(fresh)
            tmpl = leaf.ksketches[0].sfp
            rows.append([tmpl.with_k(k) for k in range(lo, hi + 1)])
        return rows

    def prefetch_union_cards(self, groups, lo, hi, experiment):
        """Cardinalities of the unions `groups` (lists of leaf nodes) for k in [lo, hi], computed by ONE batched GPU launch
        instead of one union + one card per (set, k): every pair when all groups are pairs, else every prefix of every group
        that holds all leaves (an ordering).  -> UnionTable, or None when the backend has no batch entry points (the CPU
        checkers used in tests).  The caller walks its rows (_FlatUnion), which puts them in the cardinality cache."""
        be = backend_for(experiment)
        if lo < 1 or hi < lo or not groups or os.environ.get("DD_NO_PREFETCH"):
            return None
        pair_mode = all(len(g) == 2 for g in groups)
        if not hasattr(be, "pairwise_cards" if pair_mode else "progressive_cards"):
            return None
        leaves = []
        seen = set()
        for g in groups:
            for leaf in g:
                if id(leaf) not in seen:
                    seen.add(id(leaf))
                    leaves.append(leaf)
        index = {id(leaf): i for i, leaf in enumerate(leaves)}
        paths = self._leaf_files(leaves, lo, hi)
        if pair_mode:
            table, orders = _cards_or_wide(be, "pairwise_cards", paths), None
        else:
            ords = [[index[id(leaf)] for leaf in g] for g in groups if len(g) == len(leaves)]
            if not ords:
                return None
            table, orders = _cards_or_wide(be, "progressive_cards", paths, ords), {tuple(o): i for i, o in enumerate(ords)}
        if table is None:             # (the backend has no schedule for this many leaves: the object path)
            return None
        experiment["prefetched"] = True
        return UnionTable(table, lo, hi, index, orders)

    # ---- progressive unions (lib/huffman_dandd.py:574-663) -------------------------------------------
    def progressive_fastas(self, flist_loc=None):
        """The FASTAs a `progressive` run covers, in its order (lib/huffman_dandd.py:574-588)."""
        fastas = self.fastas
        fastas.sort()
        if flist_loc:
            with open(flist_loc) as f:
                wanted = [line.strip() for line in f]
            present = set(fastas)
            fastas = [f for f in wanted if f in present]
        return fastas

    def orderings_list(self, ordering_file=None, flist_loc=None, count=0):
        fastas = self.progressive_fastas(flist_loc)
        if count == 1:
            return fastas, [tuple(range(len(fastas)))]
        default = os.path.join(self.speciesinfo.sketchdir, f"{self.speciesinfo.tag}_{len(fastas)}_orderings.pickle")
        ordering_file = ordering_file or default
        orderings = set()
        if os.path.exists(ordering_file):
            with open(ordering_file, "rb") as f:
                orderings = pickle.load(f)
            if count == 0:
                return fastas, list(orderings)
            if count <= len(orderings):
                return fastas, list(orderings)[:count]
        elif count < 1:
            raise ValueError("You must provide a value for count when there is no default ordering file")
        orderings = permute(len(fastas), count, preexist=orderings, verbose=self.experiment["verbose"])
        with open(ordering_file, "wb") as f:
            pickle.dump(orderings, f)
        return fastas, list(orderings)

    def progressive_wrapper(self, flist_loc=None, count=30, ordering_file=None, step=1, debug=False):
        fastas, orderings = self.orderings_list(ordering_file=ordering_file, flist_loc=flist_loc, count=count)
        return self.progressive_union(flist=fastas, orderings=orderings, step=step)

    def progressive_union(self, flist, orderings, step):
        spider = DeltaSpider(fasta_files=flist, speciesinfo=self.speciesinfo, experiment=self.experiment)
        # all prefix unions of all orderings in one GPU launch (running max == flat union)
        sched = None
        if step == 1 and len(flist) > 1 and not self.experiment.get("safety"):
            by_fasta = {leaf.fastas[0]: leaf for leaf in spider.leaf_nodes()}
            groups = [[by_fasta[spider.fastas[j]] for j in ordering] for ordering in orderings]
            sched = spider.prefetch_union_cards(groups, *spider._table_window(self.experiment), self.experiment)
        results, summary = [], []
        for i, ordering in enumerate(orderings):
            if self.experiment["verbose"]:
                print(f"Now sweeping for ordering {i + 1}")
            rows, srows = spider.sketch_ordering(ordering, ordering_number=i + 1, step=step, schedule=sched)
            results.extend(rows)
            summary.extend(srows)
            self.speciesinfo.save_references(fast=self.experiment["fast"])
            self.speciesinfo.save_cardkey(tool=self.experiment["tool"], fast=self.experiment["fast"])
        self.experiment.pop("prefetched", None)  # the trust flag must not outlive this run (the tree is pickled)
        return results, summary

    def sketch_ordering(self, ordering, ordering_number, step=1, schedule=None):
        """Flat union of every prefix of the ordering (NOT previous union + one)."""
        krange = self.experiment["ksweep"] or (self.mink, self.maxk)
        lo, hi = int(krange[0]), int(krange[1])
        rows, summary = [], []
        leaves = self.leaf_nodes()
        # the schedule's table holds this ordering: every prefix is a row of numbers, not a SubSpider of objects (_FlatUnion)
        o = None
        if schedule is not None and step == 1:
            by_fasta = {leaf.fastas[0]: leaf for leaf in leaves}
            key = tuple(schedule.index.get(id(by_fasta.get(self.fastas[j]))) for j in ordering)
            o = schedule.orders.get(key)
        for i in range(1, len(ordering) + 1):
            if i % step:
                continue
            prefix = [self.fastas[j] for j in ordering[:i]]
            if o is not None:
                inside = set(prefix)
                kids = [leaf for leaf in leaves if leaf.fastas[0] in inside]      # tree order, as nodes_from_fastas gives them
                sub = _FlatUnion(self, kids, self.experiment, schedule, schedule.table[o, i - 1])
                if self.experiment["ksweep"] is None:
                    sub.find_delta(self.speciesinfo.kstart)
                    sub.fill()
                    delta = sub.delta
                else:
                    sub.node_ksweep(lo, hi)
                    delta = None
                rows.append({"ngen": i, "kval": sub.bestk, "delta": delta, "ordering": ordering_number, "fastas": prefix})
                summary.extend(sub.summarize(lo, hi, ordering_number))
                continue
            sub = SubSpider(self.nodes_from_fastas(prefix), self.speciesinfo, self.experiment)
            sub.ksweep(mink=lo, maxk=hi)
            rows.append({"ngen": i, "kval": sub.root_k(), "delta": sub.delta, "ordering": ordering_number,
                         "fastas": prefix})
            summary.extend(sub.root.summarize(mink=lo, maxk=hi, ordering_number=ordering_number))
        return rows, summary

    # ---- K-independent Jaccard (lib/huffman_dandd.py:666-695) -----------------------------------------
    def pairwise_spiders(self, sublist=(), mink=0, maxk=0, jaccard=True):
        leaves = list(sublist) or self.leaf_nodes()
        pair_exp = dict(self.experiment)
        pair_exp.update({"fast": True, "safe": False, "ksweep": None})
        if jaccard and (mink == 0 or maxk == 0):
            if self.experiment["ksweep"]:
                mink, maxk = self.experiment["ksweep"]
                print("WARNING: If EITHER minimum OR maximum k are not provided with --mink and --maxk flags, "
                      "DandD will default to the --ksweep values embedded in the delta-tree input.")
            else:
                print("WARNING: If BOTH minimum AND maximum k are not provided either by the input delta-tree or "
                      "using --mink and --maxk, the --jaccard flag will be ignored.")
                jaccard = False
        kij_rows, j_rows = [], []
        # every 2-way union of every pair at every k in one GPU launch
        sched = None
        if mink and maxk and len(leaves) > 1:
            pairs = [[a, b] for i, a in enumerate(leaves) for b in leaves[i + 1:]]
            sched = self.prefetch_union_cards(pairs, int(mink), min(int(maxk), 64), pair_exp)
            if sched is not None and (int(maxk) > 64 or pair_exp.get("safety")):
                # (--safe, or ks beyond the table: the object path below, its union cardinalities cached from the table)
                for a, b in pairs:
                    tmpl = SketchPath([a.fastas[0], b.fastas[0]], 0, self.speciesinfo, pair_exp)
                    _cache_row(self.speciesinfo.cardkey, tmpl, sched.table[sched.index[id(a)], sched.index[id(b)]], sched.lo)
                sched = None
        if sched is not None:
            # ... and every pair's summary from that table (_FlatUnion): the steps SubSpider + find_delta + kij_summarize +
            # jaccard_summarize take (lib/huffman_dandd.py:685-690, 772-815), in the same order -- the climbs move
            # speciesinfo.kstart, which the next pair starts from --, without a SubSpider, a node and a Sketch per (pair, k)
            table, index = sched.table, sched.index
            if jaccard:
                for leaf in leaves:
                    leaf.node_ksweep(mink=mink, maxk=maxk)     # (once per leaf: what every pair's ksweep asks of its two leaves)
                j_rows = RowTable(("A", "B", "Atitle", "Btitle", "kval", "Acard", "Bcard", "ABcard", "jaccard"))
                jc = j_rows.cols
                ks = list(range(mink, maxk + 1))
                leaf_cards = {id(leaf): [leaf.ksketches[k].card for k in ks] for leaf in leaves}
            for i, a in enumerate(leaves):
                for b in leaves[i + 1:]:
                    pair = _FlatUnion(self, [a, b], pair_exp, sched, table[index[id(a)], index[id(b)]])
                    pair.find_delta(self.speciesinfo.kstart)       # SubSpider.__init__ ...
                    pair.fill()
                    pair.find_delta(self.root_k())                 # ... and the climb from the tree's own argmax-k
                    if pair.bestk > 0:
                        pair.touch(pair.bestk)
                    a.update_node(a.bestk)
                    b.update_node(b.bestk)
                    x, y = (a, b) if [a.node_title, b.node_title] == sorted([a.node_title, b.node_title]) else (b, a)
                    row = {"A": x.fastas[0], "B": y.fastas[0], "Adelta": x.delta, "Bdelta": y.delta, "Ak": x.bestk,
                           "Bk": y.bestk, "ABdelta": pair.delta, "ABk": pair.bestk, "Atitle": x.node_title,
                           "Btitle": y.node_title}
                    row["KIJ"] = (row["Adelta"] + row["Bdelta"] - row["ABdelta"]) / row["ABdelta"]
                    kij_rows.append(row)
                    if jaccard:
                        pair.node_ksweep(mink, maxk)
                        # tree order, never swapped (lib/huffman_dandd.py:804); a column at a time
                        ac, bc, abc = leaf_cards[id(a)], leaf_cards[id(b)], [pair.card(k) for k in ks]
                        nk = len(ks)
                        jc["A"] += [a.fastas[0]] * nk
                        jc["B"] += [b.fastas[0]] * nk
                        jc["Atitle"] += [a.node_title] * nk
                        jc["Btitle"] += [b.node_title] * nk
                        jc["kval"] += ks
                        jc["Acard"] += ac
                        jc["Bcard"] += bc
                        jc["ABcard"] += abc
                        jc["jaccard"] += [(x + y - z) / z for x, y, z in zip(ac, bc, abc)]
            return kij_rows, j_rows
        for i, a in enumerate(leaves):
            for b in leaves[i + 1:]:
                pair = SubSpider([a, b], self.speciesinfo, pair_exp)
                pair.root.find_delta(self.root_k())
                kij_rows.append(pair.kij_summarize())
                if jaccard:
                    pair.ksweep(mink=mink, maxk=maxk)
                    j_rows.extend(pair.jaccard_summarize(mink=mink, maxk=maxk))
        return kij_rows, j_rows

    def prepare_AFproject(self, kijsummary, jsummary):
        tool = self.experiment["tool"]
        out = set()
        for d in kijsummary:
            out.add((tool, d["Atitle"], d["Btitle"], 0, d["KIJ"], d["Ak"], d["Bk"], d["ABk"]))
        for d in jsummary:
            out.add((tool, d["Atitle"], d["Btitle"], d["kval"], d["jaccard"], None, None, None))
        return list(out)


def write_phylip(tuples, path, k=0):
    """Lower-triangular PHYLIP distance matrix (distance = 1 - similarity) of the `--afproject` tuples
    (tool, name1, name2, k, value, k1, k2, k12) at one k -- k = 0 selects the K-independent Jaccard rows.  The
    format the reference's helper hands to `fneighbor` (helpers/allpairs.py:182-207: count line, then one row per
    name in sorted order holding the distances to the names before it)."""
    recs, names = {}, set()
    for _tool, a, b, kk, value, _k1, _k2, _k12 in tuples:
        if kk != k:
            continue
        names.update((a, b))
        recs[(a, b)] = recs[(b, a)] = 1 - value
    if not recs:
        raise ValueError(f"no pair at k={k}")
    names = sorted(names)
    with open(path, "wt") as f:
        print(len(names), file=f)
        for i, a in enumerate(names):
            print(" ".join(map(str, [a] + [recs[(a, b)] for b in names[:i]])), file=f)
    return names


def _window_delta(cards, ks):
    """delta over a k window: max of card / k, ties going to the larger k (the hill-climb's `<=`; ordering_expectations
    states the same rule for all its rows at once) -> (delta, k)"""
    best, bestk = 0, 0
    for c, k in zip(cards, ks):
        if best <= c / k:
            best, bestk = c / k, k
    return best, bestk


def _greedy_pick(cards, ks, mode):
    """The greedy selection rule (include/dandd_hip.h: dd_greedy): among the candidates' card rows, in tie-break order, the
    index of the one with the largest (mode "max") or smallest ("min") window delta; equal deltas go to the earlier one."""
    pick, best = 0, _window_delta(cards[0], ks)[0]
    for r in range(1, len(cards)):
        d = _window_delta(cards[r], ks)[0]
        if d > best if mode == "max" else d < best:
            pick, best = r, d
    return pick


def _greedy_walk(card_of, n, nfixed, steps, mode, ks):
    """The walk of dd_greedy over card_of(chosen, c) -> the cards of the union of items `chosen` and c at every k of ks:
    items 0..nfixed-1 are given, then _greedy_pick among the items not yet chosen, in index order.
    -> (order [steps], cards [steps][K])"""
    left = list(range(nfixed, n))
    order, cards = [], []
    for j in range(steps):
        rows = [j] if j < nfixed else left
        got = [[float(c) for c in card_of(order, c)] for c in rows]
        pick = 0 if j < nfixed else _greedy_pick(got, ks, mode)
        order.append(rows[pick])
        cards.append(got[pick])
        if j >= nfixed:
            del left[pick]
    return order, cards


def abba_expectations(delta):
    """Exact expectations over all n! orderings of n items from delta[mask] of every subset (delta[0] = 0; n = log2 of the
    length).  A prefix of an ordering is a subset P, and the item b that follows it adds delta(P | b) - delta(P); every
    subset of size s stands for s! (n - s)! orderings of its prefix and suffix.
      growth      [n][5]: per ngen 1..n the count, mean, population SD, min and max of delta over the subsets of that size
                  (= the ngen-th prefix over all orderings)
      contrib     [n][3]: per item g the mean of its increment over all orderings (weights s! (n - s - 1)! / n! for |P| = s),
                  and its min and max over all P not holding g
      before, after [a][b][n]: per ordered pair (a, b) and b's position s (1..n), the mean of b's increment over the orderings
                  with a before b (P holds a), and with a after b; nan where there are none (s = 1 before, s = n after)
      before_all, after_all [a][b]: the same over all n! / 2 orderings of each side
    No Python loop over subsets or orderings."""
    delta = np.asarray(delta, dtype=np.float64)
    n = int(delta.size).bit_length() - 1
    if delta.size != 1 << n or n < 1:
        raise ValueError(f"{delta.size} deltas: not 2^n of n >= 1 items")
    masks = np.arange(1 << n, dtype=np.int64)
    size = np.zeros(1 << n, dtype=np.int64)
    for i in range(n):
        size += (masks >> i) & 1
    growth = np.zeros((n, 5))
    order = np.argsort(size, kind="stable")
    bounds = np.searchsorted(size[order], np.arange(n + 2))
    for ng in range(1, n + 1):
        v = delta[order[bounds[ng]:bounds[ng + 1]]]
        growth[ng - 1] = (v.size, v.mean(), v.std(), v.min(), v.max())
    comb = np.array([[float(_comb(a, b)) for b in range(n + 1)] for a in range(n + 1)])
    contrib = np.zeros((n, 3))
    before = np.full((n, n, n), np.nan)
    after = np.full((n, n, n), np.nan)
    before_all = np.full((n, n), np.nan)
    after_all = np.full((n, n), np.nan)
    steps = np.arange(1, n + 1)
    for b in range(n):
        P = masks[((masks >> b) & 1) == 0]                    # every subset without b: b's prefix at step |P| + 1
        inc = delta[P | (1 << b)] - delta[P]
        onehot = np.zeros((P.size, n))
        onehot[np.arange(P.size), size[P]] = inc              # row P: its increment in the column of its size
        total = onehot.sum(axis=0)                            # [s - 1]: sum over |P| = s - 1
        contrib[b] = ((total / (n * comb[n - 1, :n])).sum(), inc.min(), inc.max())
        member = ((P[None, :] >> np.arange(n)[:, None]) & 1).astype(np.float64)   # [a][P]: a in P
        sb = member @ onehot                                  # [a][s - 1]: sums with a before b
        sa = total[None, :] - sb
        nb = comb[n - 2, np.maximum(steps - 2, 0)] * (steps >= 2)          # subsets per step with a in P, b not
        na = comb[n - 2, np.minimum(steps - 1, n - 2)] * (steps <= n - 1)  # ... with neither
        with np.errstate(invalid="ignore", divide="ignore"):
            mb = np.where(nb > 0, sb / np.where(nb > 0, nb, 1), np.nan)
            ma = np.where(na > 0, sa / np.where(na > 0, na, 1), np.nan)
        for a in range(n):
            if a == b:
                continue
            before[a, b], after[a, b] = mb[a], ma[a]
            # orderings at step s: (s - 1) (n - 2)! with a before, (n - s) (n - 2)! with a after; n! / 2 each in all
            before_all[a, b] = np.nansum(mb[a] * (steps - 1)) * 2 / (n * (n - 1))
            after_all[a, b] = np.nansum(ma[a] * (n - steps)) * 2 / (n * (n - 1))
    return dict(n=n, size=size, growth=growth, contrib=contrib, before=before, after=after, before_all=before_all,
                after_all=after_all)


def _comb(a, b):
    from math import comb
    return comb(a, b) if 0 <= b <= a else 0


class SubSpider(DeltaTree):
    """Existing leaf nodes under one new union node."""

    def __init__(self, leafnodes, speciesinfo, experiment):
        self.speciesinfo = speciesinfo
        self.fastahex = speciesinfo.fastahex
        self.experiment = experiment
        self.kstart = speciesinfo.kstart
        if experiment["ksweep"] is not None:
            self.mink, self.maxk = experiment["ksweep"]
        self._build_tree(leafnodes)
        self.root = self._dt[-1]
        self.fastas = self.root.fastas
        self.ngen = len(self.fastas)
        self.delta = None
        self.fill_tree()
        if experiment["ksweep"] is None:
            self.delta = self.root_delta()
        else:
            self.mink, self.maxk = experiment["ksweep"]

    def _build_tree(self, leafnodes):
        kids = list(leafnodes)
        body = DeltaTreeNode("_".join(os.path.basename(c.node_title) for c in kids), kids, self.speciesinfo,
                             self.experiment, progeny=[leaf for c in kids for leaf in c.progeny])
        if self.experiment["ksweep"] is None:
            body.find_delta(kval=self.speciesinfo.kstart)
        else:
            body.node_ksweep(mink=self.mink, maxk=self.maxk)
        self.mink, self.maxk = body.mink, body.maxk
        self._dt = kids + [body]

    def kij_summarize(self):
        if len(self.fastas) != 2:
            raise ValueError("KIJ can only be calculated on spider/trees with 2 children")
        self.root.update_node(self.root.bestk)
        a, b = self._dt[0], self._dt[1]
        a.update_node(a.bestk)
        b.update_node(b.bestk)
        if [a.node_title, b.node_title] != sorted([a.node_title, b.node_title]):
            a, b = b, a
        row = {"A": a.fastas[0], "B": b.fastas[0], "Adelta": a.delta, "Bdelta": b.delta, "Ak": a.bestk,
               "Bk": b.bestk, "ABdelta": self.root.delta, "ABk": self.root.bestk, "Atitle": a.node_title,
               "Btitle": b.node_title}
        row["KIJ"] = (row["Adelta"] + row["Bdelta"] - row["ABdelta"]) / row["ABdelta"]
        return row

    def jaccard_summarize(self, mink=2, maxk=32):
        if len(self.fastas) != 2:
            raise ValueError("KIJ can only be calculated on spider/trees with 2 or more children")
        a, b = self._dt[0], self._dt[1]  # tree order, never swapped (lib/huffman_dandd.py:804)
        self.ksweep(mink=mink, maxk=maxk)
        rows = []
        for k in range(mink, maxk + 1):
            row = {"A": a.fastas[0], "B": b.fastas[0], "Atitle": a.node_title, "Btitle": b.node_title, "kval": k,
                   "Acard": a.ksketches[k].card, "Bcard": b.ksketches[k].card, "ABcard": self.root.ksketches[k].card}
            row["jaccard"] = (row["Acard"] + row["Bcard"] - row["ABcard"]) / row["ABcard"]
            rows.append(row)
        return rows


class DeltaSpider(DeltaTree):
    """All leaves directly under one root."""

    def __init__(self, fasta_files, speciesinfo, experiment, padding=False):
        super().__init__(fasta_files=fasta_files, speciesinfo=speciesinfo, experiment=experiment,
                         nchildren=len(fasta_files), padding=padding)


def create_delta_tree(tag, genomedir, sketchdir, kstart, nchildren=None, registers=0, flist_loc=None,
                      canonicalize=True, tool="dashing", debug=False, nthreads=0, safety=False, fast=False,
                      verbose=False, ksweep=None, lowmem=False):
    experiment = {"registers": registers, "canonicalize": canonicalize, "tool": tool, "nthreads": int(nthreads),
                  "debug": debug, "baseset": set(), "safety": safety, "fast": fast, "verbose": verbose,
                  "ksweep": ksweep, "lowmem": lowmem}
    speciesinfo = Catalog(tag=tag, genomedir=genomedir, sketchdir=sketchdir, kstart=kstart, tool=tool,
                          flist_loc=flist_loc)
    if flist_loc:
        with open(flist_loc) as f:
            fastas = [line.strip() for line in f]
    elif genomedir and os.path.exists(genomedir):
        fastas = speciesinfo.retrieve_fasta_files(full=True)
    else:
        raise ValueError("You must provide either an existing directory of fastas or a file listing the paths "
                         f"of the desired fastas. The directory you provided was {genomedir}.")
    fastas.sort()
    if nchildren:
        tree = DeltaTree(fasta_files=fastas, speciesinfo=speciesinfo, nchildren=nchildren, experiment=experiment)
    else:
        tree = DeltaSpider(fasta_files=fastas, speciesinfo=speciesinfo, experiment=experiment)
    speciesinfo.save_cardkey(tool=tool, fast=fast)
    speciesinfo.save_references(fast=fast)
    return tree

"""The reference of the wide exact union schedules (tests/test_exact_wide.py, tests/test_gpu_exact_wide.py): a Python set of
pyref.kmers per genome and k, and from those sets every pair's union, every ordering's prefix unions and every leave-out
complement -- as the arrays Engine.exact_wide_pairwise / _progressive / _leave_out return.  count() is the plain union of the
sets; the tables come from the same sets laid out as a membership matrix (one row per distinct k-mer, one column per genome),
so that 255 genomes take a moment and not a minute.  Nothing here reads the code under test."""
import numpy as np

import pyref


class WideRef:
    def __init__(self, fas, canonical=True):
        self.fas, self.canonical = [bytes(f) for f in fas], bool(canonical)
        self.n = len(self.fas)
        self._sets, self._matrix = {}, {}

    def sets(self, k):
        """[n] sets of the genomes' k-mers"""
        k = int(k)
        if k not in self._sets:
            memo = {}           # (a duplicate file is tokenised once)
            self._sets[k] = [memo.setdefault(fa, frozenset(pyref.kmers(fa, k, self.canonical))) for fa in self.fas]
        return self._sets[k]

    def count(self, members, k):
        """|union of the members' k-mers|, by set union"""
        sets = self.sets(k)
        out = set()
        for i in members:
            out |= sets[int(i)]
        return len(out)

    def matrix(self, k):
        """bool [distinct k-mers][n]: which genomes hold each"""
        k = int(k)
        if k not in self._matrix:
            sets = self.sets(k)
            index = {x: r for r, x in enumerate(sorted(set().union(*sets)))}
            m = np.zeros((len(index), self.n), dtype=bool)
            for g, s in enumerate(sets):
                m[[index[x] for x in s], g] = True
            self._matrix[k] = m
        return self._matrix[k]

    def pairwise(self, kmin, kmax):
        """uint64 [n][n][K]: |A_i U A_j|, the diagonal |A_i|"""
        out = np.zeros((self.n, self.n, kmax - kmin + 1), dtype=np.uint64)
        for kk, k in enumerate(range(kmin, kmax + 1)):
            m = self.matrix(k).astype(np.float64)           # (counts far below 2^53: the products are exact)
            own = m.sum(axis=0)
            both = m.T @ m                                  # |A_i n A_j|
            out[:, :, kk] = np.rint(own[:, None] + own[None, :] - both).astype(np.uint64)
            out[np.arange(self.n), np.arange(self.n), kk] = np.rint(own).astype(np.uint64)
        return out

    def progressive(self, kmin, kmax, orderings):
        """uint64 [o][n][K]: |union of the first j+1 genomes of ordering o|"""
        out = np.zeros((len(orderings), self.n, kmax - kmin + 1), dtype=np.uint64)
        for kk, k in enumerate(range(kmin, kmax + 1)):
            m = self.matrix(k)
            for o, order in enumerate(orderings):
                out[o, :, kk] = np.logical_or.accumulate(m[:, list(order)], axis=1).sum(axis=0)
        return out

    def leave_out(self, kmin, kmax, group, ngroups=None):
        """uint64 [G+1][K]: row g the union of the genomes outside group g (-1: never left out), row G the union of all"""
        group = [int(g) for g in group]
        G = max(group) + 1 if ngroups is None else int(ngroups)
        out = np.zeros((G + 1, kmax - kmin + 1), dtype=np.uint64)
        for kk, k in enumerate(range(kmin, kmax + 1)):
            m = self.matrix(k)
            holders = m.sum(axis=1)
            for g in range(G + 1):                          # what is lost with group g: the k-mers all of whose holders lie in it
                inside = m[:, [i for i in range(self.n) if group[i] == g]].sum(axis=1)
                out[g, kk] = len(m) - int((inside == holders).sum())
        return out

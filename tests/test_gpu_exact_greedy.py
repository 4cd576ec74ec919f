"""dd_exact_greedy on the MI355X: the steepest / flattest ordering of 17..64 genomes from one sort per k.  The truth is
Python sets of pyref.kmers, walked by deltatree._greedy_walk with _greedy_pick; `order` and every `card` cell are compared
with ==.  Sizes 17, 33 and 64 (both widths of the walk's bit loop), both modes, canonical and not, four k windows (64- and
128-bit keys, the genome's index in the key and in its own array), given starts, fewer steps than candidates, candidates
that are a permuted strict subset of the inputs, twins in both arrangements, streams whose lengths are no multiple of 64 and
differ between adjacent k, passes over parts of the k-mer space, a mask store that is too small (the error, the backend's
None, the command through the object path), the table of all subsets and dd_exact_progressive as cross-checks, the device
form, the argument rules, and `dandd greedy` one-shot and through `dandd serve` against the object path."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

import pyref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

MAX, MIN = 0, 1
WINDOWS = [(11, 13), (29, 32), (33, 35), (61, 64)]     # (key words, where the genome's index rides): (1, key) (1, array) (2, key) (2, array)
TWINS, SHORT, POLY_A = (2, 9), 5, 7                    # genome 9 is genome 2 byte for byte; 5 is 9 bases long; 7 is A x 4300; the last is empty


def genomes(n, seed):
    """An ancestor of 3000 bp and n genomes cut from its start, 300..3000 bp, with 3 % substitutions each, in two records with an
    N and a lowercase stretch; the special ones of TWINS, SHORT, POLY_A, and the last genome empty."""
    rng = np.random.default_rng(seed)
    anc = rng.integers(0, 4, 3000)
    out = []
    for i in range(n):
        length = 3000 if i == 1 else 300 + (i * 97) % 420
        s = anc[:length].copy()
        mut = rng.random(length) < 0.03
        s[mut] = rng.integers(0, 4, int(mut.sum()))
        t = "".join("ACGT"[c] for c in s)
        a, b = length // 3, 2 * length // 3
        t = t[:a] + "N" + t[a:b].lower() + t[b:]
        cut = [0, len(t) // 2 + i, len(t)]
        out.append("".join(f">g{i}_r{r}\n" + "\n".join(t[x:y][j:j + 70] for j in range(0, y - x, 70)) + "\n"
                           for r, (x, y) in enumerate(zip(cut, cut[1:]))).encode())
    out[TWINS[1]] = out[TWINS[0]]
    out[SHORT] = b">short\nACGTTGCAT\n"
    out[POLY_A] = b">polyA\n" + b"A" * 4300 + b"\n"                  # one k-mer, 4300 - k + 1 times: its run crosses chunks of 2048 slots
    out[n - 1] = b""
    return out


def write(tmp_path, fas, tag="g"):
    paths = []
    for i, f in enumerate(fas):
        p = str(tmp_path / f"{tag}{i:02d}.fa")
        with open(p, "wb") as fh:
            fh.write(f)
        paths.append(p)
    return paths


_SETS = {}


def kmer_sets(n, canonical, k):
    """[i] = the set of k-mers of genome i of genomes(n, 100 + n): computed once per (n, canonical, k), never changed"""
    key = (n, canonical, k)
    if key not in _SETS:
        fas = genomes(n, 100 + n)
        _SETS[key] = [frozenset(pyref.kmers(fa, k, canonical)) for fa in fas]
    return _SETS[key]


def set_walk(sets_by_k, ks, mode, cand, nfixed, nsteps):
    """deltatree._greedy_walk over Python sets: item r of the walk is input cand[r]; sets_by_k[kk][i] the k-mers of input i.
    -> (order as inputs, cards [nsteps][K] as ints)"""
    from dandd_amd.host.deltatree import _greedy_walk
    state = {"n": 0, "u": [set() for _ in ks]}

    def card_of(chosen, c):
        for r in chosen[state["n"]:]:                               # (the walk only ever appends to `chosen`)
            for kk in range(len(ks)):
                state["u"][kk] |= sets_by_k[kk][cand[r]]
        state["n"] = len(chosen)
        return [len(state["u"][kk]) + len(sets_by_k[kk][cand[c]] - state["u"][kk]) for kk in range(len(ks))]
    order, cards = _greedy_walk(card_of, len(cand), nfixed, nsteps, "max" if mode == MAX else "min", ks)
    return [cand[r] for r in order], [[int(c) for c in row] for row in cards]


def check(eng, paths, sets_by_k, ks, mode, cand, nfixed, nsteps):
    order, card = eng.exact_greedy(paths, ks[0], ks[-1], mode, cand, nfixed, nsteps)
    n = len(paths)
    full = list(range(n)) if cand is None else [int(c) for c in cand]
    steps = len(full) if nsteps is None else nsteps
    assert order.dtype == np.int32 and order.shape == (steps,) and card.dtype == np.uint64 and card.shape == (steps, len(ks))
    worder, wcard = set_walk(sets_by_k, ks, mode, full, nfixed, steps)
    assert [int(x) for x in order] == worder, (mode, cand, nfixed, nsteps)
    assert [[int(v) for v in row] for row in card] == wcard, (mode, cand, nfixed, nsteps)
    assert order[:nfixed].tolist() == full[:nfixed]
    return [int(x) for x in order]


# ---- 1. the walk against Python sets -----------------------------------------------------------------------------------
@pytest.mark.parametrize("window", WINDOWS, ids=[f"k{a}-{b}" for a, b in WINDOWS])
@pytest.mark.parametrize("canonical", [True, False], ids=["canon", "nocanon"])
@pytest.mark.parametrize("n", [17, 33, 64])
def test_walk_matches_python_sets(engine_factory, tmp_path, n, canonical, window):
    eng = engine_factory(canonical=canonical)
    paths = write(tmp_path, genomes(n, 100 + n))
    ks = list(range(window[0], window[1] + 1))
    sets_by_k = [kmer_sets(n, canonical, k) for k in ks]
    # the streams: more masks than a workgroup of the walk takes, no stream a multiple of 64 long, adjacent ones of different
    # lengths -- a workgroup's range crosses from one k's stream into the next somewhere inside a load of 64
    lengths = [len(frozenset().union(*s)) for s in sets_by_k]
    assert sum(lengths) > 2 * 2048 and all(x % 64 for x in lengths) and all(a != b for a, b in zip(lengths, lengths[1:])), lengths
    assert sum(len(pyref.kmers(fa, ks[0], canonical)) for fa in genomes(n, 100 + n)) > 4 * 2048      # occurrences: several chunks of the sort
    assert not sets_by_k[0][SHORT] and not sets_by_k[0][n - 1] and len(sets_by_k[0][POLY_A]) == 1
    for mode in (MAX, MIN):
        order = check(eng, paths, sets_by_k, ks, mode, None, 0, None)
        assert sorted(order) == list(range(n))
        assert order.index(TWINS[0]) < order.index(TWINS[1])                  # of two identical genomes the earlier candidate
    assert eng.last_sketch_stats()[2] == 1
    # candidates: a permuted strict subset of the inputs, a given start, fewer steps than candidates
    rng = np.random.default_rng(n + window[0])
    cand = [int(x) for x in rng.permutation(n)[: n - 4]]
    for keep in (TWINS[0], TWINS[1], POLY_A):
        if keep not in cand:
            cand[cand.index(next(c for c in cand if c not in TWINS + (POLY_A,)))] = keep
    outside = set(range(n)) - set(cand)
    for mode, nfixed, nsteps in ((MAX, 1, len(cand)), (MIN, 3, len(cand) - 5), (MAX, 3, 3), (MIN, 0, 1)):
        order = check(eng, paths, sets_by_k, ks, mode, cand, nfixed, nsteps)
        assert not outside & set(order)
    # the twins the other way round: the one that now stands first in cand is taken first, and nothing else moves
    a, b = cand.index(TWINS[0]), cand.index(TWINS[1])
    swapped = list(cand)
    swapped[a], swapped[b] = swapped[b], swapped[a]
    for mode in (MAX, MIN):
        one = check(eng, paths, sets_by_k, ks, mode, cand, 0, len(cand))
        two = check(eng, paths, sets_by_k, ks, mode, swapped, 0, len(cand))
        first, second = (TWINS[0], TWINS[1]) if a < b else (TWINS[1], TWINS[0])
        assert one.index(first) < one.index(second) and two.index(second) < two.index(first)
        swap = {TWINS[0]: TWINS[1], TWINS[1]: TWINS[0]}
        assert two == [swap.get(x, x) for x in one]


# ---- 2. passes over parts of the k-mer space ----------------------------------------------------------------------------
def related(n, length, seed, rate=0.03):
    rng = np.random.default_rng(seed)
    anc = rng.integers(0, 4, length)
    out = []
    for i in range(n):
        s = anc.copy()
        mut = rng.random(length) < rate
        s[mut] = rng.integers(0, 4, int(mut.sum()))
        t = "".join("ACGT"[c] for c in s)
        out.append((f">r{i}\n" + "\n".join(t[j:j + 80] for j in range(0, length, 80)) + "\n").encode())
    return out


@pytest.mark.parametrize("canonical", [True, False], ids=["canon", "nocanon"])
def test_multi_pass_gives_the_same_walk(engine_factory, tmp_path, canonical):
    """17 genomes of 19 kbp, 323 000 occurrences, with a 1 MiB sort budget: a pass holds at most 65 536 k-mers, so at least
    three passes append to the stream of a k -- which dd_last_sketch_stats must report -- and the walk is the single-pass one."""
    eng = engine_factory(canonical=canonical)
    paths = write(tmp_path, related(17, 19_000, 17))
    assert "DD_EXACT_MB" not in os.environ
    for kmin, kmax in [(12, 13), (31, 33), (61, 62)]:
        for mode in (MAX, MIN):
            one = eng.exact_greedy(paths, kmin, kmax, mode, None, 2, 12)
            assert eng.last_sketch_stats()[2] == 1
            os.environ["DD_EXACT_MB"] = "1"
            try:
                many = eng.exact_greedy(paths, kmin, kmax, mode, None, 2, 12)
                passes = eng.last_sketch_stats()[2]
            finally:
                del os.environ["DD_EXACT_MB"]
            assert passes >= 3, (kmin, kmax, passes)
            assert np.array_equal(one[0], many[0]) and np.array_equal(one[1], many[1]), (kmin, kmax, mode)


# ---- 3. a mask store that is too small -----------------------------------------------------------------------------------
def test_mask_budget(engine_factory, tmp_path, monkeypatch):
    """17 unrelated genomes of 12 kbp at k = 15: about 204 000 distinct k-mers, more than the 131 072 masks of a 1 MiB store.
    The engine names the knob and returns nothing; the backend says None; `dandd greedy` then takes the object path and
    writes what it writes with the default budget."""
    from dandd_amd.engine import ENOMEM, EngineError
    from dandd_amd.host import cli, deltatree
    from dandd_amd.host.backend import HipExactBackend
    rng = np.random.default_rng(15)
    data = tmp_path / "data"
    data.mkdir()
    fas = [(f">u{i}\n" + "".join("ACGT"[c] for c in rng.integers(0, 4, 12_000)) + "\n").encode() for i in range(17)]
    paths = write(data, fas, tag="u")
    eng = engine_factory()
    want = eng.exact_greedy(paths, 15, 15, MAX)
    assert int(want[1][-1, 0]) > 131_072
    monkeypatch.setenv("DD_EXACT_MASKS_MB", "1")
    with pytest.raises(EngineError, match="DD_EXACT_MASKS_MB") as err:
        eng.exact_greedy(paths, 15, 15, MAX)
    assert err.value.code == ENOMEM and "131072" in str(err.value)
    monkeypatch.delenv("DD_EXACT_MASKS_MB")
    got = eng.exact_greedy(paths, 15, 15, MAX)                        # (the context is none the worse for it)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])

    class Spy(HipExactBackend):
        answers = []

        def greedy_cards(self, *args):
            got = super().greedy_cards(*args)
            Spy.answers.append(got)
            return got

    out = {}
    try:
        deltatree.set_backend_factory(lambda r, c: Spy(r, c))
        t = str(tmp_path / "t")
        cli.main(["tree", "-d", str(data), "-o", t, "-s", "u", "-k", "15", "--exact"])
        (pk,) = glob.glob(os.path.join(t, "*dtree.pickle"))
        for name, mb in (("default", None), ("small", "1")):
            if mb:
                monkeypatch.setenv("DD_EXACT_MASKS_MB", mb)
            Spy.answers = []
            d = str(tmp_path / name)
            cli.main(["greedy", "-d", pk, "-o", d, "--ksweep", "--mink", "15", "--maxk", "15", "--mode", "max", "--steps", "4"])
            assert len(Spy.answers) == 1 and (Spy.answers[0] is None) == bool(mb)
            out[name] = {os.path.basename(f): open(f, "rb").read() for f in glob.glob(os.path.join(d, "*greedy*"))}
    finally:
        deltatree.set_backend_factory(None)
    assert len(out["default"]) == 3 and out["small"] == out["default"]


# ---- 4. cross-checks against the schedules ------------------------------------------------------------------------------
def test_twelve_genomes_equal_a_walk_over_the_subset_table(engine_factory, tmp_path):
    from dandd_amd.host.deltatree import _greedy_walk
    eng = engine_factory()
    n, kmin, kmax = 12, 20, 23
    paths = write(tmp_path, genomes(n, 12))
    table = eng.exact_subsets(paths, kmin, kmax)
    ks = list(range(kmin, kmax + 1))
    for mode, name in ((MAX, "max"), (MIN, "min")):
        for nfixed in (0, 2):
            worder, wcards = _greedy_walk(lambda chosen, c: table[sum(1 << i for i in chosen) | 1 << c], n, nfixed, n, name, ks)
            order, card = eng.exact_greedy(paths, kmin, kmax, mode, None, nfixed, n)
            assert [int(x) for x in order] == worder
            assert np.array_equal(card, np.array(wcards, dtype=np.uint64))


def test_cards_equal_exact_progressive_of_the_ordering(engine_factory, tmp_path):
    """24 genomes of 20 kbp (235 chunks of sorted slots, a gains launch of 200 workgroups): card == dd_exact_progressive of the
    ordering the walk returned, at one k per key width"""
    eng = engine_factory()
    n = 24
    paths = write(tmp_path, related(n, 20_000, 24, rate=0.05))
    for k in (21, 40):
        for mode in (MAX, MIN):
            order, card = eng.exact_greedy(paths, k, k, mode)
            assert sorted(int(x) for x in order) == list(range(n))
            assert np.array_equal(card, eng.exact_progressive(paths, k, k, [order])[0])


def test_device_form_equals_file_form(engine_factory, torch_cuda, tmp_path):
    eng = engine_factory()
    n = 17
    fas = genomes(n, 100 + n)
    paths = write(tmp_path, fas)
    bufs = [torch_cuda.from_numpy(np.frombuffer(f + b"\0" * 16, dtype=np.uint8).copy()).cuda() for f in fas]
    ptrs, sizes = [b.data_ptr() for b in bufs], [len(f) for f in fas]
    cand = [int(x) for x in np.random.default_rng(3).permutation(n)[:14]]
    for kmin, kmax in WINDOWS:
        for mode in (MAX, MIN):
            a = eng.exact_greedy_device(ptrs, sizes, kmin, kmax, mode, cand, 2, 11)
            b = eng.exact_greedy(paths, kmin, kmax, mode, cand, 2, 11)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_inputs_without_a_token(engine_factory, tmp_path):
    """every input empty: every union is empty, and the ties go down the list of candidates"""
    eng = engine_factory()
    paths = write(tmp_path, [b""] * 17)
    order, card = eng.exact_greedy(paths, 11, 13, MAX, [4, 2, 16, 0], 1, 3)
    assert order.tolist() == [4, 2, 16] and not card.any()


# ---- 5. argument rules -----------------------------------------------------------------------------------------------------
def test_argument_rules(engine_factory, tmp_path):
    from dandd_amd.engine import EngineError
    eng = engine_factory()
    one = write(tmp_path, genomes(17, 117)[:1])
    three = one * 3
    with pytest.raises(EngineError, match="n=0 outside 1..64"):
        eng.exact_greedy([], 11, 11, MAX)
    with pytest.raises(EngineError, match="n=65 outside 1..64"):
        eng.exact_greedy(one * 65, 11, 11, MAX)
    with pytest.raises(EngineError, match="k range 0..11 outside 1..64"):
        eng.exact_greedy(three, 0, 11, MAX)
    with pytest.raises(EngineError, match="k range 60..65 outside 1..64"):
        eng.exact_greedy(three, 60, 65, MAX)
    with pytest.raises(EngineError, match="is a repeat"):
        eng.exact_greedy(three, 11, 11, MAX, [0, 1, 0])
    with pytest.raises(EngineError, match=r"cand\[1\]=3 outside 0..2"):
        eng.exact_greedy(three, 11, 11, MAX, [0, 3])
    with pytest.raises(EngineError, match=r"cand\[0\]=-1 outside 0..2"):
        eng.exact_greedy(three, 11, 11, MAX, [-1])
    with pytest.raises(EngineError, match="nfixed=2 outside 0..nsteps=1"):
        eng.exact_greedy(three, 11, 11, MAX, None, 2, 1)
    with pytest.raises(EngineError, match="nsteps=4 outside 1..ncand=3"):
        eng.exact_greedy(three, 11, 11, MAX, None, 0, 4)
    with pytest.raises(EngineError, match="nsteps=0 outside 1..ncand=3"):
        eng.exact_greedy(three, 11, 11, MAX, None, 0, 0)
    with pytest.raises(EngineError, match="mode=2"):
        eng.exact_greedy(three, 11, 11, 2)
    with pytest.raises(EngineError):
        eng.exact_greedy(one + [str(tmp_path / "missing.fa")], 11, 11, MAX)


# ---- 6. the command ---------------------------------------------------------------------------------------------------------
def test_cli_one_shot_and_served_equal_the_object_path(tmp_path, sock_dir, torch_cuda):
    """`greedy` on an exact tree of 17 tiny genomes over 3 k: one-shot and through `dandd serve`, every file byte for byte
    what the same command writes under DD_NO_PREFETCH=1, one SubSpider per step and candidate."""
    data = tmp_path / "data"
    data.mkdir()
    for i, fa in enumerate(related(17, 150, 170, rate=0.1)):
        (data / f"t{i:02d}.fasta").write_bytes(fa)
    (data / "t11.fasta").write_bytes((data / "t10.fasta").read_bytes())
    env = dict(os.environ, PYTHONHASHSEED="0")
    for name in ("DANDD_SERVER", "DD_NO_PREFETCH", "DD_EXACT_MASKS_MB"):
        env.pop(name, None)
    t = str(tmp_path / "t")
    subprocess.run([sys.executable, "-m", "dandd_amd.host.cli", "tree", "-d", str(data), "-o", t, "-s", "tiny", "-k", "10", "--exact"],
                   env=env, check=True, cwd=ROOT, timeout=600, capture_output=True)
    (pk,) = glob.glob(os.path.join(t, "*dtree.pickle"))
    basef = tmp_path / "base.txt"
    basef.write_text("t03.fasta\n")
    argv = ["greedy", "-d", pk, "--ksweep", "--mink", "9", "--maxk", "11", "-b", str(basef)]

    def files(d):
        return {os.path.basename(f): open(f, "rb").read() for f in glob.glob(os.path.join(d, "*greedy*"))}

    out = {}
    for name, extra in (("walk", {}), ("object", {"DD_NO_PREFETCH": "1"})):
        d = str(tmp_path / name)
        r = subprocess.run([sys.executable, "-m", "dandd_amd.host.cli", *argv, "-o", d], env=dict(env, **extra), cwd=ROOT, timeout=600,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out[name] = files(d)
    assert len(out["walk"]) == 4 and out["walk"] == out["object"]
    for mode in ("max", "min"):
        (txt,) = [v for f, v in out["walk"].items() if f.endswith(f"greedy_{mode}.txt")]
        names = [os.path.basename(x) for x in txt.decode().split()]
        assert len(names) == 17 and names[0] == "t03.fasta" and names.index("t10.fasta") < names.index("t11.fasta")
    sock = os.path.join(sock_dir, "eg.sock")
    srv = subprocess.Popen([sys.executable, "-m", "dandd_amd.host.cli", "serve", "--socket", sock, "--idle-exit", "120"],
                           env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
        assert "listening" in srv.stdout.readline()
        cenv = dict(env, DANDD_SERVER=sock, DANDD_SERVER_REQUIRED="1")
        via = str(tmp_path / "srv")
        r = subprocess.run([sys.executable, "-m", "dandd_amd.host.client", *argv, "-o", via], env=cenv, cwd=ROOT, timeout=600,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert files(via) == out["object"]
        from dandd_amd.host.client import request
        request(sock, {"op": "shutdown"})
        srv.wait(timeout=60)
    finally:
        if srv.poll() is None:
            srv.kill()
            srv.wait()

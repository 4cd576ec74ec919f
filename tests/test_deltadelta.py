"""`dandd deltadelta` on the CPU: delta(all) - delta(all but a group), every group of a tree in one command.

The schedule path (one leave-out table for every complement, the climbs walked on it) is checked against the object path
the reference takes (DeltaTree.find_delta_delta: one SubSpider per group, lib/huffman_dandd.py:559-566),
called group after group on a fresh copy of the same tree, and against tests/golden/ref_deltadelta.json, the values the
reference's own find_delta_delta returned (tests/golden/make_golden_deltadelta.py)."""
import csv
import io
import json
import os
import shutil
from contextlib import redirect_stdout

import numpy as np
import pytest

import hostcheck

NAMES = [f"g{i}.fasta" for i in range(5)]


class LeaveOutBackend(hostcheck.ScheduleBackend):
    """The schedule backend with leave_out_cards, brute force: oracle union over each complement, then oracle card."""
    name = "oracle+leave-out"
    calls = 0

    def leave_out_cards(self, leaf_paths, group):
        LeaveOutBackend.calls += 1
        slab = self._slab(leaf_paths)
        group = [int(g) for g in group]
        G, K = max(group) + 1, len(slab[0])
        out = np.zeros((G + 1, K))
        for g in range(G + 1):
            members = [i for i, x in enumerate(group) if x != g]
            for kk in range(K):
                out[g, kk] = self.orc.card(self.orc.union(*[slab[i][kk] for i in members]), self.log2m)
        return out


@pytest.fixture
def host():
    from dandd_amd.host import deltatree
    yield deltatree
    deltatree.set_backend_factory(None)


def _tree(work, host, registers=14, extra=()):
    from dandd_amd.host import cli
    data = os.path.join(work, "data")
    if not os.path.exists(data):
        shutil.copytree(os.path.join(hostcheck.GOLD, "fasta"), data)
    out = os.path.join(work, "t")
    os.makedirs(out, exist_ok=True)
    host.set_backend_factory(lambda r, c: hostcheck.OracleBackend(r, c))
    cli.main(["tree", "-d", data, "-o", out, "-s", "gold", "-k", "10", "-r", str(registers), *extra])
    return data, os.path.join(out, "gold_5_dashing_dtree.pickle")


def _rows(path):
    with open(path, newline="") as f:
        return list(csv.DictReader(f))


def _run(host, backend, argv):
    from dandd_amd.host import cli
    host.set_backend_factory(lambda r, c: backend(r, c))
    cli.main(["deltadelta", *argv])


def _object_path(host, pickle_path, subsets):
    """find_delta_delta one group at a time on a fresh copy of the tree, plain oracle backend (no schedules)"""
    from dandd_amd.host.compat import load_tree
    host.set_backend_factory(lambda r, c: hostcheck.OracleBackend(r, c))
    tree = load_tree(pickle_path)
    got = []
    for subset in subsets:
        buf = io.StringIO()
        with redirect_stdout(buf):
            dd = tree.find_delta_delta(subset)
        sub = [float(line.split(":")[1]) for line in buf.getvalue().splitlines() if line.startswith("Subtree Delta")]
        got.append({"deltadelta": dd, "delta_rest": sub[0], "delta_all": tree.delta, "kstart": tree.speciesinfo.kstart})
    return got


def test_schedule_path_equals_find_delta_delta(host, tmp_path):
    data, pk = _tree(str(tmp_path), host)
    want = _object_path(host, pk, [[os.path.join(data, n)] for n in NAMES])
    o = str(tmp_path / "dd")
    before = LeaveOutBackend.calls
    _run(host, LeaveOutBackend, ["-d", pk, "-o", o])
    assert LeaveOutBackend.calls == before + 1          # one leave-out table for all five groups
    rows = _rows(os.path.join(o, "gold_5_dashing.deltadelta.csv"))
    assert [r["group"] for r in rows] == [n[:-6] for n in NAMES]
    for r, w in zip(rows, want):
        assert float(r["deltadelta"]) == w["deltadelta"]
        assert float(r["delta_rest"]) == w["delta_rest"]
        assert float(r["delta_all"]) == w["delta_all"]
        assert float(r["delta_all"]) - float(r["delta_rest"]) == float(r["deltadelta"])
        assert int(r["nout"]) == 1 and int(r["ngen_rest"]) == 4
        assert [os.path.basename(f) for f in r["fastas"].split("|")] == [NAMES[rows.index(r)]]
    # the climbs carry speciesinfo.kstart from one group to the next, exactly as sequential find_delta_delta calls do
    from dandd_amd.host.compat import load_tree
    host.set_backend_factory(lambda r, c: LeaveOutBackend(r, c))
    tree = load_tree(pk)
    for name, w in zip(NAMES, want):
        with redirect_stdout(io.StringIO()):
            (row,), _ = tree.leave_out_deltas([[os.path.join(data, name)]])
        assert tree.speciesinfo.kstart == w["kstart"]
        assert row["deltadelta"] == w["deltadelta"]


def test_object_path_without_leave_out_cards(host, tmp_path):
    """A backend without leave_out_cards (the CPU checkers, exact trees) goes through find_delta_delta's own steps."""
    data, pk = _tree(str(tmp_path), host)
    o1, o2 = str(tmp_path / "a"), str(tmp_path / "b")
    _run(host, LeaveOutBackend, ["-d", pk, "-o", o1])
    _run(host, hostcheck.ScheduleBackend, ["-d", pk, "-o", o2])
    a, b = _rows(os.path.join(o1, "gold_5_dashing.deltadelta.csv")), _rows(os.path.join(o2, "gold_5_dashing.deltadelta.csv"))
    assert a == b


def test_groups_file_and_floor(host, tmp_path):
    data, pk = _tree(str(tmp_path), host)
    gfile = tmp_path / "groups.tsv"
    gfile.write_text(f"{os.path.join(data, 'g3.fasta')}\tB\n{os.path.join(data, 'g0.fasta')}\tA\ng4.fasta\tB\n")
    o = str(tmp_path / "g")
    _run(host, LeaveOutBackend, ["-d", pk, "-o", o, "-g", str(gfile)])
    rows = _rows(os.path.join(o, "gold_5_dashing.deltadelta.csv"))
    assert [r["group"] for r in rows] == ["B", "A"]          # order of first appearance
    assert [int(r["nout"]) for r in rows] == [2, 1]
    assert [int(r["ngen_rest"]) for r in rows] == [3, 4]     # g1, g2 (unlisted) stay in every union
    assert [os.path.basename(f) for f in rows[0]["fastas"].split("|")] == ["g3.fasta", "g4.fasta"]
    want = _object_path(host, pk, [[os.path.join(data, "g3.fasta"), os.path.join(data, "g4.fasta")],
                                   [os.path.join(data, "g0.fasta")]])
    for r, w in zip(rows, want):
        assert float(r["deltadelta"]) == w["deltadelta"]
        assert float(r["delta_rest"]) == w["delta_rest"]
    # -f: each listed FASTA on its own, the others in every union
    flist = tmp_path / "two.txt"
    flist.write_text(f"{os.path.join(data, 'g2.fasta')}\ng1.fasta\n")
    o = str(tmp_path / "f")
    _run(host, LeaveOutBackend, ["-d", pk, "-o", o, "-f", str(flist)])
    rows = _rows(os.path.join(o, "gold_5_dashing.deltadelta.csv"))
    assert [r["group"] for r in rows] == ["g2", "g1"]
    want = _object_path(host, pk, [[os.path.join(data, "g2.fasta")], [os.path.join(data, "g1.fasta")]])
    assert [float(r["deltadelta"]) for r in rows] == [w["deltadelta"] for w in want]


def test_errors(host, tmp_path, capsys):
    data, pk = _tree(str(tmp_path), host)
    everything = tmp_path / "all.tsv"
    everything.write_text("".join(f"{n}\tX\n" for n in NAMES))
    with pytest.raises(SystemExit) as e:
        _run(host, LeaveOutBackend, ["-d", pk, "-o", str(tmp_path / "e1"), "-g", str(everything)])
    assert "holds every leaf" in str(e.value.code)
    unknown = tmp_path / "unknown.txt"
    unknown.write_text("g0.fasta\nnot_a_genome.fasta\n")
    with pytest.raises(SystemExit) as e:
        _run(host, LeaveOutBackend, ["-d", pk, "-o", str(tmp_path / "e2"), "-f", str(unknown)])
    assert "not_a_genome.fasta" in str(e.value.code) and "not a leaf" in str(e.value.code)
    ok = tmp_path / "ok.txt"
    ok.write_text("g0.fasta\n")
    with pytest.raises(SystemExit) as e:
        _run(host, LeaveOutBackend, ["-d", pk, "-o", str(tmp_path / "e3"), "-f", str(ok), "-g", str(ok)])
    assert "mutually exclusive" in str(e.value.code)
    with pytest.raises(ValueError, match="not a leaf"):
        from dandd_amd.host.compat import load_tree
        load_tree(pk).leave_out_deltas([["nowhere.fasta"]])


def test_ksweep_tree(host, tmp_path):
    """--ksweep trees: delta is max card / k over the tree's window, for the rest and for the union of all alike."""
    data, pk = _tree(str(tmp_path), host, extra=("--ksweep", "--mink", "8", "--maxk", "13"))
    o1, o2 = str(tmp_path / "s"), str(tmp_path / "o")
    _run(host, LeaveOutBackend, ["-d", pk, "-o", o1])
    _run(host, hostcheck.ScheduleBackend, ["-d", pk, "-o", o2])
    rows = _rows(os.path.join(o1, "gold_5_dashing.deltadelta.csv"))
    summ = _rows(os.path.join(o1, "gold_5_dashing_deltadeltasummary.csv"))
    assert rows == _rows(os.path.join(o2, "gold_5_dashing.deltadelta.csv"))
    assert summ == _rows(os.path.join(o2, "gold_5_dashing_deltadeltasummary.csv"))
    assert len(rows) == 5 and len(summ) == 5 * 6
    orc = __import__("oracle.dd_oracle", fromlist=["x"])
    fas = {n: np.fromfile(os.path.join(data, n), dtype=np.uint8) for n in NAMES}
    for r in rows:
        mine = [s for s in summ if s["group"] == r["group"]]
        assert [int(s["kval"]) for s in mine] == list(range(8, 14))
        rest = [n for n in NAMES if n[:-6] != r["group"]]
        for s in mine:
            k = int(s["kval"])
            want = orc.card(orc.union(*[orc.sketch(fas[n], k, 14, True) for n in rest]), 14)
            assert float(s["card_rest"]) == want
            assert float(s["delta_pos_rest"]) == want / k
        pos = [float(s["card_rest"]) / int(s["kval"]) for s in mine]
        assert float(r["delta_rest"]) == max(pos)
        assert int(r["k_rest"]) == max(int(s["kval"]) for s, p in zip(mine, pos) if p == max(pos))
        allpos = [float(s["card_all"]) / int(s["kval"]) for s in mine]
        assert float(r["delta_all"]) == max(allpos)
        assert float(r["deltadelta"]) == float(r["delta_all"]) - float(r["delta_rest"])


def test_reference_golden(host, tmp_path):
    """The values the reference's own find_delta_delta returned for each golden FASTA in order (and the subtree deltas it
    printed): the CLI rows must equal them."""
    with open(os.path.join(hostcheck.GOLD, "ref_deltadelta.json")) as f:
        gold = json.load(f)
    data, pk = _tree(str(tmp_path), host, registers=gold["registers"])
    o = str(tmp_path / "r")
    _run(host, LeaveOutBackend, ["-d", pk, "-o", o])
    rows = _rows(os.path.join(o, "gold_5_dashing.deltadelta.csv"))
    assert [os.path.basename(r["fastas"]) for r in rows] == [g["fasta"] for g in gold["groups"]]
    for r, g in zip(rows, gold["groups"]):
        assert float(r["deltadelta"]) == g["deltadelta"]
        assert float(r["delta_rest"]) == g["subtree_delta"]
        assert float(r["delta_all"]) == g["full_delta"]
    from dandd_amd.host.compat import load_tree
    host.set_backend_factory(lambda r, c: LeaveOutBackend(r, c))
    tree = load_tree(pk)
    for g in gold["groups"]:
        with redirect_stdout(io.StringIO()):
            tree.leave_out_deltas([[os.path.join(data, g["fasta"])]])
        assert tree.speciesinfo.kstart == g["kstart_after"]

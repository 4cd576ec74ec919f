"""`dandd neighbors` on the MI355X, end to end: DeltaTree.neighbor_tables through HipBackend -- the samples sketched by
sketch_files, the empty sample riding along, the rectangle against the leaf slab in HBM and its column permutation, the merged row
from the root's sketches -- behind the command, one-shot and through `dandd serve`.

The tree and the samples are tests/test_neighbors.py's; the yardsticks are the same command on the oracle backend (the same
sketch files, brute force on the CPU) and, at registers 12, tests/neighbors_ref.py fed from the FASTA files."""
import io
import os
import subprocess
import sys
from contextlib import redirect_stdout

import pytest

import test_deltadelta as dd
import test_neighbors as cpu
from test_neighbors import host  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ("neighbors", "neighbors_summary", "neighbors_j")


@pytest.fixture(autouse=True)
def _plain_environment(monkeypatch):
    for name in ("DD_PAIRWISE_STREAM", "DD_CROSS_STREAM", "DD_CROSS_HIST_MB", "DD_GRAM_PART_MB", "DANDD_SERVER", "DANDD_DEVICE_CACHE_MB"):
        monkeypatch.delenv(name, raising=False)


def _on_gpu(host, argv):
    """the command in this process, with the backend the package makes by default (HipBackend)"""
    from dandd_amd.host import cli
    host.set_backend_factory(None)
    with redirect_stdout(io.StringIO()):
        cli.main(["neighbors", *argv])


def _typed(rows):
    """csv cells as _same wants the restatement's: empty -> None, a number -> the double it is, else the text"""
    def cell(c):
        if c == "":
            return None
        try:
            return float(c)
        except ValueError:
            return c
    return [[cell(c) for c in row] for row in rows]


def _both(host, pk, tmp_path, argv, prefix, files=FILES):
    """The command on the GPU and on the oracle backend, into directories of their own: the named files must agree -- header and
    text as text, numbers as doubles.  -> the rows of each file as the GPU run wrote them."""
    gpu, chk = str(tmp_path / "gpu"), str(tmp_path / "chk")
    _on_gpu(host, ["-d", pk, "-o", gpu, *argv])
    cpu._neighbors(host, ["-d", pk, "-o", chk, *argv])
    assert sorted(os.listdir(gpu)) == sorted(os.listdir(chk)) == sorted(f"{prefix}.{name}.csv" for name in files)
    out = {}
    for name in files:
        head, got = cpu._table(os.path.join(gpu, f"{prefix}.{name}.csv"))
        head_chk, want = cpu._table(os.path.join(chk, f"{prefix}.{name}.csv"))
        assert head == head_chk and got
        cpu._same(got, _typed(want))
        out[name] = got
    return out


def test_one_shot_against_the_oracle_backend_and_the_restatement(host, tmp_path, orc, torch_cuda):
    data, pk, samples = cpu.make_world(tmp_path, host)
    fastas = [os.path.join(data, n) for n in dd.NAMES]
    before = cpu._tree_files(pk)
    got = _both(host, pk, tmp_path, ["--jaccard", *samples], "gold_5_dashing")
    assert cpu._tree_files(pk) == before
    near, summary, jac = cpu._restated(orc, fastas, samples)
    for name, want in (("neighbors", near), ("neighbors_summary", summary), ("neighbors_j", jac)):
        cpu._same(got[name], want)
    assert len(got["neighbors"]) == 15 and len(got["neighbors_j"]) == 3 * 5 * len(cpu.KS)
    twin = [r for r in got["neighbors"] if r[0] == samples[1]]
    assert os.path.basename(twin[0][1]) == "g2.fasta" and float(twin[0][8]) == 1.0 and int(twin[0][9]) == 1
    assert all(float(r[8]) < 1.0 for r in twin[1:])
    by = {r[0]: r for r in got["neighbors_summary"]}
    assert os.path.basename(by[samples[1]][3]) == "g2.fasta" and float(by[samples[1]][4]) == 1.0 and float(by[samples[1]][9]) == 0.0


def test_listing_out_of_the_slab_s_order_and_top(host, tmp_path, orc, torch_cuda, monkeypatch):
    """-f names three leaves in an order that is not the sorted one the slab in HBM keeps: the rectangle's columns go back
    through a permutation that is not the identity (watched at HipBackend._device_slab); --top 2 cuts each sample's rows."""
    from dandd_amd.host.backend import HipBackend
    data, pk, samples = cpu.make_world(tmp_path, host)
    before = cpu._tree_files(pk)
    sub = [os.path.join(data, n) for n in ("g3.fasta", "g0.fasta", "g2.fasta")]
    flist = tmp_path / "sub.txt"
    flist.write_text("".join(f + "\n" for f in sub))
    perms = []
    inner = HipBackend._device_slab

    def watched(self, leaf_paths):
        ptr, perm = inner(self, leaf_paths)
        perms.append(None if perm is None else [int(x) for x in perm])
        return ptr, perm
    monkeypatch.setattr(HipBackend, "_device_slab", watched)
    (tmp_path / "all").mkdir()
    got = _both(host, pk, tmp_path / "all", ["-f", str(flist), "-l", "sub", "--jaccard", *samples], "gold_sub_5_dashing")
    assert perms and all(sorted(p) == [0, 1, 2] and p != [0, 1, 2] for p in perms), perms
    near, summary, jac = cpu._restated(orc, sub, samples)
    for name, want in (("neighbors", near), ("neighbors_summary", summary), ("neighbors_j", jac)):
        cpu._same(got[name], want)
    twin = [r for r in got["neighbors"] if r[0] == samples[1]]
    assert os.path.basename(twin[0][1]) == "g2.fasta" and float(twin[0][8]) == 1.0
    (tmp_path / "top").mkdir()
    got = _both(host, pk, tmp_path / "top", ["-f", str(flist), "-l", "sub", "--top", "2", *samples], "gold_sub_5_dashing", FILES[:2])
    near, summary, _ = cpu._restated(orc, sub, samples, top=2)
    cpu._same(got["neighbors"], near)
    cpu._same(got["neighbors_summary"], summary)
    assert len(got["neighbors"]) == 6
    (tmp_path / "whole").mkdir()
    got = _both(host, pk, tmp_path / "whole", ["--top", "2", *samples], "gold_5_dashing", FILES[:2])
    near, summary, _ = cpu._restated(orc, [os.path.join(data, n) for n in dd.NAMES], samples, top=2)
    cpu._same(got["neighbors"], near)
    cpu._same(got["neighbors_summary"], summary)
    assert cpu._tree_files(pk) == before


@pytest.mark.parametrize("regs", [14, 20])
def test_other_register_counts_against_the_oracle_backend(host, tmp_path, torch_cuda, regs):
    """registers 14 (the sweep keeps its registers in LDS) and 20 (scatter + replay; sixteen register ranges a row in the
    rectangle): the files of the oracle-backend run of the same command"""
    data, pk, samples = cpu.make_world(tmp_path, host, registers=regs)
    before = cpu._tree_files(pk)
    got = _both(host, pk, tmp_path, ["--jaccard", *samples], "gold_5_dashing")
    assert cpu._tree_files(pk) == before
    twin = [r for r in got["neighbors"] if r[0] == samples[1]]
    assert os.path.basename(twin[0][1]) == "g2.fasta" and float(twin[0][8]) == 1.0 and all(float(r[8]) < 1.0 for r in twin[1:])


def test_through_the_server(host, tmp_path, sock_dir, torch_cuda):
    """The one-shot command in a process of its own, then twice through `dandd serve` + the client (the second time over the leaf
    slab the first left in HBM): the three files byte for byte, and what the in-process run on the oracle backend writes."""
    data, pk, samples = cpu.make_world(tmp_path, host)
    before = cpu._tree_files(pk)
    env = dict(os.environ, PYTHONHASHSEED="0")
    env.pop("DANDD_SERVER", None)
    argv = ["neighbors", "-d", pk, "--jaccard", *samples]
    one = str(tmp_path / "one")
    r = subprocess.run([sys.executable, "-m", "dandd_amd.host.cli", *argv, "-o", one], env=env, cwd=ROOT, timeout=300,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = [f"gold_5_dashing.{name}.csv" for name in FILES]
    assert sorted(os.listdir(one)) == sorted(names)
    want = {name: open(os.path.join(one, name), "rb").read() for name in names}
    chk = str(tmp_path / "chk")
    cpu._neighbors(host, ["-d", pk, "-o", chk, "--jaccard", *samples])
    for name in names:
        cpu._same(cpu._table(os.path.join(one, name))[1], _typed(cpu._table(os.path.join(chk, name))[1]))
    sock = os.path.join(sock_dir, "nb.sock")
    srv = subprocess.Popen([sys.executable, "-m", "dandd_amd.host.cli", "serve", "--socket", sock, "--idle-exit", "120"],
                           env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
        assert "listening" in srv.stdout.readline()
        cenv = dict(env, DANDD_SERVER=sock, DANDD_SERVER_REQUIRED="1")
        for visit in range(2):
            via = str(tmp_path / f"srv{visit}")
            r = subprocess.run([sys.executable, "-m", "dandd_amd.host.client", *argv, "-o", via], env=cenv, cwd=ROOT,
                               timeout=300, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            assert sorted(os.listdir(via)) == sorted(names)
            for name in names:
                with open(os.path.join(via, name), "rb") as f:
                    assert f.read() == want[name], (visit, name)
        from dandd_amd.host.client import request
        request(sock, {"op": "shutdown"})
        srv.wait(timeout=60)
    finally:
        if srv.poll() is None:
            srv.kill()
            srv.wait()
    assert cpu._tree_files(pk) == before

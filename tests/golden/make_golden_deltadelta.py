#!/usr/bin/env python3
"""Generates tests/golden/ref_deltadelta.json by RUNNING THE REFERENCE's own DeltaTree.find_delta_delta
(its lib/huffman_dandd.py, run where the golden is generated -- it is never committed), with make_golden.py's shims
for `dashing` (the CPU oracle) and `parallel` on PATH.  The reference has no command for it, so after its own `tree`
command has built the five-genome spider at -r 14 from kstart 10, a small driver loads the tree pickle it wrote and calls
find_delta_delta([fasta]) for each golden FASTA in order on that one tree -- the climbs move speciesinfo.kstart from one
call to the next, as they do in the reference -- and records what it returned and the deltas it printed.

What is committed: the recorded values only (tests/golden/ref_deltadelta.json), paths reduced to basenames.
Run from the repo root:  python tests/golden/make_golden_deltadelta.py
"""
import json
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (shims, run_ref, the reference's location)

REGISTERS = 14
FASTAS = [f"g{i}.fasta" for i in range(5)]

# runs in a child process with the reference's lib/ first on sys.path: argv = tree pickle, data directory, fasta names...
DRIVER = r'''
import contextlib, io, json, os, pickle, sys
sys.path.insert(0, os.path.dirname(sys.argv[1]))
import huffman_dandd  # noqa: F401  (the pickle's classes)
tree = pickle.load(open(sys.argv[2], "rb"))
out = []
for name in sys.argv[4:]:
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        dd = tree.find_delta_delta([os.path.join(sys.argv[3], name)])
    printed = {}
    for line in buf.getvalue().splitlines():
        key, _, val = line.partition(":")
        if key.strip() in ("Full Tree Delta", "Subtree Delta", "Larger Tree Delta", "Subtraction Result"):
            printed.setdefault(key.strip(), float(val))
    out.append({"fasta": name, "deltadelta": dd, "full_delta": printed["Full Tree Delta"],
                "subtree_delta": printed["Subtree Delta"], "kstart_after": tree.speciesinfo.kstart})
print(json.dumps(out))
'''


def main():
    work = mg.FIXTURE_ROOT + "_deltadelta"
    shutil.rmtree(work, ignore_errors=True)
    os.makedirs(work)
    try:
        bindir = os.path.join(work, "bin")
        os.makedirs(bindir)
        mg.write_exec(os.path.join(bindir, "dashing"), mg.DASHING_SHIM % {"root": mg.ROOT})
        mg.write_exec(os.path.join(bindir, "parallel"), mg.PARALLEL_SHIM)
        env = dict(os.environ, PATH=bindir + os.pathsep + os.environ["PATH"], DD_SHIM_BACKEND="hll")
        data = os.path.join(work, "data")
        shutil.copytree(os.path.join(HERE, "fasta"), data)
        o = os.path.join(work, "t1")
        os.makedirs(o)
        mg.run_ref(["tree", "-d", data, "-o", o, "-s", "gold", "-k", "10", "-r", str(REGISTERS)], env, work)
        tree_pickle = os.path.join(o, "gold_5_dashing_dtree.pickle")
        r = subprocess.run([sys.executable, "-c", DRIVER, mg.REF, tree_pickle, data] + FASTAS, env=env, cwd=work,
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"reference find_delta_delta failed:\n{r.stdout}\n{r.stderr}")
        groups = json.loads(r.stdout.strip().splitlines()[-1])
    finally:
        shutil.rmtree(work, ignore_errors=True)
    path = os.path.join(HERE, "ref_deltadelta.json")
    with open(path, "w") as f:
        json.dump({"registers": REGISTERS, "kstart": 10, "groups": groups}, f, indent=1, sort_keys=True)
    print("wrote", path, groups)


if __name__ == "__main__":
    main()

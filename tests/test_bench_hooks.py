"""bench.py's side legs: the Dashing hook of the CPU baseline and the N>1 path on one GPU."""
import json
import os
import socket
import stat
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# `dashing sketch -k<K> -S <p> --prefix <dir> <fasta>` restated with the oracle, writing Dashing's own container
# (gzip) under Dashing's own output name: what the hook has to cope with if a real binary is ever on PATH
SHIM = r'''#!/usr/bin/env python3
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np
from oracle import dd_oracle as orc
from dandd_amd.host.backend import write_sketch_file
a = sys.argv[1:]
assert a[0] == "sketch", a
k = S = prefix = fasta = None
i = 1
while i < len(a):
    t = a[i]
    if t.startswith("-k"): k = int(t[2:])
    elif t == "-S": i += 1; S = int(a[i])
    elif t == "--prefix": i += 1; prefix = a[i]
    else: fasta = t
    i += 1
regs = orc.sketch(np.fromfile(fasta, dtype=np.uint8), k, S, True)
if os.environ.get("SHIM_CORRUPT") and k == int(os.environ["SHIM_CORRUPT"]):
    mode = os.environ.get("SHIM_MODE", "one")
    regs = regs.copy()
    if mode == "one": regs[5] += 1
    elif mode == "rho": regs[regs > 0] += 1                 # another sentinel / offset in the rho rule
    elif mode == "index": regs = regs[::-1].copy()          # other bits of the hash as the index
    elif mode == "hash": regs = orc.sketch(np.fromfile(fasta, dtype=np.uint8), k, S, False)   # another hash input (here: not canonical)
write_sketch_file(os.path.join(prefix, os.path.basename(fasta) + ".w.%%d.spacing.%%d.hll" %% (k, S)), regs, S, k, True, fmt="dashing")
'''


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_cpu_baseline_uses_and_checks_a_dashing_on_path(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    base = bench.cpu_baseline(120_000, 2, 10, 13, 12)
    assert base["kind"] == "port" and base["value"] > 0 and "no `dashing` on PATH" in base["sample"]
    bindir = tmp_path / "bin"
    bindir.mkdir()
    exe = bindir / "dashing"
    exe.write_text(SHIM % {"root": ROOT})
    exe.chmod(exe.stat().st_mode | stat.S_IEXEC)
    monkeypatch.setenv("PATH", str(bindir) + os.pathsep + os.environ["PATH"])
    got = bench.cpu_baseline(120_000, 2, 10, 13, 12)
    assert got["kind"] == "dashing" and got["value"] > 0
    assert got["registers_all_equal"] is True and set(got["registers_equal_oracle"]) <= {"10", "11", "12", "13"}
    monkeypatch.setenv("SHIM_CORRUPT", "10")   # a Dashing whose registers differ must be reported, not hidden
    bad = bench.cpu_baseline(120_000, 2, 10, 13, 12)
    assert bad["kind"] == "dashing" and bad["registers_all_equal"] is False and bad["registers_equal_oracle"]["10"] is False
    # ... and the line says which RECALL assumption (oracle/POLICIES.md) the difference points at
    assert bad["mismatch_diagnosis"]["10"]["differing"] == 1 and bad["mismatch_diagnosis"]["10"]["same_support"]
    for mode, policy in (("rho", "P7"), ("index", "P6"), ("hash", "P3 / P5")):
        monkeypatch.setenv("SHIM_MODE", mode)
        d = bench.cpu_baseline(120_000, 2, 10, 13, 12)["mismatch_diagnosis"]["10"]
        assert d["points_at"].startswith(policy), (mode, d)


@pytest.mark.gpu
def test_bench_two_ranks_on_one_gpu_matches_single_process(torch_cuda):
    """The N>1 code path of bench.py (dandd_amd.dist.sharded_ksweep + the MAX all-reduce of the root) on a
    one-GPU box: two ranks share cuda:0 and reduce through gloo.  The root over both ranks' 2 x 10 genomes must be
    the root a single process computes over the same 20 genomes."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1", DD_BENCH_BACKEND="gloo", DD_BENCH_SHARE_DEVICE="1")
    common = ["--steps", "2", "--warmup", "1", "--mbp", "5", "--no-cpu-baseline", "--no-accuracy", "--no-secondary", "--no-ingest"]
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                          "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2"] + common,
                         env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert two.returncode == 0, two.stdout[-2000:] + two.stderr[-4000:]
    one = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--genomes", "20"] + common,
                         env=dict(os.environ), capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert one.returncode == 0, one.stdout[-2000:] + one.stderr[-4000:]
    j2 = json.loads([l for l in two.stdout.splitlines() if l.startswith("{")][-1])
    j1 = json.loads([l for l in one.stdout.splitlines() if l.startswith("{")][-1])
    assert j2["n_gpus"] == 2 and j2["scaling"] == "weak" and j2["config"]["genomes_per_gpu"] == 10
    assert j2["delta_root"] == j1["delta_root"] and j2["argmax_k_root"] == j1["argmax_k_root"]
    assert j2["delta_genome0"] == j1["delta_genome0"]
    assert np.isfinite(j2["value"]) and j2["value"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("config,extra", [("cfg3", ["--genomes", "8", "--mbp", "1"]), ("cfg4share", ["--mbp", "2"]),
                                          ("cfg5share", ["--genomes", "2", "--mbp", "3", "--log2m", "18"])])
def test_bench_config_presets_run(torch_cuda, tmp_path, config, extra):
    """The --config presets (BASELINE cfg 3 / 4 / 5 shapes, shrunk) produce a well-formed line: right k range, the
    extra schedule in the step, strong/weak scaling flag, finite throughput."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", config, "--steps", "1", "--warmup", "1",
                        "--full", "--no-cpu-baseline", "--detail", str(tmp_path / "detail.json")] + extra, capture_output=True, text=True, timeout=240, cwd=ROOT)
    j = _line(r)
    want_k = {"cfg3": (2, 32), "cfg4share": (2, 32), "cfg5share": (4, 64)}[config]
    assert (j["config"]["kmin"], j["config"]["kmax"]) == want_k
    assert j["scaling"] == ("strong" if config == "cfg3" else "weak") and j["value"] > 0 and np.isfinite(j["delta_root"])
    assert config in j["config"]["workload"] and j["roofline"]["kernel_ms_per_step"] > 0
    assert "accuracy_vs_exact" not in j and "secondary" not in j      # only the headline config carries those
    # the K2 object names the device form that RAN (dd_last_k2_path), on the roof that form is bound by
    k2 = _detail(j)["roofline_k2"]
    assert (j["roofline_k2"] or {}).get("path") == (k2 or {}).get("path")
    if config == "cfg3":
        assert k2["path"] == "pairwise_gram" and k2["bound"] == "mfma" and "gram_kernel" in k2["kernel"]
    elif config == "cfg4share":
        assert k2["path"] == "progressive_stream" and k2["bound"] == "hbm" and "progressive_kernel" in k2["kernel"]   # log2m 14
    else:
        assert k2 is None


@pytest.mark.gpu
def test_bench_progressive_line_names_the_bit_plane_scan_at_log2m_20(torch_cuda, tmp_path):
    """From log2m 18 on (n <= 32) dd_progressive_device runs the bit-plane AND-scan: the line must say pscan_kernel and
    price it against the LDS read rate -- round 3's line named progressive_kernel on the HBM roof for a kernel that had not run."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "cfg4share", "--steps", "1", "--warmup", "1", "--mbp", "2",
                        "--log2m", "20", "--full", "--no-cpu-baseline", "--detail", str(tmp_path / "detail.json")], capture_output=True, text=True, timeout=300, cwd=ROOT)
    j = _line(r)
    assert j["roofline_k2"]["path"] == "progressive_pscan" and j["roofline_k2"]["bound"] == "lds" and 0 < j["roofline_k2"]["frac"] < 1
    k2 = _detail(j)["roofline_k2"]
    assert k2["path"] == "progressive_pscan" and k2["bound"] == "lds" and "pscan_kernel" in k2["kernel"]
    assert k2["unit"] == "GB/s" and k2["peak"] == pytest.approx(128 * 256 * 2.4) and 0 < k2["frac"] < 1 and k2["lds_bytes_read"] > 0


def test_committed_counter_files_feed_the_issue_model():
    """bench.py's valu_bound is computed from COMMITTED evidence only: profiles/r0[456]_k1_counters_*.json (PMC passes; the newest round first) and
    profiles/r0[456]_isa_classes.json (instruction classes of the hot loops in the shipped ISA x measured issue costs).
    On the CPU: the files load for the headline workload, for DandD's default registers, for the small-genome
    regime and for the cfg 5 share; the log2m 14 kernels come out at 90-105 % of issue for their own instruction mix."""
    sys.path.insert(0, ROOT)
    import bench
    isa = bench.isa_table()
    assert isa and isa["_file"] == "profiles/r06_isa_classes.json"       # (the round's own table: the kernels of the pruned build)
    assert {f"{k}<{c}, true>" for k in ("sweep_kernel", "scatter_kernel", "scatter_first_bin_kernel") for c in range(4)} <= set(isa["kernels"])
    assert 2.2 < isa["issue_costs"]["cheap_cycles"] < 2.7 and 4.0 < isa["issue_costs"]["dear_cycles"] < 4.5
    for args in ((10, 50.0, 4, 40, 14), (10, 50.0, 4, 40, 16), (10, 50.0, 4, 40, 20), (64, 5.0, 4, 40, 20),
                 (13, 3000.0, 4, 64, 14), (13, 3000.0, 4, 64, 16), (13, 3000.0, 4, 64, 20)):
        c = bench.load_counters(*args)
        assert c is not None and c["k1_bytes_per_step"]["total"] > 0 and c["k1_valu_instr_per_update"] > 10, args
    c14 = bench.load_counters(10, 50.0, 4, 40, 14)
    k1_ms = sum(v.get("ms_per_step_in_pmc_run", 0.0) for k, v in c14["kernels"].items() if k.startswith(("sweep_kernel", "bitmap")))
    vb = bench.valu_bound(4, 40, 10 * 50e6 * 37 / (k1_ms / 1e3), c14, k1_ms / 1e3)
    assert 0.45 < vb["frac"] < 0.6 and 0.9 < vb["frac_of_mix"] < 1.05, (vb["frac"], vb["frac_of_mix"])
    assert bench.load_counters(3, 2.0, 4, 40, 14) is None


@pytest.mark.gpu
def test_bench_cfg4_two_ranks_gathers_leaves_and_splits_orderings(torch_cuda):
    """BASELINE cfg 4 (30 genomes, progressive) over two ranks: each rank sketches 15 genomes, the leaf slabs are
    all-gathered, the 10 orderings are split 5 / 5 and every ordering's last prefix equals the all-reduced root
    (bench.py exits non-zero otherwise)."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1", DD_BENCH_BACKEND="gloo", DD_BENCH_SHARE_DEVICE="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--config", "cfg4",
                        "--mbp", "1", "--steps", "1", "--warmup", "1", "--no-cpu-baseline"],
                       env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert j["n_gpus"] == 2 and j["scaling"] == "strong" and j["config"]["genomes_per_gpu"] == 15
    assert j["schedule"] == {"kind": "progressive", "genomes": 30, "orderings_this_rank": 5, "last_prefix_equals_root": True}


def _line(r):
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and len(lines[0]) <= 6000, (len(lines), len(lines[0]))     # ONE line a bounded reader can take
    return json.loads(lines[0])


def _detail(j):
    """the sidecar the line names: the full object"""
    path = j["detail"] if os.path.isabs(j["detail"]) else os.path.join(ROOT, j["detail"])
    with open(path) as f:
        return json.load(f)


@pytest.mark.gpu
def test_bench_world1_rccl_through_own_launcher(torch_cuda):
    """`python3 bench.py --gpus 1 --force-dist`: bench.py starts its own rank through torch.distributed.run, the rank
    opens an `nccl` (= RCCL) group of world size 1 and the N>1 path's exchanges -- all_reduce(MAX) of the uint8 root
    slab, the scalar max over ranks, the barrier -- all execute inside librccl.  The numbers must be the plain run's."""
    common = ["--steps", "2", "--warmup", "1", "--mbp", "5", "--no-cpu-baseline", "--no-accuracy", "--no-secondary", "--no-ingest"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "DD_BENCH_BACKEND", "DD_BENCH_SHARE_DEVICE")}
    plain = _line(subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + common,
                                 env=env, capture_output=True, text=True, timeout=240, cwd=ROOT))
    forced = _line(subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--force-dist"] + common,
                                  env=env, capture_output=True, text=True, timeout=240, cwd=ROOT))
    assert plain["collectives"]["backend"] is None and plain["collectives"]["all_reduce_max_u8"] == 0
    c = forced["collectives"]
    assert c["backend"] == "nccl" and c["launcher"] == "bench.py self-spawn"
    assert c["all_reduce_max_u8"] == 3 and c["all_reduce_scalar"] >= 1     # one root reduce per step (2 + 1 warmup)
    assert forced["n_gpus"] == 1 and forced["scaling"] == "weak" and len(forced["gpus_active"]) == 1
    assert forced["gpus_active"][0].startswith("cuda:0 ")
    for key in ("delta_root", "argmax_k_root", "delta_genome0", "argmax_k_genome0"):
        assert forced[key] == plain[key], key
    assert "RCCL" in forced["config"]["parallelism"]


@pytest.mark.gpu
def test_bench_world1_rccl_allgather_of_leaves(torch_cuda):
    """The second exchange of the N>1 path (progressive / kij need every leaf: dist.allgather_leaves) through RCCL at
    world size 1: the gathered slab must reproduce the local schedule (last prefix == root, checked inside bench.py)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "DD_BENCH_BACKEND", "DD_BENCH_SHARE_DEVICE")}
    j = _line(subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--force-dist", "--config", "cfg4share",
                              "--mbp", "2", "--steps", "1", "--warmup", "1", "--no-cpu-baseline"],
                             env=env, capture_output=True, text=True, timeout=240, cwd=ROOT))
    assert j["collectives"]["backend"] == "nccl" and j["collectives"]["all_gather"] == 6     # 3 per step, 1 + 1 steps
    assert j["schedule"]["last_prefix_equals_root"] is True and j["schedule"]["genomes"] == 8


@pytest.mark.gpu
def test_bench_plain_gpus2_starts_its_own_ranks(torch_cuda):
    """`python3 bench.py --gpus 2` with no launcher and no WORLD_SIZE (the shape of the driver's command): bench.py
    spawns the two ranks itself.  On a one-GPU box the ranks share cuda:0 and reduce through gloo (functional only)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.update(DD_BENCH_BACKEND="gloo", DD_BENCH_SHARE_DEVICE="1")
    j = _line(subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1", "--mbp", "2",
                              "--no-cpu-baseline", "--no-accuracy", "--no-secondary", "--no-ingest"],
                             env=env, capture_output=True, text=True, timeout=240, cwd=ROOT))
    assert j["n_gpus"] == 2 and len(j["gpus_active"]) == 2 and j["collectives"]["launcher"] == "bench.py self-spawn"
    assert j["collectives"]["all_reduce_max_u8"] == 2 and j["value"] > 0


def test_bench_without_enough_gpus_fails_loudly():
    """No GPU here: the self-spawned ranks must exit non-zero with a message, not hang and not print a line."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("this node really has two GPUs")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu-baseline"],
                       env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode != 0 and not [l for l in r.stdout.splitlines() if l.startswith("{")]
    # (either rank's refusal: on a box with no GPU both ranks refuse, and the launcher may tear one of them down before it has
    # printed -- asserting rank 1's message alone failed once in four loaded runs)
    assert "wants cuda:" in r.stderr


@pytest.mark.gpu
def test_bench_headline_line_has_every_object(torch_cuda, tmp_path):
    """`bench.py --full` on a shrunk workload (3 x 2 Mbp): bench.py prints ONE line of at most 6000 bytes -- round 4's
    21.9 KB line could not be read by the driver -- that carries the contract's keys, `roofline` (frac, traffic key, the VALU
    bound's three numbers), `cpu_baseline` (value, cores, kind, sample, stages), the accuracy verdict, one {value, ms, frac,
    frac_of_mix} entry per secondary step (log2m 16 / 20, small genomes, realistic genomes, the cfg 5 share) and per ingest
    probe, no prose; the FULL object (every roofline with its per-kernel issue model, every `what` / `why`) is in the sidecar
    the line names."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--genomes", "3", "--mbp", "2",
                        "--full", "--cpu-sample-mbp", "2", "--share-mbp", "3", "--detail", str(tmp_path / "bench_detail.json")],
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    j = _line(r)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
                "config", "roofline", "cpu_baseline", "accuracy_vs_exact", "secondary", "ingest", "gpus_active", "collectives", "detail"):
        assert key in j, key
    assert j["metric"].startswith("Gbp/s") and j["unit"] == "Gbp/s" and j["dtype"] == "u64" and j["vs_baseline"] is None
    assert j["n_gpus"] == 1 and j["steps"] == 2 and j["warmup"] == 1 and j["scaling"] == "weak" and j["higher_is_better"] is True
    assert set(j["config"]) == {"workload", "genomes_per_gpu", "bases_per_genome", "kmin", "kmax", "log2m", "parallelism"}
    rf = j["roofline"]
    assert rf["bound"] == "hbm" and rf["peak"] == 8000.0 and 0 < rf["frac"] < 1 and "traffic" in rf and rf["traffic"] is None and rf["valu_bound"] is None
    assert rf["kernel_ms_per_step"] > 0 and rf["launches_per_step"] > 0 and rf["algorithmic_bytes_per_step"] > 0
    cb = j["cpu_baseline"]
    assert cb["kind"] == "port" and cb["value"] > 0 and cb["cores"] >= 1 and cb["unit"] == "Gbp/s" and len(cb["sample"]) < 260
    assert set(cb["stages_s"]) == {"stage1_leaf_sketches", "leaf_cards", "stage2_progressive_unions_and_cards", "stage3_nway_union_and_card"}
    assert j["accuracy_vs_exact"]["sketches"] == 4 and "delta_within_1pct" in j["accuracy_vs_exact"]
    names = {"log2m16", "log2m20", "log2m20_64x5Mbp", "realistic_log2m14", "realistic_log2m20", "cfg5share_log2m16", "cfg5share_log2m20"}
    assert set(j["secondary"]) == names
    for name, v in j["secondary"].items():
        assert "error" not in v and v["value"] > 0 and v["ms_per_step"] > 0, (name, v)
        assert not [x for x in v.values() if isinstance(x, (str, dict, list))], (name, v)      # numbers only on the line
    for name in ("log2m16", "log2m20", "log2m20_64x5Mbp", "cfg5share_log2m16", "cfg5share_log2m20"):
        assert 0 < j["secondary"][name]["frac"] < 1, name
    small = j["secondary"]["log2m20_64x5Mbp"]           # a fixed workload with committed counters
    assert small["traffic"] > 30e9 and 0 < small["frac_of_mix"] < 1.2
    for name in ("cfg5share_log2m16", "cfg5share_log2m20"):    # the north-star share (shrunk here): its accuracy clause on the line
        assert "delta_rel_err" in j["secondary"][name] and "delta_within_1pct" in j["secondary"][name], name
    ing = j["ingest"]
    assert ing["value"] > 0 and ing["best_value"] >= ing["value"]
    for sub in ("small_files", "gzip_files", "bgzf_files", "one_big_gzip_file", "gzip_fastq_files", "multi_member_gzip_files"):
        assert "error" not in ing[sub] and ing[sub]["value"] > 0, sub
    assert ing["one_big_gzip_file"]["serial_decoder_value"] > 0
    # the sidecar: the full object
    d = _detail(j)
    assert d["value"] == pytest.approx(j["value"], rel=1e-4) and d["cpu_baseline"]["stage1_only_value"] >= d["cpu_baseline"]["value"] >= d["cpu_baseline"]["with_stage2_value"] > 0
    assert abs(d["accuracy_vs_exact"]["card_rel_err_mean_signed"]) < 0.02
    for name in ("log2m16", "log2m20", "log2m20_64x5Mbp"):
        r2 = d["secondary"][name]["roofline"]
        assert r2["bound"] == "hbm" and 0 < r2["frac"] < 1 and r2["kernel_ms_per_step"] > 0, name
    sm = d["secondary"]["log2m20_64x5Mbp"]["roofline"]
    assert "k1_counters_64x5_p20.json" in sm["traffic_from"] and sm["valu_bound"]["issue_model"]["by_kernel"]
    assert "what" in d["ingest"] and "why" in d["secondary"]["log2m16"]


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_dumps_its_last_step(torch_cuda, orc, tmp_path):
    """A plain run (no --full) times exactly --steps steps and carries none of the --full blocks; --dump-outputs writes the last
    step's registers, cardinalities and deltas, which are the oracle's for the same seeded genomes, and are the same on a second run."""
    def run(d):
        return _line(subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                                     "--genomes", "2", "--mbp", "1", "--kmin", "10", "--kmax", "13", "--dump-outputs", str(d),
                                     "--detail", str(tmp_path / "detail.json")], capture_output=True, text=True, timeout=300, cwd=ROOT))
    j = run(tmp_path / "a")
    assert j["steps"] == 3 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["value"] > 0
    for key in ("cpu_baseline", "accuracy_vs_exact", "secondary", "ingest"):
        assert key not in j, key
    assert j["roofline_k2"] is None
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert set(got) == {"registers", "cardinality", "delta", "argmax_k"}
    assert got["registers"].dtype == np.float32 and got["registers"].shape == (3, 4, 1 << 14)
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    leaves = [orc.sketch_sweep(orc.synth_fasta(0xD4ADD, g, 1_000_000, 5), 10, 13, 14) for g in range(2)]
    want = np.stack(leaves + [np.maximum(*leaves)])
    assert np.array_equal(got["registers"], want.astype(np.float32))
    card = np.array([[orc.card(want[g, kk], 14) for kk in range(4)] for g in range(3)])
    assert np.array_equal(got["cardinality"], card)
    d = card / np.arange(10, 14)
    assert np.array_equal(got["delta"], d.max(axis=1)) and np.array_equal(got["argmax_k"], d.argmax(axis=1) + 10.0)
    run(tmp_path / "b")
    for name, a in got.items():
        assert np.array_equal(np.load(tmp_path / "b" / f"{name}.npy"), a), name


def test_dump_outputs_stays_within_its_limit_with_a_fixed_sample(tmp_path):
    """bench.dump_outputs: float32 / float64 files only, the small arrays whole, an array over its share of the limit replaced
    by the same seeded sample on every call (numpy or torch input alike)."""
    sys.path.insert(0, ROOT)
    import bench
    import torch
    regs = np.random.default_rng(1).integers(0, 64, (5, 7, 4096), dtype=np.uint8)
    card = np.random.default_rng(2).random((5, 7))
    limit = 50_000
    for name, big in (("np", regs), ("torch", torch.from_numpy(regs))):
        for rep in range(2):
            d = tmp_path / f"{name}{rep}"
            bench.dump_outputs(str(d), {"registers": big, "cardinality": card, "delta": card.max(axis=1)}, limit=limit)
            assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= limit
            r, c = np.load(d / "registers.npy"), np.load(d / "cardinality.npy")
            assert r.dtype == np.float32 and c.dtype == np.float64 and np.array_equal(c, card)
            assert 0 < r.size * 4 <= limit and r.ndim == 1 and set(np.unique(r)) <= set(range(64))
    first = np.load(tmp_path / "np0" / "registers.npy")
    for other in ("np1", "torch0", "torch1"):
        assert np.array_equal(np.load(tmp_path / other / "registers.npy"), first), other
    whole = tmp_path / "whole"
    bench.dump_outputs(str(whole), {"registers": regs})
    assert np.array_equal(np.load(whole / "registers.npy"), regs.astype(np.float32))


def test_compact_line_is_bounded_and_keeps_the_contract():
    """compact_line on round 4's committed full object (21.9 KB as one line: the driver's `parsed` was null): <= 6000 bytes,
    valid JSON, the contract's keys intact, nothing but numbers in the secondary entries; and it sheds optional blocks rather
    than ever exceeding the limit."""
    sys.path.insert(0, ROOT)
    import bench
    with open(os.path.join(ROOT, "profiles", "r04_v4_bench_default.json")) as f:
        full = json.load(f)
    assert len(json.dumps(full)) > 20000
    text = bench.compact_line(full, "bench_detail.json")
    j = json.loads(text)
    assert len(text) <= bench.LINE_LIMIT == 6000 and "\n" not in text
    assert j["value"] == pytest.approx(full["value"], rel=1e-4) and j["ms_per_step"] == pytest.approx(full["ms_per_step"], rel=1e-4)
    assert j["roofline"]["frac"] == pytest.approx(full["roofline"]["frac"], rel=1e-4) and j["roofline"]["traffic"] == pytest.approx(full["roofline"]["traffic"], rel=1e-4)
    assert j["roofline"]["valu_bound"]["frac_of_mix"] == pytest.approx(0.9686, abs=1e-3)
    assert j["cpu_baseline"]["value"] > 0 and j["cpu_baseline"]["cores"] == 15 and j["cpu_baseline"]["kind"] == "port"
    assert j["secondary"]["log2m20_64x5Mbp"]["traffic"] == pytest.approx(87.3e9, rel=1e-2)
    assert j["ingest"]["bgzf_files"]["host_decoder_value"] > 0
    fat = dict(full, gpus_active=["x" * 64] * 8, ingest={f"k{i}": 1.0 for i in range(2000)})
    fat["ingest"]["value"] = 1.0
    fat["secondary"] = {f"s{i}": {"value": 1.0, "ms_per_step": 1.0} for i in range(400)}
    t2 = bench.compact_line(fat, "bench_detail.json")
    assert len(t2) <= 6000 and json.loads(t2)["value"] == j["value"]

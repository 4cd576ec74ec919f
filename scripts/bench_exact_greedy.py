"""dd_exact_greedy: what keeping the masks costs the sort, and what the walk over them costs (profiles/exact_greedy.txt).
One process, warm-up first.  Development aid, not the contract bench.

  python scripts/bench_exact_greedy.py stream [--tree DIR] [--rounds 15]
      16 x 5 Mbp synthetic genomes, device forms, k = 21 and k = 33: wall ms (median [min .. max]) of exact_leave_out (16 singleton
      groups), and, where the build has them, exact_spectrum and exact_greedy with nfixed = nsteps = 1 -- the sort plus the
      stream plus one step.  --tree: import dandd_amd from another checkout (a build of the parent commit); run the two builds
      in alternating processes.
  python scripts/bench_exact_greedy.py walk [--n 64] [--mbp 5] [--kmin 10] [--kmax 40] [--reps 3] [--object-steps 2]
      related genomes (one ancestor, 1 % divergence), both modes: wall ms of the call, of the call with one step (the sorts and
      the streams), the difference per further step, the bytes of stream a step reads over that time, the store's size per k;
      then the exact_count calls of the object path (one per step, candidate and k, from files) for the first --object-steps
      free steps of the max walk, and their cost extrapolated to the whole walk.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def med(xs):
    return f"{statistics.median(xs):.2f} [{min(xs):.2f} .. {max(xs):.2f}]"


def synth(eng, torch, n, nb, related=True):
    from dandd_amd.engine import synth_size
    size = synth_size(nb, 4)
    bufs = []
    for gi in range(n):
        t = torch.empty(size + 16, dtype=torch.uint8, device="cuda")
        eng.synth_fasta_device(0xD4ADD if related else 0xD4ADD + 7919 * (gi + 1), gi, nb, 4, t.data_ptr())
        bufs.append(t)
    eng.synchronize()
    return bufs, [size] * n


def stream(args):
    import torch
    from dandd_amd.engine import Engine
    eng = Engine(0, 14, True)
    n = 16
    bufs, sizes = synth(eng, torch, n, 5_000_000)
    ptrs = [b.data_ptr() for b in bufs]
    for k in (21, 33):
        calls = [("exact_leave_out", lambda: eng.exact_leave_out_device(ptrs, sizes, k, k, list(range(n))))]
        if hasattr(eng, "exact_spectrum_device"):
            calls.append(("exact_spectrum", lambda: eng.exact_spectrum_device(ptrs, sizes, k, k)))
        if hasattr(eng, "exact_greedy_device"):
            calls.append(("exact_greedy, one step", lambda: eng.exact_greedy_device(ptrs, sizes, k, k, 0, None, 1, 1)))
        for _, call in calls:
            call(), call()
        walls = {name: [] for name, _ in calls}
        for _ in range(args.rounds):
            for name, call in calls:
                t0 = time.perf_counter()
                call()
                walls[name].append((time.perf_counter() - t0) * 1e3)
        for name, _ in calls:
            print(f"{args.label} k={k} {name}: {med(walls[name])} ms", flush=True)
    eng.close()


def walk(args):
    import numpy as np
    import torch
    from dandd_amd.engine import Engine
    eng = Engine(0, 14, True)
    n, kmin, kmax = args.n, args.kmin, args.kmax
    K = kmax - kmin + 1
    bufs, sizes = synth(eng, torch, n, int(args.mbp * 1e6))
    ptrs = [b.data_ptr() for b in bufs]
    res = {"n": n, "mbp": args.mbp, "k": [kmin, kmax], "DD_EXACT_MASKS_MB": os.environ.get("DD_EXACT_MASKS_MB", "default (24576)")}
    orders = {}
    for mode, name in ((0, "max"), (1, "min")):
        eng.exact_greedy_device(ptrs, sizes, kmin, kmax, mode, None, 1, 1)              # warm-up: workspaces, first launches
        one, full = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            eng.exact_greedy_device(ptrs, sizes, kmin, kmax, mode, None, 1, 1)
            one.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            order, card = eng.exact_greedy_device(ptrs, sizes, kmin, kmax, mode)
            full.append((time.perf_counter() - t0) * 1e3)
        orders[name] = [int(x) for x in order]
        masks = [int(v) for v in card[-1]]                                          # |union of all| = masks of the k's stream
        per_step = (statistics.median(full) - statistics.median(one)) / (n - 1)
        res[name] = {"call_ms": med(full), "one_step_call_ms": med(one), "ms_per_further_step": round(per_step, 3),
                     "stream_gb": round(sum(masks) * 8 / 1e9, 3), "tb_per_s_per_step": round(sum(masks) * 8 / 1e9 / per_step, 3),
                     "passes": eng.last_sketch_stats()[2], "first_picks": orders[name][:4]}
        res["store_mb_per_k"] = {kmin + kk: round(m * 8 / 1e6, 1) for kk, m in enumerate(masks)}
    print(json.dumps(res), flush=True)
    if args.object_steps > 0:
        # the object path's counts: one exact_count per (step, candidate, k) over the files of the chosen genomes + the candidate
        tmp = tempfile.mkdtemp(prefix="dd_eg_")
        paths = []
        for i, (b, s) in enumerate(zip(bufs, sizes)):
            p = os.path.join(tmp, f"g{i:02d}.fa")
            b[:s].cpu().numpy().tofile(p)
            paths.append(p)
        chosen, left, per_step_s = [], list(range(n)), []
        for j in range(args.object_steps):
            t0 = time.perf_counter()
            for c in left:
                for k in range(kmin, kmax + 1):
                    eng.exact_count([paths[i] for i in chosen + [c]], k)
            per_step_s.append(time.perf_counter() - t0)
            chosen.append(orders["max"][j])
            left.remove(orders["max"][j])
        out = {"object_path_step_s": [round(x, 2) for x in per_step_s], "counts_per_step": [(n - j) * K for j in range(args.object_steps)]}
        if args.object_steps >= 2:
            # a count over f files costs a + b f: two steps give a and b; step j makes (n - j) K counts over j + 1 files
            c1, c2 = per_step_s[0] / (n * K), per_step_s[1] / ((n - 1) * K)
            b_, a_ = c2 - c1, 2 * c1 - c2
            out["extrapolated_whole_walk_s"] = round(sum((n - j) * K * (a_ + b_ * (j + 1)) for j in range(n)), 0)
            out["per_count_ms_1_file_2_files"] = [round(c1 * 1e3, 2), round(c2 * 1e3, 2)]
        print(json.dumps(out), flush=True)
        for p in paths:
            os.remove(p)
        os.rmdir(tmp)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["stream", "walk"])
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--label", default="this")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--mbp", type=float, default=5.0)
    ap.add_argument("--kmin", type=int, default=10)
    ap.add_argument("--kmax", type=int, default=40)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--object-steps", type=int, default=2)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    (stream if args.what == "stream" else walk)(args)


if __name__ == "__main__":
    main()

"""dd_greedy_device against the same walk emulated with one dd_progressive_device call per step, on two synthetic collections:
related genomes (one ancestor, 1 % divergence: the bench's) and unrelated ones (a seed each: the correction-heavy case).
One process, warm-up first, median of REPS.  Development aid, not the contract bench.

  python scripts/bench_greedy.py N MBP LOG2M KMIN KMAX [--reps 5] [--emu-reps 5] [--collections related,unrelated] [--steps]

(a) dd_greedy_device, max and min: wall ms of the call and device ms under DD_KERNEL_UNION
(b) the walk by one dd_progressive_device call per step (orderings (chosen..., g, rest...), prefix j + 1 wanted)
(c) the byte floor: sum_j (n - j) K m bytes at 3.27 TB/s, the leave-out kernel's measured rate (profiles/deltadelta_leaveout.txt)
--steps: device ms and TB/s of every dd_extend_device step of the max walk
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEAVEOUT_TBS = 3.27


def delta(cards, ks):
    best = 0.0
    for c, k in zip(cards, ks):
        if best <= c / k:
            best = c / k
    return best


def pick_of(rows, ks, mode):
    ds = [delta(r, ks) for r in rows]
    pick = 0
    for r in range(1, len(ds)):
        if (ds[r] > ds[pick]) if mode == 0 else (ds[r] < ds[pick]):
            pick = r
    return pick


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int)
    ap.add_argument("mbp", type=float)
    ap.add_argument("log2m", type=int)
    ap.add_argument("kmin", type=int)
    ap.add_argument("kmax", type=int)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--emu-reps", type=int, default=5)
    ap.add_argument("--collections", default="related,unrelated")
    ap.add_argument("--steps", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from dandd_amd.engine import Engine, KERNEL_UNION, synth_size
    n, p, kmin, kmax = args.n, args.log2m, args.kmin, args.kmax
    K, m = kmax - kmin + 1, 1 << args.log2m
    ks = list(range(kmin, kmax + 1))
    nb = int(args.mbp * 1e6)
    eng = Engine(0, p, True)
    total_bytes = sum(n - j for j in range(n)) * K * m
    floor_ms = total_bytes / (LEAVEOUT_TBS * 1e12) * 1e3
    for coll in args.collections.split(","):
        slab = torch.empty((n, K, m), dtype=torch.uint8, device="cuda")
        size = synth_size(nb, 4)
        for lo in range(0, n, 16):
            bufs = []
            for gi in range(lo, min(n, lo + 16)):
                t = torch.empty(size + 16, dtype=torch.uint8, device="cuda")
                # related: one seed, the genome index draws the 1 % of differing bases; unrelated: a seed per genome
                eng.synth_fasta_device(0xD4ADD if coll == "related" else 0xD4ADD + 7919 * (gi + 1), gi, nb, 4, t.data_ptr())
                bufs.append(t)
            eng.sketch_device([b.data_ptr() for b in bufs], [size] * len(bufs), kmin, kmax, slab[lo].data_ptr())
            eng.synchronize()
            del bufs
        ptr = slab.data_ptr()
        res = {"collection": coll, "n": n, "mbp": args.mbp, "log2m": p, "k": [kmin, kmax], "candidate_row_gb": round(total_bytes / 1e9, 2),
               "c_floor_ms_at_3.27TBs": round(floor_ms, 2)}
        orders = {}
        for mode, name in ((0, "max"), (1, "min")):
            eng.greedy_device(ptr, n, K, kmin, mode)                      # warm-up
            walls, devs = [], []
            for _ in range(args.reps):
                eng.timing_enable(True)
                eng.timing_reset()
                t0 = time.perf_counter()
                order, cards = eng.greedy_device(ptr, n, K, kmin, mode)
                walls.append((time.perf_counter() - t0) * 1e3)
                devs.append(eng.timing_read(KERNEL_UNION)[0])
                eng.timing_enable(False)
            orders[mode] = (order, cards)
            res[f"a_greedy_{name}_wall_ms"] = [round(statistics.median(walls), 2), round(min(walls), 2), round(max(walls), 2)]
            res[f"a_greedy_{name}_device_ms"] = round(statistics.median(devs), 2)
            res[f"a_over_c_{name}"] = round(statistics.median(walls) / floor_ms, 2)
            res[f"a_{name}_tb_per_s_device"] = round(total_bytes / 1e9 / statistics.median(devs), 2)
        if args.emu_reps > 0:
            eng.progressive_device(ptr, n, K, [list(range(n))])               # warm-up
            walls = []
            for _ in range(args.emu_reps):
                t0 = time.perf_counter()
                chosen, left = [], list(range(n))
                for j in range(n):
                    ords = [chosen + [g] + [x for x in left if x != g] for g in left]
                    rows = eng.progressive_device(ptr, n, K, ords)[:, j, :]
                    chosen.append(left.pop(pick_of(rows, ks, 0)))
                walls.append((time.perf_counter() - t0) * 1e3)
                assert chosen == [int(x) for x in orders[0][0]], "the emulated walk chose another ordering"
            res["b_progressive_walk_max_wall_ms"] = [round(statistics.median(walls), 1), round(min(walls), 1), round(max(walls), 1)]
            res["b_over_a_max"] = round(statistics.median(walls) / res["a_greedy_max_wall_ms"][0], 1)
        print(json.dumps(res), flush=True)
        if args.steps:
            order = [int(x) for x in orders[0][0]]
            left, base = list(range(n)), None
            print(f"# {coll}: per step of the max walk: candidates, device ms, TB/s over the candidates' rows", flush=True)
            for j in range(n):
                eng.extend_device(base.data_ptr() if j else 0, ptr, n, K, left)
                eng.timing_enable(True)
                eng.timing_reset()
                eng.extend_device(base.data_ptr() if j else 0, ptr, n, K, left)
                ms = eng.timing_read(KERNEL_UNION)[0]
                eng.timing_enable(False)
                gb = len(left) * K * m / 1e9
                print(f"step {j + 1:3d} cand {len(left):3d} {ms:8.3f} ms {gb / ms:6.2f} TB/s", flush=True)
                c = order[j]
                left.remove(c)
                base = slab[c].clone() if base is None else torch.maximum(base, slab[c])
        del slab
    eng.close()


if __name__ == "__main__":
    main()

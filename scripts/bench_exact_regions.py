"""dd_exact_locate: what painting the selected k-mers onto the genomes costs next to counting them (profiles/exact_regions.txt).
One process, warm-up first.  Development aid, not the contract bench.

  python scripts/bench_exact_regions.py [--rounds 10] [--warm 3] [--mbp 5] [--out FILE] [--only-locate]
      16 x --mbp Mbp related synthetic genomes in four groups of four, device forms, k = 21 and k = 33.  Wall ms of the C call
      through ctypes into buffers made before the clock starts (median [min .. max] of --rounds after --warm warm-ups), then
      the same calls with DD_KERNEL_EXACT timing on (device ms, median), `found` and the positions each call looks up:
        (a) dd_exact_select_device, the 12 queries core / private / signature of the four groups: the same sort, nothing located
        (b) dd_exact_locate_device, the four core queries, each on the four genomes of its group (16 jobs)
        (c) dd_exact_locate_device, all 12 queries on the genomes of their groups (48 jobs)
        (d) dd_exact_locate_device, (0, 0) on every genome (16 jobs)
      --only-locate leaves (a) out and runs every case once after one warm-up: the run to put under
      `rocprofv3 --kernel-trace --stats`, which splits the time into the sort, the ordering of the records and locate_kernel.
"""
import argparse
import ctypes as C
import math
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(xs):
    return f"{statistics.median(xs):.2f} [{min(xs):.2f} .. {max(xs):.2f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--mbp", type=float, default=5.0)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--only-locate", action="store_true")
    args = ap.parse_args()
    if args.only_locate:
        args.rounds, args.warm = 1, 1
    import torch
    from dandd_amd.engine import KERNEL_EXACT, Engine, fasta_index, synth_size
    eng = Engine(0, 14, True)
    lib, ctx = eng._lib, eng._ctx
    n, nb = 16, int(args.mbp * 1e6)
    size = synth_size(nb, 4)
    bufs, ntok = [], []
    with tempfile.TemporaryDirectory() as tmp:
        for gi in range(n):
            t = torch.empty(size + 16, dtype=torch.uint8, device="cuda")
            eng.synth_fasta_device(0xD4ADD, gi, nb, 4, t.data_ptr())
            eng.synchronize()
            bufs.append(t)
            path = os.path.join(tmp, "g.fa")                         # the shape of the answer: the host's record index
            with open(path, "wb") as f:
                f.write(t[:size].cpu().numpy().tobytes())
            ntok.append(fasta_index(path)[3])
    ptrs = (C.c_void_p * n)(*[b.data_ptr() for b in bufs])
    sizes = (C.c_size_t * n)(*[size] * n)
    full = (1 << n) - 1
    groups = [0xF << 4 * g for g in range(4)]
    twelve = [q for G in groups for q in ((G, 0), (0, full ^ G), (G, full ^ G))]
    members = {G: [i for i in range(n) if G >> i & 1] for G in groups}
    group_of = {q: G for G in groups for q in ((G, 0), (0, full ^ G), (G, full ^ G))}
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    say(f"16 x {args.mbp:g} Mbp related synthetic genomes (seed 0xD4ADD, 4 records each, canonical), four groups of four; "
        f"{args.warm} warm-ups, then {args.rounds} rounds; wall ms of the C call: median [min .. max]")
    for k in (21, 33):
        cases = []

        def select(qs):
            al, no = (np.array(x, dtype=np.uint64) for x in zip(*qs))
            out = np.zeros(len(qs), dtype=np.uint64)

            def call():
                rc = lib.dd_exact_select_device(ctx, ptrs, sizes, n, k, k, al.ctypes.data, no.ctypes.data, len(qs), out.ctypes.data)
                assert rc == 0, lib.dd_last_error().decode()
            return call, lambda: (None, 0, 0)

        def locate(jobs):
            al, no = (np.array([j[i] for j in jobs], dtype=np.uint64) for i in (0, 1))
            ge = np.array([j[2] for j in jobs], dtype=np.int32)
            off = np.zeros(len(jobs) + 1, dtype=np.uint64)
            off[1:] = np.cumsum([(ntok[g] + 63) // 64 for _, _, g in jobs])
            hits = np.zeros(int(off[-1]), dtype=np.uint64)
            found = C.c_uint64()

            def call():
                rc = lib.dd_exact_locate_device(ctx, ptrs, sizes, n, k, al.ctypes.data, no.ctypes.data, ge.ctypes.data, len(jobs),
                                                off.ctypes.data, hits.ctypes.data, C.byref(found))
                assert rc == 0, lib.dd_last_error().decode()
            # positions a walk looks up: one walk serves up to 8 jobs of a genome (kLocateJobs)
            per = {}
            for _, _, g in jobs:
                per[g] = per.get(g, 0) + 1
            positions = sum(-(-c // 8) * ntok[g] for g, c in per.items())
            return call, lambda: (found.value, positions, int(np.unpackbits(hits.view(np.uint8)).sum()))
        if not args.only_locate:
            cases.append(("(a) select, 12 queries", *select(twelve)))
        cases.append(("(b) locate, 4 cores, 16 jobs", *locate([(a, b, g) for a, b in twelve[0::3] for g in members[group_of[(a, b)]]])))
        cases.append(("(c) locate, 12 queries, 48 jobs", *locate([(a, b, g) for a, b in twelve for g in members[group_of[(a, b)]]])))
        cases.append(("(d) locate, (0, 0), 16 jobs", *locate([(0, 0, g) for g in range(n)])))
        for name, call, info in cases:
            for _ in range(args.warm):
                call()
            wall = []
            for _ in range(args.rounds):
                t0 = time.perf_counter()
                call()
                wall.append((time.perf_counter() - t0) * 1e3)
            dev = [float("nan")]
            if not args.only_locate:
                eng.timing_enable(True)
                dev = []
                for _ in range(min(args.rounds, 5)):
                    eng.timing_reset()
                    call()
                    dev.append(eng.timing_read(KERNEL_EXACT)[0])
                eng.timing_enable(False)
            found, positions, bits = info()
            probes = "" if not found else f"   positions {positions} x ceil(log2 found) {math.ceil(math.log2(found))} = {positions * math.ceil(math.log2(found))} probes   bits set {bits}"
            say(f"k={k} {name:34s} wall {med(wall):28s} ms   DD_KERNEL_EXACT {statistics.median(dev):8.2f} ms   "
                f"found {'--' if found is None else found:>10}{probes}")
    eng.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

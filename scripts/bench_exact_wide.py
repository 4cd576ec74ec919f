"""dd_exact_wide_*: what the union schedules for 65 to 255 genomes cost next to the sort they stand on, next to the narrow entries
at n = 64, and next to the only route there was before them (profiles/exact_wide.txt).  One process, warm-up first.
Development aid, not the contract bench.

  python scripts/bench_exact_wide.py [--rounds 7] [--warm 2] [--out FILE] [--once]
      Related synthetic genomes (seed 0xD4ADD, 4 records each, canonical), device forms, k = 21 and k = 33, three sets:
        128 x 2 Mbp, 255 x 1 Mbp   dd_exact_count_device of all inputs (the floor: extract + sort + count) and the three wide
                                   entries -- pairwise, progressive with 10 orderings, leave-out with every genome a group --
                                   with the passes each took
        64 x 5 Mbp                 the same, and the narrow entries on the same buffers: the ratio is the cost of W scans and
                                   wider rows
      Wall ms of the C call through ctypes into buffers made before the clock starts and DD_KERNEL_EXACT ms, each the median
      [min .. max] of --rounds after --warm warm-ups.  Then the route before: dd_exact_count (path form: read, upload, pack,
      sort) of 64 pairs of the 128-genome set written to a temporary directory, one call per pair, and that time scaled to
      the 8 128 pairs of an exact kij -- an extrapolation, labelled as one.
      --once: the 128 x 2 Mbp set only, every entry once after one warm-up: the run to put under
      `rocprofv3 --kernel-trace --stats --output-format csv`.
  python scripts/bench_exact_wide.py --split KERNEL_TRACE.csv [--out FILE]
      no GPU: the kernels of a --once run's trace summed by name, in ms, with their launches.
"""
import argparse
import csv
import ctypes as C
import os
import re
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(xs):
    return f"{statistics.median(xs):.2f} [{min(xs):.2f} .. {max(xs):.2f}]"


def split(trace, say):
    with open(trace, newline="") as f:
        rows = list(csv.DictReader(f))
    total = {}
    for r in rows:
        name = re.sub(r"\(anonymous namespace\)::|dd::|void ", "", r["Kernel_Name"]).split("(")[0]
        ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        t = total.setdefault(name, [0.0, 0])
        t[0] += ms
        t[1] += 1
    for name, (ms, launches) in sorted(total.items(), key=lambda kv: -kv[1][0]):
        say(f"{ms:10.3f} ms  {launches:5d} launches  {name}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--split", default=None, metavar="KERNEL_TRACE.csv")
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def done():
        if args.out:
            with open(args.out, "a") as f:
                f.write("\n".join(lines) + "\n")
    if args.split:
        split(args.split, say)
        return done()
    if args.once:
        args.rounds, args.warm = 1, 1
    import torch
    from dandd_amd.engine import KERNEL_EXACT, Engine, synth_size
    eng = Engine(0, 14, True)
    lib, ctx = eng._lib, eng._ctx
    say(f"related synthetic genomes (seed 0xD4ADD, 4 records each, canonical); {args.warm} warm-ups, then {args.rounds} rounds; "
        f"ms: median [min .. max]")
    sets = [(128, 2_000_000)] if args.once else [(128, 2_000_000), (255, 1_000_000), (64, 5_000_000)]
    first = None                                                    # the buffers of the 128-genome set, for the route before
    for n, nb in sets:
        size = synth_size(nb, 4)
        bufs = []
        for gi in range(n):
            t = torch.empty(size + 16, dtype=torch.uint8, device="cuda")
            eng.synth_fasta_device(0xD4ADD, gi, nb, 4, t.data_ptr())
            bufs.append(t)
        eng.synchronize()
        if first is None:
            first = (bufs, size)
        ptrs = (C.c_void_p * n)(*[b.data_ptr() for b in bufs])
        sizes = (C.c_size_t * n)(*[size] * n)
        rng = np.random.default_rng(n)
        ords = np.ascontiguousarray([rng.permutation(n) for _ in range(10)], dtype=np.int32)
        group = np.arange(n, dtype=np.int32)
        for k in (21, 33):
            distinct = C.c_uint64()
            pw = np.zeros((n, n, 1), dtype=np.uint64)
            pr = np.zeros((10, n, 1), dtype=np.uint64)
            lo = np.zeros((n + 1, 1), dtype=np.uint64)

            def entry(name, *extra):
                fn = getattr(lib, name)

                def call():
                    rc = fn(ctx, ptrs, sizes, n, *extra)
                    assert rc == 0, lib.dd_last_error().decode()
                return call
            entries = [("exact_count_device (all)", entry("dd_exact_count_device", k, C.byref(distinct)))]
            for form in ("wide_", "") if n <= 64 else ("wide_",):
                entries += [(f"exact_{form}pairwise", entry(f"dd_exact_{form}pairwise_device", k, k, pw.ctypes.data)),
                            (f"exact_{form}progressive (10)", entry(f"dd_exact_{form}progressive_device", k, k, ords.ctypes.data, 10, pr.ctypes.data)),
                            (f"exact_{form}leave_out ({n})", entry(f"dd_exact_{form}leave_out_device", k, k, group.ctypes.data, n, lo.ctypes.data))]
            for name, call in entries:
                for _ in range(args.warm):
                    call()
                wall = []
                for _ in range(args.rounds):
                    t0 = time.perf_counter()
                    call()
                    wall.append((time.perf_counter() - t0) * 1e3)
                passes = eng.last_sketch_stats()[2]
                dev = [float("nan")]
                if not args.once:
                    eng.timing_enable(True)
                    dev = []
                    for _ in range(args.rounds):
                        eng.timing_reset()
                        call()
                        dev.append(eng.timing_read(KERNEL_EXACT)[0])
                    eng.timing_enable(False)
                say(f"{n:3d} x {nb / 1e6:g} Mbp k={k} {name:32s} wall {med(wall):26s}  DD_KERNEL_EXACT {med(dev):26s}  passes {passes}")
            assert int(lo[n, 0]) == int(pr[0, n - 1, 0]) == distinct.value, (int(lo[n, 0]), distinct.value)
        del bufs
        torch.cuda.empty_cache()
    if not args.once:
        # the only route before: one dd_exact_count per union, every member read and sorted again
        bufs, size = first
        work = tempfile.mkdtemp(prefix="dd_wide_")
        try:
            paths = []
            for gi, b in enumerate(bufs):
                paths.append(os.path.join(work, f"g{gi}.fa"))
                b[:size].cpu().numpy().tofile(paths[-1])
            for k in (21, 33):
                d = C.c_uint64()

                def pair(i, j):
                    arr = (C.c_char_p * 2)(os.fsencode(paths[i]), os.fsencode(paths[j]))
                    rc = lib.dd_exact_count(ctx, arr, 2, k, C.byref(d))
                    assert rc == 0, lib.dd_last_error().decode()
                pair(0, 64)
                times = []
                for _ in range(args.rounds):
                    t0 = time.perf_counter()
                    for i in range(64):
                        pair(i, i + 64)
                    times.append((time.perf_counter() - t0) * 1e3)
                m = statistics.median(times)
                say(f"128 x 2 Mbp k={k} dd_exact_count of 64 pairs, one call each: wall {med(times)} ms; "
                    f"x 127 = {m * 127 / 1e3:.1f} s for the 8 128 pairs of a kij at this k (EXTRAPOLATED, not run)")
        finally:
            shutil.rmtree(work, ignore_errors=True)
    eng.close()
    done()


if __name__ == "__main__":
    main()

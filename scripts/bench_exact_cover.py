"""dd_exact_cover: what laying samples along the genomes of the universe costs next to counting their depths and next to
locating every k-mer of the same genomes (profiles/exact_cover.txt).  One process, warm-up first.  Development aid, not the
contract bench.

  python scripts/bench_exact_cover.py [--rounds 7] [--warm 2] [--mbp 5] [--out FILE] [--once]
      bench_exact_depth.py's universe, 16 x --mbp Mbp related synthetic genomes, device forms, k = 21 and k = 33.  Samples:
      1 (a relative of the universe that is not in it) and 16 (a genome of the universe, an unrelated one, 14 relatives).
      Targets: 1 (genome 3) and all 16.
        depth   dd_exact_depth_device, nq = 0, 64 bins, on the 1 and the 16 samples        -- the yardstick of the samples' side
        locate  dd_exact_locate_device, the query (0, 0), on the 1 and the 16 targets       -- the yardstick of the lookup
        cover   dd_exact_cover_device, clip 255: {1, 16} samples x {1, 16} targets x window {64, 4096, 192}
      Wall ms of the C call through ctypes into buffers made before the clock starts (median [min .. max] of --rounds after
      --warm warm-ups), then the same calls with DD_KERNEL_EXACT timing on (device ms, median), and `found`.
      --once runs every case once after one warm-up: the run to put under `rocprofv3 --kernel-trace --output-format csv`.
  python scripts/bench_exact_cover.py --split KERNEL_TRACE.csv [--mbp 5] [--out FILE]
      no GPU: the kernels of a --once run's trace per call -- locate_kernel of a locate call; cover_index_kernel, depth_kernel
      and cover_kernel of a cover call -- in ms, locate_kernel and cover_index_kernel in ns per target position, cover_kernel
      in ns per (target position, sample); the second call of every case is the one reported.
"""
import argparse
import csv
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOWS = (64, 4096, 192)
CASES = ([("depth", ns, 0, 0) for ns in (1, 16)] + [("locate", 0, nt, 0) for nt in (1, 16)]
         + [("cover", ns, nt, w) for ns in (1, 16) for nt in (1, 16) for w in WINDOWS])


def med(xs):
    return f"{statistics.median(xs):.2f} [{min(xs):.2f} .. {max(xs):.2f}]"


def split(trace, mbp, say):
    """per call of a --once run: its kernels in ms"""
    with open(trace, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    calls, cur = [], {}
    for r in rows:
        name = r["Kernel_Name"]
        ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        what = next((w for w in ("depth_tally_kernel", "depth_kernel", "cover_index_kernel", "cover_kernel", "locate_kernel") if w in name), None)
        if what is None:
            continue
        cur[what] = cur.get(what, 0.0) + ms
        # a depth call ends with its depth_tally_kernel, a locate call is its locate_kernel, a cover call ends with its cover_kernel
        # (one round: the default budget holds all 16 samples)
        if what in ("depth_tally_kernel", "locate_kernel", "cover_kernel"):
            calls.append(cur)
            cur = {}
    assert len(calls) == 2 * 2 * len(CASES), f"{len(calls)} calls in the trace, {4 * len(CASES)} expected"
    ntok = int(mbp * 1e6) + 4
    for ki, k in enumerate((21, 33)):
        for ci, (entry, ns, nt, window) in enumerate(CASES):
            c = calls[(ki * len(CASES) + ci) * 2 + 1]
            if entry == "depth":
                say(f"k={k} depth  {ns:2d} samples              depth_kernel {c['depth_kernel']:8.3f} ms {c['depth_kernel'] * 1e6 / (ns * ntok):6.3f} ns/pos")
            elif entry == "locate":
                say(f"k={k} locate {nt:2d} targets              locate_kernel {c['locate_kernel']:8.3f} ms {c['locate_kernel'] * 1e6 / (nt * ntok):6.3f} ns/pos")
            else:
                say(f"k={k} cover  {ns:2d} samples {nt:2d} targets W={window:<5d} cover_index_kernel {c['cover_index_kernel']:8.3f} ms "
                    f"{c['cover_index_kernel'] * 1e6 / (nt * ntok):6.3f} ns/pos   depth_kernel {c['depth_kernel']:8.3f} ms   "
                    f"cover_kernel {c['cover_kernel']:8.3f} ms {c['cover_kernel'] * 1e6 / (nt * ntok * ns):6.3f} ns/(pos, sample)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--mbp", type=float, default=5.0)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--split", default=None, metavar="KERNEL_TRACE.csv")
    ap.add_argument("--yardstick", action="store_true", help="the depth and locate cases only (a build from before dd_exact_cover)")
    ap.add_argument("--tree", default=None, metavar="DIR", help="import dandd_amd from this checkout (the parent's, built) instead of this one")
    args = ap.parse_args()
    if args.tree:
        sys.path.insert(0, os.path.abspath(args.tree))
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def done():
        if args.out:
            with open(args.out, "a") as f:
                f.write("\n".join(lines) + "\n")
    if args.split:
        split(args.split, args.mbp, say)
        return done()
    if args.once:
        args.rounds, args.warm = 1, 1
    import torch
    from dandd_amd.engine import KERNEL_EXACT, Engine, synth_size
    eng = Engine(0, 14, True)
    lib, ctx = eng._lib, eng._ctx
    n, nb = 16, int(args.mbp * 1e6)
    size = synth_size(nb, 4)

    def genome(seed, gi):
        t = torch.empty(size + 16, dtype=torch.uint8, device="cuda")
        eng.synth_fasta_device(seed, gi, nb, 4, t.data_ptr())
        eng.synchronize()
        return t
    universe = [genome(0xD4ADD, gi) for gi in range(n)]
    unrelated = genome(0xBEEF, 0)
    relatives = [genome(0xD4ADD, gi) for gi in range(n, n + 15)]
    torch.cuda.synchronize()
    ntok = nb + 4                                                       # one BREAK in front of each of the 4 records
    samples_of = {1: [relatives[14]], 16: [universe[3], unrelated] + relatives[:14]}
    targets_of = {1: [3], 16: list(range(n))}
    say(f"universe: 16 x {args.mbp:g} Mbp related synthetic genomes (seed 0xD4ADD, 4 records each, canonical); clip 255; "
        f"{args.warm} warm-ups, then {args.rounds} rounds; wall ms of the C call: median [min .. max]")
    for k in (21, 33):
        def inputs(samples):
            bufs = universe + samples
            return (C.c_void_p * len(bufs))(*[b.data_ptr() for b in bufs]), (C.c_size_t * len(bufs))(*[b.numel() - 16 for b in bufs])

        def depth(ns):
            ptrs, sizes = inputs(samples_of[ns])
            hist, total, found = np.zeros((ns, n, 64), dtype=np.uint64), np.zeros((ns, n), dtype=np.uint64), C.c_uint64()

            def call():
                rc = lib.dd_exact_depth_device(ctx, ptrs, sizes, n, ns, k, None, None, 0, 64, hist.ctypes.data, total.ctypes.data, C.byref(found))
                assert rc == 0, lib.dd_last_error().decode()
            return call, lambda: (found.value, f"hits in a genome at the most {int(total.max(1).sum())}")

        def locate(nt):
            ptrs, sizes = inputs([])
            tg = np.array(targets_of[nt], dtype=np.int32)
            zero = np.zeros(nt, dtype=np.uint64)
            off = np.arange(nt + 1, dtype=np.uint64) * np.uint64((ntok + 63) // 64)
            hits, found = np.zeros(int(off[-1]), dtype=np.uint64), C.c_uint64()

            def call():
                rc = lib.dd_exact_locate_device(ctx, ptrs, sizes, n, k, zero.ctypes.data, zero.ctypes.data, tg.ctypes.data, nt, off.ctypes.data,
                                                hits.ctypes.data, C.byref(found))
                assert rc == 0, lib.dd_last_error().decode()
            return call, lambda: (found.value, f"positions hit {int(np.unpackbits(hits.view(np.uint8)).sum())}")

        def cover(ns, nt, window):
            ptrs, sizes = inputs(samples_of[ns])
            tg = np.array(targets_of[nt], dtype=np.int32)
            off = np.arange(nt + 1, dtype=np.uint64) * np.uint64(-(-ntok // window))
            counts, found = np.zeros((ns, int(off[-1]), 6), dtype=np.uint32), C.c_uint64()

            def call():
                rc = lib.dd_exact_cover_device(ctx, ptrs, sizes, n, ns, k, tg.ctypes.data, nt, window, 255, off.ctypes.data, counts.ctypes.data,
                                               C.byref(found))
                assert rc == 0, lib.dd_last_error().decode()

            def info():
                tot = counts.astype(np.uint64).sum((0, 1))
                return found.value, f"valid {int(tot[0])} covered {int(tot[1])} depth {int(tot[2])} private {int(tot[3])} private_covered {int(tot[4])}"
            return call, info
        for entry, ns, nt, window in CASES:
            if args.yardstick and entry == "cover":
                continue
            call, info =depth(ns) if entry == "depth" else locate(nt) if entry == "locate" else cover(ns, nt, window)
            for _ in range(args.warm):
                call()
            wall = []
            for _ in range(args.rounds):
                t0 = time.perf_counter()
                call()
                wall.append((time.perf_counter() - t0) * 1e3)
            dev = [float("nan")]
            if not args.once:
                eng.timing_enable(True)
                dev = []
                for _ in range(min(args.rounds, 5)):
                    eng.timing_reset()
                    call()
                    dev.append(eng.timing_read(KERNEL_EXACT)[0])
                eng.timing_enable(False)
            found, what = info()
            name = f"{entry} {ns:2d} samples {nt:2d} targets W={window}"
            say(f"k={k} {name:40s} wall {med(wall):28s} ms   DD_KERNEL_EXACT {statistics.median(dev):8.2f} ms   found {found:>10}   {what}")
    eng.close()
    done()


if __name__ == "__main__":
    main()

"""dd_exact_paint: what painting samples window by window costs next to screening them (profiles/exact_paint.txt).
One process, warm-up first.  Development aid, not the contract bench.

  python scripts/bench_exact_paint.py [--rounds 7] [--warm 2] [--mbp 5] [--windows 64,4096,65536] [--out FILE] [--once]
      bench_exact_screen.py's universe (16 x --mbp Mbp related synthetic genomes, seed 0xD4ADD), device forms, k = 21 and
      k = 33.  Wall ms of the C call through ctypes into buffers made before the clock starts (median [min .. max] of --rounds
      after --warm warm-ups), then the same calls with DD_KERNEL_EXACT timing on (device ms, median), for three sets of samples
        hit    1 sample: genome 3 of the universe
        miss   1 sample: an unrelated genome of the same length (another seed: every lookup misses)
        16     16 samples: those two and 14 further relatives of the universe that are not in it
      each through dd_exact_screen_device with nq = 0 (the yardstick: the same sort, emission, ordering and walk, a bit per record
      kept and tallied) and through dd_exact_paint_device at every W of --windows (default 64, 4096 and 65 536).
      --once runs every case once after one warm-up: the run to put under `rocprofv3 --kernel-trace --output-format csv`.
  python scripts/bench_exact_paint.py --split KERNEL_TRACE.csv [--mbp 5] [--windows ...] [--out FILE]
      no GPU: the kernel trace of a --once run, per call (a call ends with its tally_kernel or paint_kernel; the second call of
      every case is the one reported): the walk -- screen_kernel or paint_kernel -- in ms and in ns per position walked, and
      the other kernels of the call together.
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

SETS = [("hit", 1), ("miss", 1), ("16", 16)]
WINDOWS = [64, 4096, 65536]


def cases_of(windows):
    return [(f"{name:4s} screen, nq = 0", ns) for name, ns in SETS] + [(f"{name:4s} paint, W = {w}", ns) for name, ns in SETS for w in windows]


def med(xs):
    return f"{statistics.median(xs):.2f} [{min(xs):.2f} .. {max(xs):.2f}]"


def split(trace, ntok, CASES, say):
    with open(trace, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    calls, walk, rest, name = [], 0.0, 0.0, None
    for r in rows:
        ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        kernel = r["Kernel_Name"]
        if "screen_kernel" in kernel or "paint_kernel" in kernel:
            walk, name = walk + ms, "screen_kernel" if "screen_kernel" in kernel else "paint_kernel"
        else:
            rest += ms
        if "tally_kernel" in kernel or "paint_kernel" in kernel:
            calls.append((name, walk, rest))
            walk, rest, name = 0.0, 0.0, None
    assert len(calls) == 2 * 2 * len(CASES), f"{len(calls)} calls in the trace, {4 * len(CASES)} expected"
    for ki, k in enumerate((21, 33)):
        for ci, (case, ns) in enumerate(CASES):
            name, walk, rest = calls[(ki * len(CASES) + ci) * 2 + 1]
            say(f"k={k} {case:22s} {name:14s} {walk:8.3f} ms   {walk * 1e6 / (ns * ntok):6.3f} ns per position   the call's other kernels {rest:7.2f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--mbp", type=float, default=5.0)
    ap.add_argument("--windows", default=",".join(str(w) for w in WINDOWS), help="the window sizes of the paint calls")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--split", default=None, metavar="KERNEL_TRACE.csv")
    args = ap.parse_args()
    windows = [int(w) for w in args.windows.split(",")]
    CASES = cases_of(windows)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def done():
        if args.out:
            with open(args.out, "a") as f:
                f.write("\n".join(lines) + "\n")
    n, nb = 16, int(args.mbp * 1e6)
    ntok = nb + 4                                                       # one BREAK in front of each of the 4 records
    if args.split:
        split(args.split, ntok, CASES, say)
        return done()
    if args.once:
        args.rounds, args.warm = 1, 1
    import torch
    from dandd_amd.engine import KERNEL_EXACT, Engine, synth_size
    eng = Engine(0, 14, True)
    lib, ctx = eng._lib, eng._ctx
    size = synth_size(nb, 4)

    def genome(seed, gi):
        t = torch.empty(size + 16, dtype=torch.uint8, device="cuda")
        eng.synth_fasta_device(seed, gi, nb, 4, t.data_ptr())
        eng.synchronize()
        return t
    universe = [genome(0xD4ADD, gi) for gi in range(n)]
    unrelated = genome(0xBEEF, 0)
    relatives = [genome(0xD4ADD, gi) for gi in range(n, n + 14)]
    torch.cuda.synchronize()
    sets = {"hit": [universe[3]], "miss": [unrelated], "16": [universe[3], unrelated] + relatives}
    say(f"universe: 16 x {args.mbp:g} Mbp related synthetic genomes (seed 0xD4ADD, 4 records each, canonical); {args.warm} warm-ups, then "
        f"{args.rounds} rounds; wall ms of the C call: median [min .. max]")
    for k in (21, 33):
        def frame(samples):
            bufs = universe + samples
            return (C.c_void_p * len(bufs))(*[b.data_ptr() for b in bufs]), (C.c_size_t * len(bufs))(*[size] * len(bufs))

        def screen(samples):
            ptrs, sizes = frame(samples)
            shared = np.zeros((len(samples) + 1, n), dtype=np.uint64)
            found = C.c_uint64()

            def call():
                rc = lib.dd_exact_screen_device(ctx, ptrs, sizes, n, len(samples), k, None, None, 0, shared.ctypes.data, None, C.byref(found))
                assert rc == 0, lib.dd_last_error().decode()
            return call, lambda: (found.value, shared.nbytes, f"shared with genome 3 (distinct) {[int(v) for v in shared[:-1, 3]][:2]}")

        def paint(samples, window):
            ptrs, sizes = frame(samples)
            nwin = -(-ntok // window)
            off = np.arange(len(samples) + 1, dtype=np.uint64) * np.uint64(nwin)
            counts = np.zeros((int(off[-1]), n + 2), dtype=np.uint32)
            found = C.c_uint64()

            def call():
                rc = lib.dd_exact_paint_device(ctx, ptrs, sizes, n, len(samples), k, window, off.ctypes.data, counts.ctypes.data, C.byref(found))
                assert rc == 0, lib.dd_last_error().decode()
            return call, lambda: (found.value, counts.nbytes, "valid, in_pan, in genome 3 (positions) " +
                                  str([[int(v) for v in counts[s * nwin:(s + 1) * nwin, [0, 1, 2 + 3]].sum(axis=0)] for s in range(min(len(samples), 2))]))
        cases = [screen(sets[name]) for name, _ in SETS] + [paint(sets[name], w) for name, _ in SETS for w in windows]
        for (name, ns), (call, info) in zip(CASES, cases):
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
            found, nbytes, what = info()
            say(f"k={k} {name:22s} wall {med(wall):28s} ms   DD_KERNEL_EXACT {statistics.median(dev):8.2f} ms   found {found:>10}   "
                f"positions walked {ns * ntok:>10}   answer {nbytes:>10} bytes   {what}")
    eng.close()
    done()


if __name__ == "__main__":
    main()

"""dd_exact_screen: what screening samples that are no leaves costs next to locating k-mers in a leaf (profiles/exact_screen.txt).
One process, warm-up first.  Development aid, not the contract bench.

  python scripts/bench_exact_screen.py [--rounds 7] [--warm 2] [--mbp 5] [--out FILE] [--once]
      A universe of 16 x --mbp Mbp related synthetic genomes in four groups of four, device forms, k = 21 and k = 33, the 14
      queries of `screen -g` ((0, 0), (full, 0), core / private / signature of the four groups).  Wall ms of the C call through
      ctypes into buffers made before the clock starts (median [min .. max] of --rounds after --warm warm-ups), then the same
      calls with DD_KERNEL_EXACT timing on (device ms, median), `found` and the positions each call walks:
        (a) dd_exact_locate_device, (0, 0) on ONE genome of the universe: the yardstick -- the same sort, emission and ordering,
            and one walk of --mbp Mbp that looks every k-mer up
        (b) dd_exact_screen_device, 1 sample: that genome of the universe
        (c) dd_exact_screen_device, 1 sample: an unrelated genome of the same length (another seed: every lookup misses)
        (d) dd_exact_screen_device, 16 samples: (b)'s, (c)'s and 14 further relatives of the universe that are not in it
        (e) dd_exact_screen_device, 1 sample: a further relative, its text 30 times over (a read set at 30x: every hit but the
            first finds its bit set)
      --once runs every case once after one warm-up: the run to put under `rocprofv3 --kernel-trace --output-format csv`.
  python scripts/bench_exact_screen.py --split KERNEL_TRACE.csv [--out FILE]
      no GPU: the kernel trace of a --once run split per call (a call ends with its locate_kernel or tally_kernel) into the
      sort, the emission, the ordering, the walk (locate_kernel / screen_kernel), tally_kernel, K0 and the runtime's fills and
      copies; the second call of every case is the one reported.
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

CASES = ["(a) locate, (0, 0), 1 genome", "(b) screen, 1 sample of the universe", "(c) screen, 1 unrelated sample",
         "(d) screen, 16 samples", "(e) screen, 1 sample at 30x"]


def med(xs):
    return f"{statistics.median(xs):.2f} [{min(xs):.2f} .. {max(xs):.2f}]"


def split(trace, say):
    """per call of a --once run: kernel ms by what the kernel is for"""
    with open(trace, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))

    def kind(name):
        for key, what in (("screen_kernel", "walk"), ("locate_kernel", "walk"), ("tally_kernel", "tally"), ("kmer_extract", "extract + sort"),
                          ("emit_kernel", "pre-passes + emit"), ("sched_summary", "pre-passes + emit"), ("sched_carry", "pre-passes + emit"),
                          ("pack", "K0"), ("fill", "fills and copies"), ("copy", "fills and copies"), ("Copy", "fills and copies")):
            if key in name:
                return what
        return "sort"                                                   # rocPRIM's kernels: the universe's sort, then the ordering
    calls, cur, emitted = [], {}, False
    for r in rows:
        what = kind(r["Kernel_Name"])
        if what == "sort":
            what = "ordering" if emitted else "extract + sort"
        emitted = emitted or "emit_kernel" in r["Kernel_Name"]
        cur[what] = cur.get(what, 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        if "locate_kernel" in r["Kernel_Name"] or "tally_kernel" in r["Kernel_Name"]:
            calls.append(cur)
            cur, emitted = {}, False
    # per k: every case twice (the warm-up, then the call), in CASES order; in front of them the engine's own warm-up
    assert len(calls) == 2 * 2 * len(CASES), f"{len(calls)} calls in the trace, {4 * len(CASES)} expected"
    cols = ["extract + sort", "pre-passes + emit", "ordering", "walk", "tally", "K0", "fills and copies"]
    for ki, k in enumerate((21, 33)):
        for ci, name in enumerate(CASES):
            c = calls[(ki * len(CASES) + ci) * 2 + 1]
            say(f"k={k} {name[:3]}  " + "   ".join(f"{col} {c.get(col, 0.0):7.2f}" for col in cols))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--mbp", type=float, default=5.0)
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
    deep = torch.cat([relatives[14][:size]] * 30 + [torch.zeros(16, dtype=torch.uint8, device="cuda")])
    torch.cuda.synchronize()
    ntok = nb + 4                                                       # one BREAK in front of each of the 4 records
    full = (1 << n) - 1
    qs = [(0, 0), (full, 0)] + [q for G in (0xF << 4 * g for g in range(4)) for q in ((G, 0), (0, full ^ G), (G, full ^ G))]
    al, no = (np.array(x, dtype=np.uint64) for x in zip(*qs))
    say(f"universe: 16 x {args.mbp:g} Mbp related synthetic genomes (seed 0xD4ADD, 4 records each, canonical), four groups of four, "
        f"{len(qs)} queries; {args.warm} warm-ups, then {args.rounds} rounds; wall ms of the C call: median [min .. max]")
    for k in (21, 33):
        def locate():
            ptrs = (C.c_void_p * n)(*[b.data_ptr() for b in universe])
            sizes = (C.c_size_t * n)(*[size] * n)
            a0, g0 = np.zeros(1, dtype=np.uint64), np.array([3], dtype=np.int32)
            off = np.array([0, (ntok + 63) // 64], dtype=np.uint64)
            hits = np.zeros(int(off[-1]), dtype=np.uint64)
            found = C.c_uint64()

            def call():
                rc = lib.dd_exact_locate_device(ctx, ptrs, sizes, n, k, a0.ctypes.data, a0.ctypes.data, g0.ctypes.data, 1, off.ctypes.data,
                                                hits.ctypes.data, C.byref(found))
                assert rc == 0, lib.dd_last_error().decode()
            return call, lambda: (found.value, ntok, int(np.unpackbits(hits.view(np.uint8)).sum()))

        def screen(samples):
            bufs = universe + samples
            ptrs = (C.c_void_p * len(bufs))(*[b.data_ptr() for b in bufs])
            sizes = (C.c_size_t * len(bufs))(*[b.numel() - 16 for b in bufs])
            shared = np.zeros((len(samples) + 1, n), dtype=np.uint64)
            match = np.zeros((len(samples) + 1, len(qs)), dtype=np.uint64)
            found = C.c_uint64()

            def call():
                rc = lib.dd_exact_screen_device(ctx, ptrs, sizes, n, len(samples), k, al.ctypes.data, no.ctypes.data, len(qs),
                                                shared.ctypes.data, match.ctypes.data, C.byref(found))
                assert rc == 0, lib.dd_last_error().decode()
            positions = sum((b.numel() - 16) // size * ntok for b in samples)
            return call, lambda: (found.value, positions, int(match[:-1, 0].sum()))
        cases = [locate(), screen([universe[3]]), screen([unrelated]), screen([universe[3], unrelated] + relatives[:14]), screen([deep])]
        for name, (call, info) in zip(CASES, cases):
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
            found, positions, seen = info()
            say(f"k={k} {name:38s} wall {med(wall):28s} ms   DD_KERNEL_EXACT {statistics.median(dev):8.2f} ms   found {found:>10}   "
                f"positions walked {positions:>10}   {'bits set' if name.startswith('(a)') else 'records seen'} {seen}")
    eng.close()
    done()


if __name__ == "__main__":
    main()

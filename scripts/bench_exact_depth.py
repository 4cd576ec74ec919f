"""dd_exact_depth: what counting how many times samples hold each k-mer costs next to screening them (profiles/exact_depth.txt).
One process, warm-up first.  Development aid, not the contract bench.

  python scripts/bench_exact_depth.py [--rounds 7] [--warm 2] [--mbp 5] [--bins 64] [--out FILE] [--once]
      bench_exact_screen.py's universe, 16 x --mbp Mbp related synthetic genomes in four groups of four, device forms,
      k = 21 and k = 33, and five sets of samples:
        (a) 1 sample: a genome of the universe (every lookup hits, every depth is 1 but for the genome's own repeats)
        (b) 1 sample: an unrelated genome of the same length (another seed: every lookup misses, no atomic is issued)
        (c) 16 samples: (a)'s, (b)'s and 14 further relatives of the universe that are not in it
        (d) 1 sample: a further relative, its text 30 times over (a read set at 30x: every hit is one more add on a counter)
        (e) (d)'s sample with the 14 queries of `screen -g` ((0, 0), (full, 0), core / private / signature of the four groups)
      Every set through dd_exact_screen_device -- the yardstick: the same sort, emission, ordering and walk, a bit where
      depth keeps a count -- and through dd_exact_depth_device, with nq = 0 in (a)..(d).  Wall ms of the C call through ctypes
      into buffers made before the clock starts (median [min .. max] of --rounds after --warm warm-ups), then the same calls
      with DD_KERNEL_EXACT timing on (device ms, median), `found`, the positions each call walks and the hits it counts
      (screen: records seen; depth: the sum of `total` over the pan-genome -- row (0, 0) in (e), else the genomes' rows' bound).
      --once runs every case once after one warm-up: the run to put under `rocprofv3 --kernel-trace --output-format csv`.
  python scripts/bench_exact_depth.py --split KERNEL_TRACE.csv [--mbp 5] [--out FILE]
      no GPU: the walks and tallies of a --once run's kernel trace per call -- screen_kernel and tally_kernel of a screen call,
      tally_kernel (the sizes of the rows), depth_kernel and depth_tally_kernel of a depth call -- in ms, and the walks in ns
      per position; the second call of every case is the one reported.
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

SETS = ["(a) 1 sample of the universe", "(b) 1 unrelated sample", "(c) 16 samples", "(d) 1 sample at 30x", "(e) (d), 14 queries"]
COPIES = [1, 1, 16, 30, 30]             # genome lengths of text a set holds


def med(xs):
    return f"{statistics.median(xs):.2f} [{min(xs):.2f} .. {max(xs):.2f}]"


def split(trace, mbp, say):
    """per call of a --once run: the walk and the tallies in ms"""
    with open(trace, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    calls, cur = [], {}
    for r in rows:
        name = r["Kernel_Name"]
        ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        what = next((w for w in ("depth_tally_kernel", "depth_kernel", "screen_kernel", "tally_kernel") if w in name), None)
        if what is None:
            continue
        cur[what] = cur.get(what, 0.0) + ms
        # a screen call ends with its tally_kernel; a depth call begins with one and ends with its depth_tally_kernel
        if what == "depth_tally_kernel" or (what == "tally_kernel" and "screen_kernel" in cur):
            calls.append(cur)
            cur = {}
    # per k and set: screen twice (the warm-up, then the call), then depth twice
    assert len(calls) == 2 * len(SETS) * 4, f"{len(calls)} calls in the trace, {8 * len(SETS)} expected"
    ntok = int(mbp * 1e6) + 4
    for ki, k in enumerate((21, 33)):
        for si, name in enumerate(SETS):
            sc, de = calls[(ki * len(SETS) + si) * 4 + 1], calls[(ki * len(SETS) + si) * 4 + 3]
            pos = COPIES[si] * ntok
            say(f"k={k} {name[:3]}  screen_kernel {sc['screen_kernel']:8.3f} ms {sc['screen_kernel'] * 1e6 / pos:6.3f} ns/pos   tally_kernel {sc['tally_kernel']:7.3f} ms"
                f"   |   depth_kernel {de.get('depth_kernel', 0.0):8.3f} ms {de.get('depth_kernel', 0.0) * 1e6 / pos:6.3f} ns/pos   "
                f"depth_tally_kernel {de['depth_tally_kernel']:7.3f} ms   sizes (tally_kernel) {de['tally_kernel']:7.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--mbp", type=float, default=5.0)
    ap.add_argument("--bins", type=int, default=64)
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
        split(args.split, args.mbp, say)
        return done()
    if args.once:
        args.rounds, args.warm = 1, 1
    import torch
    from dandd_amd.engine import KERNEL_EXACT, Engine, synth_size
    eng = Engine(0, 14, True)
    lib, ctx = eng._lib, eng._ctx
    n, nb, B = 16, int(args.mbp * 1e6), args.bins
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
    say(f"universe: 16 x {args.mbp:g} Mbp related synthetic genomes (seed 0xD4ADD, 4 records each, canonical), four groups of four; "
        f"bins = {B}; {args.warm} warm-ups, then {args.rounds} rounds; wall ms of the C call: median [min .. max]")
    for k in (21, 33):
        def inputs(samples):
            bufs = universe + samples
            return ((C.c_void_p * len(bufs))(*[b.data_ptr() for b in bufs]), (C.c_size_t * len(bufs))(*[b.numel() - 16 for b in bufs]),
                    sum((b.numel() - 16) // size * ntok for b in samples))

        def screen(samples, nq):
            ptrs, sizes, positions = inputs(samples)
            shared = np.zeros((len(samples) + 1, n), dtype=np.uint64)
            match = np.zeros((len(samples) + 1, max(nq, 1)), dtype=np.uint64)
            found = C.c_uint64()

            def call():
                rc = lib.dd_exact_screen_device(ctx, ptrs, sizes, n, len(samples), k, al.ctypes.data, no.ctypes.data, nq, shared.ctypes.data,
                                                match.ctypes.data, C.byref(found))
                assert rc == 0, lib.dd_last_error().decode()
            return call, lambda: (found.value, positions, f"records seen by a genome at the most {int(shared[:-1].max(1).sum())}")

        def depth(samples, nq):
            ptrs, sizes, positions = inputs(samples)
            hist = np.zeros((len(samples), n + nq, B), dtype=np.uint64)
            total = np.zeros((len(samples), n + nq), dtype=np.uint64)
            found = C.c_uint64()

            def call():
                rc = lib.dd_exact_depth_device(ctx, ptrs, sizes, n, len(samples), k, al.ctypes.data, no.ctypes.data, nq, B, hist.ctypes.data,
                                               total.ctypes.data, C.byref(found))
                assert rc == 0, lib.dd_last_error().decode()

            def info():
                hits = f"hits {int(total[:, n].sum())}" if nq else f"hits in a genome at the most {int(total.max(1).sum())}"
                return found.value, positions, f"{hits}, clipped records in a row at the most {int(hist[:, :, -1].max())}"
            return call, info
        sets = [([universe[3]], 0), ([unrelated], 0), ([universe[3], unrelated] + relatives[:14], 0), ([deep], 0), ([deep], len(qs))]
        for name, (samples, nq) in zip(SETS, sets):
            for entry, (call, info) in (("screen", screen(samples, nq)), ("depth", depth(samples, nq))):
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
                found, positions, what = info()
                say(f"k={k} {name:30s} {entry:6s} wall {med(wall):28s} ms   DD_KERNEL_EXACT {statistics.median(dev):8.2f} ms   found {found:>10}   "
                    f"positions walked {positions:>10}   {what}")
    eng.close()
    done()


if __name__ == "__main__":
    main()

"""dd_exact_select_kmers: what writing the selected k-mers costs next to counting them (profiles/exact_kmers.txt).
One process, warm-up first.  Development aid, not the contract bench.

  python scripts/bench_exact_kmers.py [--rounds 10] [--warm 3] [--mbp 5] [--out FILE]
      16 x --mbp Mbp related synthetic genomes in four groups of four, device forms, k = 21 and k = 33.  Wall ms of the C call
      through ctypes into buffers made before the clock starts (median [min .. max] of --rounds after --warm warm-ups), then
      the same calls with DD_KERNEL_EXACT timing on (device ms, median), `found` and the bytes the call returns:
        (a) dd_exact_select_device, the 12 queries core / private / signature of the four groups: the same sort, no emission
        (b) dd_exact_select_kmers_device, the same 12 queries, cap = found
        (c) dd_exact_select_kmers_device, the four signature queries only
        (d) dd_exact_select_kmers_device, (0, 0): every distinct k-mer
        (e) dd_exact_select_kmers_device, the four core queries only
      a plain device-to-host copy of the bytes (b) returns, as the scale of the copy-back,
      and the ratios (b) / (a), (c) / (a) next to (a)'s own spread.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
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
    args = ap.parse_args()
    import torch
    from dandd_amd.engine import KERNEL_EXACT, Engine, synth_size
    eng = Engine(0, 14, True)
    lib, ctx = eng._lib, eng._ctx
    n, nb = 16, int(args.mbp * 1e6)
    size = synth_size(nb, 4)
    bufs = []
    for gi in range(n):
        t = torch.empty(size + 16, dtype=torch.uint8, device="cuda")
        eng.synth_fasta_device(0xD4ADD, gi, nb, 4, t.data_ptr())
        bufs.append(t)
    eng.synchronize()
    ptrs = (C.c_void_p * n)(*[b.data_ptr() for b in bufs])
    sizes = (C.c_size_t * n)(*[size] * n)
    full = (1 << n) - 1
    groups = [0xF << 4 * g for g in range(4)]
    twelve = [q for G in groups for q in ((G, 0), (0, full ^ G), (G, full ^ G))]
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
            return call, lambda: (None, out.nbytes)

        def kmers(qs):
            al, no = (np.array(x, dtype=np.uint64) for x in zip(*qs))
            found = C.c_uint64()
            rc = lib.dd_exact_select_kmers_device(ctx, ptrs, sizes, n, k, al.ctypes.data, no.ctypes.data, len(qs), None, None, 0, C.byref(found))
            assert rc == 0, lib.dd_last_error().decode()
            cap = found.value
            recs, masks = np.zeros((cap, 2), dtype=np.uint64), np.zeros(cap, dtype=np.uint64)

            def call():
                rc = lib.dd_exact_select_kmers_device(ctx, ptrs, sizes, n, k, al.ctypes.data, no.ctypes.data, len(qs), recs.ctypes.data,
                                                      masks.ctypes.data, cap, C.byref(found))
                assert rc == 0 and found.value == cap, lib.dd_last_error().decode()
            return call, lambda: (cap, recs.nbytes + masks.nbytes)
        cases.append(("(a) select, 12 queries", *select(twelve)))
        cases.append(("(b) select_kmers, 12 queries", *kmers(twelve)))
        cases.append(("(c) select_kmers, 4 signatures", *kmers(twelve[2::3])))
        cases.append(("(d) select_kmers, (0, 0)", *kmers([(0, 0)])))
        cases.append(("(e) select_kmers, 4 cores", *kmers(twelve[0::3])))
        wall = {}
        for name, call, info in cases:
            for _ in range(args.warm):
                call()
            wall[name] = []
            for _ in range(args.rounds):
                t0 = time.perf_counter()
                call()
                wall[name].append((time.perf_counter() - t0) * 1e3)
            eng.timing_enable(True)
            dev = []
            for _ in range(min(args.rounds, 5)):
                eng.timing_reset()
                call()
                dev.append(eng.timing_read(KERNEL_EXACT)[0])
            eng.timing_enable(False)
            found, nbytes = info()
            say(f"k={k} {name:32s} wall {med(wall[name]):28s} ms   DD_KERNEL_EXACT {statistics.median(dev):8.2f} ms   "
                f"found {'--' if found is None else found:>10}   returns {nbytes} bytes")
        # the copy-back's scale: the bytes (b) returns, device -> pageable host memory, nothing else
        nbytes = cases[1][2]()[1]
        blob = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        host = np.empty(nbytes, dtype=np.uint8)
        host[:] = 0
        copies = []
        for _ in range(args.warm + min(args.rounds, 5)):
            t0 = time.perf_counter()
            torch.from_numpy(host).copy_(blob)
            copies.append((time.perf_counter() - t0) * 1e3)
        say(f"k={k} a plain copy of (b)'s {nbytes} bytes, device -> pageable host: {med(copies[args.warm:])} ms")
        del blob, host
        a = wall[cases[0][0]]
        ma = statistics.median(a)
        say(f"k={k} (a)'s own spread: min / median {min(a) / ma:.3f}, max / median {max(a) / ma:.3f};   "
            f"(b) / (a) = {statistics.median(wall[cases[1][0]]) / ma:.3f}   (c) / (a) = {statistics.median(wall[cases[2][0]]) / ma:.3f}   "
            f"(d) / (a) = {statistics.median(wall[cases[3][0]]) / ma:.3f}")
    eng.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

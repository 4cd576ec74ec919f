"""dd_exact_patterns: what the membership-pattern table costs next to the cheapest accumulator of the same sort and next to the
only route to the table there was before (profiles/exact_patterns.txt).  One process, warm-up first.  Development aid, not the
contract bench.

  python scripts/bench_exact_patterns.py [--rounds 10] [--warm 3] [--mbp 5] [--out FILE]
      16 x --mbp Mbp related synthetic genomes in four groups of four (the inputs of scripts/bench_exact_kmers.py), device
      forms, k = 21 and k = 33.  Wall ms of the C call through ctypes into buffers made before the clock starts (median
      [min .. max] of --rounds after --warm warm-ups), then the same calls with DD_KERNEL_EXACT timing on (device ms, median):
        (a) dd_exact_spectrum_device at the one k: the same sort, the cheapest accumulator -- the floor
        (b) dd_exact_patterns_device, cap = found: found, the four stats, the bytes returned
        (c) dd_exact_patterns_device with DD_PATTERNS_SLOTS=64: what spills cost on the same inputs
        (d) dd_exact_select_kmers_device (0, 0), then numpy.unique over the masks: the route before this entry
      and the ratios to (a) next to (a)'s own spread.  Then the two adversarial inputs of tests/test_gpu_patterns.py:
        (e) 64 random genomes x 8 000 bases, k = 7: 8 192 patterns of one k-mer each; default table and 64 slots
        (f) 64 random genomes x 300 kbp, k = 12: the default table spills; spectrum as its floor
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
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def measure(name, call, info):
        for _ in range(args.warm):
            call()
        wall = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e3)
        eng.timing_enable(True)
        dev = []
        for _ in range(min(args.rounds, 5)):
            eng.timing_reset()
            call()
            dev.append(eng.timing_read(KERNEL_EXACT)[0])
        eng.timing_enable(False)
        say(f"{name:44s} wall {med(wall):28s} ms   DD_KERNEL_EXACT {statistics.median(dev):8.2f} ms   {info()}")
        return wall

    def cases(ptrs, sizes, n, k, old_route):
        def spectrum():
            out = np.zeros(n + 1, dtype=np.uint64)

            def call():
                rc = lib.dd_exact_spectrum_device(ctx, ptrs, sizes, n, k, k, out.ctypes.data)
                assert rc == 0, lib.dd_last_error().decode()
            return call, lambda: f"returns {out.nbytes} bytes"

        def patterns(slots=None):
            found, stats = C.c_uint64(), np.zeros(4, dtype=np.uint64)

            def run(masks, counts, cap):
                if slots is not None:
                    os.environ["DD_PATTERNS_SLOTS"] = str(slots)
                try:
                    rc = lib.dd_exact_patterns_device(ctx, ptrs, sizes, n, k, masks, counts, cap, C.byref(found), stats.ctypes.data)
                finally:
                    os.environ.pop("DD_PATTERNS_SLOTS", None)
                assert rc == 0, lib.dd_last_error().decode()
            run(None, None, 0)
            cap = found.value
            masks, counts = np.zeros(max(cap, 1), dtype=np.uint64), np.zeros(max(cap, 1), dtype=np.uint64)
            return (lambda: run(masks.ctypes.data, counts.ctypes.data, cap),
                    lambda: f"found {found.value}   stats {[int(v) for v in stats]}   returns {16 * cap} bytes")

        def kmers_then_unique():
            zero = np.zeros(1, dtype=np.uint64)
            found = C.c_uint64()
            rc = lib.dd_exact_select_kmers_device(ctx, ptrs, sizes, n, k, zero.ctypes.data, zero.ctypes.data, 1, None, None, 0, C.byref(found))
            assert rc == 0, lib.dd_last_error().decode()
            cap = found.value
            recs, masks = np.zeros((cap, 2), dtype=np.uint64), np.zeros(cap, dtype=np.uint64)
            rows = [0]

            def call():
                rc = lib.dd_exact_select_kmers_device(ctx, ptrs, sizes, n, k, zero.ctypes.data, zero.ctypes.data, 1, recs.ctypes.data,
                                                      masks.ctypes.data, cap, C.byref(found))
                assert rc == 0 and found.value == cap, lib.dd_last_error().decode()
                rows[0] = len(np.unique(masks, return_counts=True)[0])
            return call, lambda: f"k-mers {cap}   patterns {rows[0]}   returns {recs.nbytes + masks.nbytes} bytes"
        out = [("(a) spectrum", *spectrum()), ("(b) patterns", *patterns()), ("(c) patterns, DD_PATTERNS_SLOTS=64", *patterns(64))]
        if old_route:
            out.append(("(d) select_kmers (0, 0) + numpy.unique", *kmers_then_unique()))
        return out

    def report(label, ptrs, sizes, n, k, old_route=False):
        wall = {}
        for name, call, info in cases(ptrs, sizes, n, k, old_route):
            wall[name] = measure(f"{label} k={k} {name}", call, info)
        a = wall["(a) spectrum"]
        ma = statistics.median(a)
        say(f"{label} k={k} (a)'s own spread: min / median {min(a) / ma:.3f}, max / median {max(a) / ma:.3f};   " +
            "   ".join(f"{name[:3]} / (a) = {statistics.median(w) / ma:.3f}" for name, w in wall.items() if name[:3] != "(a)"))

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
    say(f"16 x {args.mbp:g} Mbp related synthetic genomes (seed 0xD4ADD, 4 records each, canonical), four groups of four; "
        f"{args.warm} warm-ups, then {args.rounds} rounds; wall ms of the C call: median [min .. max]")
    for k in (21, 33):
        report("related", ptrs, sizes, n, k, old_route=True)
    del bufs

    def random_genomes(count, bases, seed):
        gen = torch.Generator(device="cuda").manual_seed(seed)
        letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
        head = torch.tensor(list(b">r\n"), dtype=torch.uint8, device="cuda")
        held = [torch.cat([head, letters[torch.randint(0, 4, (bases,), device="cuda", generator=gen)],
                           torch.full((17,), 10, dtype=torch.uint8, device="cuda")]) for _ in range(count)]
        torch.cuda.synchronize()
        return held, (C.c_void_p * count)(*[b.data_ptr() for b in held]), (C.c_size_t * count)(*[bases + 4] * count)
    for label, bases, k in (("(e) 64 random x 8 000 bases", 8_000, 7), ("(f) 64 random x 300 kbp", 300_000, 12)):
        held, rp, rs = random_genomes(64, bases, 20261020)
        report(label, rp, rs, 64, k)
        del held
    eng.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

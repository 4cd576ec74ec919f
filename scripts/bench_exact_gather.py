"""dd_exact_gather: what walking the greedy set cover of samples costs on top of counting their depths (profiles/exact_gather.txt).
One process, warm-up first.  Development aid, not the contract bench.

  python scripts/bench_exact_gather.py [--rounds 7] [--warm 2] [--mbp 5] [--out FILE] [--once]
      bench_exact_depth.py's universe, 16 x --mbp Mbp related synthetic genomes, device forms, k = 21 and k = 33, and three
      sets of samples:
        (a) 1 sample: a genome of the universe
        (b) 1 sample: three genomes of the universe, one text behind the other (a mixture)
        (c) 16 samples: (a)'s, an unrelated genome and 14 further relatives of the universe that are not in it
      Every set through dd_exact_depth_device with no query and 64 bins -- the yardstick: the same sort, emission, ordering
      and depth_kernel, then one tally -- and through dd_exact_gather_device with min_hits = 1 and steps = 16 (the whole walk)
      and steps = 3.  Wall ms of the C call through ctypes into buffers made before the clock starts (median [min .. max] of
      --rounds after --warm warm-ups), then the same calls with DD_KERNEL_EXACT timing on (device ms, median), `found`, and what
      the walk found.  --once runs every case once after one warm-up: the run to put under
      `rocprofv3 --kernel-trace --output-format csv`.
  python scripts/bench_exact_gather.py --split KERNEL_TRACE.csv [--out FILE]
      no GPU: gather_kernel pass by pass and the sum of gather_pick_kernel of every gather call of a --once run's kernel
      trace, in ms, next to the call's depth_kernel; the second call of every case is the one reported.
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

SETS = ["(a) 1 sample of the universe", "(b) 1 mixture of three", "(c) 16 samples"]
STEPS = (16, 3)


def med(xs):
    return f"{statistics.median(xs):.2f} [{min(xs):.2f} .. {max(xs):.2f}]"


def split(trace, say):
    """per gather call of a --once run: depth_kernel, every pass of gather_kernel, the picks together, in ms"""
    with open(trace, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    calls, cur = [], None
    for r in rows:
        name = r["Kernel_Name"]
        ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        if "depth_kernel" in name:                                         # a call's walks begin behind its depth_kernel
            cur = {"depth": ms, "gather": [], "pick": 0.0}
            calls.append(cur)
        elif "gather_pick_kernel" in name:
            cur["pick"] += ms
        elif "gather_kernel" in name:
            cur["gather"].append(ms)
    calls = [c for c in calls if c["gather"]]                              # (the depth calls have none)
    assert len(calls) == 2 * len(SETS) * len(STEPS) * 2, f"{len(calls)} gather calls in the trace"
    at = 0
    for k in (21, 33):
        for name in SETS:
            for steps in STEPS:
                c = calls[at + 1]
                at += 2
                assert len(c["gather"]) == steps + 1
                say(f"k={k} {name[:3]} steps={steps:<2}  depth_kernel {c['depth']:7.3f} ms   gather_kernel {sum(c['gather']):7.3f} ms in {steps + 1} passes: "
                    + " ".join(f"{ms:.3f}" for ms in c["gather"]) + f"   gather_pick_kernel {c['pick']:6.3f} ms in {steps + 1}")


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
    n, nb, B = 16, int(args.mbp * 1e6), 64
    size = synth_size(nb, 4)

    def genome(seed, gi):
        t = torch.empty(size + 16, dtype=torch.uint8, device="cuda")
        eng.synth_fasta_device(seed, gi, nb, 4, t.data_ptr())
        eng.synchronize()
        return t
    universe = [genome(0xD4ADD, gi) for gi in range(n)]
    unrelated = genome(0xBEEF, 0)
    relatives = [genome(0xD4ADD, gi) for gi in range(n, n + 14)]
    mixture = torch.cat([universe[g][:size] for g in (3, 9, 14)] + [torch.zeros(16, dtype=torch.uint8, device="cuda")])
    torch.cuda.synchronize()
    say(f"universe: 16 x {args.mbp:g} Mbp related synthetic genomes (seed 0xD4ADD, 4 records each, canonical); {args.warm} warm-ups, then "
        f"{args.rounds} rounds; wall ms of the C call: median [min .. max]")
    for k in (21, 33):
        def inputs(samples):
            bufs = universe + samples
            return (C.c_void_p * len(bufs))(*[b.data_ptr() for b in bufs]), (C.c_size_t * len(bufs))(*[b.numel() - 16 for b in bufs])

        def depth(samples):
            ptrs, sizes = inputs(samples)
            hist = np.zeros((len(samples), n, B), dtype=np.uint64)
            total = np.zeros((len(samples), n), dtype=np.uint64)
            found = C.c_uint64()

            def call():
                rc = lib.dd_exact_depth_device(ctx, ptrs, sizes, n, len(samples), k, None, None, 0, B, hist.ctypes.data, total.ctypes.data, C.byref(found))
                assert rc == 0, lib.dd_last_error().decode()
            return call, lambda: (found.value, f"hits in a genome at the most {int(total.max(1).sum())}")

        def gather(samples, steps):
            ptrs, sizes = inputs(samples)
            ns = len(samples)
            pick = np.zeros((ns, steps), dtype=np.int32)
            unique, deep = np.zeros((ns, steps), dtype=np.uint64), np.zeros((ns, steps), dtype=np.uint64)
            shared, total = np.zeros((ns, n), dtype=np.uint64), np.zeros((ns, 2), dtype=np.uint64)
            found = C.c_uint64()

            def call():
                rc = lib.dd_exact_gather_device(ctx, ptrs, sizes, n, ns, k, 1, steps, pick.ctypes.data, unique.ctypes.data, deep.ctypes.data,
                                                shared.ctypes.data, total.ctypes.data, C.byref(found))
                assert rc == 0, lib.dd_last_error().decode()

            def info():
                picks = (pick >= 0).sum(1)
                return found.value, (f"picks per sample {int(picks.min())}..{int(picks.max())}, first sample: pick {pick[0][:4].tolist()} unique "
                                     f"{unique[0][:4].tolist()}, held {int(total[0, 0])}, explained {int(unique[0].sum())}")
            return call, info
        sets = [[universe[3]], [mixture], [universe[3], unrelated] + relatives]
        for name, samples in zip(SETS, sets):
            for entry, (call, info) in [("depth", depth(samples))] + [(f"gather {s:>2}", gather(samples, s)) for s in STEPS]:
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
                say(f"k={k} {name:30s} {entry:9s} wall {med(wall):28s} ms   DD_KERNEL_EXACT {statistics.median(dev):8.2f} ms   found {found:>10}   {what}")
    eng.close()
    done()


if __name__ == "__main__":
    main()

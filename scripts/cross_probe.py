"""dd_cross_device against the only route there was before it, dd_pairwise_device on the rows of both slabs behind one
another, on one MI355X.  One process, warm-up first, REPS timed calls each: wall ms of the C call and device ms under
DD_KERNEL_UNION, median [min, max].  Development aid, not the contract bench; its output goes into profiles/cross_gram.txt.

  python scripts/cross_probe.py [--reps 7] [--out FILE] [--shapes P:NA:NB:K,...] [--only cross|square]

Default shapes: log2m 20, K = 31, na in {1, 8, 64} against nb in {64, 256}; na = 32 and 33 against 64 (the half-height and
the full form side by side); 1024 leaves at log2m 16.  Registers are geometric with a per-row offset, about 30 thresholds
per column at log2m 20, as sketches of genomes have.  --only runs one side (for a kernel trace in a run of its own).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT = "20:1:64:31,20:8:64:31,20:32:64:31,20:33:64:31,20:64:64:31,20:1:256:31,20:8:256:31,20:64:256:31,16:1:1024:31,16:8:1024:31,16:64:1024:31"


def slab(torch, n, K, p, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    out = torch.empty((n, K, 1 << p), dtype=torch.uint8, device="cuda")
    for lo in range(0, n, 8):                                    # (eight rows at a time: the float draws are four times the slab)
        rows = min(8, n - lo)
        regs = torch.empty((rows, K, 1 << p), dtype=torch.float32, device="cuda").geometric_(0.5, generator=g)
        regs += torch.randint(0, 9, (rows, K, 1), device="cuda", generator=g)
        out[lo:lo + rows] = regs.clamp_(0, 64 - p + 1).to(torch.uint8)
    return out


def timed(eng, union, reps, call):
    call()                                                       # warm-up: modules, workspaces
    walls, devs = [], []
    for _ in range(reps):
        eng.timing_enable(True)
        eng.timing_reset()
        t0 = time.perf_counter()
        out = call()
        walls.append((time.perf_counter() - t0) * 1e3)
        devs.append(eng.timing_read(union)[0])
        eng.timing_enable(False)
    spread = lambda v: [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)]
    return out, spread(walls), spread(devs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=DEFAULT)
    ap.add_argument("--only", choices=("cross", "square"), default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from dandd_amd.engine import Engine, KERNEL_UNION
    engines = {}
    lines = []
    for spec in args.shapes.split(","):
        p, na, nb, K = (int(x) for x in spec.split(":"))
        eng = engines.get(p) or engines.setdefault(p, Engine(0, p, True))
        both = torch.cat([slab(torch, na, K, p, 1), slab(torch, nb, K, p, 2)])
        a, b = both[:na], both[na:]
        res = {"log2m": p, "na": na, "nb": nb, "K": K}
        cross = square = None
        if args.only != "square":
            cross, res["cross_wall_ms"], res["cross_union_ms"] = timed(eng, KERNEL_UNION, args.reps,
                                                                        lambda: eng.cross_device(a.data_ptr(), na, b.data_ptr(), nb, K))
            res["path"] = eng.last_k2_path()
        if args.only != "cross":
            square, res["square_wall_ms"], res["square_union_ms"] = timed(eng, KERNEL_UNION, args.reps,
                                                                          lambda: eng.pairwise_device(both.data_ptr(), na + nb, K))
        if cross is not None and square is not None:
            assert np.array_equal(cross, square[:na, na:]), "the rectangle differs from the square"
            res["wall_ratio"] = round(res["cross_wall_ms"][0] / res["square_wall_ms"][0], 4)
            res["union_ratio"] = round(res["cross_union_ms"][0] / res["square_union_ms"][0], 4)
            res["square_wall_spread"] = round(res["square_wall_ms"][2] / res["square_wall_ms"][1], 3)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        del both, a, b, cross, square
        torch.cuda.empty_cache()
    for eng in engines.values():
        eng.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

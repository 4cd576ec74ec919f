"""dd_exact_reads: what calling samples record by record costs next to painting them (profiles/exact_reads.txt).
One process, warm-up first.  Development aid, not the contract bench.

  python scripts/bench_exact_reads.py [--rounds 7] [--warm 2] [--mbp 5] [--coverage 30] [--out FILE] [--once]
      bench_exact_paint.py's universe (16 x --mbp Mbp related synthetic genomes, seed 0xD4ADD), device forms, k = 21 and
      k = 33.  Wall ms of the C call through ctypes into buffers made before the clock starts (median [min .. max] of --rounds
      after --warm warm-ups), then the same calls with DD_KERNEL_EXACT timing on (device ms, median), for
        hit    1 sample: genome 3 of the universe          miss   1 sample: an unrelated genome of the same length
        16     16 samples: those two and 14 further relatives of the universe that are not in it
      each through dd_exact_paint_device at W = 4096 (the yardstick) and through dd_exact_reads_device with one row per
      record, once with every output and once tally-only; and for
        reads  1 sample: genome 3 cut into 150-base reads at --coverage x (about 1 M records, 151 M tokens at 5 Mbp, 30 x)
      through paint at W = 4096, through reads with ONE row (the ballot path on the same text), with one row per record and
      every output, with calls and sets but no counts, and with one row per record tally-only.
      --once runs every case once after one warm-up: the run to put under `rocprofv3 --kernel-trace --stats`.
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


def base_mask(text):
    """which bytes of FASTA bytes (uint8 array) are bases: not in a header line, no newline"""
    heads = np.flatnonzero(text == ord(">"))
    newline = np.flatnonzero(text == ord("\n"))
    ends = newline[np.searchsorted(newline, heads)]                      # the end of every header line
    in_head = np.zeros(len(text) + 1, dtype=np.int64)
    np.add.at(in_head, heads, 1)
    np.add.at(in_head, ends + 1, -1)
    return heads, (np.cumsum(in_head[:-1]) == 0) & (text != ord("\n"))


def record_starts(text):
    """(tok_start of every record, ntok) of FASTA bytes: one BREAK in front of every record's bases"""
    heads, base = base_mask(text)
    before = np.concatenate([[0], np.cumsum(base)])
    return (before[heads] + np.arange(len(heads)) + 1).astype(np.uint64), int(before[-1]) + len(heads)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--mbp", type=float, default=5.0)
    ap.add_argument("--coverage", type=float, default=30.0)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
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
    relatives = [genome(0xD4ADD, gi) for gi in range(n, n + 14)]
    torch.cuda.synchronize()
    starts_of = lambda t: record_starts(t[:size].cpu().numpy())
    # the read set: genome 3's bases, 150 at a time from random places, as FASTA records ">r\n" + bases + "\n"
    text = universe[3][:size].cpu().numpy()
    g3_starts, g3_ntok = record_starts(text)
    assert g3_ntok == nb + 4, (g3_ntok, nb)
    bases = text[base_mask(text)[1]]
    nreads = int(args.coverage * nb / 150)
    rng = np.random.default_rng(150)
    at = rng.integers(0, len(bases) - 150, nreads)
    fa = np.empty((nreads, 154), dtype=np.uint8)
    fa[:, 0], fa[:, 1], fa[:, 2], fa[:, 153] = ord(">"), ord("r"), ord("\n"), ord("\n")
    fa[:, 3:153] = bases[at[:, None] + np.arange(150)[None, :]]
    reads_dev = torch.from_numpy(np.concatenate([fa.reshape(-1), np.zeros(16, dtype=np.uint8)])).cuda()
    reads_size, reads_ntok = nreads * 154, nreads * 151
    reads_starts = (np.arange(nreads, dtype=np.uint64) * np.uint64(151) + np.uint64(1))
    samples = {"hit": [(universe[3], size)], "miss": [(unrelated, size)],
               "16": [(universe[3], size), (unrelated, size)] + [(r, size) for r in relatives], "reads": [(reads_dev, reads_size)]}
    borders = {"hit": [g3_starts], "miss": [starts_of(unrelated)[0]], "reads": [reads_starts]}
    borders["16"] = borders["hit"] + borders["miss"] + [starts_of(r)[0] for r in relatives]
    ntoks = {"hit": [nb + 4], "miss": [nb + 4], "16": [nb + 4] * 16, "reads": [reads_ntok]}
    say(f"universe: 16 x {args.mbp:g} Mbp related synthetic genomes (seed 0xD4ADD, 4 records each, canonical); read set: {nreads} records of 150 "
        f"bases of genome 3, {reads_ntok} tokens; {args.warm} warm-ups, then {args.rounds} rounds; wall ms of the C call: median [min .. max]")
    for k in (21, 33):
        def frame(name):
            bufs = [(u, size) for u in universe] + samples[name]
            return (C.c_void_p * len(bufs))(*[b.data_ptr() for b, _ in bufs]), (C.c_size_t * len(bufs))(*[s for _, s in bufs])

        def paint(name, window=4096):
            ptrs, sizes = frame(name)
            off = np.concatenate([[0], np.cumsum([-(-t // window) for t in ntoks[name]])]).astype(np.uint64)
            counts = np.zeros((int(off[-1]), n + 2), dtype=np.uint32)
            found = C.c_uint64()

            def call():
                rc = lib.dd_exact_paint_device(ctx, ptrs, sizes, n, len(samples[name]), k, window, off.ctypes.data, counts.ctypes.data, C.byref(found))
                assert rc == 0, lib.dd_last_error().decode()
            return call, lambda: (counts.nbytes, f"valid, in_pan, in genome 3 of sample 0: {[int(v) for v in counts[:int(off[1]), [0, 1, 5]].sum(axis=0)]}")

        def reads(name, rows, mode):                                   # mode: all | calls (no counts) | tally
            ptrs, sizes = frame(name)
            ns = len(samples[name])
            off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
            start = np.concatenate(list(rows) + [np.zeros(1, dtype=np.uint64)]).astype(np.uint64)
            total = int(off[-1])
            calls = np.zeros((total, 6), dtype=np.uint32) if mode != "tally" else None
            sets = np.zeros((total, 2), dtype=np.uint64) if mode != "tally" else None
            counts = np.zeros((total, n + 2), dtype=np.uint32) if mode == "all" else None
            tally = np.zeros((ns, n + 3), dtype=np.uint64)
            found = C.c_uint64()
            ptr = lambda a: None if a is None else a.ctypes.data

            def call():
                rc = lib.dd_exact_reads_device(ctx, ptrs, sizes, n, ns, k, off.ctypes.data, start.ctypes.data, 1, ptr(calls), ptr(sets), ptr(counts),
                                               tally.ctypes.data, C.byref(found))
                assert rc == 0, lib.dd_last_error().decode()
            nbytes = tally.nbytes + sum(a.nbytes for a in (calls, sets, counts) if a is not None)
            return call, lambda: (nbytes, f"rows {total}, tally of sample 0: {[int(v) for v in tally[0]]}")
        cases = []
        for name in ("hit", "miss", "16"):
            cases += [(f"{name:5s} paint, W = 4096", name, paint(name)), (f"{name:5s} reads, records, all outputs", name, reads(name, borders[name], "all")),
                      (f"{name:5s} reads, records, tally only", name, reads(name, borders[name], "tally"))]
        cases += [("reads paint, W = 4096", "reads", paint("reads")),
                  ("reads reads, one row, all outputs", "reads", reads("reads", [np.zeros(1, dtype=np.uint64)], "all")),
                  ("reads reads, records, all outputs", "reads", reads("reads", borders["reads"], "all")),
                  ("reads reads, records, calls and sets", "reads", reads("reads", borders["reads"], "calls")),
                  ("reads reads, records, tally only", "reads", reads("reads", borders["reads"], "tally"))]
        for label, name, (call, info) in cases:
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
            nbytes, what = info()
            say(f"k={k} {label:36s} wall {med(wall):30s} ms   DD_KERNEL_EXACT {statistics.median(dev):8.2f} ms   positions walked "
                f"{sum(ntoks[name]):>10}   answer {nbytes:>10} bytes   {what}")
    eng.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Randomized check of the ingestion pipeline around the decoders (dd_sketch_files, dandd_amd/csrc/dd_ingest.hip): calls of 1-60 files
of six kinds (plain FASTA, one gzip member, two members, BGZF, plain FASTQ, FASTQ .gz) and four size classes, with DD_BATCH_MB
1, 2 or unset, 1-16 loader threads, log2m 10 / 14 / 17 and a 1-3 wide k range.  One engine per log2m lives through all draws, so
the host buffer pool, its promotion to pinned memory, device buffers that shrink and grow and the plan cache carry over from
draw to draw.  Every draw: the registers of every file == the oracle's on the text `cat` / `zcat` prints, and the call made at
least the batches its plan guarantees; one draw in eight first meets a missing path, must raise, and is then repeated without it.
DD_INFLATE_STRICT=1: a file the device decoder refuses fails the draw instead of going to the host decoder.
    python scripts/fuzz_ingest.py [N] [SEED] [KEEP_DIR]
draws(n, seed) and build(cfg) need no GPU (tests/test_ingest_draws.py inspects what the sweep draws)."""
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import ingest_worker as iw  # noqa: E402

TEXT_CAP = 8 << 20      # text per draw: the oracle stays about a second
CLASSES = ("header", "tiny", "mid", "large")


def draws(n, seed):
    """the sweep's configurations, one dict per draw"""
    rng = np.random.default_rng(seed)
    for it in range(n):
        kmin = int(rng.integers(1, 65))
        kmax = min(64, kmin + int(rng.integers(0, 3)))
        nfiles = int(rng.choice([int(rng.integers(1, 8)), int(rng.integers(8, 30)), int(rng.integers(30, 61)), int(rng.integers(30, 61))]))
        files, total = [], 0
        for f in range(nfiles):
            cls = str(rng.choice(CLASSES, p=[0.05, 0.12, 0.79, 0.04]))
            nbases = {"header": 0, "tiny": int(rng.integers(1, 2001)), "mid": int(rng.integers(50_000, 600_001)),
                      "large": int(rng.integers(2_000_000, 5_000_001))}[cls]
            kind = str(rng.choice(iw.KINDS))
            text_bytes = int(nbases * (2.15 if kind in ("fq", "fqgz") else 1.03)) + 64      # (with headers and line ends: an upper bound)
            if total + text_bytes > TEXT_CAP - 4096 * (nfiles - f):      # the cap: what is left of the call is tiny files
                cls, nbases = "tiny", int(rng.integers(1, 2001))
                text_bytes = int(2.15 * nbases) + 64
            total += text_bytes
            files.append({"kind": kind, "class": cls, "nbases": nbases, "gi": 1000 * it + f})
        yield {"draw": it, "log2m": int(rng.choice([10, 14, 17])), "kmin": kmin, "kmax": kmax, "files": files,
               "batch_mb": [1, 1, 2, None][int(rng.integers(0, 4))], "nthreads": int(rng.choice([1, 2, 3, 8, 16])),
               "missing_at": int(rng.integers(0, nfiles + 1)) if it % 8 == 1 else None}


def build(cfg, seed):
    """[(file name, bytes on disk, text)] of a draw (zlib level 6 for the tiny files, 1 for the others: the sweep is about the
    pipeline, scripts/fuzz_inflate.py about what compressors write)"""
    out = []
    for i, f in enumerate(cfg["files"]):
        if f["class"] == "header":
            text = b"@r0\n\n+\n\n" if f["kind"] in ("fq", "fqgz") else b">x\n"
            suffix, data = iw.NAMES[f["kind"]], iw.container(f["kind"], text)
        else:
            suffix, data, text = iw.make_file(f["kind"], seed, f["gi"], f["nbases"], *((1, 6) if f["class"] == "tiny" else (1 + i % 3, 1)))
        out.append((f"d{i:02d}.{suffix}", data, text))
    return out


def guaranteed(cfg, files):
    """(files per batch the call plan wants, the fewest batches the call can make, the loaders' window)"""
    want, full = iw.want_of([(n, len(d)) for n, d, _ in files], cfg["batch_mb"], True, cfg["log2m"])
    return want, iw.min_batches(len(files), want, full), iw.window_of(cfg["nthreads"], want)


def main():
    import torch  # noqa: F401
    from dandd_amd.engine import Engine, EngineError
    from oracle import dd_oracle as orc
    n_cfg = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    # a failing draw's files go to KEEP_DIR (the third argument; the system's temporary directory without it); the printed draw
    # and `N SEED` make them again in any case
    keep_dir = sys.argv[3] if len(sys.argv) > 3 else tempfile.gettempdir()
    os.environ["DD_INFLATE_STRICT"] = "1"
    os.environ["DD_GUNZIP_MIN_KB"] = "1"
    engines = {}
    top = tempfile.mkdtemp()
    t0 = time.time()
    nfiles_all = nbatches_all = nmissing = 0

    def fail(cfg, files, what):
        print(f"MISMATCH draw {cfg['draw']}: {what}\n  {({k: v for k, v in cfg.items() if k != 'files'})}\n  files: "
              f"{[(n, len(d)) for n, d, _ in files]}\n  replay: python scripts/fuzz_ingest.py {n_cfg} {seed}")
        keep = os.path.join(keep_dir, f"fuzz_ingest_fail_{cfg['draw']}")
        shutil.rmtree(keep, ignore_errors=True)
        shutil.copytree(os.path.join(top, f"draw{cfg['draw']}"), keep)
        print(f"  the draw's files are kept in {keep}")
        sys.exit(1)

    for cfg in draws(n_cfg, seed):
        files = build(cfg, seed)
        d = os.path.join(top, f"draw{cfg['draw']}")
        os.makedirs(d)
        paths = []
        for name, data, _ in files:
            paths.append(os.path.join(d, name))
            with open(paths[-1], "wb") as f:
                f.write(data)
        p, kmin, kmax = cfg["log2m"], cfg["kmin"], cfg["kmax"]
        if p not in engines:
            engines[p] = Engine(0, p, True)
        eng = engines[p]
        if cfg["batch_mb"]:
            os.environ["DD_BATCH_MB"] = str(cfg["batch_mb"])
        else:
            os.environ.pop("DD_BATCH_MB", None)
        if cfg["missing_at"] is not None:
            nope = os.path.join(d, "no_such_file.fa.gz")
            try:
                eng.sketch_files(paths[:cfg["missing_at"]] + [nope] + paths[cfg["missing_at"]:], kmin, kmax, nthreads=cfg["nthreads"])
                fail(cfg, files, "a call with a missing path did not raise")
            except EngineError as e:
                if nope not in str(e):
                    fail(cfg, files, f"the error does not name the missing path: {e}")
            nmissing += 1
        got = eng.sketch_files(paths, kmin, kmax, nthreads=cfg["nthreads"])
        nbatches = eng.last_ingest_stats()[2]
        want, least, _ = guaranteed(cfg, files)
        if nbatches < least:
            fail(cfg, files, f"{nbatches} batches, fewer than the {least} that {len(files)} files in batches of {want} need")
        for i, (name, _, text) in enumerate(files):
            ref = orc.sketch_sweep(np.frombuffer(text, np.uint8), kmin, kmax, p)
            if not np.array_equal(got[i], ref):
                fail(cfg, files, f"file {i} ({name}): {int((got[i] != ref).sum())} registers differ from the oracle's")
        nfiles_all += len(files)
        nbatches_all += nbatches
        shutil.rmtree(d)
    for eng in engines.values():
        eng.close()
    shutil.rmtree(top, ignore_errors=True)
    print(f"{n_cfg} random calls of dd_sketch_files ({nfiles_all} files in {nbatches_all} batches, {nmissing} calls with a missing path refused): "
          f"every file's registers equal the oracle's, in {time.time() - t0:.1f} s")


if __name__ == "__main__":
    main()

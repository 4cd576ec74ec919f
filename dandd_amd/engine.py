"""ctypes binding of libdandd_hip.so (include/dandd_hip.h) -- the only way Python reaches the GPU.

This is the host-side stub a DandD maintainer would drop next to lib/sketch_classes.py in
place of the `subprocess` calls at /root/reference/lib/sketch_classes.py:190,198,221,229,268,274
and /root/reference/lib/huffman_dandd.py:233.

There is NO CPU fallback: `Engine(...)` raises `EngineError` when the shared library is missing
or no gfx950 device is usable.  numpy arrays are host buffers; device buffers are passed as
integer addresses (e.g. `torch.Tensor.data_ptr()`), so no torch type crosses the C ABI.
"""
import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libdandd_hip.so")

KERNEL_PACK, KERNEL_SWEEP, KERNEL_UNION, KERNEL_EXACT = 0, 1, 2, 3
ABI_VERSION = 4   # include/dandd_hip.h: DD_ABI_VERSION
GREEDY_MAX, GREEDY_MIN = 0, 1   # include/dandd_hip.h: DD_GREEDY_*

EXPORTS = [
    "dd_abi_version", "dd_last_error", "dd_create", "dd_destroy", "dd_set_stream", "dd_synchronize",
    "dd_sketch_buffer", "dd_sketch_fasta", "dd_sketch_files", "dd_inflate_files", "dd_last_ingest_stats", "dd_sketch_device", "dd_union", "dd_union_device",
    "dd_card", "dd_card_batch", "dd_card_batch_device", "dd_hist_batch_device", "dd_ertl_mle",
    "dd_progressive", "dd_progressive_device", "dd_pairwise", "dd_pairwise_device", "dd_leave_out", "dd_leave_out_device",
    "dd_cross", "dd_cross_device", "dd_cross_host_device",
    "dd_subsets", "dd_subsets_device", "dd_extend", "dd_extend_device", "dd_greedy", "dd_greedy_device",
    "dd_exact_count", "dd_exact_count_device",
    "dd_exact_pairwise", "dd_exact_progressive", "dd_exact_leave_out", "dd_exact_subsets",
    "dd_exact_pairwise_device", "dd_exact_progressive_device", "dd_exact_leave_out_device", "dd_exact_subsets_device",
    "dd_exact_subsets_from_hist",
    "dd_exact_wide_pairwise", "dd_exact_wide_progressive", "dd_exact_wide_leave_out",
    "dd_exact_wide_pairwise_device", "dd_exact_wide_progressive_device", "dd_exact_wide_leave_out_device",
    "dd_exact_spectrum", "dd_exact_core_progressive", "dd_exact_select",
    "dd_exact_spectrum_device", "dd_exact_core_progressive_device", "dd_exact_select_device",
    "dd_exact_greedy", "dd_exact_greedy_device",
    "dd_exact_select_kmers", "dd_exact_select_kmers_device",
    "dd_exact_locate", "dd_exact_locate_device", "dd_fasta_index",
    "dd_exact_screen", "dd_exact_screen_device",
    "dd_exact_paint", "dd_exact_paint_device",
    "dd_exact_reads", "dd_exact_reads_device",
    "dd_exact_depth", "dd_exact_depth_device",
    "dd_exact_cover", "dd_exact_cover_device",
    "dd_exact_gather", "dd_exact_gather_device",
    "dd_exact_patterns", "dd_exact_patterns_device",
    "dd_timing_enable", "dd_timing_read", "dd_timing_reset", "dd_last_sketch_stats", "dd_last_k2_path", "dd_last_k2_launches",
    "dd_synth_size", "dd_synth_fasta_device", "dd_synth_realistic_size", "dd_synth_realistic_device", "dd_plan_sweep",
    "dd_comm_unique_id", "dd_comm_init", "dd_comm_destroy", "dd_comm_info", "dd_allreduce_max_u8", "dd_allgather_u8",
]
COMM_ID_BYTES = 128   # include/dandd_hip.h: DD_COMM_ID_BYTES


class EngineError(RuntimeError):
    code = None   # the library's DD_E* code, where the library raised it
    found = None  # exact_select_kmers with a cap that was too small: the number of k-mers that match


ENOMEM = -5   # include/dandd_hip.h: DD_ENOMEM


_lib = None


def load_library(path=None):
    """dlopen libdandd_hip.so and declare every prototype.  Raises EngineError if absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("DANDD_LIB") or LIB_PATH  # DANDD_LIB: an alternative build (development)
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so (same SONAME as
    # /opt/rocm's).  If this library were loaded first it would pull in the system copy, a later
    # `import torch` would add the bundled one, and the second runtime to initialise reports "no
    # ROCm-capable device".  Importing torch first (when it is installed) makes the dynamic loader
    # resolve our NEEDED libamdhip64.so.7 to the copy torch already mapped.
    # A process that will never import torch (the `dandd` CLI) sets DANDD_NO_TORCH=1 and saves the
    # ~1 s import; the library then binds to the system HIP runtime.
    if "torch" not in sys.modules and os.environ.get("DANDD_NO_TORCH") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    if not os.path.exists(p):
        raise EngineError(
            f"{p} not found: build it with `python -m dandd_amd.build` (hipcc, gfx950). "
            "dandd_amd has no CPU implementation of the sketching path.")
    try:
        lib = C.CDLL(p)
    except OSError as e:  # e.g. libamdhip64 missing
        raise EngineError(f"cannot load {p}: {e}") from e
    vp, sz, i32, u64 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint64
    lib.dd_abi_version.restype = i32
    lib.dd_abi_version.argtypes = []
    if lib.dd_abi_version() != ABI_VERSION:
        raise EngineError(f"{p} has ABI version {lib.dd_abi_version()}, this binding is written against {ABI_VERSION} "
                          "(include/dandd_hip.h: DD_ABI_VERSION); rebuild with `python -m dandd_amd.build --force`")
    lib.dd_last_error.restype = C.c_char_p
    lib.dd_last_error.argtypes = []
    lib.dd_create.restype = vp
    lib.dd_create.argtypes = [i32, i32, i32]
    lib.dd_destroy.restype = None
    lib.dd_destroy.argtypes = [vp]
    lib.dd_set_stream.restype = i32
    lib.dd_set_stream.argtypes = [vp, vp]
    lib.dd_synchronize.restype = i32
    lib.dd_synchronize.argtypes = [vp]
    lib.dd_sketch_buffer.restype = i32
    lib.dd_sketch_buffer.argtypes = [vp, vp, sz, i32, i32, vp]
    lib.dd_sketch_fasta.restype = i32
    lib.dd_sketch_fasta.argtypes = [vp, C.c_char_p, i32, i32, vp]
    lib.dd_sketch_files.restype = i32
    lib.dd_sketch_files.argtypes = [vp, C.POINTER(C.c_char_p), i32, i32, i32, vp, i32]
    lib.dd_comm_unique_id.restype = i32
    lib.dd_comm_unique_id.argtypes = [vp]
    lib.dd_comm_init.restype = i32
    lib.dd_comm_init.argtypes = [vp, i32, i32, vp]
    lib.dd_comm_destroy.restype = i32
    lib.dd_comm_destroy.argtypes = [vp]
    lib.dd_comm_info.restype = i32
    lib.dd_comm_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    lib.dd_allreduce_max_u8.restype = i32
    lib.dd_allreduce_max_u8.argtypes = [vp, vp, C.c_size_t]
    lib.dd_allgather_u8.restype = i32
    lib.dd_allgather_u8.argtypes = [vp, vp, C.c_size_t, vp]
    lib.dd_inflate_files.restype = i32
    lib.dd_inflate_files.argtypes = [vp, C.POINTER(C.c_char_p), i32, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), i32]
    lib.dd_last_ingest_stats.restype = i32
    lib.dd_last_ingest_stats.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(i32), C.POINTER(u64)]
    lib.dd_sketch_device.restype = i32
    lib.dd_sketch_device.argtypes = [vp, C.POINTER(vp), C.POINTER(sz), i32, i32, i32, vp]
    # the entries on register slabs, each in two forms: the slab (dd_union: the rows) in host memory, or `_device`, in HBM
    for name, args in (("dd_union", [C.POINTER(vp), i32, sz, vp]), ("dd_card_batch", [vp, i32, vp]),
                       ("dd_progressive", [vp, i32, i32, vp, i32, vp]), ("dd_pairwise", [vp, i32, i32, vp]),
                       ("dd_leave_out", [vp, i32, i32, vp, i32, vp]), ("dd_subsets", [vp, i32, i32, vp]),
                       ("dd_extend", [vp, vp, i32, i32, vp, i32, vp]),
                       ("dd_greedy", [vp, i32, i32, i32, i32, vp, i32, i32, i32, vp, vp])):
        for suffix in ("", "_device"):
            fn = getattr(lib, name + suffix)
            fn.restype = i32
            fn.argtypes = [vp] + args
    for name in ("dd_cross", "dd_cross_device", "dd_cross_host_device"):   # two slabs: a and b in host memory, in HBM, or a host / b HBM
        fn = getattr(lib, name)
        fn.restype = i32
        fn.argtypes = [vp, vp, i32, vp, i32, i32, vp]
    lib.dd_card.restype = i32
    lib.dd_card.argtypes = [vp, vp, C.POINTER(C.c_double)]
    lib.dd_hist_batch_device.restype = i32
    lib.dd_hist_batch_device.argtypes = [vp, vp, i32, vp]
    lib.dd_ertl_mle.restype = C.c_double
    lib.dd_ertl_mle.argtypes = [vp, i32]
    lib.dd_exact_count.restype = i32
    lib.dd_exact_count.argtypes = [vp, C.POINTER(C.c_char_p), i32, i32, C.POINTER(u64)]
    lib.dd_exact_count_device.restype = i32
    lib.dd_exact_count_device.argtypes = [vp, C.POINTER(vp), C.POINTER(sz), i32, i32, C.POINTER(u64)]
    paths_t, ptrs_t, sizes_t = C.POINTER(C.c_char_p), C.POINTER(vp), C.POINTER(sz)
    for name, src, extra in (("dd_exact_pairwise", [paths_t], []), ("dd_exact_progressive", [paths_t], [vp, i32]),
                             ("dd_exact_leave_out", [paths_t], [vp, i32]), ("dd_exact_subsets", [paths_t], []),
                             ("dd_exact_pairwise_device", [ptrs_t, sizes_t], []), ("dd_exact_progressive_device", [ptrs_t, sizes_t], [vp, i32]),
                             ("dd_exact_leave_out_device", [ptrs_t, sizes_t], [vp, i32]), ("dd_exact_subsets_device", [ptrs_t, sizes_t], []),
                             ("dd_exact_wide_pairwise", [paths_t], []), ("dd_exact_wide_progressive", [paths_t], [vp, i32]),
                             ("dd_exact_wide_leave_out", [paths_t], [vp, i32]), ("dd_exact_wide_pairwise_device", [ptrs_t, sizes_t], []),
                             ("dd_exact_wide_progressive_device", [ptrs_t, sizes_t], [vp, i32]),
                             ("dd_exact_wide_leave_out_device", [ptrs_t, sizes_t], [vp, i32]),
                             ("dd_exact_spectrum", [paths_t], []), ("dd_exact_core_progressive", [paths_t], [vp, i32]),
                             ("dd_exact_select", [paths_t], [vp, vp, i32]), ("dd_exact_spectrum_device", [ptrs_t, sizes_t], []),
                             ("dd_exact_core_progressive_device", [ptrs_t, sizes_t], [vp, i32]),
                             ("dd_exact_select_device", [ptrs_t, sizes_t], [vp, vp, i32])):
        fn = getattr(lib, name)
        fn.restype = i32
        fn.argtypes = [vp] + src + [i32, i32, i32] + extra + [vp]
    for name, src in (("dd_exact_greedy", [paths_t]), ("dd_exact_greedy_device", [ptrs_t, sizes_t])):
        fn = getattr(lib, name)
        fn.restype = i32
        fn.argtypes = [vp] + src + [i32, i32, i32, i32, vp, i32, i32, i32, vp, vp]
    for name, src in (("dd_exact_select_kmers", [paths_t]), ("dd_exact_select_kmers_device", [ptrs_t, sizes_t])):
        fn = getattr(lib, name)
        fn.restype = i32
        fn.argtypes = [vp] + src + [i32, i32, vp, vp, i32, vp, vp, sz, C.POINTER(u64)]
    lib.dd_exact_subsets_from_hist.restype = i32
    lib.dd_exact_subsets_from_hist.argtypes = [vp, i32, vp]
    for name, src in (("dd_exact_locate", [paths_t]), ("dd_exact_locate_device", [ptrs_t, sizes_t])):
        fn = getattr(lib, name)
        fn.restype = i32
        fn.argtypes = [vp] + src + [i32, i32, vp, vp, vp, i32, vp, vp, C.POINTER(u64)]
    # a universe and samples: (paths, n, samples, ns) | (ptrs, sizes, n, ns)
    for name, src, extra in (("dd_exact_screen", [paths_t, i32, paths_t, i32], [vp, vp, i32, vp, vp]),
                             ("dd_exact_paint", [paths_t, i32, paths_t, i32], [u64, vp, vp]),
                             ("dd_exact_screen_device", [ptrs_t, sizes_t, i32, i32], [vp, vp, i32, vp, vp]),
                             ("dd_exact_paint_device", [ptrs_t, sizes_t, i32, i32], [u64, vp, vp]),
                             ("dd_exact_reads", [paths_t, i32, paths_t, i32], [vp, vp, C.c_uint32, vp, vp, vp, vp]),
                             ("dd_exact_reads_device", [ptrs_t, sizes_t, i32, i32], [vp, vp, C.c_uint32, vp, vp, vp, vp]),
                             ("dd_exact_depth", [paths_t, i32, paths_t, i32], [vp, vp, i32, i32, vp, vp]),
                             ("dd_exact_depth_device", [ptrs_t, sizes_t, i32, i32], [vp, vp, i32, i32, vp, vp]),
                             ("dd_exact_cover", [paths_t, i32, paths_t, i32], [vp, i32, u64, C.c_uint32, vp, vp]),
                             ("dd_exact_cover_device", [ptrs_t, sizes_t, i32, i32], [vp, i32, u64, C.c_uint32, vp, vp]),
                             ("dd_exact_gather", [paths_t, i32, paths_t, i32], [C.c_uint32, i32, vp, vp, vp, vp, vp]),
                             ("dd_exact_gather_device", [ptrs_t, sizes_t, i32, i32], [C.c_uint32, i32, vp, vp, vp, vp, vp])):
        fn = getattr(lib, name)
        fn.restype = i32
        fn.argtypes = [vp] + src + [i32] + extra + [C.POINTER(u64)]
    for name, src in (("dd_exact_patterns", [paths_t]), ("dd_exact_patterns_device", [ptrs_t, sizes_t])):
        fn = getattr(lib, name)
        fn.restype = i32
        fn.argtypes = [vp] + src + [i32, i32, vp, vp, sz, C.POINTER(u64), vp]
    lib.dd_fasta_index.restype = i32
    lib.dd_fasta_index.argtypes = [C.c_char_p, vp, vp, sz, C.POINTER(u64), vp, sz, C.POINTER(sz), C.POINTER(u64)]
    lib.dd_timing_enable.restype = i32
    lib.dd_timing_enable.argtypes = [vp, i32]
    lib.dd_timing_read.restype = i32
    lib.dd_timing_read.argtypes = [vp, i32, C.POINTER(C.c_double), C.POINTER(i32)]
    lib.dd_timing_reset.restype = i32
    lib.dd_timing_reset.argtypes = [vp]
    lib.dd_last_sketch_stats.restype = i32
    lib.dd_last_sketch_stats.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(i32)]
    lib.dd_last_k2_path.restype = i32
    lib.dd_last_k2_path.argtypes = [vp]
    lib.dd_last_k2_launches.restype = i32
    lib.dd_last_k2_launches.argtypes = [vp]
    lib.dd_synth_size.restype = sz
    lib.dd_synth_size.argtypes = [u64, i32]
    lib.dd_synth_fasta_device.restype = i32
    lib.dd_synth_fasta_device.argtypes = [vp, u64, i32, u64, i32, vp]
    lib.dd_synth_realistic_size.restype = sz
    lib.dd_synth_realistic_size.argtypes = [u64, u64]
    lib.dd_synth_realistic_device.restype = i32
    lib.dd_synth_realistic_device.argtypes = [vp, u64, i32, u64, vp]
    lib.dd_plan_sweep.restype = C.c_long
    lib.dd_plan_sweep.argtypes = [i32, C.POINTER(sz), i32, i32, i32, vp, C.c_long]
    if path is None:
        _lib = lib
    return lib


def ertl_mle(hist, log2m):
    """Host-side Ertl ML estimate of one 64-bin histogram (no device needed)."""
    h = np.ascontiguousarray(hist, dtype=np.uint32)
    if h.size != 64:
        raise ValueError("histogram must have 64 bins")
    return float(load_library().dd_ertl_mle(h.ctypes.data, int(log2m)))


def exact_subsets_from_hist(hist, n):
    """Host-side (no device needed): hist[mask] = k-mers with that membership mask over n <= 16 genomes -> uint64 [2^n],
    entry s the number of k-mers of the union of the genomes in s (dd_exact_subsets_from_hist)."""
    lib = load_library()
    h = np.ascontiguousarray(hist, dtype=np.uint64)
    if not 1 <= int(n) <= 16 or h.size != 1 << int(n):
        raise ValueError("histogram must have 2^n bins, 1 <= n <= 16")
    card = np.empty(h.size, dtype=np.uint64)
    rc = lib.dd_exact_subsets_from_hist(h.ctypes.data, int(n), card.ctypes.data)
    if rc != 0:
        raise EngineError(f"libdandd_hip error {rc}: {lib.dd_last_error().decode()}")
    return card


def fasta_index(path):
    """Host-side (no device needed): the records of one FASTA / FASTQ file, plain or gzip, as the exact calls read it ->
    (names list of str, seq_len uint64 [r], tok_start uint64 [r], ntok): tok_start[r] is the index in the file's token stream
    of the first base of record r (every record's BREAK token stands in front of it), ntok the stream's length
    (dd_fasta_index)."""
    lib = load_library()
    cap, names_cap = 1024, 1 << 16
    for _ in range(2):
        seq_len, tok_start = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint64)
        names = C.create_string_buffer(max(names_cap, 1))
        nrec, need, ntok = C.c_uint64(), C.c_size_t(), C.c_uint64()
        rc = lib.dd_fasta_index(os.fsencode(path), seq_len.ctypes.data, tok_start.ctypes.data, cap, C.byref(nrec), names, names_cap,
                                C.byref(need), C.byref(ntok))
        if rc != 0:
            err = EngineError(f"libdandd_hip error {rc}: {lib.dd_last_error().decode()}")
            err.code = rc
            raise err
        if nrec.value <= cap and need.value <= names_cap:
            r = int(nrec.value)
            text = names.raw[:need.value].split(b"\0")[:r]
            return [t.decode("utf-8", "replace") for t in text], seq_len[:r].copy(), tok_start[:r].copy(), int(ntok.value)
        cap, names_cap = max(cap, int(nrec.value)), max(names_cap, int(need.value))
    raise EngineError(f"dd_fasta_index: {path} changed between two reads")


def regions_from_hits(words, k, tok_start, seq_len):
    """Host-side, pure numpy: one job's hit bitmap of exact_locate (uint64 words, bit b of word w = token 64 w + b: a marked
    k-mer ENDS there) and the file's record index (fasta_index) -> per record an int64 [m][2] array of 0-based half-open
    (start, end) base intervals: the union of the spans [t - k + 1, t] of its hits, two hits merging iff they overlap or abut
    (t2 - t1 <= k).  A k-mer holds no BREAK, so a span lies inside its record; hits of different records never merge."""
    k = int(k)
    w = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
    bits = np.unpackbits(w.astype("<u8").view(np.uint8), bitorder="little")   # (little-endian bytes: byte i holds bits 8 i ..)
    t = np.flatnonzero(bits).astype(np.int64)
    starts, lens = np.asarray(tok_start, dtype=np.int64).reshape(-1), np.asarray(seq_len, dtype=np.int64).reshape(-1)
    rec = np.searchsorted(starts, t, side="right") - 1                  # the last record that starts at or before the hit
    out = []
    for r in range(starts.size):
        e = t[rec == r] - starts[r] + 1                                   # ends of the spans, in the record's bases
        if e.size and (e[0] < k or e[-1] > lens[r]):
            raise ValueError(f"record {r}: a hit outside the record's k-mers (k={k}, {int(lens[r])} bases)")
        fresh = np.ones(e.size, dtype=bool)
        fresh[1:] = np.diff(e) > k
        first = np.flatnonzero(fresh)
        last = np.append(first[1:], e.size) - 1
        out.append(np.stack([e[first] - k, e[last]], axis=1) if e.size else np.zeros((0, 2), dtype=np.int64))
    return out


def paint_windows(nwin, window, tok_start, seq_len):
    """Host-side, pure numpy: the windows of exact_paint (window w covers the tokens w * window .. (w + 1) * window - 1 of a
    file's token stream) and the file's record index (fasta_index) -> (record int64 [nwin], start int64 [nwin], end int64
    [nwin], records int64 [nwin]): the record that holds the window's first base, the 0-based half-open interval of that
    record's bases the window covers, and the number of records the window touches (holds a base of).  A window without a
    base -- nothing but BREAKs of empty records -- has record -1, the interval (0, 0) and 0 records."""
    nwin, window = int(nwin), int(window)
    starts, lens = np.asarray(tok_start, dtype=np.int64).reshape(-1), np.asarray(seq_len, dtype=np.int64).reshape(-1)
    lo = np.arange(nwin, dtype=np.int64) * window
    hi = lo + window                                                   # tokens [lo, hi)
    full = np.flatnonzero(lens > 0)                                    # the records that hold a base, by token: ascending, disjoint
    fs, fe = starts[full], starts[full] + lens[full]
    first = np.searchsorted(fe, lo, side="right")                      # the first of them that ends behind the window's start
    behind = np.searchsorted(fs, hi, side="left")                      # ... and the first that starts at or behind its end
    count = np.maximum(behind - first, 0)
    has = count > 0
    at = np.where(has, first, 0)
    record, start, end = np.full(nwin, -1, dtype=np.int64), np.zeros(nwin, dtype=np.int64), np.zeros(nwin, dtype=np.int64)
    if full.size:
        record[has] = full[at[has]]
        start[has] = np.maximum(lo[has] - fs[at[has]], 0)
        end[has] = np.minimum(hi[has], fe[at[has]]) - fs[at[has]]
    return record, start, end, count.astype(np.int64)


NO_GENOME = 0xFFFFFFFF   # exact_reads' calls: no best / no second genome


def read_classes(calls, sets, min_hits, n=64):
    """Host-side, pure numpy: the call arrays of exact_reads (calls uint32 [r][6], sets uint64 [r][2]) over n genomes (64: the
    most a universe holds) ->
    (classes int64 [r], tally uint64 [n+3]).  A row's class: n + 2 without a valid k-mer, n + 1 unclassified (its best column
    is below min_hits), the best genome's index where exactly one genome holds the best column, n -- ambiguous -- where
    several do.  tally[c]: the rows of class c, what the device counts per sample."""
    n, min_hits = int(n), int(min_hits)
    if min_hits < 1:
        raise ValueError("min_hits must be at least 1")
    calls = np.asarray(calls, dtype=np.uint32).reshape(-1, 6)
    ties = np.asarray(sets, dtype=np.uint64).reshape(-1, 2)[:, 0]
    several = (ties & (ties - np.uint64(1))) != 0                        # (ties = 0 only below min_hits: best_count = 0)
    classes = np.where(calls[:, 0] == 0, n + 2,
                       np.where(calls[:, 3] < min_hits, n + 1, np.where(several, n, calls[:, 2].astype(np.int64)))).astype(np.int64)
    return classes, np.bincount(classes, minlength=n + 3).astype(np.uint64)


def depth_stats(hist, total):
    """Host-side, pure numpy: the arrays of exact_depth (hist [...][bins], total [...]) -> a dict of arrays over the leading
    indices.  kmers (int64): the row's k-mers, the sum of all bins; covered (int64): those the sample holds, the bins >= 1;
    breadth = covered / kmers; mean = total / kmers; mean_covered = total / covered; median: the lower median of the depths
    of ALL the row's k-mers, zeros included -- the smallest d with hist[0] + .. + hist[d] >= (kmers + 1) // 2 --;
    median_covered: the same over the k-mers with depth >= 1; clipped (bool): a median lies in the last bin and is a lower
    bound only.  The five ratios and medians are float64 and NaN where they have nothing to stand on: all five for a row
    without a k-mer, mean_covered and median_covered for a row the sample holds nothing of (never None, never a raise)."""
    hist = np.asarray(hist, dtype=np.uint64).astype(np.int64)
    total = np.asarray(total, dtype=np.uint64).astype(np.float64)
    if hist.ndim < 1 or hist.shape[-1] < 2 or total.shape != hist.shape[:-1]:
        raise ValueError(f"hist {hist.shape} needs at least two bins and total {total.shape} its leading shape")
    last = hist.shape[-1] - 1
    kmers, covered = hist.sum(-1), hist[..., 1:].sum(-1)

    def ratio(a, b):
        return np.divide(a, b, out=np.full(b.shape, np.nan), where=b > 0)

    def median(h, count):   # the first bin at which the running sum reaches the lower median's rank; NaN without a record
        at = (np.cumsum(h, axis=-1) >= ((count + 1) // 2)[..., None]).argmax(-1)
        return np.where(count > 0, at, np.nan).astype(np.float64)
    med = median(hist, kmers)
    head = hist.copy()
    head[..., 0] = 0
    med_cov = median(head, covered)
    return {"kmers": kmers, "covered": covered, "breadth": ratio(covered.astype(np.float64), kmers), "mean": ratio(total, kmers),
            "mean_covered": ratio(total, covered), "median": med, "median_covered": med_cov, "clipped": (med == last) | (med_cov == last)}


COVER_EMPTY, COVER_PRESENT, COVER_ABSENT = 0, 1, 2   # cover_states' states of a window


def cover_states(counts, min_percent):
    """Host-side, pure numpy: one sample's rows of exact_cover along one target (uint32 [nwin][6]) -> (states int64 [nwin],
    runs int64 [m][3]).  A window's state: COVER_EMPTY where no valid k-mer ends in it (valid == 0), COVER_PRESENT where the
    sample holds at least min_percent per cent of its positions -- 100 * covered >= min_percent * valid, in integers --,
    COVER_ABSENT otherwise.  runs: the maximal runs of consecutive windows with the same state, in order, as (state, first
    window, windows); an empty window is a run of its own kind, it joins no neighbour."""
    min_percent = int(min_percent)
    if not 1 <= min_percent <= 100:
        raise ValueError(f"min_percent={min_percent} is outside 1..100")
    rows = np.asarray(counts, dtype=np.uint32).reshape(-1, 6).astype(np.int64)
    valid, covered = rows[:, 0], rows[:, 1]
    states = np.where(valid == 0, COVER_EMPTY, np.where(100 * covered >= min_percent * valid, COVER_PRESENT, COVER_ABSENT)).astype(np.int64)
    first = np.flatnonzero(np.append(True, states[1:] != states[:-1])) if states.size else np.zeros(0, dtype=np.int64)
    length = np.diff(np.append(first, states.size))
    return states, np.stack([states[first], first, length], axis=1).astype(np.int64).reshape(-1, 3)


def kmer_text(kmers, k):
    """Host-side (no device needed): uint64 [m][2] (lo, hi) records of dd_exact_select_kmers -> list of m strings of k bases,
    two bits per base, A = 0, C = 1, G = 2, T = 3, the first base most significant."""
    k = int(k)
    if not 1 <= k <= 64:
        raise ValueError(f"k={k} outside 1..64")
    rec = np.ascontiguousarray(kmers, dtype=np.uint64).reshape(-1, 2)
    pos = 2 * (k - 1 - np.arange(k))                                   # base j of the text: bits pos[j], pos[j] + 1 of the key
    word = np.where(pos >= 64, 1, 0)                                   # ... which lie in hi (column 1) from bit 64 on
    codes = (rec[:, word] >> (pos % 64).astype(np.uint64)) & np.uint64(3)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[codes.astype(np.intp)].reshape(-1, k)
    return [row.tobytes().decode("ascii") for row in text]


def synth_realistic_size(seed, nbases):
    return int(load_library().dd_synth_realistic_size(int(seed), int(nbases)))


def synth_size(nbases, nrec=1):
    return int(load_library().dd_synth_size(int(nbases), int(nrec)))


PLAN_JOB = np.dtype([("kclass", np.int32), ("mode", np.int32), ("lds_bytes", np.int32), ("genome", np.int32),
                     ("kfirst", np.int32), ("nk", np.int32), ("tile_begin", np.uint32), ("tile_end", np.uint32),
                     ("slice", np.int32)])


def plan_sweep(log2m, nbytes, kmin, kmax):
    """The K1 job table dd_sketch_device would use for genomes of `nbytes` bytes (structured array, launch
    order).  Pure host code in the library: works without a GPU."""
    lib = load_library()
    sizes = (C.c_size_t * len(nbytes))(*[int(n) for n in nbytes])
    n = lib.dd_plan_sweep(int(log2m), sizes, len(nbytes), int(kmin), int(kmax), None, 0)
    if n < 0:
        raise EngineError(f"libdandd_hip error {n}: {lib.dd_last_error().decode()}")
    out = np.zeros(n, dtype=PLAN_JOB)
    got = lib.dd_plan_sweep(int(log2m), sizes, len(nbytes), int(kmin), int(kmax), out.ctypes.data, n)
    assert got == n
    return out


def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def comm_unique_id():
    """The 128-byte id rank 0 makes for an RCCL communicator (dd_comm_unique_id); every rank passes it to Engine.comm_init."""
    lib = load_library()
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    rc = lib.dd_comm_unique_id(buf)
    if rc != 0:
        raise EngineError(f"libdandd_hip error {rc}: {lib.dd_last_error().decode()}")
    return bytes(buf)


class Engine:
    """One context = one GPU, one HLL size (log2m), canonical or not."""

    def __init__(self, device=0, log2m=14, canonical=True):
        self._lib = load_library()
        self.log2m = int(log2m)
        self.m = 1 << self.log2m
        self.canonical = bool(canonical)
        self.device = int(device)
        self._ctx = self._lib.dd_create(self.device, self.log2m, int(self.canonical))
        if not self._ctx:
            raise EngineError("dd_create failed: " + self._lib.dd_last_error().decode())

    # -- lifetime -------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.dd_destroy(self._ctx)
            self._ctx = None

    # -- plain device memory for callers without torch (the host layer keeps a collection's leaf slab resident) --------------
    _hip = None

    @classmethod
    def _hip_runtime(cls):
        """The HIP runtime libdandd_hip.so is bound to (same SONAME -> the copy already mapped), for hipMalloc / hipMemcpy / hipFree."""
        if cls._hip is None:
            for name in ("libamdhip64.so.7", "libamdhip64.so.6", "libamdhip64.so"):
                try:
                    h = C.CDLL(name)
                    break
                except OSError:
                    h = None
            if h is None:
                raise EngineError("libamdhip64.so not found")
            h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            h.hipFree.argtypes = [C.c_void_p]
            h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            h.hipSetDevice.argtypes = [C.c_int]
            cls._hip = h
        return cls._hip

    def device_alloc(self, nbytes):
        h = self._hip_runtime()
        ptr = C.c_void_p()
        if h.hipSetDevice(self.device) != 0 or h.hipMalloc(C.byref(ptr), int(nbytes)) != 0 or not ptr.value:
            raise EngineError(f"hipMalloc of {nbytes} bytes failed")
        return ptr.value

    def device_free(self, ptr):
        if ptr:
            self._hip_runtime().hipFree(C.c_void_p(int(ptr)))

    def device_upload(self, ptr, host):
        host = _u8(host)
        self.synchronize()
        if self._hip_runtime().hipMemcpy(C.c_void_p(int(ptr)), host.ctypes.data, host.nbytes, 1) != 0:   # hipMemcpyHostToDevice
            raise EngineError("hipMemcpy (host to device) failed")

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc):
        if rc != 0:
            err = EngineError(f"libdandd_hip error {rc}: {self._lib.dd_last_error().decode()}")
            err.code = rc
            raise err

    def set_stream(self, hip_stream):
        self._check(self._lib.dd_set_stream(self._ctx, C.c_void_p(int(hip_stream) if hip_stream else 0)))

    def synchronize(self):
        self._check(self._lib.dd_synchronize(self._ctx))

    # -- sketch ---------------------------------------------------------------------------
    def sketch_buffer(self, fasta, kmin, kmax):
        """FASTA bytes (host) -> registers [K][m] uint8."""
        a = _u8(np.frombuffer(fasta, dtype=np.uint8) if not isinstance(fasta, np.ndarray) else fasta)
        regs = np.empty((kmax - kmin + 1, self.m), dtype=np.uint8)
        self._check(self._lib.dd_sketch_buffer(self._ctx, a.ctypes.data, a.size, kmin, kmax, regs.ctypes.data))
        return regs

    def sketch_fasta(self, path, kmin, kmax):
        regs = np.empty((kmax - kmin + 1, self.m), dtype=np.uint8)
        self._check(self._lib.dd_sketch_fasta(self._ctx, os.fsencode(path), kmin, kmax, regs.ctypes.data))
        return regs

    def sketch_files(self, paths, kmin, kmax, nthreads=0):
        """Plain or .gz FASTA files -> registers [n][K][m]; read/inflate overlaps the GPU work."""
        n = len(paths)
        arr = (C.c_char_p * n)(*[os.fsencode(p) for p in paths])
        regs = np.empty((n, kmax - kmin + 1, self.m), dtype=np.uint8)
        self._check(self._lib.dd_sketch_files(self._ctx, arr, n, kmin, kmax, regs.ctypes.data, int(nthreads)))
        return regs

    # -- multi-GPU: RCCL behind the C ABI (one context = one process = one GPU) --------------
    def comm_init(self, rank, world, unique_id):
        """Join the communicator `unique_id` names (collective: every rank calls it, each on the GPU it owns)."""
        assert len(unique_id) == COMM_ID_BYTES
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id)
        self._check(self._lib.dd_comm_init(self._ctx, int(rank), int(world), buf))

    def comm_destroy(self):
        self._check(self._lib.dd_comm_destroy(self._ctx))

    def comm_info(self):
        """(rank, world, all-reduces issued, all-gathers issued); world 0 = no communicator."""
        r, w, a, g = C.c_int(), C.c_int(), C.c_ulonglong(), C.c_ulonglong()
        self._check(self._lib.dd_comm_info(self._ctx, C.byref(r), C.byref(w), C.byref(a), C.byref(g)))
        return r.value, w.value, a.value, g.value

    def allreduce_max_u8(self, regs_ptr, n):
        """In-place byte-max all-reduce of n register bytes at device address regs_ptr (ncclUint8 / ncclMax), on the context's stream."""
        self._check(self._lib.dd_allreduce_max_u8(self._ctx, C.c_void_p(int(regs_ptr)), int(n)))

    def allgather_u8(self, send_ptr, n, recv_ptr):
        """n bytes from every rank -> recv[world][n] on every rank (device addresses), on the context's stream."""
        self._check(self._lib.dd_allgather_u8(self._ctx, C.c_void_p(int(send_ptr)), int(n), C.c_void_p(int(recv_ptr))))

    def inflate_files(self, paths, nthreads=0):
        """The bytes the tokenizer reads for every file of a sketch_files pass (dd_inflate_files): for a .gz FASTA file the
        text `zcat` prints, inflated on the device where the device decoder takes the file.  -> list of uint8 arrays."""
        n = len(paths)
        arr = (C.c_char_p * n)(*[os.fsencode(p) for p in paths])
        caps = []
        for p in paths:       # room: the trailer's ISIZE for a .gz (a multi-member file's is too small: second try below), else the file
            size = os.path.getsize(p)
            with open(p, "rb") as f:
                head = f.read(2)
                if head == b"\x1f\x8b" and size >= 18:
                    f.seek(size - 4)
                    size = max(int.from_bytes(f.read(4), "little"), 4 * size)
            caps.append(size + 64)
        for _ in range(2):
            bufs = [np.empty(c, dtype=np.uint8) for c in caps]
            outs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
            ccaps = (C.c_size_t * n)(*caps)
            lens = (C.c_size_t * n)()
            rc = self._lib.dd_inflate_files(self._ctx, arr, n, outs, ccaps, lens, int(nthreads))
            if rc == 0 or all(lens[i] <= caps[i] for i in range(n)):
                break
            caps = [max(int(lens[i]), caps[i]) + 64 for i in range(n)]
        self._check(rc)
        return [bufs[i][:lens[i]] for i in range(n)]

    def last_ingest_stats(self):
        """(wall ms, ms waiting for the loader threads, batched launches, FASTA bytes) of the last sketch_files."""
        w, l, b, n = C.c_double(), C.c_double(), C.c_int(), C.c_uint64()
        self._check(self._lib.dd_last_ingest_stats(self._ctx, C.byref(w), C.byref(l), C.byref(b), C.byref(n)))
        return w.value, l.value, b.value, n.value

    def sketch_device(self, fasta_ptrs, nbytes, kmin, kmax, regs_ptr):
        """Batched HBM-resident sketch: device addresses in, regs_ptr[ng][K][m] device address out."""
        n = len(fasta_ptrs)
        ptrs = (C.c_void_p * n)(*[int(x) for x in fasta_ptrs])
        ns = (C.c_size_t * n)(*[int(x) for x in nbytes])
        self._check(self._lib.dd_sketch_device(self._ctx, ptrs, ns, n, kmin, kmax, C.c_void_p(int(regs_ptr))))

    # -- union / card ---------------------------------------------------------------------
    def union(self, sketches):
        arrs = [_u8(s) for s in sketches]
        n = arrs[0].size
        if any(a.size != n for a in arrs):
            raise ValueError("union inputs differ in size")
        out = np.empty_like(arrs[0])
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        self._check(self._lib.dd_union(self._ctx, ptrs, len(arrs), n, out.ctypes.data))
        return out

    def union_device(self, in_ptrs, nbytes, out_ptr):
        ptrs = (C.c_void_p * len(in_ptrs))(*[int(x) for x in in_ptrs])
        self._check(self._lib.dd_union_device(self._ctx, ptrs, len(in_ptrs), int(nbytes), C.c_void_p(int(out_ptr))))

    def card(self, regs):
        r = _u8(regs)
        if r.size != self.m:
            raise ValueError(f"expected {self.m} registers, got {r.size}")
        est = C.c_double()
        self._check(self._lib.dd_card(self._ctx, r.ctypes.data, C.byref(est)))
        return est.value

    def card_batch(self, regs):
        r = _u8(regs).reshape(-1, self.m)
        est = np.empty(r.shape[0], dtype=np.float64)
        self._check(self._lib.dd_card_batch(self._ctx, r.ctypes.data, r.shape[0], est.ctypes.data))
        return est

    def card_batch_device(self, regs_ptr, njobs):
        est = np.empty(njobs, dtype=np.float64)
        self._check(self._lib.dd_card_batch_device(self._ctx, C.c_void_p(int(regs_ptr)), njobs, est.ctypes.data))
        return est

    def hist_batch_device(self, regs_ptr, njobs):
        h = np.empty((njobs, 64), dtype=np.uint32)
        self._check(self._lib.dd_hist_batch_device(self._ctx, C.c_void_p(int(regs_ptr)), njobs, h.ctypes.data))
        return h

    # -- the schedules on register slabs: one body each, the slab in host memory or in HBM (dd_k2_api.hip) -----------------
    def _slab_src(self, leaf=None, leaf_ptr=None, n=None, K=None):
        """-> (the argument that names a slab entry's slab, n, K, the entry's suffix): a host array [n][K][m] (the argument
        keeps it alive for the call), or the device address of one with its n and K."""
        if leaf_ptr is not None:
            return C.c_void_p(int(leaf_ptr)), int(n), int(K), "_device"
        leaf = _u8(leaf)
        return leaf.ctypes, leaf.shape[0], leaf.shape[1], ""

    def _slab_sched(self, what, src, shape, *extra):
        leaf, n, K, suffix = src
        card = np.empty(shape + (K,), dtype=np.float64)
        self._check(getattr(self._lib, f"dd_{what}{suffix}")(self._ctx, leaf, n, K, *extra, card.ctypes.data))
        return card

    def _progressive(self, src, orderings):
        n = src[1]
        ords = np.ascontiguousarray(orderings, dtype=np.int32).reshape(-1, n)
        return self._slab_sched("progressive", src, (ords.shape[0], n), ords.ctypes.data, ords.shape[0])

    def _pairwise(self, src):
        return self._slab_sched("pairwise", src, (src[1], src[1]))

    def _subsets(self, src):
        return self._slab_sched("subsets", src, (1 << min(max(src[1], 0), 16),))

    def _leave_out(self, src, group, ngroups):
        grp = np.ascontiguousarray(group, dtype=np.int32).reshape(src[1])
        ngroups = int(grp.max()) + 1 if ngroups is None else int(ngroups)
        return self._slab_sched("leave_out", src, (max(ngroups, 0) + 1,), grp.ctypes.data, ngroups)

    def _extend(self, src, base, rows):
        leaf, n, K, suffix = src
        if rows is None:
            rows_ptr, nrows = None, n
        else:
            rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
            rows_ptr, nrows = rows.ctypes.data, rows.size
        card = np.empty((max(nrows, 0), K), dtype=np.float64)
        self._check(getattr(self._lib, "dd_extend" + suffix)(self._ctx, base, leaf, n, K, rows_ptr, nrows, card.ctypes.data))
        return card

    def _greedy(self, src, kmin, mode, cand, nfixed, nsteps):
        leaf, n, K, suffix = src
        cand = np.ascontiguousarray(np.arange(n) if cand is None else cand, dtype=np.int32).reshape(-1)
        nsteps = cand.size if nsteps is None else int(nsteps)
        order = np.empty(max(nsteps, 0), dtype=np.int32)
        card = np.empty((max(nsteps, 0), K), dtype=np.float64)
        self._check(getattr(self._lib, "dd_greedy" + suffix)(self._ctx, leaf, n, K, int(kmin), int(mode), cand.ctypes.data, cand.size,
                                                             int(nfixed), nsteps, order.ctypes.data, card.ctypes.data))
        return order, card

    def progressive(self, leaf, orderings):
        """leaf [n][K][m] uint8 (host), orderings [o][n] int -> card [o][n][K] float64."""
        return self._progressive(self._slab_src(leaf), orderings)

    def progressive_device(self, leaf_ptr, n, K, orderings):
        return self._progressive(self._slab_src(None, leaf_ptr, n, K), orderings)

    def pairwise(self, leaf):
        return self._pairwise(self._slab_src(leaf))

    def pairwise_device(self, leaf_ptr, n, K):
        return self._pairwise(self._slab_src(None, leaf_ptr, n, K))

    def _cross(self, entry, a, na, b, nb, K):
        card = np.empty((max(na, 0), max(nb, 0), max(K, 0)), dtype=np.float64)
        self._check(getattr(self._lib, entry)(self._ctx, a, na, b, nb, K, card.ctypes.data))
        return card

    def cross(self, a, b):
        """a [na][K][m], b [nb][K][m] uint8 (host) -> card [na][nb][K] float64: |a_s U b_j| at every k column."""
        a, b = _u8(a), _u8(b)
        if a.ndim != 3 or b.ndim != 3 or a.shape[1:] != b.shape[1:]:
            raise ValueError("cross: a and b must be [rows][K][m] slabs of the same K and m")
        return self._cross("dd_cross", a.ctypes.data, a.shape[0], b.ctypes.data, b.shape[0], a.shape[1])

    def cross_device(self, a_ptr, na, b_ptr, nb, K):
        """The same with both slabs in device memory."""
        return self._cross("dd_cross_device", C.c_void_p(int(a_ptr or 0)), int(na), C.c_void_p(int(b_ptr or 0)), int(nb), int(K))

    def cross_host_device(self, a, b_ptr, nb):
        """a [na][K][m] uint8 (host) against a slab of nb rows that stays where it is in device memory: new samples against
        a resident leaf slab."""
        a = _u8(a)
        if a.ndim != 3:
            raise ValueError("cross: a must be a [rows][K][m] slab")
        return self._cross("dd_cross_host_device", a.ctypes.data, a.shape[0], C.c_void_p(int(b_ptr or 0)), int(nb), a.shape[1])

    def leave_out(self, leaf, group, ngroups=None):
        """leaf [n][K][m] uint8 (host), group [n] int (-1: in every union) -> card [G+1][K] float64: row g the union of the
        leaves outside group g, row G the union of all.  G = max(group) + 1 unless given."""
        return self._leave_out(self._slab_src(leaf), group, ngroups)

    def leave_out_device(self, leaf_ptr, n, K, group, ngroups=None):
        return self._leave_out(self._slab_src(None, leaf_ptr, n, K), group, ngroups)

    def subsets(self, leaf):
        """leaf [n][K][m] uint8 (host), n <= 16 -> card [2^n][K] float64: row s the union of the leaves i with bit i of s set
        (row 0, the empty set, 0.0)."""
        return self._subsets(self._slab_src(leaf))

    def subsets_device(self, leaf_ptr, n, K):
        return self._subsets(self._slab_src(None, leaf_ptr, n, K))

    def extend(self, base, leaf, rows=None):
        """base [K][m] uint8 (host) or None (the empty sketch), leaf [n][K][m] uint8 (host), rows: leaf rows (None: all, in
        order; repeats allowed) -> card [nrows][K] float64: |base U leaf[rows[r]]|."""
        leaf = _u8(leaf)
        if base is not None:
            base = _u8(base)
            if base.size != leaf[0].size:
                raise ValueError("base is not one [K][m] sketch row of the slab")
        return self._extend(self._slab_src(leaf), None if base is None else base.ctypes.data, rows)

    def extend_device(self, base_ptr, leaf_ptr, n, K, rows=None):
        """The same with base (0 / None: the empty sketch) and the slab in device memory."""
        return self._extend(self._slab_src(None, leaf_ptr, n, K), C.c_void_p(int(base_ptr)) if base_ptr else None, rows)

    def greedy(self, leaf, kmin, mode, cand=None, nfixed=0, nsteps=None):
        """leaf [n][K][m] uint8 (host), columns k = kmin .. kmin + K - 1; mode GREEDY_MAX / GREEDY_MIN; cand: distinct leaf rows
        in tie-break order (None: all), the first nfixed of them a given start -> (order int32 [nsteps], card float64
        [nsteps][K]): the steepest (flattest) ordering by the selection rule of include/dandd_hip.h and its prefix unions."""
        return self._greedy(self._slab_src(leaf), kmin, mode, cand, nfixed, nsteps)

    def greedy_device(self, leaf_ptr, n, K, kmin, mode, cand=None, nfixed=0, nsteps=None):
        return self._greedy(self._slab_src(None, leaf_ptr, n, K), kmin, mode, cand, nfixed, nsteps)

    # -- exact distinct k-mer count (KMC stand-in) ----------------------------------------
    def exact_count(self, paths, k):
        """Distinct (canonical per the context) k-mers over all the FASTA files together."""
        arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
        d = C.c_uint64()
        self._check(self._lib.dd_exact_count(self._ctx, arr, len(paths), int(k), C.byref(d)))
        return d.value

    def exact_count_device(self, fasta_ptrs, nbytes, k):
        n = len(fasta_ptrs)
        ptrs = (C.c_void_p * n)(*[int(x) for x in fasta_ptrs])
        ns = (C.c_size_t * n)(*[int(x) for x in nbytes])
        d = C.c_uint64()
        self._check(self._lib.dd_exact_count_device(self._ctx, ptrs, ns, n, int(k), C.byref(d)))
        return d.value

    # -- exact union schedules: one sort of all n inputs per k (dd_exact_sched.hip) -----------
    def _exact_src(self, paths=None, fasta_ptrs=None, nbytes=None, samples=None, n=None):
        """-> (the arguments that name an exact entry's inputs, n, the entry's suffix).  A universe and samples -- `samples`
        beside paths, or the first `n` of the device buffers the universe and the rest the samples -- -> (.., n, ns, suffix),
        the arguments with both counts behind them as dd_exact_screen and dd_exact_paint take them."""
        if paths is not None:
            names = lambda files: (C.c_char_p * max(len(files), 1))(*[os.fsencode(p) for p in files])
            if samples is None:
                return [names(paths)], len(paths), ""
            return [names(paths), len(paths), names(samples), len(samples)], len(paths), len(samples), ""
        total = len(fasta_ptrs)
        args = [(C.c_void_p * total)(*[int(x) for x in fasta_ptrs]), (C.c_size_t * total)(*[int(x) for x in nbytes])]
        return (args, total, "_device") if n is None else (args + [int(n), total - int(n)], int(n), total - int(n), "_device")

    def _exact_sched(self, what, src, shape, kmin, kmax, *extra):
        args, n, suffix = src
        K = max(int(kmax) - int(kmin) + 1, 1)
        card = np.zeros(shape(n) + (K,), dtype=np.uint64)
        self._check(getattr(self._lib, f"dd_exact_{what}{suffix}")(self._ctx, *args, n, int(kmin), int(kmax), *extra, card.ctypes.data))
        return card

    def _exact_pairwise(self, src, kmin, kmax, wide=""):
        return self._exact_sched(wide + "pairwise", src, lambda n: (n, n), kmin, kmax)

    def _exact_progressive(self, src, kmin, kmax, orderings, wide=""):
        n = src[1]
        ords = np.ascontiguousarray(orderings, dtype=np.int32).reshape(-1, max(n, 1))
        return self._exact_sched(wide + "progressive", src, lambda n: (ords.shape[0], n), kmin, kmax, ords.ctypes.data, ords.shape[0])

    def _exact_leave_out(self, src, kmin, kmax, group, ngroups, wide=""):
        grp = np.ascontiguousarray(group, dtype=np.int32).reshape(-1)
        ngroups = int(grp.max()) + 1 if ngroups is None else int(ngroups)
        return self._exact_sched(wide + "leave_out", src, lambda n: (max(ngroups, 0) + 1,), kmin, kmax, grp.ctypes.data, ngroups)

    def _exact_subsets(self, src, kmin, kmax):
        return self._exact_sched("subsets", src, lambda n: (1 << min(max(n, 0), 16),), kmin, kmax)

    def exact_pairwise(self, paths, kmin, kmax):
        """FASTA files (n <= 64) -> uint64 [n][n][K]: distinct k-mers of every 2-way union (diagonal: of the file itself)."""
        return self._exact_pairwise(self._exact_src(paths=paths), kmin, kmax)

    def exact_pairwise_device(self, fasta_ptrs, nbytes, kmin, kmax):
        return self._exact_pairwise(self._exact_src(fasta_ptrs=fasta_ptrs, nbytes=nbytes), kmin, kmax)

    def exact_progressive(self, paths, kmin, kmax, orderings):
        """-> uint64 [o][n][K]: distinct k-mers of the union of the first j+1 files of every ordering (a permutation of 0..n-1)."""
        return self._exact_progressive(self._exact_src(paths=paths), kmin, kmax, orderings)

    def exact_progressive_device(self, fasta_ptrs, nbytes, kmin, kmax, orderings):
        return self._exact_progressive(self._exact_src(fasta_ptrs=fasta_ptrs, nbytes=nbytes), kmin, kmax, orderings)

    def exact_leave_out(self, paths, kmin, kmax, group, ngroups=None):
        """-> uint64 [G+1][K]: row g the union of the files outside group g (group[i] == -1: never left out), row G the union of all."""
        return self._exact_leave_out(self._exact_src(paths=paths), kmin, kmax, group, ngroups)

    def exact_leave_out_device(self, fasta_ptrs, nbytes, kmin, kmax, group, ngroups=None):
        return self._exact_leave_out(self._exact_src(fasta_ptrs=fasta_ptrs, nbytes=nbytes), kmin, kmax, group, ngroups)

    # ... and for up to 255 inputs (dd_exact_wide.hip): the same arguments, shapes and numbers, a row of up to four words per
    # distinct k-mer where the entries above keep one 64-bit mask
    def exact_wide_pairwise(self, paths, kmin, kmax):
        """exact_pairwise for 1 <= n <= 255 files -> uint64 [n][n][K]"""
        return self._exact_pairwise(self._exact_src(paths=paths), kmin, kmax, "wide_")

    def exact_wide_pairwise_device(self, fasta_ptrs, nbytes, kmin, kmax):
        return self._exact_pairwise(self._exact_src(fasta_ptrs=fasta_ptrs, nbytes=nbytes), kmin, kmax, "wide_")

    def exact_wide_progressive(self, paths, kmin, kmax, orderings):
        """exact_progressive for 1 <= n <= 255 files -> uint64 [o][n][K]"""
        return self._exact_progressive(self._exact_src(paths=paths), kmin, kmax, orderings, "wide_")

    def exact_wide_progressive_device(self, fasta_ptrs, nbytes, kmin, kmax, orderings):
        return self._exact_progressive(self._exact_src(fasta_ptrs=fasta_ptrs, nbytes=nbytes), kmin, kmax, orderings, "wide_")

    def exact_wide_leave_out(self, paths, kmin, kmax, group, ngroups=None):
        """exact_leave_out for 1 <= n <= 255 files -> uint64 [G+1][K]"""
        return self._exact_leave_out(self._exact_src(paths=paths), kmin, kmax, group, ngroups, "wide_")

    def exact_wide_leave_out_device(self, fasta_ptrs, nbytes, kmin, kmax, group, ngroups=None):
        return self._exact_leave_out(self._exact_src(fasta_ptrs=fasta_ptrs, nbytes=nbytes), kmin, kmax, group, ngroups, "wide_")

    def exact_subsets(self, paths, kmin, kmax):
        """n <= 16 files -> uint64 [2^n][K]: row s the union of the files i with bit i of s set (row 0: 0)."""
        return self._exact_subsets(self._exact_src(paths=paths), kmin, kmax)

    def exact_subsets_device(self, fasta_ptrs, nbytes, kmin, kmax):
        return self._exact_subsets(self._exact_src(fasta_ptrs=fasta_ptrs, nbytes=nbytes), kmin, kmax)

    # -- exact intersection schedules: the same sort, masks asked what they contain ---------------
    def _exact_spectrum(self, src, kmin, kmax):
        return self._exact_sched("spectrum", src, lambda n: (min(max(n, 0), 64) + 1,), kmin, kmax)

    def _exact_core_progressive(self, src, kmin, kmax, orderings):
        n = src[1]
        ords = np.ascontiguousarray(orderings, dtype=np.int32).reshape(-1, max(n, 1))
        return self._exact_sched("core_progressive", src, lambda n: (ords.shape[0], n), kmin, kmax, ords.ctypes.data, ords.shape[0])

    @staticmethod
    def _query_masks(all_masks, none_masks):
        """-> (all, none, nq): the queries of select and select_kmers as two uint64 arrays the library can read."""
        al = np.ascontiguousarray([int(x) for x in all_masks], dtype=np.uint64).reshape(-1)
        no = np.ascontiguousarray([int(x) for x in none_masks], dtype=np.uint64).reshape(-1)
        if al.size != no.size:
            raise ValueError("all_masks and none_masks must have the same length")
        if al.size == 0:   # (the library rejects nq = 0 by its own rule; it still wants two pointers)
            return np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64), 0
        return al, no, al.size

    def _exact_select(self, src, kmin, kmax, all_masks, none_masks):
        al, no, nq = self._query_masks(all_masks, none_masks)
        return self._exact_sched("select", src, lambda n: (nq,), kmin, kmax, al.ctypes.data, no.ctypes.data, nq)

    def exact_spectrum(self, paths, kmin, kmax):
        """FASTA files (n <= 64) -> uint64 [n+1][K]: row j the distinct k-mers held by exactly j of the files (row 0: 0)."""
        return self._exact_spectrum(self._exact_src(paths=paths), kmin, kmax)

    def exact_spectrum_device(self, fasta_ptrs, nbytes, kmin, kmax):
        return self._exact_spectrum(self._exact_src(fasta_ptrs=fasta_ptrs, nbytes=nbytes), kmin, kmax)

    def exact_core_progressive(self, paths, kmin, kmax, orderings):
        """-> uint64 [o][n][K]: distinct k-mers held by every one of the first j+1 files of every ordering (a permutation of 0..n-1)."""
        return self._exact_core_progressive(self._exact_src(paths=paths), kmin, kmax, orderings)

    def exact_core_progressive_device(self, fasta_ptrs, nbytes, kmin, kmax, orderings):
        return self._exact_core_progressive(self._exact_src(fasta_ptrs=fasta_ptrs, nbytes=nbytes), kmin, kmax, orderings)

    def exact_select(self, paths, kmin, kmax, all_masks, none_masks):
        """-> uint64 [nq][K]: row q the distinct k-mers held by every file of all_masks[q] and by no file of none_masks[q] (bit i: file i)."""
        return self._exact_select(self._exact_src(paths=paths), kmin, kmax, all_masks, none_masks)

    def exact_select_device(self, fasta_ptrs, nbytes, kmin, kmax, all_masks, none_masks):
        return self._exact_select(self._exact_src(fasta_ptrs=fasta_ptrs, nbytes=nbytes), kmin, kmax, all_masks, none_masks)

    # -- the selected k-mers themselves: the same sort for one k, the matching k-mers written out (emit_kernel) ------------
    KMERS_FIRST_CAP = 1 << 20

    def _exact_select_kmers(self, src, k, all_masks, none_masks, cap):
        args, n, suffix = src
        al, no, nq = self._query_masks(all_masks, none_masks)
        fn = getattr(self._lib, f"dd_exact_select_kmers{suffix}")
        room = self.KMERS_FIRST_CAP if cap is None else int(cap)
        for _ in range(2):
            kmers, masks = np.zeros((room, 2), dtype=np.uint64), np.zeros(room, dtype=np.uint64)
            found = C.c_uint64()
            self._check(fn(self._ctx, *args, n, int(k), al.ctypes.data, no.ctypes.data, nq, kmers.ctypes.data if room else None,
                           masks.ctypes.data if room else None, room, C.byref(found)))
            if found.value <= room:
                return kmers[:found.value], masks[:found.value]
            if cap is not None:
                err = EngineError(f"exact_select_kmers: {found.value} k-mers match, cap={room} records were asked for")
                err.found = found.value
                raise err
            room = found.value
        raise EngineError(f"exact_select_kmers: {found.value} k-mers match on the second call, {room} on the first")

    def exact_select_kmers(self, paths, k, all_masks, none_masks, cap=None):
        """FASTA files (n <= 64), one k, at most 1024 queries -> (kmers uint64 [found][2] (lo, hi), masks uint64 [found]): the
        distinct k-mers held by every file of all_masks[q] and by no file of none_masks[q] for at least one q, ascending
        (alphabetical; kmer_text decodes them), each with its membership mask.  cap=None: room for 2^20 records, and one more
        call with the count when there are more; a given cap that is too small raises EngineError naming the count."""
        return self._exact_select_kmers(self._exact_src(paths=paths), k, all_masks, none_masks, cap)

    def exact_select_kmers_device(self, fasta_ptrs, nbytes, k, all_masks, none_masks, cap=None):
        return self._exact_select_kmers(self._exact_src(fasta_ptrs=fasta_ptrs, nbytes=nbytes), k, all_masks, none_masks, cap)

    # -- the entries that look k-mers up in the ordered records: locate, and the five over samples that are no leaves --------
    def _exact_lookup(self, what, src, *rest):
        """dd_exact_{what} in the source's form: (ctx, the source's arguments, *rest, &found), checked; last_{what}_found = found."""
        found = C.c_uint64()
        self._check(getattr(self._lib, f"dd_exact_{what}{src[-1]}")(self._ctx, *src[0], *rest, C.byref(found)))
        setattr(self, f"last_{what}_found", int(found.value))

    @staticmethod
    def _window_offsets(ntok, which, window):
        """off uint64 [len(which) + 1]: stream which[j] owns ceil(ntok[which[j]] / window) rows from off[j] on; none where the
        window is no count or which[j] no stream, so that the library, not numpy, refuses them."""
        off = np.zeros(len(which) + 1, dtype=np.uint64)
        for j, t in enumerate(which):
            off[j + 1] = off[j] + np.uint64(-(-int(ntok[t]) // window) if window > 0 and 0 <= t < len(ntok) else 0)
        return off

    # -- where the selected k-mers lie: the same sort and emission, then every position looked up (dd_exact_locate.hip) ---
    last_locate_found = None   # of the last exact_locate call: the distinct k-mers that match at least one job's query
    def _exact_locate(self, src, k, jobs, ntok):
        _, n, _ = src
        jobs = [(int(a), int(b), int(g)) for a, b, g in jobs]
        nj = len(jobs)
        al = np.array([a for a, _, _ in jobs] or [0], dtype=np.uint64)
        no = np.array([b for _, b, _ in jobs] or [0], dtype=np.uint64)
        ge = np.array([g for _, _, g in jobs] or [0], dtype=np.int32)
        off = np.zeros(nj + 1, dtype=np.uint64)
        for j, (_, _, g) in enumerate(jobs):
            off[j + 1] = off[j] + np.uint64((int(ntok[g]) + 63) // 64 if 0 <= g < len(ntok) else 0)
        hits = np.zeros(max(int(off[nj]), 1), dtype=np.uint64)
        self._exact_lookup("locate", src, n, int(k), al.ctypes.data, no.ctypes.data, ge.ctypes.data, nj, off.ctypes.data, hits.ctypes.data)
        return [hits[int(off[j]):int(off[j + 1])].copy() for j in range(nj)]

    def exact_locate(self, paths, k, jobs, ntok=None):
        """FASTA files (n <= 64), one k, at most 1024 jobs (all_mask, none_mask, file index) -> list of uint64 arrays, one per
        job: a bitmap over the tokens of that file (fasta_index gives the records' places in it), bit b of word w set iff a
        valid k-mer ends at token 64 w + b and its membership mask contains all_mask and meets none_mask nowhere
        (regions_from_hits turns one into base intervals).  ntok: the files' token counts where the caller has them, else one
        fasta_index per file.  last_locate_found: the distinct k-mers that match at least one job's query."""
        if ntok is None:                                              # the shape of the answer: the inputs' token counts
            ntok = [fasta_index(p)[3] for p in paths]
        return self._exact_locate(self._exact_src(paths=paths), k, jobs, ntok)

    def exact_locate_device(self, fasta_ptrs, nbytes, k, jobs, ntok):
        """exact_locate over FASTA bytes on the device; ntok: every input's token count (the library checks them)."""
        return self._exact_locate(self._exact_src(fasta_ptrs=fasta_ptrs, nbytes=nbytes), k, jobs, ntok)

    # -- samples that are no leaves, screened against the universe's records (dd_exact_screen.hip) ------------------------
    last_screen_found = None   # of the last exact_screen call: the distinct k-mers of the universe
    def _exact_screen(self, src, k, all_masks, none_masks):
        _, n, ns, _ = src
        al, no, nq = self._query_masks(all_masks, none_masks)
        shared = np.zeros((max(ns, 0) + 1, max(n, 0)), dtype=np.uint64)
        match = np.zeros((max(ns, 0) + 1, nq), dtype=np.uint64)
        self._exact_lookup("screen", src, int(k), al.ctypes.data if nq else None, no.ctypes.data if nq else None, nq, shared.ctypes.data,
                           match.ctypes.data if nq else None)
        return shared, match

    def exact_screen(self, paths, samples, k, all_masks, none_masks):
        """FASTA files (n <= 64: the universe), sample files (FASTA / FASTQ, plain or gzip, ns <= 1024), one k, at most 1024
        queries -> (shared uint64 [ns+1][n], match uint64 [ns+1][nq]): shared[s][i] the distinct k-mers of sample s that
        file i also holds, match[s][q] those whose universe mask contains all_masks[q] and meets none_masks[q] nowhere; row
        ns is the universe itself (|file i|; what exact_select counts).  last_screen_found: the universe's distinct k-mers."""
        return self._exact_screen(self._exact_src(paths=paths, samples=samples), k, all_masks, none_masks)

    def exact_screen_device(self, fasta_ptrs, nbytes, n, k, all_masks, none_masks):
        """exact_screen over FASTA bytes on the device: the n universe inputs first, the samples behind them."""
        return self._exact_screen(self._exact_src(fasta_ptrs=fasta_ptrs, nbytes=nbytes, n=n), k, all_masks, none_masks)

    # -- samples painted window by window: the same records, then a walk that keeps the position (dd_exact_paint.hip) ------
    last_paint_found = None   # of the last exact_paint call: the distinct k-mers of the universe
    def _exact_paint(self, src, k, window, ntok):
        _, n, ns, _ = src
        window = int(window)
        off = self._window_offsets(ntok, range(ns), window)
        counts = np.zeros((max(int(off[-1]), 1), max(n, 0) + 2), dtype=np.uint32)
        self._exact_lookup("paint", src, int(k), window, off.ctypes.data, counts.ctypes.data)
        return [counts[int(off[s]):int(off[s + 1])].copy() for s in range(ns)]

    def exact_paint(self, paths, samples, k, window, ntok=None):
        """FASTA files (n <= 64: the universe), sample files (FASTA / FASTQ, plain or gzip, ns <= 1024), one k, a window of
        `window` tokens (a multiple of 64 in 64 .. 2^22) -> list of uint32 [nwin_s][n+2] arrays, one per sample, a row per
        window of the sample's token stream (paint_windows gives the windows' places in the records): column 0 the tokens of
        the window at which a valid k-mer ends, column 1 those whose k-mer the universe holds, column 2 + i those whose k-mer
        file i holds.  Counts are over positions.  ntok: the samples' token counts where the caller has them, else one
        fasta_index per sample.  last_paint_found: the universe's distinct k-mers."""
        if ntok is None:                                              # the shape of the answer: the samples' token counts
            ntok = [fasta_index(p)[3] for p in samples]
        return self._exact_paint(self._exact_src(paths=paths, samples=samples), k, window, ntok)

    def exact_paint_device(self, fasta_ptrs, nbytes, n, k, window, ntok):
        """exact_paint over FASTA bytes on the device: the n universe inputs first, the samples behind them; ntok: every
        sample's token count (the library checks them)."""
        return self._exact_paint(self._exact_src(fasta_ptrs=fasta_ptrs, nbytes=nbytes, n=n), k, window, ntok)

    # -- samples called row by row: paint's walk with the caller's borders, a vote per row, a tally per sample (dd_exact_reads.hip)
    last_reads_found = None   # of the last exact_reads call: the distinct k-mers of the universe
    def _exact_reads(self, src, k, min_hits, rows, calls, counts):
        _, n, ns, _ = src
        if len(rows) != ns:
            raise ValueError(f"{len(rows)} border arrays for {ns} samples")
        starts = [np.ascontiguousarray(r, dtype=np.uint64).reshape(-1) for r in rows]
        off = np.zeros(max(ns, 0) + 1, dtype=np.uint64)
        off[1:ns + 1] = np.cumsum([len(r) for r in starts], dtype=np.uint64) if ns > 0 else []
        total = int(off[max(ns, 0)])
        start = np.concatenate(starts + [np.zeros(1, dtype=np.uint64)])
        call_arr = np.zeros((max(total, 1), 6), dtype=np.uint32) if calls else None
        set_arr = np.zeros((max(total, 1), 2), dtype=np.uint64) if calls else None
        count_arr = np.zeros((max(total, 1), max(n, 0) + 2), dtype=np.uint32) if counts else None
        tally = np.zeros((max(ns, 1), max(n, 0) + 3), dtype=np.uint64)
        ptr = lambda a: None if a is None else a.ctypes.data
        self._exact_lookup("reads", src, int(k), off.ctypes.data, start.ctypes.data, int(min_hits), ptr(call_arr), ptr(set_arr), ptr(count_arr),
                           tally.ctypes.data)
        cut = lambda a, s: None if a is None else a[int(off[s]):int(off[s + 1])].copy()
        return [(cut(call_arr, s), cut(set_arr, s), cut(count_arr, s)) for s in range(ns)], tally[:max(ns, 0)]

    def exact_reads(self, paths, samples, k, min_hits=1, index=None, rows=None, calls=True, counts=False):
        """FASTA files (n <= 64: the universe), sample files (FASTA / FASTQ, plain or gzip, ns <= 1024), one k -> (per sample
        (calls uint32 [r][6], sets uint64 [r][2], counts uint32 [r][n+2] or None), tally uint64 [ns][n+3]).  By default a
        row is a record of the sample -- a read, a contig: the borders are tok_start of fasta_index(sample), or of `index`
        where the caller has it ([(names, seq_len, tok_start, ntok)] per sample); rows= gives per-sample border arrays of
        its own (tokens, strictly ascending, <= ntok; row r runs to the next border, the last to the sample's end).
        counts: exact_paint's columns per row.  calls: valid, hit, best, best_count, second, second_count (NO_GENOME: none);
        sets: the genomes tied at best_count, the genomes that hold every universe position of the row.  tally[s]: the rows
        uniquely called to genome i, then the ambiguous, the unclassified (best_count < min_hits) and those without a valid
        k-mer (read_classes).  calls=False returns (None, None, counts) per sample: with counts=False the tally alone comes
        back from the device.  last_reads_found: the universe's distinct k-mers."""
        if rows is None:
            rows = [ix[2] for ix in (index if index is not None else [fasta_index(p) for p in samples])]
        return self._exact_reads(self._exact_src(paths=paths, samples=samples), k, min_hits, rows, calls, counts)

    def exact_reads_device(self, fasta_ptrs, nbytes, n, k, rows, min_hits=1, calls=True, counts=False):
        """exact_reads over FASTA bytes on the device: the n universe inputs first, the samples behind them; rows: every
        sample's borders (the library checks them against the token counts)."""
        return self._exact_reads(self._exact_src(fasta_ptrs=fasta_ptrs, nbytes=nbytes, n=n), k, min_hits, rows, calls, counts)

    # -- samples counted record by record: screen's walk with a counter per record, binned by depth (dd_exact_depth.hip) -------
    last_depth_found = None   # of the last exact_depth call: the distinct k-mers of the universe
    def _exact_depth(self, src, k, all_masks, none_masks, bins):
        _, n, ns, _ = src
        al, no, nq = self._query_masks(all_masks, none_masks)
        rows, bins = max(n, 0) + nq, int(bins)
        hist = np.zeros((max(ns, 1), max(rows, 1), min(max(bins, 1), 1 << 16)), dtype=np.uint64)
        total = np.zeros((max(ns, 1), max(rows, 1)), dtype=np.uint64)
        self._exact_lookup("depth", src, int(k), al.ctypes.data if nq else None, no.ctypes.data if nq else None, nq, bins, hist.ctypes.data,
                           total.ctypes.data)
        return hist, total

    def exact_depth(self, paths, samples, k, alls=(), nones=(), bins=64):
        """FASTA files (n <= 64: the universe), sample files (FASTA / FASTQ, plain or gzip, ns <= 1024), one k, at most 1024
        queries, 2 <= bins <= 256 -> (hist uint64 [ns][n+nq][bins], total uint64 [ns][n+nq]).  Row i < n: the distinct k-mers
        of file i; row n + q: those whose universe mask contains alls[q] and meets nones[q] nowhere.  hist[s][row][d]:
        the k-mers of the row that stand d times in sample s (positions, as exact_paint counts them; d = 0: the sample lacks
        them), the last bin taking every depth >= bins - 1; total: the sum of the depths, unclipped (depth_stats turns both
        into breadth, mean and median).  last_depth_found: the universe's distinct k-mers."""
        return self._exact_depth(self._exact_src(paths=paths, samples=samples), k, alls, nones, bins)

    def exact_depth_device(self, fasta_ptrs, nbytes, n, k, alls=(), nones=(), bins=64):
        """exact_depth over FASTA bytes on the device: the n universe inputs first, the samples behind them."""
        return self._exact_depth(self._exact_src(fasta_ptrs=fasta_ptrs, nbytes=nbytes, n=n), k, alls, nones, bins)

    # -- samples laid along the genomes of the universe: depth's counters gathered per window of a target (dd_exact_cover.hip) --
    last_cover_found = None   # of the last exact_cover call: the distinct k-mers of the universe
    def _exact_cover(self, src, k, window, targets, clip, ntok):
        _, n, ns, _ = src
        window = int(window)
        targets = list(range(max(n, 0))) if targets is None else [int(t) for t in targets]
        nt = len(targets)
        tg = np.array(targets or [0], dtype=np.int32)
        off = self._window_offsets(ntok, targets, window)
        counts = np.zeros((max(ns, 1), max(int(off[nt]), 1), 6), dtype=np.uint32)
        self._exact_lookup("cover", src, int(k), tg.ctypes.data, nt, window, int(clip), off.ctypes.data, counts.ctypes.data)
        return [counts[:max(ns, 0), int(off[j]):int(off[j + 1])].copy() for j in range(nt)]

    def exact_cover(self, paths, samples, k, window, targets=None, clip=255, ntok=None):
        """FASTA files (n <= 64: the universe), sample files (FASTA / FASTQ, plain or gzip, ns <= 1024), one k, a window of
        `window` tokens (a multiple of 64 in 64 .. 2^22), targets: indices of `paths`, each once (None: all of them), 1 <= clip
        <= 1023 -> list of uint32 [ns][nwin_t][6] arrays, one per target, a row per sample and window of the TARGET's token
        stream (paint_windows gives the windows' places in its records).  With c the times the sample holds the k-mer that
        ends at a position (exact_depth's depth): column 0 the positions of the window at which a valid k-mer ends, column 1
        those with c >= 1, column 2 the sum of min(c, clip) over them; columns 3..5 the same over the positions whose k-mer no
        other file of the universe holds.  Columns 0 and 3 do not depend on the sample (cover_states turns a sample's rows
        into present / absent windows and their runs).  ntok: the token counts of `paths` where the caller has them, else
        one fasta_index per target.  last_cover_found: the universe's distinct k-mers."""
        if ntok is None:                                              # the shape of the answer: the targets' token counts
            want = range(len(paths)) if targets is None else [int(t) for t in targets]
            ntok = [fasta_index(p)[3] if i in want else 0 for i, p in enumerate(paths)]
        return self._exact_cover(self._exact_src(paths=paths, samples=samples), k, window, targets, clip, ntok)

    def exact_cover_device(self, fasta_ptrs, nbytes, n, k, window, ntok, targets=None, clip=255):
        """exact_cover over FASTA bytes on the device: the n universe inputs first, the samples behind them; ntok: every
        universe input's token count (the library checks the targets')."""
        return self._exact_cover(self._exact_src(fasta_ptrs=fasta_ptrs, nbytes=nbytes, n=n), k, window, targets, clip, ntok)

    # -- samples explained by the genomes one by one: a greedy set cover over depth's counters, walked on the device (dd_exact_gather.hip) --
    last_gather_found = None   # of the last exact_gather call: the distinct k-mers of the universe
    def _exact_gather(self, src, k, min_hits, steps):
        _, n, ns, _ = src
        steps = max(n, 0) if steps is None else int(steps)
        if not 0 <= int(min_hits) < 1 << 32:
            raise ValueError(f"min_hits={min_hits} is no 32-bit count")   # (ctypes would wrap it; 0 is the library's to refuse)
        rows, cols = max(ns, 1), min(max(steps, 1), 64)                   # (room for the library to refuse what is out of range)
        pick = np.full((rows, cols), -1, dtype=np.int32)
        unique, depth = np.zeros((rows, cols), dtype=np.uint64), np.zeros((rows, cols), dtype=np.uint64)
        shared, total = np.zeros((rows, max(n, 1)), dtype=np.uint64), np.zeros((rows, 2), dtype=np.uint64)
        self._exact_lookup("gather", src, int(k), int(min_hits), steps, pick.ctypes.data, unique.ctypes.data, depth.ctypes.data, shared.ctypes.data,
                           total.ctypes.data)
        return pick, unique, depth, shared, total

    def exact_gather(self, paths, samples, k, min_hits=1, steps=None):
        """FASTA files (n <= 64: the universe), sample files (FASTA / FASTQ, plain or gzip, ns <= 1024), one k, min_hits >= 1,
        1 <= steps <= n (None: n) -> (pick int32 [ns][steps], unique uint64 [ns][steps], depth uint64 [ns][steps], shared
        uint64 [ns][n], total uint64 [ns][2]): the greedy set cover of every sample's k-mers by the files.  pick[s][t]: the
        file that holds most of the distinct k-mers of sample s (of those the universe holds) that no earlier pick holds,
        ties to the lowest index; unique[s][t]: how many those are, depth[s][t]: the times the sample holds them, summed
        (exact_depth's depth).  The walk stops at a pick with fewer than min_hits k-mers; behind the stop pick = -1 and
        zeros.  shared[s][i]: exact_screen's shared; total[s]: the sample's distinct k-mers in the universe and the sum of
        their depths.  last_gather_found: the universe's distinct k-mers."""
        return self._exact_gather(self._exact_src(paths=paths, samples=samples), k, min_hits, steps)

    def exact_gather_device(self, fasta_ptrs, nbytes, n, k, min_hits=1, steps=None):
        """exact_gather over FASTA bytes on the device: the n universe inputs first, the samples behind them."""
        return self._exact_gather(self._exact_src(fasta_ptrs=fasta_ptrs, nbytes=nbytes, n=n), k, min_hits, steps)

    # -- the membership-pattern table: the distinct masks and how many k-mers carry each (dd_exact_patterns.hip) ------------
    last_patterns_stats = None   # of the last exact_patterns call: (distinct k-mers, pairs written to HBM, forced flushes, single masks)

    def _exact_patterns(self, src, k, cap):
        args, n, suffix = src
        fn = getattr(self._lib, f"dd_exact_patterns{suffix}")

        def call(room):
            masks, counts = np.zeros(room, dtype=np.uint64), np.zeros(room, dtype=np.uint64)
            found, stats = C.c_uint64(), np.zeros(4, dtype=np.uint64)
            self._check(fn(self._ctx, *args, n, int(k), masks.ctypes.data if room else None, counts.ctypes.data if room else None, room,
                           C.byref(found), stats.ctypes.data))
            self.last_patterns_stats = tuple(int(v) for v in stats)
            m = min(int(found.value), room)
            return masks[:m], counts[:m], int(found.value)
        if cap is not None:
            return call(max(int(cap), 0))
        got = call(0)                     # a pure count, then room for every row
        return call(got[2]) if got[2] else got

    def exact_patterns(self, paths, k, cap=None):
        """FASTA files (n <= 64), one k -> (masks uint64 [m], counts uint64 [m], found): the distinct membership masks (bit i:
        file i) and the distinct k-mers that carry exactly each, count descending, ties by mask ascending; found: the number
        of distinct masks, m = min(found, cap) -- a cap below found gives the top cap rows.  cap=None: two calls, one that
        counts and one with room for every row.  last_patterns_stats: the stats of the last call (include/dandd_hip.h)."""
        return self._exact_patterns(self._exact_src(paths=paths), k, cap)

    def exact_patterns_device(self, fasta_ptrs, nbytes, k, cap=None):
        return self._exact_patterns(self._exact_src(fasta_ptrs=fasta_ptrs, nbytes=nbytes), k, cap)

    # -- exact greedy: the masks of every k kept on the device, one read of them per step (dd_exact_greedy.hip) ---------
    def _exact_greedy(self, src, kmin, kmax, mode, cand, nfixed, nsteps):
        args, n, suffix = src
        K = max(int(kmax) - int(kmin) + 1, 1)
        cand = np.ascontiguousarray(np.arange(n) if cand is None else cand, dtype=np.int32).reshape(-1)
        nsteps = cand.size if nsteps is None else int(nsteps)
        order = np.zeros(max(nsteps, 0), dtype=np.int32)
        card = np.zeros((max(nsteps, 0), K), dtype=np.uint64)
        self._check(getattr(self._lib, f"dd_exact_greedy{suffix}")(self._ctx, *args, n, int(kmin), int(kmax), int(mode), cand.ctypes.data,
                                                                  cand.size, int(nfixed), nsteps, order.ctypes.data, card.ctypes.data))
        return order, card

    def exact_greedy(self, paths, kmin, kmax, mode, cand=None, nfixed=0, nsteps=None):
        """FASTA files (n <= 64); mode GREEDY_MAX / GREEDY_MIN; cand: distinct files in tie-break order (None: all), the first
        nfixed of them a given start -> (order int32 [nsteps], card uint64 [nsteps][K]): the steepest (flattest) ordering by the
        selection rule of include/dandd_hip.h and the distinct k-mers of its prefix unions.  EngineError with code ENOMEM when
        the masks of the window do not fit DD_EXACT_MASKS_MB."""
        return self._exact_greedy(self._exact_src(paths=paths), kmin, kmax, mode, cand, nfixed, nsteps)

    def exact_greedy_device(self, fasta_ptrs, nbytes, kmin, kmax, mode, cand=None, nfixed=0, nsteps=None):
        return self._exact_greedy(self._exact_src(fasta_ptrs=fasta_ptrs, nbytes=nbytes), kmin, kmax, mode, cand, nfixed, nsteps)

    # -- measurement ----------------------------------------------------------------------
    def timing_enable(self, on=True):
        self._check(self._lib.dd_timing_enable(self._ctx, int(bool(on))))

    def timing_reset(self):
        self._check(self._lib.dd_timing_reset(self._ctx))

    def timing_read(self, which):
        ms, n = C.c_double(), C.c_int()
        self._check(self._lib.dd_timing_read(self._ctx, which, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def last_sketch_stats(self):
        t, u, b = C.c_uint64(), C.c_uint64(), C.c_int()
        self._check(self._lib.dd_last_sketch_stats(self._ctx, C.byref(t), C.byref(u), C.byref(b)))
        return t.value, u.value, b.value

    K2_PATHS = {0: None, 1: "progressive_stream", 2: "progressive_pscan", 3: "pairwise_stream", 4: "pairwise_gram", 5: "cross_stream", 6: "cross_gram"}

    def last_k2_path(self):
        """Which device form the last progressive / pairwise call took (include/dandd_hip.h: DD_K2_*)."""
        rc = self._lib.dd_last_k2_path(self._ctx)
        if rc < 0:
            self._check(rc)
        return self.K2_PATHS[rc]

    def last_k2_launches(self):
        """How many gram_kernel / cross_kernel launches the last pairwise / cross call enqueued, summed over cross's rounds
        (0: a streaming form).  DD_GRAM_PART_MB sets what the partial counts of one launch may take."""
        rc = self._lib.dd_last_k2_launches(self._ctx)
        if rc < 0:
            self._check(rc)
        return rc

    def warmup(self):
        """One tiny sketch + cardinality: HIP loads a kernel module at its first launch, this makes the first launches
        happen now (on whichever thread calls it) instead of inside the first real call."""
        fa = np.frombuffer(b">w\n" + b"ACGTTGCAACGGTCA" * 16 + b"\n", dtype=np.uint8)
        self.card_batch(self.sketch_buffer(fa, 15, 17))

    def synth_realistic_device(self, seed, genome_index, nbases, out_ptr):
        self._check(self._lib.dd_synth_realistic_device(self._ctx, int(seed), int(genome_index), int(nbases), C.c_void_p(int(out_ptr))))

    def synth_fasta_device(self, seed, genome_index, nbases, nrec, out_ptr):
        self._check(self._lib.dd_synth_fasta_device(self._ctx, int(seed), int(genome_index), int(nbases),
                                                    int(nrec), C.c_void_p(int(out_ptr))))

// dd_ingest.hip -- the file-ingestion pipeline of the C ABI (dd_sketch_fasta, dd_sketch_files, dd_inflate_files,
// dd_last_ingest_stats).  Host code only; the device decoders are dd_ginflate.hip, dd_gunzip.hip and dd_fastq.hip.
// Many FASTA files (plain or .gz, as DandD's species directories hold them); regs is [nfiles][K][m] on the host.
// A pipeline:
//   loader threads   read + inflate into pinned host buffers of the context's pool, ahead of the GPU,
//                    bounded by the pool (a directory of whole genomes cannot exhaust host memory);
//   copy stream      H2D of batch b+1 while the compute stream sketches batch b, D2H of batch b-1's
//                    register slabs into a pinned bounce buffer (event-chained, no per-file sync);
//   compute stream   ONE dd_sketch_device launch per batch -- consecutive small files are coalesced until a
//                    batch holds ~128 MB, so a directory of 5 Mbp genomes fills the chip instead of
//                    launching 77 workgroups per file.
// The reference's loop is one genome at a time, each re-read and re-inflated once per k.
#include <sys/stat.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include "dd_ctx.h"
using dd::FileBuf;
using dd::GzMember;
namespace {
double now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// ------------------------------------------------------------------------------ knobs
int env_int(const char* name, int lo, int unset) { return getenv(name) ? std::max(lo, atoi(getenv(name))) : unset; }
// every DD_* setting the pipeline reads, read once per dd_sketch_files call (constructing one reads them)
bool env_set(const char* name) { return getenv(name) != nullptr; }
struct Knobs {
    int batch_mb = env_int("DD_BATCH_MB", 1, 0);                                    // text per launch (0: the call plan's choice)
    size_t gunzip_min = (size_t)env_int("DD_GUNZIP_MIN_KB", 1, 1024) << 10;         // the smallest .gz the device gunzip takes
    size_t raw_pieces_from = (size_t)env_int("DD_GUNZIP_PIECES_MB", 1, 32) << 20;   // a .gz this large is read in pieces
    int guess_kb = env_int("DD_GUNZIP_GUESS_KB", 4, 0);                             // the gunzip's range per piece (0: by file size)
    bool no_gpu_inflate = env_set("DD_NO_GPU_INFLATE"), no_gpu_gunzip = env_set("DD_NO_GPU_GUNZIP"), no_gpu_fastq = env_set("DD_NO_GPU_FASTQ");
    bool strict = env_set("DD_INFLATE_STRICT");                                     // no second try with the host decoder ...
    int strict_level = strict ? atoi(getenv("DD_INFLATE_STRICT")) : 0;              // ... and at 2 a context switched to it says so
    bool trace = env_set("DD_TRACE_FILES");                                         // a stderr line per batch and one per call
    // (single-member gzip files: the finder looks at one range of `guess_bits` per piece; 32 KiB of compressed data are ~2
    // deflate blocks of gzip -6 DNA, so a third of every range is scanned before its first block start turns up)
    // (files of 48 MB and more take 64 KiB ranges: half as many links in the chain of windows, which one workgroup per
    // file walks at ~7 us a piece -- 1 x 400 Mbp: 5.4 -> 6.9 Gbp/s, 3 x 300 Mbp: 7.2 -> 8.1)
    // (round 5, with the windows composed in two levels: 16 KiB up to 400 MB of compressed file (was 32, and 64 from 48 MB: one
    // 400 Mbp member 7.5-7.7 -> 8.3 Gbp/s at gzip -1, 9.7-10.1 -> 10.3 at gzip -6) -- ten 50 Mbp gzip -1 files 7.2 -> 7.9-8.3
    // Gbp/s with 16 / 8 KiB, gzip -6 11.1 -> 11.5 / 11.3, 64 x 5 Mbp 9.1 -> 9.2 / 9.6; profiles/r05_gunzip.txt)
    size_t guess_bits(size_t compressed_bytes) const {
        return (size_t)(guess_kb ? guess_kb : (compressed_bytes >= ((size_t)400 << 20) ? 128 : 16)) << 13;
    }
};
// a range's symbols: 5 x its compressed bytes (DNA inflates 3-4 x) + 32 Ki; a piece that needs more takes the arena -- and a
// second and third pass of the decoder over it (count, then write).  Round 6: the factor follows the MEMBER's own ratio
// (twice ISIZE / compressed length: a piece runs from the first block start of its range to the first of the next, up to
// two ranges' worth of bits) when that is larger -- four-line FASTQ whose quality text compresses well inflates 6 x, most
// pieces overflowed, and inflate_kernel<1> + <2> cost a batch 12.5 ms beside the 9.9 of <3> (profiles/r06_ingest.txt);
// capped at 64 x: beyond that (runs of N) the arena is the right place
size_t range_syms_of(size_t guess_bits, size_t isize, size_t clen) {
    const double ratio = clen ? 2.0 * (double)isize / (double)clen : 0.0;
    const double f = std::min(64.0, std::max(5.0, ratio));
    return (size_t)(f * (double)(guess_bits / 8)) + 32768;
}
// ------------------------------------------------------------------------------ file formats
// One BGZF file's blocks, found on the host (a walk over the 'BC' size fields: ~800 per 50 Mbp file); the blocks
// themselves are inflated on the device.  false: not a BGZF file the device path takes (the host decoder reads it).
struct BgzfBlock {
    size_t in_off;
    uint32_t in_len, out_len;
    size_t out_off;
};
// the n bytes of an open file into fb (closes f)
bool read_whole(FILE* f, size_t n, dd::FileBuf& fb) {
    fb.len = 0;
    const bool ok = fb.reserve(n + 16) && fseeko(f, 0, SEEK_SET) == 0 && fread(fb.p, 1, n, f) == n;
    fclose(f);
    return ok;
}
// (for a file whose bytes are in memory: large files are read in pieces by several loaders)
bool bgzf_parse(const uint8_t* data, size_t n, std::vector<BgzfBlock>& blks, size_t& out_size, bool& fastq, bool no_gpu_fastq) {
    using namespace dd::inflate_detail;
    blks.clear();
    size_t p = 0, total = 0;
    while (p < n) {
        const size_t bs = bgzf_block_size(data + p, n - p);
        if (!bs) {
            for (size_t q = p; q < n; ++q)
                if (data[q]) return false;   // (trailing zeros are tolerated, as gzread tolerates them)
            break;
        }
        const uint8_t* t = data + p + bs - 4;
        const size_t isize = (size_t)t[0] | ((size_t)t[1] << 8) | ((size_t)t[2] << 16) | ((size_t)t[3] << 24);
        if (isize > 65536) return false;
        blks.push_back(BgzfBlock{p, (uint32_t)bs, (uint32_t)isize, total});   // (empty members too -- the EOF block --: their CRC-32 and ISIZE are checked like any other's)
        total += isize;
        p += bs;
    }
    if (blks.empty()) return false;
    // (the text rules of dd_fastq.hip and TextJob hold offsets in 32 bits, as the gzip path's do: a text of 4 GiB or more is
    // for the host decoder -- the same bound as gzip_members_parse's)
    if (total >= ((uint64_t)1 << 32) - 65536) return false;
    // FASTQ (reads, not assemblies) starts with '@': look at the first block's text
    {
        uint8_t first[256];
        z_stream zs;
        memset(&zs, 0, sizeof zs);
        if (inflateInit2(&zs, 15 + 16) != Z_OK) return false;
        zs.next_in = const_cast<uint8_t*>(data) + blks[0].in_off;
        zs.avail_in = blks[0].in_len;
        zs.next_out = first;
        zs.avail_out = sizeof first;
        const int zr = inflate(&zs, Z_SYNC_FLUSH);
        const size_t made = sizeof first - zs.avail_out;
        inflateEnd(&zs);
        if ((zr != Z_OK && zr != Z_STREAM_END) || !made) return false;
        // (round 5: a text that starts with '@' stays on the device as four-line FASTQ, checked record by record there: dd_fastq.hip)
        fastq = first[0] == '@';
        if (fastq ? no_gpu_fastq : dd::has_plus_line(first, made)) return false;
    }
    out_size = total;
    return true;
}
bool bgzf_for_device(const char* path, FileBuf& fb, std::vector<BgzfBlock>& blks, size_t& out_size, bool& fastq, bool no_gpu_fastq) {
    using namespace dd::inflate_detail;
    struct stat sb;
    if (stat(path, &sb) != 0 || !S_ISREG(sb.st_mode) || sb.st_size < 28 || (size_t)sb.st_size > ((size_t)3 << 30)) return false;
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint8_t head[64];
    const size_t got = fread(head, 1, sizeof head, f);
    if (!bgzf_block_size(head, std::max<size_t>(got, 65536))) {   // (only the header is needed here; the size is checked in the walk)
        fclose(f);
        return false;
    }
    const size_t n = (size_t)sb.st_size;
    if (!read_whole(f, n, fb) || !bgzf_parse(fb.p, n, blks, out_size, fastq, no_gpu_fastq)) return false;
    fb.len = n;
    return true;
}
// One single-member gzip file for the device path (dd_gunzip.hip: launch_gunzip_members): the raw bytes into `fb`, where
// the deflate data starts, the trailer's CRC-32 and ISIZE.  false: not a file that path takes (small, huge, not gzip,
// FASTQ): the host decoder reads it.  (Whether the file is ONE member only the decoding shows: the device refuses a
// stream whose final block is not followed by exactly the 8 trailer bytes.)
bool gzip_member_size_ok(size_t n, size_t min_bytes) {
    // (below 1 GiB: ISIZE is the text's length mod 2^32 and DNA inflates 3.5-4 x, so a larger member's text may lie beyond
    // 4 GiB, which the device path's 32-bit offsets cannot hold -- a 3 Gbp assembly's .gz is ~0.98 GB; larger files take the
    // host's parallel decoder.  gzip_member_parse looks at the ratio as well, piece_offsets_kernel sums in 64 bits.)
    return n >= min_bytes && n < ((size_t)1 << 30);
}
bool gzip_member_for_device(const char* path, FileBuf& fb, std::vector<GzMember>& gms, size_t min_bytes) {
    struct stat sb;
    if (stat(path, &sb) != 0 || !S_ISREG(sb.st_mode) || !gzip_member_size_ok((size_t)sb.st_size, min_bytes)) return false;
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    const size_t n = (size_t)sb.st_size;
    if (!read_whole(f, n, fb) || !dd::gzip_members_parse(fb.p, n, gms)) return false;
    fb.len = n;
    return true;
}
// bounce buffer -> the caller's (pageable) array: one thread moves ~10 GB/s, and a log2m 20 batch is 37 MB per file
void parallel_copy(uint8_t* dst, const uint8_t* src, size_t n, int nthreads) {
    const size_t kPer = (size_t)8 << 20;
    const int parts = (int)std::min<size_t>((size_t)std::max(1, std::min(nthreads, 8)), (n + kPer - 1) / kPer);
    if (parts <= 1) {
        memcpy(dst, src, n);
        return;
    }
    std::vector<std::thread> th;
    const size_t step = ((n / parts) + 4095) & ~(size_t)4095;
    for (int t = 1; t < parts; ++t) {
        const size_t off = step * t;
        if (off >= n) break;
        th.emplace_back([=] { memcpy(dst + off, src + off, std::min(step, n - off)); });
    }
    memcpy(dst, src, std::min(step, n));
    for (auto& t : th) t.join();
}
// ------------------------------------------------------------------------------ call plan
struct CallPlan {
    bool any_gz = false, gpu_inflate = false, gpu_gunzip = false;   // a file is named .gz; BGZF / single-member gzip on the device
    bool full_batches = false;  // device-inflated batches: full ones, two at least, no small one at the end
    int batch_files = 1, window = 1;   // files per batch; files that may hold a host buffer at once
};
CallPlan plan_call(const dd_ctx* c, const Knobs& k, const char* const* paths, int nfiles, int nthreads) {
    CallPlan pl;
    // batch size in files: ~128 MB of FASTA per launch, judged by what is on disk (a .gz inflates ~4x)
    size_t disk_bytes = 0;
    for (int i = 0; i < nfiles; ++i) {
        struct stat sb;
        if (stat(paths[i], &sb) == 0 && sb.st_size > 0) {
            const size_t n = (size_t)sb.st_size, L = strlen(paths[i]);
            const bool gz = L > 3 && strcmp(paths[i] + L - 3, ".gz") == 0;
            pl.any_gz |= gz;
            disk_bytes += gz ? 4 * n : n;
        }
    }
    pl.gpu_inflate = !c->ingest.no_gpu_inflate && !k.no_gpu_inflate;
    pl.gpu_gunzip = pl.gpu_inflate && !k.no_gpu_gunzip;
    const size_t avg = std::max<size_t>(1, disk_bytes / (size_t)nfiles);
    // (log2m >= 17: the scatter/sort/replay path runs epoch by epoch over all rows of a launch and wants many rows)
    // (Batches that grow -- 64, 128, 256 MB -- were measured against fixed 128 MB ones once the job tables of several
    // batch shapes could be kept: 20.6-22.9 ms against 19.1 for 10 x 50 Mbp.  Fixed it is.)
    // (a context's FIRST call at log2m >= 17 keeps to 128 MB: the record areas and the pinned register staging are
    // allocated for a batch's rows, and hipMalloc + hipHostMalloc of a 512 MB batch's 5.5 GB + 0.4 GB cost a one-shot
    // `dandd tree -r 20` 0.23 s against 0.06 s; a long-lived context grows them on its second call)
    // (BGZF files inflated on the device: a launch of the inflate kernel takes as long as ONE block does -- 3 ms, the
    // serial walk of a deflate stream by one wave -- whether it holds 1 block or the 4 000 the chip keeps in flight, so
    // those calls batch ~320 MB of text -- five 50 Mbp files, one round of blocks --, in two batches at least (the
    // second's inflate runs under the first's sweep), and a batch waits up to 3 ms for its files instead of leaving
    // with the first one loaded: 64 x 5 Mbp went out as 2 + 8 + 8 + 46 files, four launches one behind the other)
    const size_t kBatchBytes = (size_t)(k.batch_mb ? k.batch_mb
                                        : (c->p >= 17 ? (c->ingest.calls == 0 ? 128 : 512) : (pl.any_gz && pl.gpu_inflate ? 320 : 128))) << 20;
    // (at most 256 files per launch: the loaders' window is two batches of host buffers of 2 MiB at least; with 64,
    // a thousand 100 kbp plasmids took 23 launches of ~3 ms each)
    const size_t kMaxBatchFiles = 256;
    pl.batch_files = (int)std::max<size_t>(1, std::min<size_t>(kMaxBatchFiles, kBatchBytes / avg));
    pl.full_batches = pl.any_gz && pl.gpu_inflate;
    if (pl.full_batches && nfiles >= 2) {
        // two batches at least (the second's inflate runs under the first's sweep), and EQUAL ones; and rather two batches a
        // quarter larger than three: there are two sets of buffers, so a third batch is issued only when the first has retired
        // -- ten gzip -1 files went out as 4 + 4 at t = 4 ms and 2 at t = 40 ms, whose find + inflate + sweep then ran alone
        // for the call's last 22 of 62 ms (DD_TRACE_FILES; profiles/r05_gunzip.txt)
        int nb = (nfiles + pl.batch_files - 1) / pl.batch_files;
        if (nb == 3 && nfiles * 2 <= pl.batch_files * 5) nb = 2;
        nb = std::max(nb, 2);
        pl.batch_files = (nfiles + nb - 1) / nb;
    }
    // loaders may run two batches ahead of the GPU
    pl.window = std::max(nthreads + 2, 2 * pl.batch_files + nthreads);
    return pl;
}
// the streams and events of the pipeline, made at a context's first call
int ensure_ingest_streams(dd_ctx* c) {
    IngestState& in = c->ingest;
    if (in.copy_stream) return DD_OK;
    for (hipStream_t* s : {&in.copy_stream, &in.copy_stream_b, &in.out_stream}) DD_HIP(hipStreamCreateWithFlags(s, hipStreamNonBlocking));
    for (PipeSet& s : in.pipe)
        for (hipEvent_t* e : {&s.h2d, &s.done, &s.d2h}) DD_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
    return DD_OK;
}
// ------------------------------------------------------------------------------ files
// How a file's bytes become the text K0 reads.  Classification sets the first three; the loader that finishes a file
// refines HostRead and RawGzPieces into the device routes (or RawGzPieces into HostRead).
enum class Route {
    HostRead,     // one item: the whole file through read_fasta_file (zlib / libdeflate for a .gz); the buffer holds the text
    PlainPieces,  // not gzip: read in pieces by several loaders, FASTQ records resolved once the file is whole
    RawGzPieces,  // a large .gz read as it is, in pieces by several loaders: meant for the device
    DevBgzf,      // BGZF: the buffer holds the COMPRESSED file, the device inflates its blocks
    DevGunzip,    // gzip members (usually ONE): the buffer holds the compressed file, the device inflates it in pieces
};
bool on_device(Route r) { return r == Route::DevBgzf || r == Route::DevGunzip; }
struct Slot {
    int buf = -1, pieces_left = 0;
    std::string err;
    bool ok = true, done = false;
    bool claimed = false, ready = false;  // a loader took the file's buffer / the buffer can be written to
    Route route = Route::HostRead;
    size_t piece_bytes = 0;               // PlainPieces / RawGzPieces: the file's size, read in pieces
    bool plus = false;                    // a piece of the file holds a line that starts with '+': FASTQ (dd_io.h)
    size_t out_size = 0;                  // DevBgzf / DevGunzip: bytes of text the device inflates
    bool fastq = false;                   // a device-inflated text that starts with '@': four-line FASTQ, checked and resolved on the device
    std::vector<BgzfBlock> blks;          // DevBgzf
    std::vector<GzMember> gms;            // DevGunzip
    std::vector<size_t> magic;            // a .gz read in pieces: where 1f 8b 08 stands (member headers?), found piece by piece by the loaders
};
// DevGunzip: the members' texts stand one behind the other in the file's text buffer
void member_totals(Slot& sl) {
    sl.out_size = 0;
    for (const GzMember& gm : sl.gms) sl.out_size += gm.isize;
    sl.fastq = sl.gms[0].fastq;
}
// Work items in file order.  A plain file is cut into 8 MiB pieces that different loaders pread into the
// file's pinned buffer -- the first file of a directory is then in memory after one piece-time instead of
// one file-time, which is what the GPU waits for at the start; a gzip file is one item (zlib is serial).
struct Item { int file; size_t off, len; };  // len 0: the whole file through zlib
// the file's route before loading: HostRead, or PlainPieces / RawGzPieces with its size in *size
Route sniff(const char* path, const Knobs& k, const CallPlan& pl, size_t* size) {
    struct stat sb;
    unsigned char magic[18] = {0};
    if (stat(path, &sb) != 0 || !S_ISREG(sb.st_mode) || sb.st_size <= 0) return Route::HostRead;
    FILE* f = fopen(path, "rb");
    if (!f) return Route::HostRead;
    const size_t got = fread(magic, 1, sizeof magic, f);
    fclose(f);
    *size = (size_t)sb.st_size;
    if (got >= 2 && !(magic[0] == 0x1f && magic[1] == 0x8b)) return Route::PlainPieces;
    // a large gzip file -- BGZF, or one that may be ONE member --: its compressed bytes are read
    // like a plain file's, by several loaders (one fread of a 700 MB file held the device path back 150 ms)
    const bool bc = (magic[3] & 4) && magic[12] == 'B' && magic[13] == 'C';   // BGZF's extra field
    if (got >= 2 && got == sizeof magic && magic[2] == 8 && *size >= k.raw_pieces_from && *size < ((size_t)3 << 30) &&
        (bc ? pl.gpu_inflate : (pl.gpu_gunzip && gzip_member_size_ok(*size, k.gunzip_min))))
        return Route::RawGzPieces;
    return Route::HostRead;
}
// ------------------------------------------------------------------------------ batches
// one gzip member inflated on the device: its share of the batch's gunzip tables, computed once (BatchLayout::add_member)
struct Member {
    int file;                        // in the batch; its text starts at text_at in that file's text
    GzMember gm;
    size_t text_at;
    size_t guess_bits, range_syms, pieces, groups, nchunks;
    size_t piece0, group0, chunk0;   // its first piece, group and 64 KiB chunk in the batch
    size_t sym_at, arena_at, win_at; // byte offsets of its ranges' symbols, its arena, its windows
};
// Every offset and size of one batch, from one pass over its files: the reserves are sized from it, the tables filled from it.
struct BatchLayout {
    int first = 0, count = 0;
    std::vector<size_t> sizes, offs, gz_off;   // per file: text bytes, text offset in `fasta`, compressed bytes' offset in `gz`
    size_t text_tot = 0, gz_tot = 0, njobs = 0;   // njobs: BGZF blocks
    std::vector<Member> members;
    size_t npieces = 0, ngroups = 0, nchunks = 0, sym_tot = 0, win_tot = 0;
    // the piece tables of the batch's gzip members, one block of device memory: RawFile[nmem],
    // starts (u64) / lens / offs / over / abase [npieces], chunk0 [nmem + 1], crcs [nchunks]
    size_t raw_files = 0, raw_u32 = 0, raw_chunk0 = 0, raw_bytes = 0;
    // the text rules' table (offsets from the start of `fasta` and in words from the table's end: pointers once reserved)
    std::vector<dd::TextJob> text_jobs;
    size_t text_blocks = 0, text_words = 0, text_tab = 0;
    bool any_fastq = false;
    bool inflated() const { return njobs || !members.empty(); }
    void add_member(int j, const GzMember& gm, size_t text_at, const Knobs& k) {   // every member a "file" of the decoder's tables
        Member m{};
        m.file = j, m.gm = gm, m.text_at = text_at;
        const size_t clen = gm.end - gm.first_bit / 8;
        m.guess_bits = k.guess_bits(clen);
        m.range_syms = range_syms_of(m.guess_bits, gm.isize, clen);
        m.pieces = (gm.end * 8 - gm.first_bit + m.guess_bits - 1) / m.guess_bits;
        m.groups = (m.pieces + dd::kPieceGroup - 1) / dd::kPieceGroup;
        m.nchunks = (gm.isize + 65535u) / 65536u;
        m.piece0 = npieces, m.group0 = ngroups, m.chunk0 = nchunks, m.sym_at = sym_tot, m.win_at = win_tot;
        m.arena_at = sym_tot + align_up(m.pieces * m.range_syms * 2 + 256, 256);   // the ranges' symbols, then the arena
        npieces += m.pieces, ngroups += m.groups, nchunks += m.nchunks;
        sym_tot = m.arena_at + align_up((size_t)gm.isize * 2 + 256, 256);
        win_tot += align_up(dd::gunzip_window_bytes(m.pieces), 256);
        members.push_back(m);
    }
    // kseq's record rules over the texts the device inflates (dd_fastq.hip)
    int add_text_job(int j, bool fastq) {
        if (sizes[j] >= ((uint64_t)1 << 32))   // (bgzf_parse / gzip_members_parse refuse such files: never reached)
            return fail(DD_EINVAL, "a device-inflated text of %zu bytes does not fit the text rules' 32-bit offsets", (size_t)sizes[j]);
        dd::TextJob t{};
        t.text = reinterpret_cast<uint8_t*>(offs[j]);
        t.n = (uint32_t)sizes[j];
        t.fastq = fastq ? 1u : 0u;
        t.block0 = (uint32_t)text_blocks;
        const size_t nb4k = (sizes[j] + 4095) / 4096;
        text_blocks += nb4k;
        if (fastq) {
            any_fastq = true;
            t.nl_cap = (uint32_t)(sizes[j] / 8 + 16);
            t.blk_count = reinterpret_cast<uint32_t*>(text_words);
            t.nl = reinterpret_cast<uint32_t*>(text_words + nb4k);
            t.nl_total = reinterpret_cast<uint32_t*>(text_words + nb4k + t.nl_cap);
            text_words += nb4k + t.nl_cap + 4;
        }
        text_jobs.push_back(t);
        return DD_OK;
    }
};
// the CRC-32 of one member's text, composed from those of its 64 KiB chunks (the device's, in chunk order)
uint32_t member_crc(const Member& m, const uint32_t* crcs) {
    uint32_t crc = 0;
    const uint32_t full = dd::crc_x8n(65536u);
    for (uint32_t k = 0; k < m.nchunks; ++k) {
        const uint32_t len = std::min<uint32_t>(65536u, m.gm.isize - k * 65536u);
        crc = k ? (dd::crc_multmodp(len == 65536u ? full : dd::crc_x8n(len), crc) ^ crcs[m.chunk0 + k]) : crcs[m.chunk0];
    }
    return crc;
}
// ------------------------------------------------------------------------------ one call
// one dd_sketch_files call: its files, the loader threads, the batches in flight
struct Ingest {
    dd_ctx* const c; IngestState& in;
    const Knobs& k; const CallPlan& pl;
    const char* const* paths;
    const int nfiles, kmin, kmax, nthreads;
    uint8_t* const regs;
    const bool promote;        // buffers taken again by this call are re-made pinned
    const double t_begin;
    const size_t slab;         // registers of one file
    std::vector<Slot> slots; std::vector<Item> items;
    int gz_par = 1;            // threads per gzip file read on the host
    std::mutex mu; std::condition_variable cv;   // loaders <-> driver: slots, free_bufs, consumed
    std::atomic<size_t> next{0};   // the next item a loader takes
    std::vector<int> free_bufs;
    int consumed = 0;          // files whose host buffer went back to the pool
    BatchLayout fly[2];        // the batches on the GPU by buffer set (count 0: none); a set is busy until its batch is retired
    int rc = DD_OK, nbatches = 0;
    std::string first_err;
    double t_wait = 0;         // ms waiting for loaders
    size_t total_bytes = 0;
    Ingest(dd_ctx* c, const Knobs& k, const CallPlan& pl, const char* const* paths, int nfiles, int kmin, int kmax, uint8_t* regs,
           int nthreads, bool promote, double t_begin)
        : c(c), in(c->ingest), k(k), pl(pl), paths(paths), nfiles(nfiles), kmin(kmin), kmax(kmax), nthreads(nthreads), regs(regs),
          promote(promote), t_begin(t_begin), slab((size_t)(kmax - kmin + 1) << c->p), slots(nfiles) {
        for (int b = 0; b < pl.window; ++b) free_bufs.push_back(b);
    }
    void sync_copy_streams() const { (void)hipStreamSynchronize(in.copy_stream), (void)hipStreamSynchronize(in.copy_stream_b); }
    uint8_t* text_dev(const PipeSet& ps, const BatchLayout& L, int j) const { return static_cast<uint8_t*>(ps.fasta.p) + L.offs[j]; }
    uint8_t* gz_dev(const PipeSet& ps, const BatchLayout& L, int j) const { return static_cast<uint8_t*>(ps.gz.p) + L.gz_off[j]; }
    void classify() {
        const size_t kPiece = (size_t)8 << 20, kFirstPiece = (size_t)2 << 20;
        int ngz = 0;
        for (int i = 0; i < nfiles; ++i) {
            Slot& sl = slots[i];
            sl.route = sniff(paths[i], k, pl, &sl.piece_bytes);
            if (sl.route == Route::HostRead) {
                sl.piece_bytes = 0, sl.pieces_left = 1, ++ngz;
                items.push_back(Item{i, 0, 0});
                continue;
            }
            // (the first files in finer pieces still: every loader works on file 0 until it is complete, and the GPU
            // sits idle until then)
            const size_t piece = i < 2 ? kFirstPiece : kPiece;
            for (size_t off = 0; off < sl.piece_bytes; off += piece) {
                items.push_back(Item{i, off, std::min(piece, sl.piece_bytes - off)});
                ++sl.pieces_left;
            }
        }
        // A gzip file is one item, but not one thread's worth of work: with fewer .gz files than loaders every one of them
        // is inflated by its share of the CPUs (BGZF blocks / pieces of a plain member, dd_inflate.h); a directory of many
        // .gz files keeps one (libdeflate) thread per file, which is the faster decoder per core.
        gz_par = ngz ? std::max(1, nthreads / ngz) : 1;
    }
    // The loader that takes a file's first item sets its host buffer up; the others wait until it can be written to.
    // false: this loader could not get the buffer (the file's error is recorded).
    bool claim(const Item& it) {
        Slot& sl = slots[it.file];
        {
            // Only files consumed .. consumed+window-1 may hold a buffer: they are consumed in
            // order, so a later file must never take the buffer an earlier one is waiting for.
            std::unique_lock<std::mutex> lk(mu);
            if (sl.claimed) return cv.wait(lk, [&] { return sl.ready; }), true;
            sl.claimed = true;
            cv.wait(lk, [&] { return it.file < consumed + pl.window && !free_bufs.empty(); });
            sl.buf = free_bufs.back();
            free_bufs.pop_back();
        }
        // Pinning host memory costs ~0.4 ms per MB: a buffer starts pageable (a one-shot `dandd tree` process never
        // pays that) and is re-made pinned when a LATER call takes it again -- a long-lived context (a pipeline, a
        // benchmark loop) has a fully pinned pool from its third call on.
        FileBuf& fb = *in.file_pool[sl.buf];
        if (promote && !fb.pinned && fb.p) fb.release(), fb.pinned = true;
        fb.len = 0;
        const bool ok = !sl.piece_bytes || fb.reserve(sl.piece_bytes + 16);
        if (ok) fb.len = sl.piece_bytes;
        {
            std::lock_guard<std::mutex> lk(mu);
            sl.ready = true;
            if (!ok) sl.ok = false, sl.err = std::string("out of pinned host memory reading ") + paths[it.file];
        }
        cv.notify_all();
        return ok;
    }
    // the loader threads' body: items in file order, each read (and scanned) by whoever takes it
    void load() {
        (void)hipSetDevice(c->device);  // pinned allocations belong to the context's device
        for (;;) {
            const size_t w = next.fetch_add(1);
            if (w >= items.size()) return;
            const Item it = items[w];
            Slot& sl = slots[it.file];
            bool ok = claim(it);
            FileBuf& fb = *in.file_pool[sl.buf];
            const char* path = paths[it.file];
            std::string err;
            if (it.len == 0) {
                if (pl.gpu_inflate && bgzf_for_device(path, fb, sl.blks, sl.out_size, sl.fastq, k.no_gpu_fastq)) sl.route = Route::DevBgzf;
                else if (pl.gpu_gunzip && gzip_member_for_device(path, fb, sl.gms, k.gunzip_min)) sl.route = Route::DevGunzip, member_totals(sl);
                else ok = dd::read_fasta_file(path, fb, err, gz_par);
            } else if (ok && fb.cap >= sl.piece_bytes) {
                FILE* f = fopen(path, "rb");
                ok = f && fseeko(f, (off_t)it.off, SEEK_SET) == 0 && fread(fb.p + it.off, 1, it.len, f) == it.len;
                if (!ok) err = std::string("read error on ") + path;
                if (f) fclose(f);
            } else {
                ok = false;   // (the loader that set the buffer up could not: the file's error is recorded already)
            }
            // (every loader looks through the piece it has just read -- the bytes are still in its cache -- instead of one
            // of them through the whole file at the end: that pass held every file back 2-3 ms)
            const bool plus_here = it.len && ok && sl.route == Route::PlainPieces && dd::piece_has_plus_line(fb.p, it.off, it.len);
            std::vector<size_t> magic_here;   // (a .gz read in pieces: every loader scans what it has just read for member headers)
            if (it.len && ok && sl.route == Route::RawGzPieces && it.len > 2) dd::gzip_magic_scan(fb.p, it.off, it.off + it.len - 2, magic_here);
            bool last, plus;
            {
                std::lock_guard<std::mutex> lk(mu);
                if (!ok && sl.ok) sl.ok = false, sl.err = err;
                sl.plus |= plus_here;
                sl.magic.insert(sl.magic.end(), magic_here.begin(), magic_here.end());
                plus = sl.plus;
                last = --sl.pieces_left == 0;
            }
            if (last) {
                if (it.len && ok) finish_file(it, fb, ok, err, plus);
                std::lock_guard<std::mutex> lk(mu);
                if (!ok && sl.ok) sl.ok = false, sl.err = err;
                sl.done = true;
            }
            cv.notify_all();
        }
    }
    // the last piece of a file read in pieces is in: the file is whole
    void finish_file(const Item& it, FileBuf& fb, bool& ok, std::string& err, bool plus) {
        Slot& sl = slots[it.file];
        if (sl.route == Route::PlainPieces) {
            // a plain file read in pieces is whole now: FASTQ records are resolved before K0 sees the bytes (dd_io.h;
            // read_fasta_file has done the same for the files that came through zlib)
            for (const Item& o : items)
                if (o.file == it.file && !plus) plus = dd::plus_at_piece_start(fb.p, o.off);
            if (!dd::normalize_records(fb, plus ? 1 : 0)) ok = false, err = std::string("out of host memory reading ") + paths[it.file];
            return;
        }
        // the compressed file is whole: one member for the device, or (FASTQ, an odd header) the host decoder after all
        if (bgzf_parse(fb.p, sl.piece_bytes, sl.blks, sl.out_size, sl.fastq, k.no_gpu_fastq)) {
            sl.route = Route::DevBgzf;
            return;
        }
        if (pl.gpu_gunzip) {
            // (the positions that straddle two pieces, then all of them in order)
            for (const Item& o : items)
                if (o.file == it.file && o.off >= 2)
                    for (size_t q = o.off - 2; q < o.off && q + 2 < sl.piece_bytes; ++q)
                        if (fb.p[q] == 0x1f && fb.p[q + 1] == 0x8b && fb.p[q + 2] == 0x08) sl.magic.push_back(q);
            std::sort(sl.magic.begin(), sl.magic.end());
            sl.magic.erase(std::unique(sl.magic.begin(), sl.magic.end()), sl.magic.end());
            if (dd::gzip_members_parse(fb.p, sl.piece_bytes, sl.gms, &sl.magic)) {
                sl.route = Route::DevGunzip;
                member_totals(sl);
                return;
            }
        }
        sl.route = Route::HostRead;
        ok = dd::read_fasta_file(paths[it.file], fb, err, gz_par);
    }
    bool all_done(int from, int to) const {
        return std::all_of(slots.begin() + from, slots.begin() + to, [](const Slot& s) { return s.done; });
    }
    // the next batch from file i: consecutive files, as many as are wanted and already loaded (at least one)
    int choose_batch(int i) {
        const int want = pl.batch_files;
        int count = 0;
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return slots[i].done; });
        if (pl.full_batches) cv.wait_for(lk, std::chrono::milliseconds(3), [&] { return all_done(i, std::min(nfiles, i + want)); });
        // as many as a batch wants and are already loaded (at least one): the GPU is never kept waiting for a
        // full batch; equal batches also let dd_sketch_device reuse its job tables and the buffers below
        while (count < want && i + count < nfiles && slots[i + count].done) ++count;
        // (device-inflated batches: no small batch at the end -- a launch of the inflate kernel over two files' pieces takes as
        // long as one over five, with a quarter of the chip: ten gzip -1 files went out as 4 + 4 + 2 and the last two cost
        // 22 of the call's 60 ms.  What would be left is fewer than half a batch: it joins this one, waited for.)
        // (Only where the loaders can bring those files NOW.  A file beyond the window gets its buffer when a batch in flight
        // is retired, and that happens after this returns: waiting for it here is waiting for ever -- ten BGZF files in
        // batches of three with three loaders, a window of nine: the third batch waited for file 9.  Such a call ends
        // with a small batch instead.)
        if (pl.full_batches && i + count < nfiles && nfiles - (i + count) < (want + 1) / 2 && nfiles <= consumed + pl.window) {
            cv.wait(lk, [&] { return all_done(i + count, nfiles); });
            count = nfiles - i;
        }
        // (a directory of small files: batch sizes come from a short list -- powers of two, the full batch, the
        // tail -- so that the job tables of every shape are in the plan cache from the second call on; planning
        // a shape never seen costs ~2 ms of host time with the GPU waiting)
        if (!pl.full_batches && count < want && i + count < nfiles)
            while (count & (count - 1)) count &= count - 1;
        return count;
    }
    int layout(int first, int count, BatchLayout& L) const {
        L.first = first, L.count = count;
        L.sizes.assign(count, 0), L.offs.assign(count, 0), L.gz_off.assign(count, 0);
        for (int j = 0; j < count; ++j) {
            const Slot& sj = slots[first + j];
            const FileBuf& fb = *in.file_pool[sj.buf];
            const bool dev = on_device(sj.route);
            L.sizes[j] = dev ? sj.out_size : fb.size();
            L.offs[j] = L.text_tot;
            L.text_tot += align_up(L.sizes[j] + 16, 256);
            if (!dev) continue;
            L.gz_off[j] = L.gz_tot;
            L.gz_tot += align_up(fb.size() + 16, 256);
            if (sj.route == Route::DevBgzf) {
                L.njobs += sj.blks.size();
            } else {
                size_t text_at = 0;   // the members' texts one behind the other
                for (const GzMember& gm : sj.gms) {
                    L.add_member(j, gm, text_at, k);
                    text_at += gm.isize;
                }
            }
            if (int rc2 = L.sizes[j] ? L.add_text_job(j, sj.fastq) : DD_OK) return rc2;
        }
        const size_t nmem = L.members.size();
        L.raw_files = align_up(nmem * sizeof(dd::RawFile), 256);
        L.raw_u32 = align_up(L.npieces * 4, 256);
        L.raw_chunk0 = align_up((nmem + 1) * 4, 256);
        L.raw_bytes = L.raw_files + 6 * L.raw_u32 + L.raw_chunk0 + align_up(L.nchunks * 4, 256);   // (starts are 64-bit: two of the six)
        L.text_tab = align_up(L.text_jobs.size() * sizeof(dd::TextJob), 256);
        return DD_OK;
    }
    // every buffer of the batch, each reserved once.  (Growing a device buffer frees the old one: the compute stream may still
    // read it for the batch before last only if that batch has not been retired -- it has, before this is called.)
    int reserve(PipeSet& ps, const BatchLayout& L) {
        // (a 3 Gbp assembly's .gz takes 16 GB of symbol area per buffer set: a long-lived context gives that back when a later
        // batch needs an eighth of it or less -- not at the end of every call: hipFree + hipMalloc of 16 GB per call cost an
        // occasional 2 s.  The set's previous batch has been retired: nothing reads the buffer any more.)
        if (ps.sym.cap > ((size_t)4 << 30) && L.sym_tot <= ps.sym.cap / 8) ps.sym.release(), ps.win.release();
        const bool gunzip = !L.members.empty();
        int rc;
        if (L.inflated() &&
            ((rc = ps.gz.reserve(L.gz_tot + 16)) != DD_OK ||
             (gunzip && ((rc = ps.sym.reserve(L.sym_tot)) != DD_OK || (rc = ps.win.reserve(L.win_tot)) != DD_OK ||
                         (rc = ps.raw.reserve(L.raw_bytes)) != DD_OK || (rc = ps.raw_host.reserve(L.raw_files + L.raw_chunk0)) != DD_OK ||
                         (rc = ps.crc_host.reserve(L.nchunks * 4 + 256)) != DD_OK)) ||
             (rc = ps.err.reserve(256)) != DD_OK || (rc = ps.err_host.reserve(256)) != DD_OK)) {
            // (10 x the compressed bytes + 2 x the text of symbol area, 64 KiB of windows per piece: a device that cannot
            // give that can still sketch the file -- the call runs again with the host decoder; not a strike)
            if (rc == DD_ENOMEM && gunzip) in.inflate_retry = true;
            return rc;
        }
        if (L.njobs && ((rc = ps.jobs.reserve(L.njobs * sizeof(dd::InflateJob))) != DD_OK ||
                        (rc = ps.jobs_host.reserve(L.njobs * sizeof(dd::InflateJob))) != DD_OK))
            return rc;
        if ((rc = ps.fasta.reserve(L.text_tot + 16)) != DD_OK || (rc = ps.regs.reserve((size_t)L.count * slab)) != DD_OK ||
            (rc = ps.out.reserve((size_t)L.count * slab)) != DD_OK)
            return rc;
        if (!L.text_jobs.empty() &&
            ((rc = ps.txt.reserve(L.text_tab + L.text_words * 4 + 256)) != DD_OK || (rc = ps.txt_host.reserve(L.text_tab)) != DD_OK))
            return rc;
        return DD_OK;
    }
    // ---- issue: the copy stream `cs` gets the batch's uploads and decoders, the compute stream waits for them, sketches, and
    // the out stream brings the registers back.  On failure the caller waits for all four streams before the buffers go back.
    hipError_t issue_uploads(const PipeSet& ps, const BatchLayout& L, hipStream_t cs) const {
        hipError_t e = hipSuccess;
        for (int j = 0; j < L.count && e == hipSuccess; ++j) {
            const Slot& sj = slots[L.first + j];
            const FileBuf& fb = *in.file_pool[sj.buf];
            // a device-inflated file: the COMPRESSED file goes over PCIe (a quarter of the text), inflated into its text below
            if (on_device(sj.route)) e = hipMemcpyAsync(gz_dev(ps, L, j), fb.data(), fb.size(), hipMemcpyHostToDevice, cs);
            else if (L.sizes[j]) e = hipMemcpyAsync(text_dev(ps, L, j), fb.data(), L.sizes[j], hipMemcpyHostToDevice, cs);
        }
        return e;
    }
    // block starts -> piece lengths -> offsets -> symbols -> windows -> text -> CRC-32 of every 64 KiB (dd_gunzip.hip)
    hipError_t issue_gunzip(PipeSet& ps, const BatchLayout& L, hipStream_t cs) const {
        const size_t nmem = L.members.size();
        if (!nmem) return hipSuccess;
        dd::RawFile* raw_host = static_cast<dd::RawFile*>(ps.raw_host.p);
        uint32_t* chunk0_host = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(ps.raw_host.p) + L.raw_files);
        uint8_t* sym = static_cast<uint8_t*>(ps.sym.p);
        for (size_t mi = 0; mi < nmem; ++mi) {
            const Member& m = L.members[mi];
            // (positions are the FILE's: its bytes start on a 256-byte boundary, a member's need not; in_len: the member ends
            // there, CRC-32 and ISIZE right behind its final block)
            raw_host[mi] = dd::RawFile{gz_dev(ps, L, m.file), (uint32_t)m.gm.end, m.gm.first_bit, (uint32_t)m.guess_bits, (uint32_t)m.pieces,
                                       (uint32_t)m.piece0, m.gm.isize, reinterpret_cast<uint16_t*>(sym + m.sym_at), (uint32_t)m.range_syms,
                                       reinterpret_cast<uint16_t*>(sym + m.arena_at), static_cast<uint8_t*>(ps.win.p) + m.win_at,
                                       (uint32_t)m.group0, (uint32_t)m.groups, text_dev(ps, L, m.file) + m.text_at};
            chunk0_host[mi] = (uint32_t)m.chunk0;
        }
        chunk0_host[nmem] = (uint32_t)L.nchunks;
        uint8_t* rb = static_cast<uint8_t*>(ps.raw.p);
        uint32_t* crcs_dev = reinterpret_cast<uint32_t*>(rb + L.raw_files + 6 * L.raw_u32 + L.raw_chunk0);
        hipError_t e = hipMemcpyAsync(rb, raw_host, nmem * sizeof(dd::RawFile), hipMemcpyHostToDevice, cs);
        if (e == hipSuccess) e = hipMemcpyAsync(rb + L.raw_files + 6 * L.raw_u32, chunk0_host, (nmem + 1) * 4, hipMemcpyHostToDevice, cs);
        if (e != hipSuccess) return e;
        dd::launch_gunzip_members(reinterpret_cast<const dd::RawFile*>(rb), (int)nmem, (int)L.npieces, (int)L.ngroups, (int)L.nchunks,
                                  reinterpret_cast<uint64_t*>(rb + L.raw_files), reinterpret_cast<uint32_t*>(rb + L.raw_files + 2 * L.raw_u32),
                                  L.raw_u32 / 4, reinterpret_cast<const uint32_t*>(rb + L.raw_files + 6 * L.raw_u32), crcs_dev,
                                  static_cast<uint32_t*>(ps.err.p), cs);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(ps.crc_host.p, crcs_dev, L.nchunks * 4, hipMemcpyDeviceToHost, cs);
        return e;
    }
    hipError_t issue_bgzf(PipeSet& ps, const BatchLayout& L, hipStream_t cs) const {
        if (!L.njobs) return hipSuccess;
        dd::InflateJob* jobs_host = static_cast<dd::InflateJob*>(ps.jobs_host.p);
        size_t nj = 0;
        for (int j = 0; j < L.count; ++j) {
            const Slot& sj = slots[L.first + j];
            if (sj.route != Route::DevBgzf) continue;
            for (const BgzfBlock& b : sj.blks)
                jobs_host[nj++] = dd::InflateJob{gz_dev(ps, L, j) + b.in_off, b.in_len, b.out_len, text_dev(ps, L, j) + b.out_off};
        }
        if (hipError_t e = hipMemcpyAsync(ps.jobs.p, jobs_host, L.njobs * sizeof(dd::InflateJob), hipMemcpyHostToDevice, cs)) return e;
        dd::launch_inflate_bgzf(static_cast<const dd::InflateJob*>(ps.jobs.p), (int)L.njobs, static_cast<uint32_t*>(ps.err.p), cs);
        return hipGetLastError();
    }
    // kseq's record rules over the texts the device has just inflated (dd_fastq.hip): no line of a FASTA-classed text may
    // start with '+'; a FASTQ-classed text must be four-line FASTQ, and its '+' and quality lines become header lines
    hipError_t issue_text_rules(PipeSet& ps, BatchLayout& L, hipStream_t cs) const {
        if (L.text_jobs.empty()) return hipSuccess;
        uint8_t* const text = static_cast<uint8_t*>(ps.fasta.p);
        uint32_t* const base = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(ps.txt.p) + L.text_tab);
        for (dd::TextJob& t : L.text_jobs) {
            t.text = text + reinterpret_cast<size_t>(t.text);
            if (t.fastq) {
                t.blk_count = base + reinterpret_cast<size_t>(t.blk_count);
                t.nl = base + reinterpret_cast<size_t>(t.nl);
                t.nl_total = base + reinterpret_cast<size_t>(t.nl_total);
            }
        }
        const size_t n = L.text_jobs.size();
        memcpy(ps.txt_host.p, L.text_jobs.data(), n * sizeof(dd::TextJob));
        if (hipError_t e = hipMemcpyAsync(ps.txt.p, ps.txt_host.p, n * sizeof(dd::TextJob), hipMemcpyHostToDevice, cs)) return e;
        dd::launch_text_rules(static_cast<const dd::TextJob*>(ps.txt.p), (int)n, (uint32_t)L.text_blocks, L.any_fastq,
                              static_cast<uint32_t*>(ps.err.p), cs);
        return hipGetLastError();
    }
    // dd_inflate_files: every file's text as it stands in the buffer K0 reads -- inflated by the kernels above where
    // the device decoder took the file -- back to the caller, on the stream that made it
    hipError_t issue_text_sink(const PipeSet& ps, const BatchLayout& L, hipStream_t cs) const {
        IngestState::TextSink* sink = in.text_sink;
        hipError_t e = hipSuccess;
        for (int j = 0; j < L.count && e == hipSuccess; ++j) {
            const int f = L.first + j;
            sink->lens[f] = L.sizes[j];
            if (L.sizes[j] > sink->caps[f]) sink->short_buffer = true;
            else if (L.sizes[j]) e = hipMemcpyAsync(sink->out[f], text_dev(ps, L, j), L.sizes[j], hipMemcpyDeviceToHost, cs);
        }
        return e;
    }
    // the batch's registers to the pinned bounce buffer, on the out stream once the sketch is done
    hipError_t issue_d2h(PipeSet& ps, const BatchLayout& L) const {
        hipError_t e = hipEventRecord(ps.done, c->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(in.out_stream, ps.done, 0);
        if (e == hipSuccess) e = hipMemcpyAsync(ps.out.p, ps.regs.p, (size_t)L.count * slab, hipMemcpyDeviceToHost, in.out_stream);
        if (e == hipSuccess) e = hipEventRecord(ps.d2h, in.out_stream);
        return e;
    }
    int issue(int set, BatchLayout& L) {
        PipeSet& ps = in.pipe[set];
        const bool inflated = L.inflated();
        hipStream_t cs = (inflated && set) ? in.copy_stream_b : in.copy_stream;
        hipError_t e = issue_uploads(ps, L, cs);
        if (inflated && e == hipSuccess) e = hipMemsetAsync(ps.err.p, 0, 4, cs);
        // (round 5, measured and dropped: the second batch's decoders BEHIND the first's -- an event between the two copy streams --
        // instead of side by side: ten gzip -1 files 55.0 -> 60.4 ms, gzip -6 43.2 -> 47.5, 64 x 5 Mbp 33.9 -> 38.8: a lone
        // inflate launch cannot fill the chip, its time is its longest piece's, and two launches hide each other's tails)
        if (e == hipSuccess) e = issue_gunzip(ps, L, cs);
        if (e == hipSuccess) e = issue_bgzf(ps, L, cs);
        if (e == hipSuccess) e = issue_text_rules(ps, L, cs);
        if (inflated && e == hipSuccess) e = hipMemcpyAsync(ps.err_host.p, ps.err.p, 4, hipMemcpyDeviceToHost, cs);
        if (in.text_sink && e == hipSuccess) e = issue_text_sink(ps, L, cs);
        if (e == hipSuccess) e = hipEventRecord(ps.h2d, cs);
        if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, ps.h2d, 0);
        if (e != hipSuccess) return fail(DD_EHIP, "ingestion pipeline: %s", hipGetErrorString(e));
        std::vector<const uint8_t*> ptrs(L.count);
        for (int j = 0; j < L.count; ++j) ptrs[j] = text_dev(ps, L, j);
        const int rc = dd_sketch_device(c, ptrs.data(), L.sizes.data(), L.count, kmin, kmax, static_cast<uint8_t*>(ps.regs.p));
        if (rc != DD_OK) return rc;
        if ((e = issue_d2h(ps, L)) != hipSuccess) return fail(DD_EHIP, "ingestion pipeline: %s", hipGetErrorString(e));
        return DD_OK;
    }
    // ---- the end of a batch
    // error path: the loaders must never wait for ever
    void give_back(int first, int count) {
        std::unique_lock<std::mutex> lk(mu);
        for (int i = first; i < first + count; ++i)
            if (slots[i].buf >= 0) free_bufs.push_back(slots[i].buf);
        consumed = first + count;
        lk.unlock();
        cv.notify_all();
    }
    // error path: the batches in flight give their buffers back (once nothing reads them) BEFORE any later file does.  `consumed`
    // may only pass files whose buffers are back in the pool: the window then never admits more files than there are
    // buffers, which is what keeps a later file from taking the buffer the next file to be drained still waits for.
    void drop_in_flight() {
        if (!fly[0].count && !fly[1].count) return;
        sync_copy_streams(), (void)hipStreamSynchronize(c->stream), (void)hipStreamSynchronize(in.out_stream);
        for (int k2 = 0; k2 < 2; ++k2) {   // (the older of the two first)
            BatchLayout& f = fly[(nbatches + k2) & 1];
            if (f.count) give_back(f.first, f.count), f.count = 0;
        }
    }
    // a batch that could not be sent: its error is the call's, its buffers go back (once nothing reads them, if it was issued)
    void abandon(int first, int count, bool issued) {
        first_err = g_err;
        if (issued)  // nothing may still read the host buffers
            sync_copy_streams(), (void)hipStreamSynchronize(c->stream), (void)hipStreamSynchronize(in.out_stream);
        drop_in_flight();
        give_back(first, count);
    }
    // hand a finished batch's results to the caller and its host buffers back to the pool
    int retire(int set) {
        BatchLayout f;
        std::swap(f, fly[set]);
        if (!f.count) return DD_OK;
        PipeSet& ps = in.pipe[set];
        uint32_t* ecount = static_cast<uint32_t*>(ps.err_host.p);   // (reserved for batches with device-inflated files only)
        const bool arrived = hipEventSynchronize(ps.d2h) == hipSuccess;
        bool refused = arrived && f.inflated() && *ecount != 0;
        if (arrived && !refused)
            for (const Member& m : f.members)
                if (member_crc(m, static_cast<const uint32_t*>(ps.crc_host.p)) != m.gm.crc) refused = true, *ecount = 1;
        if (arrived && !refused)
            parallel_copy(regs + (size_t)f.first * slab, static_cast<const uint8_t*>(ps.out.p), (size_t)f.count * slab, nthreads);
        else
            sync_copy_streams();  // nothing may still read the host buffers that go back below
        // (a failed batch has still given its buffers back: the loaders must never wait for ever)
        give_back(f.first, f.count);
        if (refused) {
            in.inflate_retry = true;
            // (a CRC that does not match, a block the decoder would not take: counted; pieces that decode but do not add up
            // to the trailer's ISIZE: the file's matter, not the decoder's)
            if ((*ecount & (dd::kSizeMismatch - 1u)) != 0u || *ecount < dd::kSizeMismatch) in.inflate_retry_counts = true;
            return fail(DD_EIO, "ingestion pipeline: %u block(s) / piece(s) / file(s) refused by the device decoder", *ecount);
        }
        return arrived ? DD_OK : fail(DD_EHIP, "ingestion pipeline: D2H failed");
    }
    int run() {
        classify();
        std::vector<std::thread> pool;
        for (int t = 0; t < nthreads; ++t) pool.emplace_back([this] { load(); });
        int i = 0;
        while (i < nfiles) {
            const int set = nbatches & 1;
            const double ta = now();
            const int count = choose_batch(i);
            t_wait += now() - ta;
            for (int j = i; j < i + count && rc == DD_OK; ++j)
                if (!slots[j].ok) rc = DD_EIO, first_err = slots[j].err;
            if (rc != DD_OK) {  // drain: give every buffer back as its file arrives
                drop_in_flight();
                give_back(i, count), i += count;
                continue;
            }
            // this buffer set was used by batch nbatches-2: finish that one first
            const double tr = now();
            if ((rc = retire(set)) != DD_OK) {
                first_err = g_err;   // (the batch is chosen again and drained)
                continue;
            }
            const double ti = now();
            BatchLayout L;
            if ((rc = layout(i, count, L)) != DD_OK || (rc = reserve(in.pipe[set], L)) != DD_OK) {
                abandon(i, count, false), i += count;
                continue;
            }
            const size_t tot = L.text_tot;
            total_bytes += tot;
            if ((rc = issue(set, L)) != DD_OK) abandon(i, count, true);
            else fly[set] = std::move(L), ++nbatches;
            if (k.trace)
                fprintf(stderr, "[dd_sketch_files] t=%.2f batch %d: files %d..%d (%.1f MB): waited %.2f ms for loaders, %.2f ms retiring, %.2f ms issuing\n",
                        now() - t_begin, nbatches - 1, i, i + count - 1, tot / 1e6, tr - ta, ti - tr, now() - ti);
            i += count;
        }
        // batches retire in order: the older of the two first
        for (int k2 = 0; k2 < 2; ++k2) {
            const int set = (nbatches + k2) & 1;
            if (rc == DD_OK) {
                if ((rc = retire(set)) != DD_OK) first_err = g_err;
            } else if (fly[set].count) {
                sync_copy_streams();
                give_back(fly[set].first, fly[set].count);
                fly[set].count = 0;
            }
        }
        for (auto& t : pool) t.join();
        in.ms[0] = now() - t_begin;
        in.ms[1] = t_wait;
        in.ms[2] = nbatches;
        in.ms[3] = (double)total_bytes;
        if (k.trace)
            fprintf(stderr, "[dd_sketch_files] %d files, %d batches of <= %d files, %.1f ms (%.1f ms waiting for loaders), %.1f MB\n",
                    nfiles, nbatches, pl.batch_files, in.ms[0], t_wait, total_bytes / 1e6);
        if (rc != DD_OK) return fail(rc, "%s", first_err.c_str());
        return DD_OK;
    }
};
int sketch_files_impl(dd_ctx* c, const Knobs& k, const char* const* paths, int nfiles, int kmin, int kmax, uint8_t* regs, int nthreads) {
    if (nfiles < 0 || (nfiles && (!paths || !regs))) return fail(DD_EINVAL, "null argument");
    if (kmin < 1 || kmax > 64 || kmin > kmax) return fail(DD_EINVAL, "k range %d..%d outside 1..64", kmin, kmax);
    for (int i = 0; i < nfiles; ++i)
        if (!paths[i]) return fail(DD_EINVAL, "null path at index %d", i);
    if (!nfiles) return DD_OK;
    DeviceGuard guard(c->device);
    if (nthreads <= 0) nthreads = std::min(16, usable_cpus());
    const double t_begin = now();
    const CallPlan pl = plan_call(c, k, paths, nfiles, nthreads);
    // (DD_INFLATE_STRICT=2, tests: a context whose device decoder has been switched off by three refusals says so instead of
    // quietly decoding on the host)
    if (pl.any_gz && c->ingest.no_gpu_inflate && k.strict_level >= 2)
        return fail(DD_EIO, "the device decoder is switched off on this context (three refused calls)");
    IngestState& in = c->ingest;
    while ((int)in.file_pool.size() < pl.window) in.file_pool.push_back(new FileBuf());
    const bool promote = ++in.calls >= 2;
    int rc;
    if ((rc = ensure_ingest_streams(c)) != DD_OK) return rc;
    return Ingest(c, k, pl, paths, nfiles, kmin, kmax, regs, nthreads, promote, t_begin).run();
}
}  // namespace

extern "C" {
int dd_sketch_fasta(dd_ctx* c, const char* path, int kmin, int kmax, uint8_t* regs) {
    if (check_ctx(c)) return DD_EINVAL;
    if (!path) return fail(DD_EINVAL, "null path");
    // A file of some size takes the ingestion pipeline of dd_sketch_files (loader threads reading slices into pinned buffers, the
    // copy under way while they read, .gz inflated on the device): one plain 50 Mbp file 12.7 -> 4.2 ms, 250 Mbp 60 -> 18 ms at
    // log2m 14 (scripts/ab_one_file.py); below 4 MiB this path's one read + one copy is the shorter one (20 kbp: 0.4 against 0.9 ms).
    {
        struct stat sb;
        if (stat(path, &sb) == 0 && S_ISREG(sb.st_mode) && sb.st_size >= ((off_t)4 << 20)) {
            const char* one[1] = {path};
            return dd_sketch_files(c, one, 1, kmin, kmax, regs, 0);
        }
    }
    FileBuf buf;
    std::string err;
    // (one file: a .gz is inflated by every CPU this process may use -- BGZF blocks, or pieces of a plain member)
    if (!dd::read_fasta_file(path, buf, err, usable_cpus())) return fail(DD_EIO, "%s", err.c_str());
    return dd_sketch_buffer(c, buf.data(), buf.size(), kmin, kmax, regs);
}
int dd_sketch_files(dd_ctx* c, const char* const* paths, int nfiles, int kmin, int kmax, uint8_t* regs,
                    int nthreads) {
    if (check_ctx(c)) return DD_EINVAL;
    const Knobs k;
    IngestState& in = c->ingest;
    in.inflate_retry = false;
    in.inflate_retry_counts = false;
    int rc = sketch_files_impl(c, k, paths, nfiles, kmin, kmax, regs, nthreads);
    // (DD_INFLATE_STRICT=1: no second try -- the tests and scripts/fuzz_inflate.py set it so that a decoder bug cannot hide
    // behind the fallback)
    if (rc != DD_OK && in.inflate_retry && !k.strict) {
        // a BGZF block the device decoder would not take: the whole call again with every .gz inflated on the host, whose
        // decoder either reads the file or says what is wrong with it
        // (only this call -- one damaged file must not cost a long-lived context its device path --, unless it keeps
        // happening: three refusals and the context stays on the host)
        in.inflate_retry = false;
        const bool was = in.no_gpu_inflate;
        in.no_gpu_inflate = true;
        rc = sketch_files_impl(c, k, paths, nfiles, kmin, kmax, regs, nthreads);
        in.no_gpu_inflate = was || (in.inflate_retry_counts && ++in.inflate_refusals >= 3);
    }
    return rc;
}
int dd_last_ingest_stats(dd_ctx* c, double* wall_ms, double* loader_wait_ms, int* batches, uint64_t* bytes) {
    if (check_ctx(c)) return DD_EINVAL;
    if (wall_ms) *wall_ms = c->ingest.ms[0];
    if (loader_wait_ms) *loader_wait_ms = c->ingest.ms[1];
    if (batches) *batches = (int)c->ingest.ms[2];
    if (bytes) *bytes = (uint64_t)c->ingest.ms[3];
    return DD_OK;
}
// The ingestion pipeline's text, for checking the device decoders byte by byte (tests/test_gpu_parity.py, scripts/fuzz_inflate.py):
// one dd_sketch_files pass (k = 21 only) whose batches also copy every file's text -- as K0 is about to read it -- to the caller.
int dd_inflate_files(dd_ctx* c, const char* const* paths, int nfiles, uint8_t* const* out, const size_t* caps, size_t* lens, int nthreads) {
    if (check_ctx(c)) return DD_EINVAL;
    if (nfiles < 0 || (nfiles && (!paths || !out || !caps || !lens))) return fail(DD_EINVAL, "null argument");
    for (int i = 0; i < nfiles; ++i) {
        if (!out[i] && caps[i]) return fail(DD_EINVAL, "null buffer at index %d", i);
        lens[i] = 0;
    }
    std::vector<uint8_t> regs((size_t)nfiles << c->p);
    IngestState::TextSink sink{out, caps, lens, false};
    c->ingest.text_sink = &sink;
    const int rc = dd_sketch_files(c, paths, nfiles, 21, 21, regs.data(), nthreads);
    c->ingest.text_sink = nullptr;
    if (rc != DD_OK) return rc;
    if (sink.short_buffer) return fail(DD_EINVAL, "a buffer is smaller than its file's text (the sizes needed are in lens[])");
    return DD_OK;
}
}  // extern "C"

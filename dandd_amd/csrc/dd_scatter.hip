// dd_scatter.hip -- K1 at log2m >= 17: the registers stay in HBM and are reached through record streams.
//
// scatter (scatter_first_bin_kernel in the first epoch of a call, scatter_kernel behind its filter afterwards) walks the
// token stream as dd_sweep.hip does -- the same tile input, segment walk, windows and hash: dd_k1.h -- and turns every
// update that may raise a register into a 4-byte record in its row's stream; sort_chunks_kernel orders the chunks of the
// filtered epochs' streams by index tile; replay_kernel applies a row's records to one 64 KiB index tile in LDS and
// writes the tile and its part of the row's filter back; reset_cursors_kernel empties the streams for the next epoch.
#include "dd_common.h"
#include "dd_kernels.h"
#include "dd_k1.h"

namespace dd {
namespace {

constexpr uint32_t kQueueEntries = 128;  // per wave and queue (scatter_kernel); a push adds <= 64 to < 64 waiting

// ---- log2m >= 17, bucket mode: scatter + sort + replay (dd_kernels.h) -------------------------------
// A compare-and-swap path (RegsGlobal, dd_k1.h: what a full stream falls back to) is bound by the device's scattered-atomic rate (27 G/s measured, any
// atomic, any footprint: profiles/r01_ubench_atomics.txt).  Two earlier forms of this path were measured
// (profiles/r02_bucket_path.txt): records stored one by one to per-index-tile chunks ran into the same
// wall (a 4-byte store that is not part of a whole line leaves the L2 as a fabric write of its own);
// records staged per (wave, index tile) in LDS and flushed as 128-byte lines made the stores cheap but
// cost 30 VALU + 30 SALU per wave-update for the staging -- the kernel is issue-bound, so that doubled it.
// Hence: scatter does NO partitioning.  A wave appends its surviving records to one LDS queue (ballot +
// mbcnt + one ds_write) and, whenever 64 wait, stores them as one 256-byte block to the ROW's record
// stream; the chunks of the stream are sorted by index tile afterwards (sort_chunks_kernel, or the first epoch's
// scatter itself), and the replay workgroups of a row (one per 64 KiB index tile) read only their own segments.
// The rows a sort / replay / reset launch covers: rows k0 .. k0+nks-1 of every genome (one k class), numbered
// densely; table index = genome * K + k0 + local % nks.
struct RowSet {
    int K, k0, nks, nrows;  // nrows = genomes * nks, or the rows of one row group
    int row0;               // ... which starts at this row of the class
    DD_D int index(uint32_t local) const {
        local += (uint32_t)row0;
        return (int)(local / (uint32_t)nks) * K + k0 + (int)(local % (uint32_t)nks);
    }
};
constexpr uint32_t kChunkRecords = 1024;         // 4 KiB; one global atomic hands out one chunk of the row's stream

struct Scatter {
    uint32_t queue;        // byte offset in g_lds of this wave's two record queues (2 x kQueueEntries x 4 B)
    uint32_t* area;        // the row's record stream, chunk c at area + c * kChunkRecords
    uint32_t* cursor;      // records reserved so far (may run past the capacity: readers clamp)
    uint8_t* regs;         // the row itself: what candidates are probed against, and where records go when the stream is full
    uint32_t cap_chunks;
    int fshift;            // hash high word >> fshift = index of the register group's filter entry (32 - p + logg)
    int ishift;            // hash high word >> ishift = register index (32 - p)
    uint32_t himask;       // the index bits of the hash high word
};
constexpr uint32_t kScatterUnit = 256;  // records a wave reserves at a time (a multiple of 64)
DD_D uint32_t& lds32(uint32_t off) { return *reinterpret_cast<uint32_t*>(g_lds + off); }
DD_D uint32_t gadd32(void* p, uint32_t v) {
    return __hip_atomic_fetch_add((DD_GLOBAL uint32_t*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// 64 records (one per lane; null records have rho 0) leave for the row's stream.  The stream is DENSE: the row's
// cursor counts records, a wave reserves kScatterUnit of them with one atomic add (`cur` / `left` = its reservation), so
// the 1024-record chunks the sort and the replay work on are all full whatever the job sizes were.  (Round 2's first
// form gave every wave of every job a chunk of its own: 4.4 M chunks per log2m 20 step for 1.7 G records, i.e. 38 % full,
// and the replay's per-tile segments 30 records long.)  Whole waves, uniform state.
DD_D void scatter_block(const Scatter& s, uint32_t rec, uint32_t& cur, uint32_t& left) {
    const uint32_t lane = threadIdx.x & 63u;
    if (left == 0u) {
        uint32_t c = 0;
        if (lane == 0) c = gadd32(s.cursor, kScatterUnit);
        cur = __builtin_amdgcn_readfirstlane(c);
        left = kScatterUnit / 64u;
    }
    const uint32_t pos = cur;
    cur += 64u;
    --left;
    if (pos + 64u > s.cap_chunks * kChunkRecords) {
        // the stream is full: the records go to their registers directly (exact, slow, rare)
        if (rec >> 24) {
            uint8_t* a = s.regs + (rec & 0xFFFFFFu);
            (void)cas_raise<RegsGlobal>(a, RegsGlobal::load32(a), rec >> 24);
        }
        return;
    }
    gstore4(s.area + pos + lane, rec);
}
// Second-level filter: 64 queued candidates are checked against the ROW ITSELF -- one byte load per
// lane from the registers as the last replay left them (the row of the jobs an XCD is running stays in that
// XCD's L2: job order, dd_plan.hip) -- and only those that really exceed their register move on to a second
// queue and, 64 at a time, to the stream.  The group-minimum filter lets ~25 % of the updates through at log2m
// 20; about 10 % really raise a register.  Exact either way: a register only rises, so its last stored value is
// a lower bound.
// Candidates wait in the first queue as the hash word's index bits with rho - 1 in the low byte (one v_and_or when
// they are queued -- that code runs on nearly every update of the wave; 0xFF = no candidate); what survives the
// probe is put into record form, idx | rho << 24, here, once per 64 candidates.
DD_D void scatter_probe(const Scatter& s, uint32_t cand, uint32_t& waiting2, uint32_t& cur, uint32_t& left) {
    const uint32_t rm1 = cand & 0xFFu, idx = cand >> s.ishift;
    bool live = rm1 != 0xFFu;
    if (live) live = rm1 >= (uint32_t)*(const DD_GLOBAL uint8_t*)(s.regs + idx);  // rho > register
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(live);
    if (mask) {
        if (live) {
            const uint32_t rank = lanes_below(mask);
            lds32(s.queue + kQueueEntries * 4u + 4u * (waiting2 + rank)) = idx | ((rm1 + 1u) << 24);
        }
        waiting2 += (uint32_t)__builtin_popcountll(mask);
        if (waiting2 >= 64u) {
            waiting2 -= 64u;
            scatter_block(s, lds32(s.queue + kQueueEntries * 4u + 4u * (waiting2 + (threadIdx.x & 63u))), cur, left);
        }
    }
}
// One update.  Reached by whole waves (`valid`: the lane has a k-mer); `waiting`, `waiting2`, `cur` are wave-uniform.
// The filter holds 4-bit bounds (saturating at 15), two register groups per byte: twice the resolution of byte entries
// in the same 64 KiB of LDS for three more instructions per update (measured better at log2m 18, 19 and 20).
DD_D void scatter_update(const Scatter& s, uint32_t& waiting, uint32_t& waiting2, uint32_t& cur, uint32_t& left, uint64_t h, int p, bool valid) {
    const Probe q = probe(h, p);
    // entry e = hi >> fshift sits in nibble e & 1 of byte e >> 1: address and nibble shift straight from hi (three
    // instructions instead of five; fshift >= 32 - 20 + 1).  The byte is read at its absolute LDS address: this
    // kernel has no static LDS, so the dynamic array starts at 0 (checked when the job starts), and going through
    // the g_lds symbol costs a v_add of its link-time address, 0, on every update.
    const uint32_t at = q.hi >> (s.fshift + 1);
    const uint32_t bound = __builtin_amdgcn_ubfe((uint32_t)*(const __attribute__((address_space(3))) uint8_t*)(uintptr_t)at, (q.hi >> (s.fshift - 2)) & 4u, 4u);
    const bool cand = valid && q.lz >= bound;  // rho > bound (or hiw == 0: rho >= 33)
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(cand);
    if (mask) {
        if (cand) {
            const uint32_t rank = lanes_below(mask);
            lds32(s.queue + 4u * (waiting + rank)) = (q.hi & s.himask) | (rho_of(q, p) - 1u);  // (scatter_probe's form)
        }
        waiting += (uint32_t)__builtin_popcountll(mask);
        if (waiting >= 64u) {
            waiting -= 64u;
            scatter_probe(s, lds32(s.queue + 4u * (waiting + (threadIdx.x & 63u))), waiting2, cur, left);
        }
    }
}

// The filtered epochs' scatter: one k per job.  (Two consecutive ks per job -- shared token loads and window push, 7 of the
// ~50 VALU instructions of an update -- measured SLOWER on MI355X both with two 64 KiB filters = one workgroup per CU and
// with two 16 KiB filters at two workgroups per CU: profiles/r02_bucket_path.txt, profiles/r03_bucket_path.txt.)
template <int KC, bool CANON>
__global__ __launch_bounds__(1024) void scatter_kernel(const SweepGenome* __restrict__ genomes,
                                                      const SweepJob* __restrict__ jobs, int p, ScatterParams sp) {
    const SweepJob job = jobs[blockIdx.x];
    if (job.tile_begin >= job.tile_end) return;  // filler of the XCD-affine order
    lds_starts_at_zero();  // scatter_update reads the filter at absolute LDS addresses
    const SweepGenome g = genomes[job.genome];
    const int k = job.kfirst;
    const uint32_t m = 1u << p;
    const unsigned long long ntok = gload8u(g.ntok);
    const uint32_t nflt = (m >> sp.logg) >> 1;  // bytes of the filter

    TileIn next;
    fetch_tile(g, job, ntok, job.tile_begin, next);

    // the row's filter as the previous epoch's replay left it (plain loads: written by an earlier kernel) at LDS offset 0,
    // then the per-wave queues
    const BucketRow row = sp.rows[(size_t)job.genome * sp.K + job.krow];
    {
        uint4* f4 = reinterpret_cast<uint4*>(g_lds);
        for (uint32_t i = threadIdx.x; i < (nflt >> 4); i += blockDim.x) f4[i] = gload16(row.filter + (size_t)i * 16);
    }
    Scatter s;
    s.queue = nflt + (threadIdx.x >> 6) * (kQueueEntries * 4u * 2u);
    s.area = row.area;
    s.cursor = row.cursor;
    s.regs = row.regs;
    s.cap_chunks = sp.cap_chunks;
    s.fshift = 32 - p + sp.logg;
    s.ishift = 32 - p;
    s.himask = ~((1u << (32 - p)) - 1u);
    uint32_t waiting = 0, waiting2 = 0, cur = 0, left = 0;
    __syncthreads();

    for (unsigned tile = job.tile_begin; tile < job.tile_end; ++tile) {
        const TileIn in = next;
        fetch_tile(g, job, ntok, tile + 1, next);
        // Lanes beyond the stream stay in the loop as all-BREAK segments while any lane of their wave has
        // tokens: the queue counters and the stream offsets must stay wave-uniform.
        if (!__any(in.live)) continue;
        ScatterWindows<KC> win;
        walk_segment(in, win, [&](auto clean, int run) {
            scatter_update(s, waiting, waiting2, cur, left, win.template hash<CANON>(k), p, decltype(clean)::value || run >= k);
        });
    }
    // what still waits leaves as a block padded with null records, and what is left of the wave's last reservation is
    // filled with null blocks (the stream has no holes: sort and replay read all of it)
    const uint32_t lane = threadIdx.x & 63u;
    if (waiting) scatter_probe(s, lane < waiting ? lds32(s.queue + 4u * lane) : 0xFFu, waiting2, cur, left);
    if (waiting2) scatter_block(s, lane < waiting2 ? lds32(s.queue + kQueueEntries * 4u + 4u * lane) : 0u, cur, left);
    while (left) scatter_block(s, 0u, cur, left);
}

// ---- first epoch, BINNED tiles of tokens (round 4, what runs) ----------------------------------------------------
// Sorting 16 384 records per workgroup still costs two LDS atomics per record (count, then place) plus the pass over
// the collection area: 2.4 of the 4.5 ms of a class-0 launch over 64 x 5 Mbp at log2m 20, against 2.1 ms of hashing
// (timing-only builds, profiles/r04_bucket_path.txt).  A record's index tile is the top bits of a hash, so the 65 536
// records a workgroup makes of one tile of tokens spread over the 16 bins (index tile x copy) as evenly as coin flips
// do: 4096 per bin, sigma 62.  So every bin of a chunk gets a FIXED region of kBinCap = 4480 records (+ 6 sigma) in
// the row's stream, a record's slot is ONE returning LDS atomic on the workgroup's counter of its bin, and the record
// goes straight from the hash to its slot -- no collection area, no counting pass, no placement pass, one workgroup
// barrier per 64 updates (the counters of odd and even tiles alternate; wave 0 saves and clears a tile's counters
// behind the barrier while the others already fill the next tile's).  A bin that should ever overflow sends the
// record to its register by compare-and-swap (exact; ~3e-10 per bin).  The replay reads a bin's records -- 16 KiB
// in one piece -- with 16-byte loads.  Stream space: 70 instead of 64 chunks of 1024 records per tile of tokens.
constexpr uint32_t kBinCap = 4480;                        // records per (chunk, bin): a multiple of 64
constexpr uint32_t kBinChunkRecords = 16u * kBinCap;      // 71 680 = 70 x 1024: stream space of one tile of tokens
constexpr uint32_t kBinPosSlot = 128u;                    // LDS: counters [2][16] at 0, the job's position behind them
constexpr uint32_t kBinLdsBytes = 256u;
constexpr int kOnesLog2Max = 19;                          // registers of a row whose rho = 1 updates are bits in LDS (below)

// Updates of rho = 1 (round 5): HALF of all updates have rho = 1, and all a register can learn from them is that it
// is not empty.  They leave no record: the workgroup keeps one bit per register of its row in LDS (m / 8 bytes behind the
// counters, 64 KiB at most), sets it with a ds_or and ORs the words into the row's bitmap in HBM
// when its job ends (BucketRow::ones; 32 K atomics per job against the ~330 K four-byte stores they stand for); the replay
// raises a register that is still 0 behind a set bit to 1 when it writes the tile back.  Exact: max(rho) over a register's
// updates is 1 iff there is an update and none has rho >= 2.
template <int KC, bool CANON>
__global__ __launch_bounds__(1024) void scatter_first_bin_kernel(
    const SweepGenome* __restrict__ genomes, const SweepJob* __restrict__ jobs, int p, ScatterParams sp) {
    const SweepJob job = jobs[blockIdx.x];
    if (job.tile_begin >= job.tile_end) return;  // filler of the XCD-affine order
    lds_starts_at_zero();
    const SweepGenome g = genomes[job.genome];
    const int k = job.kfirst;
    const unsigned long long ntok = uniform64(gload8u(g.ntok));
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;

    TileIn next;
    fetch_tile(g, job, ntok, job.tile_begin, next);

    const BucketRow row = sp.rows[(size_t)job.genome * sp.K + job.krow];
    uint32_t* const area = uniform_ptr(row.area);
    uint16_t* const counts = uniform_ptr(row.seg);  // [chunk][16]: records in each bin
    uint8_t* const regs = uniform_ptr(row.regs);
    const uint32_t cap_records = sp.cap_chunks * kChunkRecords;
    const int cshift = 4 - sp.nb_log2, tile_sh = 32 - sp.nb_log2;
    if (threadIdx.x < 32u) lds32(4u * threadIdx.x) = 0;
    if (threadIdx.x == 0) lds32(kBinPosSlot) = gadd32(row.cursor, (job.tile_end - job.tile_begin) * kBinChunkRecords);
    // (at most 2^19 bits = 64 KiB, so that two workgroups still share a CU: at log2m 20 only the updates of the lower half of the
    // row's registers are bits, the others stay records -- one workgroup per CU costs this kernel 6 %, profiles/r05_bucket_path.txt)
    const uint32_t ones_regs = 1u << (p < kOnesLog2Max ? p : kOnesLog2Max), ones_words = ones_regs >> 5;
    for (uint32_t w = threadIdx.x; w < ones_words; w += blockDim.x) lds32(kBinLdsBytes + 4u * w) = 0;
    __syncthreads();
    const uint32_t pos0 = __builtin_amdgcn_readfirstlane(lds32(kBinPosSlot));
    const uint32_t copy = lane & ((1u << cshift) - 1u);

    for (unsigned tile = job.tile_begin; tile < job.tile_end; ++tile) {
        const TileIn in = next;
        fetch_tile(g, job, ntok, tile + 1, next);
        const uint32_t t = tile - job.tile_begin;
        const uint32_t ctr = (t & 1u) * 64u;
        const uint32_t cpos = pos0 + t * kBinChunkRecords;
        const bool room = cpos + kBinChunkRecords <= cap_records;  // else: the stream is full, records go to the registers (exact, slow, rare)
        if (__any(in.live)) {
            uint8_t* const chunk = reinterpret_cast<uint8_t*>(area + cpos);   // (wave-uniform: the store below is base + 32-bit offset)
            // (deferring a record's store until the next update's atomic is out, so that the slot's LDS round trip overlaps a
            // hash, and unrolling the token loop by two were both measured: no difference -- the loop is not waiting there)
            ScatterWindows<KC> win;
            auto update = [&](bool valid) {
                const Probe q = probe(win.template hash<CANON>(k), p);
                if (!valid) return;
                const uint32_t rho = rho_of(q, p);
                if (rho == 1u && (q.hi >> (32 - p)) < ones_regs) {
                    const uint32_t idx = q.hi >> (32 - p);
                    atomicOr(&lds32(kBinLdsBytes + ((idx >> 5) << 2)), 1u << (idx & 31u));
                    return;
                }
                const uint32_t rec = (q.hi >> (32 - p)) | (rho << 24);
                const uint32_t bin0 = (q.hi >> tile_sh) << cshift;  // + copy = the bin
                uint32_t slot = kBinCap;
                if (room) slot = atomicAdd(&lds32(ctr + ((bin0 | copy) << 2)), 1u);
                if (__builtin_expect(slot < kBinCap, 1)) {
                    // (round 5: the slot's address as the chunk's uniform base + a 32-bit byte offset -- one v_mad_u32_u24 and a shift
                    // in front of a store with an SGPR base instead of a multiply and two 64-bit adds; A/B on one box: 23.3-23.6 against
                    // 23.4-23.8 ms for 64 x 5 Mbp at log2m 20, 25.0-25.2 against 24.9-25.0 for 10 x 50 Mbp -- within the noise: the kernel is
                    // not waiting for its VALU, profiles/r05_bucket_path.txt)
                    gstore4(chunk + (__umul24(bin0 | copy, kBinCap) + slot) * 4u, rec);
                } else {
                    uint8_t* a = regs + (rec & 0xFFFFFFu);
                    (void)cas_raise<RegsGlobal>(a, RegsGlobal::load32(a), rec >> 24);
                }
            };
            // (lanes beyond the stream walk an all-BREAK segment, as in scatter_kernel: the barrier below is the workgroup's)
            walk_segment(in, win, [&](auto clean, int run) {
                update(decltype(clean)::value || run >= k);
            });
        }
        __syncthreads();  // the tile's records are placed and counted; the other parity's counters are clear
        if (wave == 0u && lane < 16u) {
            const uint32_t c = lds32(ctr + 4u * lane);
            lds32(ctr + 4u * lane) = 0;
            if (room) ((DD_GLOBAL uint16_t*)counts)[(size_t)(cpos / kBinChunkRecords) * 16u + lane] = (uint16_t)(c < kBinCap ? c : kBinCap);
        }
    }
    // (behind the last tile's barrier: every ds_or of the job is in)
    uint32_t* const ones = uniform_ptr(row.ones);
    for (uint32_t w = threadIdx.x; w < ones_words; w += blockDim.x) {
        const uint32_t v = lds32(kBinLdsBytes + 4u * w);
        if (v) atomicOr(ones + w, v);
    }
}

// Between scatter and replay when a row has more than one index tile (log2m >= 17): every chunk of every
// stream is sorted by index tile in place (one wave per chunk: LDS counting sort), null records dropped,
// and the start of each tile's segment is noted in seg[chunk][tile].  A replay workgroup then reads only
// its own segments; without this every one of the 8 workgroups of a log2m 20 row (128 KiB tiles then)
// inspected every record (measured: 42 of 72 ms).  HBM-bound: each record is read and written once more.
__global__ __launch_bounds__(256) void sort_chunks_kernel(const BucketRow* __restrict__ rows, RowSet rs, int p, int nb_log2,
                                                         uint32_t cap_chunks, int wgs_per_row) {
    __shared__ uint32_t sorted[4][kChunkRecords];
    __shared__ uint32_t hist[4][16];
    const BucketRow row = rows[rs.index(blockIdx.x / (uint32_t)wgs_per_row)];
    if (!row.area) return;
    const uint32_t handed = gload4(row.cursor);
    const uint32_t nrec = handed < cap_chunks * kChunkRecords ? handed : cap_chunks * kChunkRecords;  // reservations are multiples of 64, the capacity of 1024
    const uint32_t nchunks = (nrec + kChunkRecords - 1u) / kChunkRecords;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, nb = 1u << nb_log2;
    const int tshift = p - nb_log2;
    for (uint32_t c = (blockIdx.x % wgs_per_row) * 4u + wave; c < nchunks; c += (uint32_t)wgs_per_row * 4u) {
        const uint32_t f = nrec - c * kChunkRecords < kChunkRecords ? nrec - c * kChunkRecords : kChunkRecords;
        uint32_t e[16];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t pos = (uint32_t)i * 256u + lane * 4u;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (pos < f) v = gload16(row.area + (size_t)c * kChunkRecords + pos);
            e[4 * i] = v.x, e[4 * i + 1] = v.y, e[4 * i + 2] = v.z, e[4 * i + 3] = v.w;
        }
        if (lane < 16) hist[wave][lane] = 0;
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (e[i] >> 24) atomicAdd(&hist[wave][(e[i] & 0xFFFFFFu) >> tshift], 1u);
        __builtin_amdgcn_wave_barrier();
        // exclusive prefix over the (at most 16) tiles: lanes 0..15
        const uint32_t mine = lane < nb ? hist[wave][lane] : 0u;
        uint32_t incl = mine;
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= (uint32_t)d) incl += up;
        }
        const uint32_t total = __shfl(incl, (int)nb - 1);
        __builtin_amdgcn_wave_barrier();
        if (lane < nb) {
            hist[wave][lane] = incl - mine;
            ((DD_GLOBAL uint16_t*)row.seg)[(size_t)c * 16u + lane] = (uint16_t)(incl - mine);
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (e[i] >> 24) sorted[wave][atomicAdd(&hist[wave][(e[i] & 0xFFFFFFu) >> tshift], 1u)] = e[i];
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t pos = (uint32_t)i * 256u + lane * 4u;
            if (pos < total) {
                const uint4 v = *reinterpret_cast<const uint4*>(&sorted[wave][pos]);  // past `total`: stale, never read
                gstore16(row.area + (size_t)c * kChunkRecords + pos, v);
            }
        }
        if (lane == 0) gstore4(row.fill + c, total);
        __builtin_amdgcn_wave_barrier();
    }
}

// One workgroup per (row, index tile); LDS: the tile (64 KiB, or m bytes if smaller); two workgroups per
// CU.  BINS = false (filtered epochs): a wave takes every 16th chunk of the row's stream, U at a time, and reads only the
// segment of its own tile that sort_chunks_kernel left; segment headers, records and the LDS work of three consecutive steps
// overlap.  BINS = true (the first epoch's binned tiles, scatter_first_bin_kernel): chunk C = 16 bins of kBinCap records'
// room, counts in seg[C][16]; unit u = (chunk, copy of this tile's bin); the 512-record pieces of a unit go round the 16
// waves, so every wave has a 2 KiB piece in flight while it applies the previous one; the rho = 1 updates, which left a bit
// instead of a record, are applied when the tile is written back.
template <bool BINS>
__global__ __launch_bounds__(1024) void replay_kernel(const BucketRow* __restrict__ rows, RowSet rs, int p, int logg,
                                                     int nb_log2, uint32_t cap_chunks) {
    lds_starts_at_zero();
    const uint32_t nb = 1u << nb_log2;
    const uint32_t within = blockIdx.x >> 3, xcd = blockIdx.x & 7u;
    const uint32_t r = (within >> nb_log2) * 8u + xcd, b = within & (nb - 1u);
    if (r >= (uint32_t)rs.nrows) return;
    const BucketRow row = rows[rs.index(r)];
    if (!row.area) return;
    const uint32_t handed = gload4(row.cursor);
    if (handed == 0u) return;  // nothing was recorded for this row in this epoch: registers and filter stand
    const uint32_t nrec = handed < cap_chunks * kChunkRecords ? handed : cap_chunks * kChunkRecords;
    const uint32_t nchunks = (nrec + kChunkRecords - 1u) / kChunkRecords;
    const uint32_t tile = 1u << (p - nb_log2);
    uint8_t* const tile_g = row.regs + (size_t)b * tile;
    uint4* l4 = reinterpret_cast<uint4*>(g_lds);
    for (uint32_t i = threadIdx.x; i < (tile >> 4); i += blockDim.x) l4[i] = gload16(tile_g + (size_t)i * 16);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    auto apply = [&](uint32_t e) { lds_raise(e & (tile - 1u), e >> 24); };  // null records (rho 0) fall through
    constexpr int U = 4;
    const DD_GLOBAL uint16_t* seg = (const DD_GLOBAL uint16_t*)row.seg;
    // U records of a lane in three sweeps -- all register words read, all first compare-and-swaps issued, then the
    // (rare) retries -- instead of read / compare / CAS record by record: the LDS round trips of one lane's records
    // overlap (an LDS atomic orders every later LDS access of the wave behind it, so the record-by-record form ran
    // them back to back; while the registers are still filling, half the records raise one).  A word changed in
    // between -- by a neighbour, or by this lane's previous record -- fails its CAS and is retried from the value
    // that came back.
    auto apply_u = [&](const uint32_t (&e)[U]) {
        uint32_t wd[U];
        uint32_t retry = 0;  // bit i: record i's first CAS found another value than the one read
#pragma unroll
        for (int i = 0; i < U; ++i) wd[i] = RegsLds::load32(e[i] & (tile - 1u));
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const uint32_t a = e[i] & (tile - 1u), rho = e[i] >> 24, sh = RegsLds::shift(a), cur = (wd[i] >> sh) & 0xFFu;
            if (rho > cur) {
                const uint32_t prev = RegsLds::cas32(a, wd[i], wd[i] + ((rho - cur) << sh));
                if (prev != wd[i]) retry |= 1u << i;
                wd[i] = prev;
            }
        }
        if (__any(retry != 0u)) {
#pragma unroll
            for (int i = 0; i < U; ++i)
                if ((retry >> i) & 1u) (void)cas_raise<RegsLds>(e[i] & (tile - 1u), wd[i], e[i] >> 24);
        }
    };
    if (BINS) {
        const int cshift = 4 - nb_log2;
        const uint32_t nunits = (nrec / kBinChunkRecords) << cshift;
        const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        struct Piece {
            uint4 a, b;
            uint32_t off, cnt;  // wave-uniform: the piece's first record within its bin, the bin's records
        };
        auto header = [&](uint32_t u) -> uint32_t {  // records in unit u's bin
            return u < nunits ? (uint32_t)seg[(size_t)(u >> cshift) * 16u + ((b << cshift) | (u & ((1u << cshift) - 1u)))] : 0u;
        };
        auto issue = [&](uint32_t u, uint32_t cnt, Piece& P) {
            P.off = ((wave - u) & 15u) * 512u;
            P.cnt = __builtin_amdgcn_readfirstlane(cnt);
            P.a = P.b = make_uint4(0, 0, 0, 0);
            if (P.off >= P.cnt) return;
            const uint32_t* base = row.area + (size_t)(u >> cshift) * kBinChunkRecords + ((b << cshift) | (u & ((1u << cshift) - 1u))) * kBinCap + P.off;
            if (P.off + 4u * lane < P.cnt) P.a = gload16(base + 4u * lane);  // (a quad may straddle the bin's last record: still inside its region)
            if (P.off + 256u + 4u * lane < P.cnt) P.b = gload16(base + 256u + 4u * lane);
        };
        uint32_t c0 = header(0), c1 = header(1), c2 = header(2);
        Piece cur, nxt;
        issue(0, c0, cur);
        for (uint32_t u = 0; u < nunits; ++u) {
            issue(u + 1u, c1, nxt);
            c1 = c2;
            c2 = header(u + 3u);
            if (cur.off < cur.cnt) {
                uint32_t ea[U] = {cur.a.x, cur.a.y, cur.a.z, cur.a.w}, eb[U] = {cur.b.x, cur.b.y, cur.b.z, cur.b.w};
                if (cur.off + 512u > cur.cnt) {  // the bin's last piece: what lies behind its last record is nulled
                    const uint32_t d = cur.off + 4u * lane;
#pragma unroll
                    for (int j = 0; j < U; ++j) {
                        ea[j] = d + (uint32_t)j < cur.cnt ? ea[j] : 0u;
                        eb[j] = d + 256u + (uint32_t)j < cur.cnt ? eb[j] : 0u;
                    }
                }
                apply_u(ea);
                apply_u(eb);
            }
            cur = nxt;
        }
    } else {
    struct Head {
        uint32_t st[U], en[U];
    };
    struct Recs {
        uint32_t r0[U], r1[U];
    };
    auto heads = [&](uint32_t c, Head& h) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t cc = c + 16u * u;
            h.st[u] = h.en[u] = 0;
            if (cc < nchunks) {
                if (nb > 1u) {
                    h.st[u] = seg[(size_t)cc * 16u + b];
                    h.en[u] = b + 1u < nb ? (uint32_t)seg[(size_t)cc * 16u + b + 1u] : gload4(row.fill + cc);
                } else {  // unsorted single-tile rows: the raw stream, null records included
                    h.en[u] = nrec - cc * kChunkRecords < kChunkRecords ? nrec - cc * kChunkRecords : kChunkRecords;
                }
            }
        }
    };
    auto records = [&](uint32_t c, const Head& h, Recs& v) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t* base = row.area + (size_t)(c + 16u * u) * kChunkRecords;
            const uint32_t i0 = h.st[u] + lane, i1 = i0 + 64u;
            v.r0[u] = i0 < h.en[u] ? gload4(base + i0) : 0u;
            v.r1[u] = i1 < h.en[u] ? gload4(base + i1) : 0u;
        }
    };
    const uint32_t step = 16u * U, c_first = threadIdx.x >> 6;
    Head h1, h2;
    Recs v1;
    heads(c_first, h1);
    heads(c_first + step, h2);
    records(c_first, h1, v1);
    for (uint32_t c = c_first; c < nchunks; c += step) {
        const Head h0 = h1;
        const Recs v0 = v1;
        h1 = h2;
        heads(c + 2u * step, h2);      // headers two steps ahead
        records(c + step, h1, v1);     // records one step ahead
        // The 2U records of the step, U at a time (apply_u; all 2U together need 75+ VGPRs, and above 64 only one
        // 1024-thread workgroup fits a CU)
        apply_u(v0.r0);
        apply_u(v0.r1);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t* base = row.area + (size_t)(c + 16u * u) * kChunkRecords;
            for (uint32_t i = h0.st[u] + 128u + lane; i < h0.en[u]; i += 64u) apply(gload4(base + i));  // longer than twice the expected size
        }
    }
    }
    __syncthreads();
    if (BINS) {
        // the updates with rho = 1 left no record, only a bit (scatter_first_bin_kernel): a register still 0 behind
        // a set bit becomes 1.  Thread i holds registers 16 i .. 16 i + 15 of the tile = halfword i of the tile's bits.
        const DD_GLOBAL uint16_t* bits = (const DD_GLOBAL uint16_t*)row.ones + (((size_t)b * tile) >> 4);
        for (uint32_t i = threadIdx.x; i < (tile >> 4); i += blockDim.x) {
            const uint32_t h = bits[i];
            if (!h) continue;
            uint4 v = l4[i];
            auto raise = [](uint32_t w, uint32_t nib) {
                const uint32_t set = ((nib & 0xFu) * 0x00204081u) & 0x01010101u;                 // bit j of the nibble -> byte j
                const uint32_t zero = (~(w + 0x7F7F7F7Fu) & 0x80808080u) >> 7;                    // 1 in every byte that is 0 (bytes < 128)
                return w | (set & zero);
            };
            v.x = raise(v.x, h), v.y = raise(v.y, h >> 4), v.z = raise(v.z, h >> 8), v.w = raise(v.w, h >> 12);
            l4[i] = v;
        }
        __syncthreads();
    }
    for (uint32_t i = threadIdx.x; i < (tile >> 4); i += blockDim.x) gstore16(tile_g + (size_t)i * 16, l4[i]);
    // the tile's part of the filter: minimum of every group of 2^logg registers
    const uint32_t G = 1u << logg;
    auto group_min = [&](uint32_t f) {
        uint32_t lo = 0xFFu;
        if (G >= 4u) {
            for (uint32_t w = 0; w < G; w += 4) {
                const uint32_t mn = min4(*reinterpret_cast<const uint32_t*>(g_lds + f * G + w));
                lo = mn < lo ? mn : lo;
            }
        } else {
            for (uint32_t w = 0; w < G; ++w) lo = g_lds[f * G + w] < lo ? g_lds[f * G + w] : lo;
        }
        return lo;
    };
    // (4-bit entries, saturating at 15, two register groups per byte: measured better than byte entries at log2m 18, 19, 20)
    const uint32_t ngroups = tile >> logg;
    uint8_t* const flt = row.filter + ((((size_t)b * tile) >> logg) >> 1);
    for (uint32_t f = threadIdx.x; f < (ngroups >> 1); f += blockDim.x) {
        const uint32_t a = group_min(2u * f), c = group_min(2u * f + 1u);
        flt[f] = (uint8_t)((a < 15u ? a : 15u) | ((c < 15u ? c : 15u) << 4));
    }
}

// the stream cursors of all rows back to zero for the next epoch (replay's workgroups of a row cannot do
// it themselves: its sibling tiles may still be reading the cursor)
__global__ void reset_cursors_kernel(const BucketRow* __restrict__ rows, RowSet rs) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < rs.nrows && rows[rs.index((uint32_t)r)].area) gstore4(rows[rs.index((uint32_t)r)].cursor, 0u);
}

}  // namespace

// One scatter launch of a k class (log2m >= 17).  first_epoch: every register of the call is still zero -- the unfiltered,
// binned form (scatter_first_bin_kernel); later epochs: the filtered form (scatter_kernel).
void launch_scatter(const SweepGenome* genomes, const SweepJob* jobs, int njobs, int kclass, const SweepPlan& plan,
                    const ScatterParams& sp, hipStream_t st, bool first_epoch) {
    if (njobs <= 0) return;
    dispatch_kc_canon(kclass, plan.canonical, [&](auto kc, auto cn) {
        constexpr int KC = decltype(kc)::value;
        constexpr bool CN = decltype(cn)::value;
        if (first_epoch)
            launch_full_lds<scatter_first_bin_kernel<KC, CN>>(dim3((unsigned)njobs), dim3(1024),
                                                              (size_t)kBinLdsBytes + (((size_t)1 << std::min(plan.log2m, kOnesLog2Max)) >> 3), st,
                                                              genomes, jobs, plan.log2m, sp);
        else
            launch_full_lds<scatter_kernel<KC, CN>>(dim3((unsigned)njobs), dim3((unsigned)plan.threads), (size_t)plan.lds_bytes, st, genomes, jobs, plan.log2m, sp);
    });
}

// first_epoch: the records are the binned tiles scatter_first_bin_kernel left (+ the rows' rho = 1 bits); else the filtered
// scatter's dense stream, whose chunks are sorted by index tile first
void launch_replay(const BucketRow* rows, int ngenomes, int K, int k0, int nks, const SweepPlan& plan, hipStream_t st, bool first_epoch) {
    const RowSet rs{K, k0, nks, ngenomes * nks, 0};
    if (rs.nrows <= 0) return;
    const size_t tile = (size_t)1 << (plan.log2m - plan.nb_log2);
    const unsigned blocks = (unsigned)((rs.nrows + 7) / 8) * 8u << plan.nb_log2;
    if (!first_epoch) {
        const int wgs_per_row = 32;
        hipLaunchKernelGGL(sort_chunks_kernel, dim3((unsigned)rs.nrows * wgs_per_row), dim3(256), 0, st, rows, rs, plan.log2m,
                           plan.nb_log2, plan.cap_chunks, wgs_per_row);
    }
    dispatch_bool(first_epoch, [&](auto bins) {
        launch_full_lds<replay_kernel<decltype(bins)::value>>(dim3(blocks), dim3(1024), tile, st, rows, rs, plan.log2m, plan.logg, plan.nb_log2, plan.cap_chunks);
    });
    hipLaunchKernelGGL(reset_cursors_kernel, dim3((unsigned)(rs.nrows + 255) / 256), dim3(256), 0, st, rows, rs);
}

}  // namespace dd

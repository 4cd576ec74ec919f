// dd_exact_host.h -- what the exact entry points share on the host (defined in dd_exact_passes.hip; called by dd_exact_api.hip,
// dd_exact_emit_api.hip and dd_exact_samples_api.hip): the call frame, the path forms' upload, K0 over the inputs and their token counts read back, the
// pass driver, and the ordered-record step: the emission, its sanity check and the room that puts the records in order.
#pragma once
#include <functional>
#include "dd_ctx.h"

// What every entry checks first, in this order: the context, n against the entry's limit (64; 16: all subsets; 255: the wide rows), inputs and
// `out` for null, the k range.  exact_frame, the device forms': then nbytes (and what else may not be null), then the buffers.
int exact_args(dd_ctx* c, const void* inputs, int n, int nmax, int kmin, int kmax, const void* out);
int exact_frame(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, int nmax, int kmin, int kmax,
                const void* out, bool more_null = false);
int exact_check_inputs(const uint8_t* const* fasta_dev, const size_t* nbytes, int n);
// query (job) i of a call over n inputs sets no bit outside 0..n-1; `who`: "query" / "job", for the message
int exact_check_bits(const char* who, int i, uint64_t all, uint64_t none, int n);
// The shape of a ragged answer: `who` i ("job" / "sample" / "target") owns off[i+1] - off[i] `parts` ("words" / "rows") of it,
// one per `unit` tokens (a `unit_name`: "word" / "window") of a stream of ntok tokens.  input: the input that stream is, for
// the message (< 0: `who` itself, "it").
struct ExactShape { const char *who, *parts; uint64_t unit; const char* unit_name; };
int exact_check_shape(const ExactShape& s, int i, const uint64_t* off, int input, unsigned long long ntok);
// select's argument rules -> the (all, none) pairs its accumulator and the emission read
int select_table(const uint64_t* all, const uint64_t* none, int nq, int n, std::vector<uint64_t>& table);
using ExactDeviceForm = std::function<int(const uint8_t* const* fasta_dev, const size_t* nbytes)>;
// the files of a path form read, uploaded into the context's FASTA buffer and handed to the device form, on the context's device
int exact_upload_files(dd_ctx* c, const char* const* paths, int n, const ExactDeviceForm& device_form);
// a path form: exact_args, no null path, exact_upload_files (the device form checks the entry's own arguments)
int exact_path_form(dd_ctx* c, const char* const* paths, int n, int nmax, int kmin, int kmax, const void* out, const ExactDeviceForm& device_form);

// K0 over the n inputs of an exact call (once per call, whatever the number of ks) and where each genome's k-mers go
struct ExactInputs {
    const dd::ExactGenome* etab_dev = nullptr;
    size_t slots = 0, max_segments = 0;   // slots = 0: no input has a token
    std::vector<dd::ExactGenome> etab;    // the host's copy of etab_dev (dd_exact_locate: where each stream and its ntok lie)
};
int exact_prepare(dd_ctx* c, const uint8_t* const* fasta_dev, const size_t* nbytes, int n, ExactInputs& in);
// ntok of the inputs first .. first + count - 1, read back from where K0 left them (all 0 where no input has a token)
int exact_read_ntok(dd_ctx* c, const ExactInputs& in, int first, int count, std::vector<unsigned long long>& ntok);
size_t exact_budget(const char* env_mb = "DD_EXACT_MB", size_t unset = (size_t)24 << 30);   // bytes of k-mers a pass may hold: 24 GiB, or what the variable says (MiB)

// What a caller of exact_passes says about its part of the k-mer workspace.
struct ExactLayout {
    const char* what;                           // "exact count" / "exact schedule", for the messages
    int tag;                                    // launch_kmer_extract's tag mode; 2 adds the g | g_alt arrays (a byte per slot each)
    size_t (*temp_bytes)(size_t keys, int k);   // of the caller's sort
    size_t (*scratch_bytes)(size_t keys);       // what the caller wants behind the sort's temp (null: nothing)
};

// c->exact carved for `keys` k-mers:
// counters (256 B) | bin histogram (32 KiB) | lo | lo_alt [| hi | hi_alt] [| g | g_alt] | sort temp | scratch
struct ExactArrays {
    unsigned long long *counters, *hist;
    uint64_t *lo, *lo_alt, *hi, *hi_alt;   // hi: k > 32
    uint8_t *g, *g_alt;                    // tag mode 2
    void *temp, *scratch;
    size_t temp_bytes;
};
int exact_carve(dd_ctx* c, const ExactLayout& L, int k, size_t keys, ExactArrays& a);

// a pass is extracted: launch the sort of its `count` k-mers and what follows
using ExactConsume = std::function<int(const ExactArrays& a, size_t count)>;
// the counters of a pass, read back (dd_kernels.h, launch_kmer_extract); single: the pass held every slot of the inputs
using ExactCounted = std::function<void(const unsigned long long* h, bool single)>;
int exact_passes(dd_ctx* c, const ExactInputs& in, int n, int k, const ExactLayout& L, const ExactConsume& consume,
                 const ExactCounted& counted = nullptr);

// exact_passes with the consumer of the schedules and the emission: launch_exact_sort_tagged, then `then` on what it left.
// scratch_bytes: what `then` wants behind the sort's temp (null: exact_sched_scratch_bytes, launch_exact_sched's and the emission's)
using ExactSortedThen = std::function<hipError_t(const dd::ExactSorted& sorted, size_t count, void* scratch)>;
int exact_sorted_passes(dd_ctx* c, const ExactInputs& in, int n, int k, const char* what, const ExactSortedThen& then,
                        size_t (*scratch_bytes)(size_t keys) = nullptr);

// The ordered-record step.  exact_records reserves c->emit (cursor (256 B) | lo | hi | mask, dcap records each) and leaves
// there the distinct k-mers of one k whose mask matches a query, in the order the chunks of the sort finished, over all passes.
// `image` is staged into c->ord: its first 2 nq words are the (all, none) pairs, what the caller appended follows there.
// found = the cursor.  `slots` says whose k-mer slots dcap counts: more records than slots is DD_EHIP.  Null: dcap is the
// caller's own cap, the cursor counts on past it, and then no record was kept whole: the count is the answer.
// kept: 0 < found <= dcap, and c->exact -- free after the last pass, grown if a multi-pass call found more than a pass holds --
// has room for order(): ascending (hi, lo), launched by the caller inside its timing span, in front of the kernel that reads
// the set.  `what` names the entry in the messages.
struct ExactSlotsOf { const char *of, *have; };
constexpr ExactSlotsOf kSlotsOfInputs{"inputs", "inputs have"}, kSlotsOfUniverse{"universe", "universe has"};
struct ExactRecords {
    dd::ExactEmit e{};
    unsigned long long found = 0;
    bool kept = false;
    hipError_t order(dd_ctx* c, int k, dd::LocateSet* set) const {
        return dd::launch_exact_emit_order(e.lo, e.hi, e.mask, (size_t)found, k, c->exact.p, c->stream, set);
    }
};
int exact_records(dd_ctx* c, const ExactInputs& in, int n, int k, const char* what, const ExactSlotsOf* slots, int nq, const void* image,
                  size_t image_bytes, size_t dcap, ExactRecords& r);

// Host-only sanitizer build of the record index (dd_io.h: index_records, fasta_index_file, and fastq_to_fasta with names):
// hand-made buffers whose tables are written out here, every buffer again at every truncation (a header, a '\r', a '+' line
// or a quality text cut by the end of the buffer) in a heap block of exactly its size, and files through the loaders, plain
// and gzip.  No device code is compiled and no HIP call is made; built and run by tests/test_sanitize_index.py with
// g++ -x c++ under AddressSanitizer + UBSan.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include <string>
#include <vector>

#include "dd_io.h"

static int failures = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            ++failures;                       \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);     \
            fprintf(stderr, "\n");            \
        }                                     \
    } while (0)

struct Want {
    std::vector<std::string> names;
    std::vector<uint64_t> len, start;
    uint64_t ntok;
};

// the index of text[0..n) in a heap block of exactly n bytes (FASTQ: n + 16, what normalize_records asks for)
static dd::FastaIndex index_exact(const char* text, size_t n) {
    dd::FastaIndex ix;
    const bool fastq = dd::has_plus_line(reinterpret_cast<const uint8_t*>(text), n);
    uint8_t* p = static_cast<uint8_t*>(malloc(n + (fastq ? 16 : 0) + (n ? 0 : 1)));
    memcpy(p, text, n);
    std::vector<std::string> names;
    size_t m = n;
    if (fastq) m = dd::fastq_to_fasta(p, n, p, &names);
    dd::index_records(p, m, ix, fastq ? &names : nullptr);
    free(p);
    return ix;
}

static void check_table(const char* what, const dd::FastaIndex& ix, const Want& w) {
    CHECK(ix.names == w.names, "%s: names", what);
    CHECK(ix.seq_len == w.len, "%s: lengths", what);
    CHECK(ix.tok_start == w.start, "%s: starts", what);
    CHECK(ix.ntok == w.ntok, "%s: ntok %llu, %llu expected", what, (unsigned long long)ix.ntok, (unsigned long long)w.ntok);
}

// what every index must satisfy, whatever the text
static void check_shape(const char* what, size_t cut, const dd::FastaIndex& ix) {
    const size_t r = ix.seq_len.size();
    CHECK(ix.names.size() == r && ix.tok_start.size() == r, "%s cut %zu: ragged", what, cut);
    uint64_t at = 0;
    for (size_t i = 0; i < r; ++i) {
        CHECK(ix.tok_start[i] == at + 1, "%s cut %zu: record %zu starts at %llu", what, cut, i, (unsigned long long)ix.tok_start[i]);
        at += 1 + ix.seq_len[i];
    }
    CHECK(ix.ntok == at, "%s cut %zu: ntok", what, cut);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    const char* fa = "junk\n>r1 first\nACGTNNAC\r\nacgt\r\n>e\n>r3\tx\nAC>GT\nTTTT\n>cut";
    check_table("fasta", index_exact(fa, strlen(fa)), Want{{"r1", "e", "r3", "cut"}, {12, 0, 9, 0}, {1, 14, 15, 25}, 25});
    const char* fq = "@q1 x\nACGT\n+\nIIII\n@q2\nGGN\n+q2\nIII\n@q3\nAC\n+\nI";
    check_table("fastq", index_exact(fq, strlen(fq)), Want{{"q1", "q2"}, {4, 3}, {1, 6}, 9});
    check_table("empty", index_exact("", 0), Want{{}, {}, {}, 0});
    check_table("no header", index_exact("ACGT\nACGT\n", 10), Want{{}, {}, {}, 0});
    check_table("bare", index_exact(">", 1), Want{{""}, {0}, {1}, 1});
    check_table("cr at end", index_exact(">a\nAC\r", 6), Want{{"a"}, {2}, {1}, 3});
    for (const char* text : {fa, fq, ">a b\r\nAC\rGT\r\n\r\n>\n\n@x\n+\n\n", "@a\nACGT\n+\nII\nII\n@b\nA\n+\n"})
        for (size_t cut = 0; cut <= strlen(text); ++cut) check_shape(text == fa ? "fasta" : "text", cut, index_exact(text, cut));
    // through the loaders: plain and gzip, many records
    std::string many;
    Want w;
    uint64_t at = 0;
    for (int i = 0; i < 5000; ++i) {
        const std::string name = "rec" + std::to_string(i);
        const size_t len = (size_t)(i * 37 % 211);
        many += ">" + name + " comment\n";
        for (size_t j = 0; j < len; ++j) {
            many += "ACGTN"[(i + j * 7) % 5];
            if (j % 60 == 59) many += '\n';
        }
        many += '\n';
        w.names.push_back(name), w.len.push_back(len), w.start.push_back(at + 1);
        at += 1 + len;
    }
    w.ntok = at;
    const std::string plain = dir + "/many.fa", gz = dir + "/many.fa.gz";
    FILE* f = fopen(plain.c_str(), "wb");
    if (!f || fwrite(many.data(), 1, many.size(), f) != many.size()) return 3;
    fclose(f);
    gzFile g = gzopen(gz.c_str(), "wb");
    if (!g || gzwrite(g, many.data(), (unsigned)many.size()) != (int)many.size()) return 3;
    gzclose(g);
    for (const std::string& path : {plain, gz})
        for (int par : {1, 4}) {
            dd::FastaIndex ix;
            std::string err;
            CHECK(dd::fasta_index_file(path.c_str(), ix, err, par), "%s: %s", path.c_str(), err.c_str());
            check_table(path.c_str(), ix, w);
        }
    dd::FastaIndex ix;
    std::string err;
    CHECK(!dd::fasta_index_file((dir + "/nowhere.fa").c_str(), ix, err, 1) && !err.empty(), "a missing file must be an error");
    if (failures) return 1;
    printf("sanitize_index: ok\n");
    return 0;
}

// inflate_conformance.cpp -- the host's piece decoder (dandd_amd/csrc/dd_inflate.h) against zlib's verdict on crafted deflate
// streams, as a stand-alone program (tests/test_inflate_conformance.py writes the cases of tests/deflate_craft.py as data files,
// builds this under AddressSanitizer + UBSan where that links, runs it and reads its report).
//     inflate_conformance DIR
// DIR/manifest: one line per case -- name, valid (1 / 0), bits of deflate data, number of block starts, then bit:textpos of each;
// DIR/<name>.deflate and DIR/<name>.text: the raw deflate data and the text zlib reads out of it (the intended text where zlib
// refuses the data); DIR/member.gz and DIR/member.text: one gzip member of several hundred KB for gunzip_member_parallel.
// Three checks, none of which takes "not applicable" for an answer:
//   whole     decode_piece(known_start = true) gives 0 and exactly the text (every symbol below 256, the final block seen, the
//             reader standing at the data's last bit) for a valid case, -1 for an invalid one
//   pieces    from every block start behind the first of a valid case, decode_piece(known_start = false): a symbol below 256 is
//             the text's byte, a placeholder 256 + w names the byte at w of the 32 KiB in front of the piece -- which must exist
//             and be the text's byte
//   member    gunzip_member_parallel returns 1 (not 0) with the text
// Prints one line per failure, the placeholder range met, and "inflate_conformance: ok" when there was none.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "dd_inflate.h"

static int g_fail = 0, g_checks = 0;
#define FAIL(...)                      \
    do {                               \
        ++g_fail;                      \
        printf("FAIL " __VA_ARGS__);   \
        printf("\n");                  \
    } while (0)

static bool slurp(const std::string& path, std::vector<uint8_t>& out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    out.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    return true;
}

struct TestBuf {   // the part of FileBuf the decoders use
    uint8_t* p = nullptr;
    size_t len = 0, cap = 0;
    ~TestBuf() { free(p); }
    bool reserve(size_t n) {
        if (n <= cap) return true;
        uint8_t* q = static_cast<uint8_t*>(realloc(p, n));
        if (!q) return false;
        p = q;
        cap = n;
        return true;
    }
};

int main(int argc, char** argv) {
    using namespace dd::inflate_detail;
    if (argc != 2) {
        fprintf(stderr, "usage: inflate_conformance DIR\n");
        return 2;
    }
    const std::string dir = argv[1];
    std::ifstream manifest(dir + "/manifest");
    if (!manifest) {
        fprintf(stderr, "no manifest in %s\n", dir.c_str());
        return 2;
    }
    int ncases = 0, npieces = 0;
    long w_min = 1 << 20, w_max = -1;
    size_t placeholders = 0;
    std::string line;
    SymBuf sym;
    while (std::getline(manifest, line)) {
        std::istringstream ls(line);
        std::string name;
        int valid = 0;
        uint64_t bits = 0;
        size_t nstarts = 0;
        ls >> name >> valid >> bits >> nstarts;
        std::vector<std::pair<uint64_t, size_t>> starts(nstarts);
        for (auto& s : starts) {
            char colon;
            ls >> s.first >> colon >> s.second;
        }
        std::vector<uint8_t> data, text;
        if (!ls || !slurp(dir + "/" + name + ".deflate", data) || !slurp(dir + "/" + name + ".text", text)) {
            FAIL("%s: unreadable case", name.c_str());
            continue;
        }
        ++ncases;
        // ---- whole streams
        {
            PieceResult res;
            const int rc = decode_piece(data.data(), data.size(), 0, 0, true, 0, &sym, &res);
            ++g_checks;
            if (!valid) {
                if (rc != -1) FAIL("%s: whole: zlib refuses the data, decode_piece returns %d with %zu symbols", name.c_str(), rc, sym.len);
            } else if (rc != 0) {
                FAIL("%s: whole: decode_piece returns %d (%zu symbols of %zu)", name.c_str(), rc, sym.len, text.size());
            } else {
                size_t bad = 0, first = 0;
                for (size_t i = 0; i < sym.len && i < text.size(); ++i)
                    if (sym.p[i] != text[i] && !bad++) first = i;
                if (sym.len != text.size() || bad)
                    FAIL("%s: whole: %zu symbols for %zu bytes of text, %zu of them wrong (first at %zu)", name.c_str(), sym.len, text.size(), bad, first);
                if (!res.final_seen || res.end_bit != bits)
                    FAIL("%s: whole: final block %s, reader at bit %llu of %llu", name.c_str(), res.final_seen ? "seen" : "not seen",
                         (unsigned long long)res.end_bit, (unsigned long long)bits);
            }
        }
        // ---- pieces without their history
        if (valid && nstarts >= 2) {
            for (size_t k = 1; k < nstarts; ++k) {
                const uint64_t bit = starts[k].first;
                const size_t at = starts[k].second;
                PieceResult res;
                const int rc = decode_piece(data.data(), data.size(), bit, 0, false, 0, &sym, &res);
                ++g_checks;
                ++npieces;
                if (rc != 0) {
                    FAIL("%s: piece from block %zu (bit %llu): decode_piece returns %d", name.c_str(), k, (unsigned long long)bit, rc);
                    continue;
                }
                if (sym.len != text.size() - at || !res.final_seen || res.end_bit != bits) {
                    FAIL("%s: piece from block %zu: %zu symbols for %zu bytes, reader at bit %llu of %llu", name.c_str(), k, sym.len, text.size() - at,
                         (unsigned long long)res.end_bit, (unsigned long long)bits);
                    continue;
                }
                size_t bad = 0, first = 0;
                for (size_t i = 0; i < sym.len; ++i) {
                    const uint16_t v = sym.p[i];
                    bool ok;
                    if (v < 256) ok = v == text[at + i];
                    else {
                        const long w = (long)v - 256, src = (long)at - 32768 + w;
                        ok = w < 32768 && src >= 0 && text[(size_t)src] == text[at + i];
                        ++placeholders;
                        if (w < w_min) w_min = w;
                        if (w > w_max) w_max = w;
                    }
                    if (!ok && !bad++) first = i;
                }
                if (bad) FAIL("%s: piece from block %zu: %zu symbols wrong (first at %zu of the piece: %u)", name.c_str(), k, bad, first, (unsigned)sym.p[first]);
            }
        }
    }
    printf("cases %d pieces %d checks %d placeholders %zu w_min %ld w_max %ld\n", ncases, npieces, g_checks, placeholders, w_min, w_max);
    // ---- a whole member through gunzip_member_parallel
    {
        std::vector<uint8_t> gz, text;
        if (!slurp(dir + "/member.gz", gz) || !slurp(dir + "/member.text", text)) FAIL("member: unreadable");
        else {
            for (int threads : {2, 4}) {
                TestBuf out;
                const int rc = dd::gunzip_member_parallel(gz.data(), gz.size(), out, threads, (size_t)16 << 10);
                ++g_checks;
                if (rc != 1) FAIL("member: gunzip_member_parallel with %d threads returns %d, not 1", threads, rc);
                else if (out.len != text.size() || memcmp(out.p, text.data(), text.size()) != 0)
                    FAIL("member: %d threads: %zu bytes that are not the text (%zu)", threads, out.len, text.size());
                else printf("member %zu -> %zu bytes, %d threads: 1\n", gz.size(), out.len, threads);
            }
        }
    }
    if (g_fail) {
        printf("inflate_conformance: %d FAILURES in %d checks\n", g_fail, g_checks);
        return 1;
    }
    printf("inflate_conformance: ok (%d checks)\n", g_checks);
    return 0;
}

// Stand-alone driver for the host-only pieces of gk_minimizers (genome-kmers_amd/csrc/gkm_minimizer_host.h):
// the order hash, the canonical key, the local selection rule over an array of ords and the two-sided
// chunk arithmetic, built with -fsanitize=address,undefined by tests/test_minimizer_host.py.  With a file
// of cases as its argument (written by the test from tests/minimizerref.py) it selects every case's
// minimizers chunk by chunk, each chunk seeing only the bytes it carries, and compares positions, keys
// and strands with the file's.  Every buffer is heap-allocated at its exact size so that a read or
// write past an end is caught.  Prints "ok" and exits 0 when every check holds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "gkm_minimizer_host.h"

using namespace gkm::minimizer;

static int g_fail = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "line %d: %s failed\n", __LINE__, #cond); \
            ++g_fail;                                                      \
        }                                                                  \
    } while (0)

// every position owned exactly once; every owned position has its full halo or reaches the batch edge
static void check_chunks(uint64_t total, uint64_t step, uint32_t k, uint32_t w) {
    std::vector<int> owned(total, 0);
    const uint64_t n = chunk_count(total, step);
    uint64_t next = 0;
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t own_lo, own_n, held_lo, held_n;
        chunk_range(total, step, k, w, i, &own_lo, &own_n, &held_lo, &held_n);
        CHECK(own_lo == next && own_n >= 1 && (i + 1 == n || own_n == step));
        CHECK(held_lo <= own_lo && held_lo + held_n >= own_lo + own_n && held_lo + held_n <= total);
        CHECK(held_n <= chunk_bytes_max(total, step, k, w));
        CHECK(held_lo == 0 || held_lo + (w - 1) == own_lo);
        CHECK(held_lo + held_n == total || held_lo + held_n == own_lo + own_n + (w - 1) + (k - 1));
        for (uint64_t p = own_lo; p < own_lo + own_n; ++p) ++owned[p];
        next = own_lo + own_n;
    }
    CHECK(next == total);
    for (uint64_t p = 0; p < total; ++p) CHECK(owned[p] == 1);
}

struct Case {
    uint32_t k, w, flags;
    std::vector<uint64_t> offsets;
    std::string bytes;
    std::vector<uint64_t> pos, key;
    std::vector<uint32_t> strand;
};

// one chunk as the kernel sees one tile: codes of the owned positions and both halos from the bytes
// the chunk carries, sequence starts from the offsets, rolled keys, ords and flags, the local rule
static void select_chunk(const Case &c, uint64_t total, uint64_t step, uint64_t ci, std::vector<uint64_t> *pos,
                         std::vector<uint64_t> *key, std::vector<uint32_t> *strand) {
    uint64_t own_lo, own_n, held_lo, held_n;
    chunk_range(total, step, c.k, c.w, ci, &own_lo, &own_n, &held_lo, &held_n);
    std::vector<uint8_t> held(c.bytes.begin() + held_lo, c.bytes.begin() + held_lo + held_n);  // exact size
    const int k = (int)c.k, w = (int)c.w;
    const int64_t e_lo = (int64_t)own_lo - (w - 1);
    const int E = (int)own_n + 2 * (w - 1), ncodes = E + k - 1;
    std::vector<uint8_t> code(ncodes), flag(E);
    std::vector<uint64_t> ord(E), ckeys(E);
    for (int i = 0; i < ncodes; ++i) {
        const int64_t p = e_lo + i;
        uint8_t v = 4;
        if (p >= (int64_t)held_lo && (uint64_t)p < held_lo + held_n) {
            const uint8_t b = held[p - held_lo];
            v = b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : 4;
            CHECK(v == 4 || v == gkm::canon_code<2>(b, nullptr));
        }
        code[i] = v;
    }
    for (size_t j = 1; j + 1 < c.offsets.size(); ++j) {
        const int64_t i = (int64_t)c.offsets[j] - e_lo;
        if (i > 0 && i < ncodes && c.offsets[j] < total) code[i] |= 8;
    }
    const uint64_t mask = k >= 32 ? ~0ull : (1ull << (2 * k)) - 1;
    uint64_t kk = 0, rc = 0;
    int clean = 0;
    for (int i = 0; i < ncodes; ++i) {
        const uint32_t cd = code[i];
        kk = ((kk << 2) | (cd & 3)) & mask;
        rc = (rc >> 2) | ((uint64_t)(3 - (cd & 3)) << (2 * (k - 1)));
        clean = (cd & 4) ? 0 : (cd & 8) ? 1 : clean + 1;
        const int e = i - (k - 1);  // the k-mer that ends at code i starts at ord e
        if (e < 0) continue;
        if (clean >= k) CHECK(rc == revcomp_key(kk, k));
        uint32_t s;
        ckeys[e] = canonical_key(kk, rc, (c.flags & kFlagCanonical) != 0, &s);
        ord[e] = ord_of(ckeys[e], (c.flags & kFlagLex) != 0);
        flag[e] = (uint8_t)((clean >= k ? kValid : 0) | (s ? kStrand : 0) | ((code[e] & 8) ? kSeqStart : 0));
    }
    for (int li = 0; li < (int)own_n; ++li) {
        const int e = li + (w - 1);
        if (!selected(ord.data(), flag.data(), e, E, w)) continue;
        pos->push_back(own_lo + li);
        key->push_back(ckeys[e]);
        strand->push_back((flag[e] & kStrand) ? 1 : 0);
    }
}

static void run_cases(const char *path) {
    std::ifstream in(path);
    size_t ncases = 0;
    in >> ncases;
    CHECK(in.good() && ncases > 0);
    for (size_t t = 0; t < ncases; ++t) {
        Case c;
        size_t nseq = 0, nsel = 0;
        in >> c.k >> c.w >> c.flags >> nseq >> nsel;
        c.offsets.resize(nseq + 1);
        for (auto &o : c.offsets) in >> o;
        in >> c.bytes;
        if (c.bytes == "-") c.bytes.clear();
        c.pos.resize(nsel), c.key.resize(nsel), c.strand.resize(nsel);
        for (auto &v : c.pos) in >> v;
        for (auto &v : c.key) in >> v;
        for (auto &v : c.strand) in >> v;
        CHECK(!in.fail() && c.bytes.size() == c.offsets.back());
        if (in.fail()) return;
        const uint64_t total = c.bytes.size();
        const uint64_t steps[] = {1, 2, 7, (uint64_t)c.w, (uint64_t)c.w + c.k, 97, 1024, total + 1};
        for (uint64_t step : steps) {
            std::vector<uint64_t> pos, key;
            std::vector<uint32_t> strand;
            for (uint64_t ci = 0; ci < chunk_count(total, step); ++ci) select_chunk(c, total, step, ci, &pos, &key, &strand);
            CHECK(pos == c.pos);
            CHECK(key == c.key);
            CHECK(strand == c.strand);
        }
    }
}

int main(int argc, char **argv) {
    // the order hash on fixed inputs (the values: tests/test_minimizerref.py computes them with big integers)
    CHECK(fmix64(0) == 0 && mix(0) == fmix64(0x9E3779B97F4A7C15ull) && mix(0) != 0);
    CHECK(mix(0x9E3779B97F4A7C15ull) == 0);
    CHECK(mix(0) == 0x9ca066f1a4ab2eeaull && mix(1) == 0x25b775faeca8f520ull && mix(~0ull) == 0x3cd617bbbcc39640ull);
    // reverse complement of right-aligned 2-bit keys against the symbol loop
    for (int k = 1; k <= 32; ++k) {
        uint64_t x = 0x0123456789ABCDEFull * (uint64_t)(2 * k + 1);
        if (k < 32) x &= (1ull << (2 * k)) - 1;
        uint64_t r = 0, y = x;
        for (int t = 0; t < k; ++t) {
            r = (r << 2) | (3 - (y & 3));
            y >>= 2;
        }
        CHECK(revcomp_key(x, k) == r && revcomp_key(r, k) == x);
    }
    CHECK(revcomp_key(~0ull, 32) == 0 && revcomp_key(0, 32) == ~0ull && revcomp_key(0, 1) == 3);
    {
        uint32_t s = 9;
        CHECK(canonical_key(5, 3, true, &s) == 3 && s == 1);
        CHECK(canonical_key(5, 3, false, &s) == 5 && s == 0);
        CHECK(canonical_key(3, 3, true, &s) == 3 && s == 0);  // its own reverse complement: strand 0
        CHECK(ord_of(7, true) == 7 && ord_of(7, false) == mix(7));
    }
    // the chunk knob: lowers the default, never raises it, any value from 1 on
    CHECK(chunk_positions(nullptr) == kChunkPositions && chunk_positions("") == kChunkPositions &&
          chunk_positions("0") == kChunkPositions && chunk_positions("abc") == kChunkPositions &&
          chunk_positions("-3") == kChunkPositions && chunk_positions("99999999999") == kChunkPositions);
    CHECK(chunk_positions("1") == 1 && chunk_positions("1500") == 1500);
    CHECK(chunk_count(0, 5) == 0 && chunk_count(5, 5) == 1 && chunk_count(6, 5) == 2);
    {
        const uint64_t totals[] = {1, 2, 31, 257, 1000, 3001};
        const uint64_t steps[] = {1, 2, 3, 64, 255, 256, 999, 1000, 5000};
        const uint32_t ks[] = {1, 2, 31, 32}, ws[] = {1, 2, 10, 256};
        for (uint64_t total : totals)
            for (uint64_t step : steps)
                for (uint32_t k : ks)
                    for (uint32_t w : ws) check_chunks(total, step, k, w);
    }
    // the local rule on a hand-made array: ords 5 3 3 7 | 1 (a sequence starts at the last), w = 2
    {
        std::vector<uint64_t> ord = {5, 3, 3, 7, 1};
        std::vector<uint8_t> flag = {kValid, kValid, kValid, kValid, (uint8_t)(kValid | kSeqStart)};
        const bool want[] = {false, true, true, false, false};  // windows (5,3) (3,3) (3,7): the tie goes left
        for (int i = 0; i < 5; ++i) CHECK(selected(ord.data(), flag.data(), i, 5, 2) == want[i]);
        for (int i = 0; i < 5; ++i) CHECK(selected(ord.data(), flag.data(), i, 5, 1));
        flag[2] = 0;  // an invalid start in the middle: runs of 2 and 1, then the lone one of the next sequence
        const bool want2[] = {false, true, false, false, false};
        for (int i = 0; i < 5; ++i) CHECK(selected(ord.data(), flag.data(), i, 5, 2) == want2[i]);
    }
    if (argc > 1) run_cases(argv[1]);
    if (g_fail) return 1;
    std::puts("ok");
    return 0;
}

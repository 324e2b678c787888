// records_sanitize.cpp -- the HIP-free builder of the min-sum family's check records (csrc/tile_plan.hpp: ms_records,
// ms_record_words, kMsPosEdge) under AddressSanitizer + UBSan on the CPU: the empty graph, graphs without checks or
// without bits, checks of degree 0, 1, 32, 33, 64 and 65 side by side, and random graphs; every rec_off, edge_rec and
// edge_pos and the word count against a plain restatement.  Built and run by tests/test_tile_plan_cpu.py:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I ldpcdecoders.jl_amd/csrc ...
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "tile_plan.hpp"

using namespace ldpc;

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) {                                                               \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            return false;                                                         \
        }                                                                         \
    } while (0)

// A graph as the bits of every check (ascending).  The arrays ms_records() reads are built here in the layout of
// ldpc_detail::TannerGraph: CSR row pointers, and per CSC edge (bits in order, a bit's checks ascending) its check and its
// place in the CSR order.  The vectors hand out exact-size heap blocks, so a read or write past an end is caught.
static bool one_graph(int n, const std::vector<std::vector<int>> &checks)
{
    const int64_t s = (int64_t)checks.size();
    std::vector<int> row_ptr((size_t)s + 1, 0);
    for (int64_t i = 0; i < s; ++i) row_ptr[(size_t)i + 1] = row_ptr[(size_t)i] + (int)checks[(size_t)i].size();
    const int64_t nnz = row_ptr[(size_t)s];
    std::vector<int> csc_row, csc2csr;
    for (int j = 0; j < n; ++j)
        for (int64_t i = 0; i < s; ++i) {
            const std::vector<int> &c = checks[(size_t)i];
            const auto at = std::lower_bound(c.begin(), c.end(), j);
            if (at != c.end() && *at == j) {
                csc_row.push_back((int)i);
                csc2csr.push_back(row_ptr[(size_t)i] + (int)(at - c.begin()));
            }
        }
    CHECK((int64_t)csc_row.size() == nnz);
    csc_row.shrink_to_fit();
    csc2csr.shrink_to_fit();

    const MsRecords r = ms_records(s, nnz, row_ptr.data(), csc_row.data(), csc2csr.data());

    // the restatement: records in check order, 0 / 4 / 5 / degree words; an edge names its check's record and the place of
    // its bit in the check, flagged where the check keeps a word per edge
    CHECK((int64_t)r.rec_off.size() == std::max<int64_t>(s, 1) && (int64_t)r.edge_rec.size() == nnz && (int64_t)r.edge_pos.size() == nnz);
    int64_t words = 0;
    std::vector<int64_t> off((size_t)s, 0);
    for (int64_t i = 0; i < s; ++i) {
        const int deg = (int)checks[(size_t)i].size();
        off[(size_t)i] = words;
        CHECK(r.rec_off[(size_t)i] == words);
        words += deg == 0 ? 0 : deg <= 32 ? 4 : deg <= 64 ? 5 : deg;
    }
    if (s == 0) CHECK(r.rec_off[0] == 0);
    CHECK(r.words == words);
    int64_t e = 0;
    for (int j = 0; j < n; ++j)
        for (int64_t i = 0; i < s; ++i) {
            const std::vector<int> &c = checks[(size_t)i];
            for (size_t k = 0; k < c.size(); ++k)
                if (c[k] == j) {
                    CHECK(r.edge_rec[(size_t)e] == off[(size_t)i]);
                    const int want = c.size() > 64 ? (int)((unsigned)k | 0x80000000u) : (int)k;
                    CHECK(r.edge_pos[(size_t)e] == want);
                    CHECK((r.edge_pos[(size_t)e] < 0) == (c.size() > 64) && (r.edge_pos[(size_t)e] & 0x7fffffff) == (int)k);
                    ++e;
                }
        }
    CHECK(e == nnz);
    return true;
}

static std::vector<int> first_bits(int deg, int from, int n)   // deg distinct bits, ascending, starting at `from` (cyclic)
{
    std::vector<int> c;
    for (int k = 0; k < deg; ++k) c.push_back((from + k) % n);
    std::sort(c.begin(), c.end());
    return c;
}

int main()
{
    int graphs = 0;
    auto run = [&](int n, const std::vector<std::vector<int>> &checks) { ++graphs; return one_graph(n, checks); };
    if (!run(0, {})) return 1;                                   // the empty graph
    if (!run(5, {})) return 2;                                   // s = 0 with n > 0
    if (!run(0, {{}, {}, {}})) return 3;                         // n = 0 with s > 0: empty checks only
    {   // every form of record side by side, empty checks first, between and last
        const int n = 70;
        std::vector<std::vector<int>> checks;
        int from = 0;
        for (int deg : {0, 1, 32, 0, 33, 64, 65, 2, 70, 0}) {
            checks.push_back(first_bits(deg, from, n));
            from += 7;
        }
        if (!run(n, checks)) return 4;
    }
    std::mt19937 rng(20240607u);
    for (int g = 0; g < 24; ++g) {
        const int n = 1 + (int)(rng() % 90), s = (int)(rng() % 12);
        std::vector<std::vector<int>> checks;
        for (int i = 0; i < s; ++i) {
            std::vector<int> c;
            const unsigned keep = rng() % 100;   // a check takes each bit with this chance in a hundred: degrees from 0 to beyond 64
            for (int j = 0; j < n; ++j)
                if (rng() % 100 < keep) c.push_back(j);
            checks.push_back(c);
        }
        if (!run(n, checks)) return 5;
    }
    std::printf("OK %d record sets\n", graphs);
    return 0;
}

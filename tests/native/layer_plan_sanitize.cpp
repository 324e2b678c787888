// layer_plan_sanitize.cpp -- drives the HIP-free layer planner of the layered min-sum schedule (layer_plan.cpp) under
// AddressSanitizer and UBSan on the CPU: g++ -fsanitize=address,undefined, built and run by
// tests/test_layer_plan_cpu.py::test_layer_plan_under_sanitizers.  The graphs come from the test, in the file named by
// argv[1] -- the ones it holds the library against: per graph a line "s n nnz K", then row_ptr [s + 1], csr_col [nnz] and
// the layer of every check as the numpy model assigns it (-1: none).  Each plan is checked against that assignment, by
// layer_plan_verify and against a dense restatement of what the kernel relies on.  Then the refusals: patterns
// layer_plan_build rejects, and tampered plans layer_plan_verify must reject.  Exit code 0 and "OK ..." = nothing found.
#include "../../ldpcdecoders.jl_amd/csrc/layer_plan.hpp"

#include <cstdio>

using namespace ldpc;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return false; } } while (0)

struct Graph {
    int64_t s = 0, n = 0;
    std::vector<int32_t> row_ptr, csr_col, want;
    int K = 0;
};

static bool read_ints(std::FILE *f, size_t count, std::vector<int32_t> *out)
{
    out->assign(count, 0);
    for (size_t q = 0; q < count; ++q) {
        long v;
        if (std::fscanf(f, "%ld", &v) != 1) return false;
        (*out)[q] = (int32_t)v;
    }
    return true;
}

static bool graph_ok(const Graph &g)
{
    LayerPlan p;
    std::string why;
    CHECK(layer_plan_build(g.s, g.n, g.row_ptr.data(), g.csr_col.data(), &p, &why) == kLayerPlanOk);
    CHECK(p.K == g.K && p.layer_of == g.want);
    CHECK(layer_plan_verify(g.s, g.n, g.row_ptr.data(), g.csr_col.data(), p, &why));
    CHECK(p.layer_ptr.size() == (size_t)p.K + 1 && p.layer_ptr[0] == 0 && (size_t)p.layer_ptr[(size_t)p.K] == p.layer_checks.size());
    // dense: per layer a mark per bit; the checks ascending inside a layer; every non-empty check once
    std::vector<int> times((size_t)g.s, 0);
    for (int l = 0; l < p.K; ++l) {
        std::vector<char> mark((size_t)g.n, 0);
        CHECK(p.layer_ptr[(size_t)l] < p.layer_ptr[(size_t)l + 1]);   // first fit leaves no layer empty
        for (int32_t q = p.layer_ptr[(size_t)l]; q < p.layer_ptr[(size_t)l + 1]; ++q) {
            const int32_t i = p.layer_checks[(size_t)q];
            CHECK(i >= 0 && i < g.s && p.layer_of[(size_t)i] == l);
            CHECK(q == p.layer_ptr[(size_t)l] || i > p.layer_checks[(size_t)q - 1]);
            ++times[(size_t)i];
            for (int32_t e = g.row_ptr[(size_t)i]; e < g.row_ptr[(size_t)i + 1]; ++e) {
                CHECK(!mark[(size_t)g.csr_col[(size_t)e]]);
                mark[(size_t)g.csr_col[(size_t)e]] = 1;
            }
        }
    }
    for (int64_t i = 0; i < g.s; ++i) CHECK(times[(size_t)i] == (g.row_ptr[(size_t)i] < g.row_ptr[(size_t)i + 1] ? 1 : 0));
    // ... and first fit: a check shares a bit with some check before it in every lower layer
    for (int64_t i = 0; i < g.s; ++i)
        for (int l = 0; l < p.layer_of[(size_t)i]; ++l) {
            bool meets = false;
            for (int32_t q = p.layer_ptr[(size_t)l]; q < p.layer_ptr[(size_t)l + 1] && !meets; ++q) {
                const int32_t o = p.layer_checks[(size_t)q];
                if (o >= i) break;
                for (int32_t e = g.row_ptr[(size_t)i]; e < g.row_ptr[(size_t)i + 1] && !meets; ++e)
                    for (int32_t f = g.row_ptr[(size_t)o]; f < g.row_ptr[(size_t)o + 1]; ++f)
                        if (g.csr_col[(size_t)e] == g.csr_col[(size_t)f]) { meets = true; break; }
            }
            CHECK(meets);
        }
    return true;
}

static bool refused(int64_t s, int64_t n, const int32_t *row_ptr, const int32_t *csr_col, LayerPlanStatus status, const char *needle)
{
    LayerPlan p;
    p.K = 7;
    std::string why;
    CHECK(layer_plan_build(s, n, row_ptr, csr_col, &p, &why) == status);
    CHECK(p.K == 0 && p.layer_ptr.empty() && p.layer_checks.empty() && p.layer_of.empty());
    if (why.find(needle) == std::string::npos) {
        std::printf("FAILED: message \"%s\" does not hold \"%s\"\n", why.c_str(), needle);
        return false;
    }
    return true;
}

static bool refusals()
{
    // three checks over four bits: {0, 1}, {1, 2}, {3}: layers 0, 1, 0
    const std::vector<int32_t> row_ptr{0, 2, 4, 5}, col{0, 1, 1, 2, 3};
    LayerPlan good;
    std::string why;
    CHECK(layer_plan_build(3, 4, row_ptr.data(), col.data(), &good, &why) == kLayerPlanOk);
    CHECK(good.K == 2 && good.layer_of == std::vector<int32_t>({0, 1, 0}) && good.layer_checks == std::vector<int32_t>({0, 2, 1}));
    CHECK(layer_plan_verify(3, 4, row_ptr.data(), col.data(), good, &why));
    CHECK(refused(-1, 4, row_ptr.data(), col.data(), kLayerPlanInvalid, "negative"));
    CHECK(refused(3, -4, row_ptr.data(), col.data(), kLayerPlanInvalid, "negative"));
    CHECK(refused(3, 4, nullptr, col.data(), kLayerPlanInvalid, "row_ptr is NULL"));
    CHECK(refused(3, 4, row_ptr.data(), nullptr, kLayerPlanInvalid, "csr_col is NULL"));
    CHECK(refused((int64_t)1 << 28, 4, row_ptr.data(), col.data(), kLayerPlanTooLarge, "too large"));
    CHECK(refused(3, (int64_t)1 << 28, row_ptr.data(), col.data(), kLayerPlanTooLarge, "too large"));
    std::vector<int32_t> bad_ptr{1, 2, 4, 5};
    CHECK(refused(3, 4, bad_ptr.data(), col.data(), kLayerPlanInvalid, "row_ptr[0]"));
    bad_ptr = {0, 4, 2, 5};
    CHECK(refused(3, 4, bad_ptr.data(), col.data(), kLayerPlanInvalid, "row_ptr[2] is below"));
    std::vector<int32_t> bad_col{0, 1, 1, 4, 3};
    CHECK(refused(3, 4, row_ptr.data(), bad_col.data(), kLayerPlanInvalid, "csr_col[3]"));
    bad_col = {0, 1, -1, 2, 3};
    CHECK(refused(3, 4, row_ptr.data(), bad_col.data(), kLayerPlanInvalid, "csr_col[2]"));
    // what the verification is for: plans that would race on the device
    LayerPlan p = good;
    p.layer_checks = {0, 1, 2};                      // checks 0 and 1 in layer 0: they meet in bit 1
    p.layer_of = {0, 0, 1};
    CHECK(!layer_plan_verify(3, 4, row_ptr.data(), col.data(), p, &why) && why.find("meet in bit 1") != std::string::npos);
    p = good;
    p.layer_checks = {0, 0, 1};                      // check 0 twice, check 2 never
    CHECK(!layer_plan_verify(3, 4, row_ptr.data(), col.data(), p, &why));
    p = good;
    p.layer_checks = {0, 3, 1};                      // out of range
    CHECK(!layer_plan_verify(3, 4, row_ptr.data(), col.data(), p, &why));
    p = good;
    p.layer_ptr = {0, 1, 2};                         // check 1 dropped from the lists
    p.layer_checks = {0, 1};
    CHECK(!layer_plan_verify(3, 4, row_ptr.data(), col.data(), p, &why));
    p = good;
    p.layer_ptr = {0, 2};                            // sizes that do not fit K
    CHECK(!layer_plan_verify(3, 4, row_ptr.data(), col.data(), p, &why));
    p = good;
    p.layer_ptr = {0, 3, 2};                         // a ptr array that falls
    CHECK(!layer_plan_verify(3, 4, row_ptr.data(), col.data(), p, &why));
    p = good;
    p.layer_of = {0, 1};
    CHECK(!layer_plan_verify(3, 4, row_ptr.data(), col.data(), p, &why));
    // an empty check listed in a layer
    const std::vector<int32_t> ptr_e{0, 2, 2}, col_e{0, 1};
    LayerPlan pe;
    CHECK(layer_plan_build(2, 2, ptr_e.data(), col_e.data(), &pe, &why) == kLayerPlanOk && pe.K == 1 && pe.layer_of == std::vector<int32_t>({0, -1}));
    pe.layer_ptr = {0, 2};
    pe.layer_checks = {0, 1};
    CHECK(!layer_plan_verify(2, 2, ptr_e.data(), col_e.data(), pe, &why));
    // a bit twice in one check (no valid pattern; create's own pattern check refuses it earlier): built, then refused
    const std::vector<int32_t> ptr_d{0, 2}, col_d{1, 1};
    LayerPlan pd;
    CHECK(layer_plan_build(1, 2, ptr_d.data(), col_d.data(), &pd, &why) == kLayerPlanOk);
    CHECK(!layer_plan_verify(1, 2, ptr_d.data(), col_d.data(), pd, &why) && why.find("meet in bit 1") != std::string::npos);
    // no checks at all, with and without bits
    const std::vector<int32_t> ptr_0{0};
    LayerPlan p0;
    CHECK(layer_plan_build(0, 0, ptr_0.data(), nullptr, &p0, &why) == kLayerPlanOk && p0.K == 0 && p0.layer_ptr == std::vector<int32_t>({0}));
    CHECK(layer_plan_verify(0, 0, ptr_0.data(), nullptr, p0, &why));
    CHECK(layer_plan_build(0, 5, ptr_0.data(), nullptr, &p0, &why) == kLayerPlanOk && p0.K == 0);
    return true;
}

int main(int argc, char **argv)
{
    if (argc < 2) {
        std::printf("usage: layer_plan_sanitize GRAPHS\n");
        return 2;
    }
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) {
        std::printf("FAILED: cannot open %s\n", argv[1]);
        return 2;
    }
    int graphs = 0;
    for (;;) {
        long s, n, nnz, K;
        if (std::fscanf(f, "%ld %ld %ld %ld", &s, &n, &nnz, &K) != 4) break;
        Graph g;
        g.s = s; g.n = n; g.K = (int)K;
        if (s < 0 || n < 0 || nnz < 0 || !read_ints(f, (size_t)s + 1, &g.row_ptr) || !read_ints(f, (size_t)nnz, &g.csr_col) || !read_ints(f, (size_t)s, &g.want)) {
            std::printf("FAILED: graph %d of %s is cut short\n", graphs, argv[1]);
            std::fclose(f);
            return 2;
        }
        if (!graph_ok(g)) {
            std::printf("FAILED: graph %d (s = %ld, n = %ld)\n", graphs, s, n);
            std::fclose(f);
            return 1;
        }
        ++graphs;
    }
    std::fclose(f);
    if (!refusals()) return 1;
    std::printf("OK %d graphs, 10 refused patterns, 9 refused plans\n", graphs);
    return 0;
}

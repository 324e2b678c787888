// window_plan_sanitize.cpp -- drives the HIP-free table builder of the sliding-window step (window_plan.cpp) under
// AddressSanitizer and UBSan on the CPU: g++ -fsanitize=address,undefined, built and run by
// tests/test_windows_cpu.py::test_window_tables_under_sanitizers.  The shapes: the phenomenological model of a 36 x 72
// check matrix of row weight 6 (the shape of BB-72 H_X) at (R, W, C) = (5, 3, 1), (6, 4, 2), (4, 4, 1) and (3, 5, 2), a
// hand-made model with shuffled detector order, a mechanism over three layers and one without a detector, an empty
// plan, and every refusal.  Each table is checked against a dense restatement of what it must say.  Exit code 0 and
// "OK ..." = nothing found.
#include "../../ldpcdecoders.jl_amd/csrc/window_plan.hpp"

#include <algorithm>
#include <cstdio>

using namespace ldpc;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return false; } } while (0)

struct Model {
    int64_t D = 0, N = 0;
    std::vector<int64_t> colptr{0}, rowval, layers;
    void column(std::vector<int64_t> rows)
    {
        std::sort(rows.begin(), rows.end());
        rowval.insert(rowval.end(), rows.begin(), rows.end());
        colptr.push_back((int64_t)rowval.size());
        ++N;
    }
};

struct Lists {
    std::vector<int64_t> det_ptr{0}, det_idx, mech_ptr{0}, mech_idx, commit_ptr{0}, commit_idx;
    int64_t K = 0;
};

// the plan rule of ldpcdecoders.jl_amd/windows.py
static Lists plan_of(const Model &m, int64_t width, int64_t commit)
{
    Lists l;
    const int64_t R = m.layers.empty() ? 0 : *std::max_element(m.layers.begin(), m.layers.end()) + 1;
    for (int64_t k = 0; R > 0; ++k) {
        const int64_t a = k * commit, b = std::min(a + width, R);
        for (int64_t d = 0; d < m.D; ++d)
            if (m.layers[(size_t)d] >= a && m.layers[(size_t)d] < b) l.det_idx.push_back(d);
        int64_t pos = 0;
        for (int64_t j = 0; j < m.N; ++j) {
            if (m.colptr[(size_t)j] == m.colptr[(size_t)j + 1]) continue;
            int64_t first = INT64_MAX;
            for (int64_t e = m.colptr[(size_t)j]; e < m.colptr[(size_t)j + 1]; ++e) first = std::min(first, m.layers[(size_t)m.rowval[(size_t)e]]);
            if (first < a || first >= b) continue;
            l.mech_idx.push_back(j);
            if (b == R || first < a + commit) l.commit_idx.push_back(pos);
            ++pos;
        }
        l.det_ptr.push_back((int64_t)l.det_idx.size());
        l.mech_ptr.push_back((int64_t)l.mech_idx.size());
        l.commit_ptr.push_back((int64_t)l.commit_idx.size());
        ++l.K;
        if (b == R) break;
    }
    return l;
}

static WindowPlanIn input_of(const Model &m, const Lists &l)
{
    WindowPlanIn in;
    in.D = m.D; in.N = m.N; in.nnz = (int64_t)m.rowval.size(); in.colptr = m.colptr.data(); in.rowval = m.rowval.data();
    in.K = l.K;
    in.det_ptr = l.det_ptr.data(); in.det_idx = l.det_idx.data(); in.mech_ptr = l.mech_ptr.data(); in.mech_idx = l.mech_idx.data();
    in.commit_ptr = l.commit_ptr.data(); in.commit_idx = l.commit_idx.data();
    return in;
}

// every table against the dense statement: entry (d, c) is in U_k's ranges iff c is committed and (d, mech_k[c]) is in H
static bool tables_ok(const Model &m, const Lists &l)
{
    WindowTables t;
    std::string why;
    CHECK(window_tables_build(input_of(m, l), &t, &why) == kWindowPlanOk);
    CHECK((int64_t)t.win.size() == l.K);
    std::vector<int> committed((size_t)m.N, 0);
    for (int64_t k = 0; k < l.K; ++k) {
        const WindowTable &w = t.win[(size_t)k];
        const int64_t d0 = l.det_ptr[(size_t)k], m0 = l.mech_ptr[(size_t)k], c0 = l.commit_ptr[(size_t)k];
        CHECK(w.ndet == l.det_ptr[(size_t)k + 1] - d0 && w.nmech == l.mech_ptr[(size_t)k + 1] - m0 && w.nc == l.commit_ptr[(size_t)k + 1] - c0);
        CHECK(w.nnext == (k + 1 < l.K ? l.det_ptr[(size_t)k + 2] - l.det_ptr[(size_t)k + 1] : 0));
        CHECK(w.u_next + (size_t)w.nu <= t.ints.size() && w.u_ptr + (size_t)w.nu + 1 <= t.ints.size());
        CHECK(t.longest >= w.nmech && t.longest >= w.nu && t.longest >= w.ndet && t.max_mech >= w.nmech);
        for (int q = 0; q < w.ndet; ++q) CHECK(t.ints[w.det + (size_t)q] == l.det_idx[(size_t)(d0 + q)]);
        std::vector<std::vector<int>> want((size_t)m.D);   // detector -> committed positions
        for (int q = 0; q < w.nc; ++q) {
            const int c = t.ints[w.c_pos + (size_t)q], j = t.ints[w.c_mech + (size_t)q];
            CHECK(c == l.commit_idx[(size_t)(c0 + q)] && j == l.mech_idx[(size_t)(m0 + c)]);
            ++committed[(size_t)j];
            for (int64_t e = m.colptr[(size_t)j]; e < m.colptr[(size_t)j + 1]; ++e) want[(size_t)m.rowval[(size_t)e]].push_back(c);
        }
        std::vector<int> place((size_t)m.D, -1);
        for (int q = 0; q < w.nnext; ++q) place[(size_t)l.det_idx[(size_t)(l.det_ptr[(size_t)k + 1] + q)]] = q;
        int seen = 0;
        CHECK(t.ints[w.u_ptr] == 0 && t.ints[w.u_ptr + (size_t)w.nu] == w.nupos);
        for (int u = 0; u < w.nu; ++u) {
            const int d = t.ints[w.u_det + (size_t)u], e0 = t.ints[w.u_ptr + (size_t)u], e1 = t.ints[w.u_ptr + (size_t)u + 1];
            CHECK(d >= 0 && d < m.D && (u == 0 || d > t.ints[w.u_det + (size_t)u - 1]));
            CHECK(e0 <= e1 && e1 <= w.nupos);
            CHECK(std::vector<int>(t.ints.begin() + (long)(w.u_pos + (size_t)e0), t.ints.begin() + (long)(w.u_pos + (size_t)e1)) == want[(size_t)d]);
            CHECK(t.ints[w.u_next + (size_t)u] == place[(size_t)d]);
            CHECK(e0 < e1 || place[(size_t)d] >= 0);
            ++seen;
        }
        int owned = 0;
        for (int64_t d = 0; d < m.D; ++d) owned += !want[(size_t)d].empty() || place[(size_t)d] >= 0;
        CHECK(seen == owned);
    }
    for (int64_t j = 0; j < m.N; ++j) CHECK(committed[(size_t)j] == (m.colptr[(size_t)j] < m.colptr[(size_t)j + 1] ? 1 : 0));
    return true;
}

// [I_R (x) H | D (x) I_s] of the circulant 36 x 72 matrix with ones at (i, (2 i + o) mod 72), o = 0, 1, 5, 30, 31, 47
static Model phenomenological(int R)
{
    const int s = 36, n = 72, offsets[6] = {0, 1, 5, 30, 31, 47};
    std::vector<std::vector<int64_t>> cols((size_t)n);
    for (int i = 0; i < s; ++i)
        for (int o : offsets) cols[(size_t)((2 * i + o) % n)].push_back(i);
    Model m;
    m.D = (int64_t)R * s;
    for (int t = 0; t < R; ++t)
        for (int i = 0; i < s; ++i) m.layers.push_back(t);
    for (int t = 0; t < R; ++t)
        for (int j = 0; j < n; ++j) {
            std::vector<int64_t> rows;
            for (int64_t i : cols[(size_t)j]) rows.push_back((int64_t)t * s + i);
            m.column(rows);
        }
    for (int t = 0; t + 1 < R; ++t)
        for (int i = 0; i < s; ++i) m.column({(int64_t)t * s + i, (int64_t)(t + 1) * s + i});
    return m;
}

static Model hand_made()
{
    Model m;
    m.D = 7;
    m.layers = {2, 0, 3, 1, 0, 2, 1};            // shuffled
    m.column({1, 4});                            // layer 0 only
    m.column({4, 3});                            // layers 0, 1
    m.column({1, 6, 0});                         // layers 0, 1, 2: three layers
    m.column({});                                // no detector
    m.column({3, 5});                            // layers 1, 2
    m.column({0, 2});                            // layers 2, 3
    m.column({2});                               // layer 3
    m.column({6, 5, 2});                         // layers 1, 2, 3
    return m;
}

static bool refused(const Model &m, Lists l, const char *needle)
{
    WindowTables t;
    std::string why;
    CHECK(window_tables_build(input_of(m, l), &t, &why) == kWindowPlanInvalid);
    CHECK(t.win.empty() && t.ints.empty());
    if (why.find(needle) == std::string::npos) {
        std::printf("FAILED: message \"%s\" does not hold \"%s\"\n", why.c_str(), needle);
        return false;
    }
    return true;
}

static bool refusals()
{
    const Model m = hand_made();
    const Lists good = plan_of(m, 3, 1);
    CHECK(good.K == 2 && tables_ok(m, good));
    Lists l = good;
    l.det_idx[(size_t)l.det_ptr[1] + 1] = m.D;                   // out of range
    CHECK(refused(m, l, "window 1: det_idx[1]"));
    l = good;
    l.mech_idx[0] = -1;
    CHECK(refused(m, l, "window 0: mech_idx[0]"));
    l = good;
    l.commit_idx[(size_t)l.commit_ptr[1]] = l.mech_ptr[2] - l.mech_ptr[1];   // a position past the window's list
    CHECK(refused(m, l, "window 1: commit_idx[0]"));
    l = good;
    std::swap(l.det_idx[0], l.det_idx[1]);                       // not ascending
    CHECK(refused(m, l, "window 0: det_idx[1]"));
    l = good;
    l.mech_idx[1] = l.mech_idx[0];                               // not distinct
    CHECK(refused(m, l, "window 0: mech_idx[1]"));
    l = good;                                                    // window 1 commits what window 0 committed
    {
        Lists twice = good;
        twice.mech_idx.assign(good.mech_idx.begin(), good.mech_idx.begin() + (long)good.mech_ptr[1]);
        twice.mech_idx.insert(twice.mech_idx.end(), good.mech_idx.begin(), good.mech_idx.begin() + (long)good.mech_ptr[1]);
        twice.mech_ptr = {0, good.mech_ptr[1], 2 * good.mech_ptr[1]};
        twice.commit_idx = {0, 0};
        twice.commit_ptr = {0, 1, 2};
        CHECK(refused(m, twice, "is committed by window 0 already"));
    }
    l.det_ptr[1] = l.det_ptr[2] + 1;                             // a ptr array that falls
    CHECK(refused(m, l, "det_ptr"));
    l = good;
    l.mech_ptr[0] = 1;
    CHECK(refused(m, l, "mech_ptr[0] must be 0"));
    WindowPlanIn in = input_of(m, good);
    in.commit_ptr = nullptr;
    WindowTables t;
    std::string why;
    CHECK(window_tables_build(in, &t, &why) == kWindowPlanInvalid && why.find("NULL") != std::string::npos);
    in = input_of(m, good);
    in.K = -1;
    CHECK(window_tables_build(in, &t, &why) == kWindowPlanInvalid);
    in = input_of(m, good);
    in.N = (int64_t)1 << 28;
    CHECK(window_tables_build(in, &t, &why) == kWindowPlanTooLarge);
    return true;
}

int main()
{
    const int shapes[4][3] = {{5, 3, 1}, {6, 4, 2}, {4, 4, 1}, {3, 5, 2}};
    const int64_t windows[4] = {3, 2, 1, 1};
    for (int q = 0; q < 4; ++q) {
        const Model m = phenomenological(shapes[q][0]);
        const Lists l = plan_of(m, shapes[q][1], shapes[q][2]);
        if (l.K != windows[q] || !tables_ok(m, l)) {
            std::printf("FAILED: phenomenological (R, W, C) = (%d, %d, %d)\n", shapes[q][0], shapes[q][1], shapes[q][2]);
            return 1;
        }
    }
    const Model h = hand_made();
    for (int w = 1; w <= 5; ++w)
        for (int c = 1; c <= w; ++c)
            if (!tables_ok(h, plan_of(h, w, c))) {
                std::printf("FAILED: hand-made model, width %d commit %d\n", w, c);
                return 1;
            }
    Model none;                                  // no detector, no mechanism, no window
    if (!tables_ok(none, plan_of(none, 3, 1)) || !refusals()) return 1;
    std::printf("OK 4 phenomenological plans, 15 hand-made plans, the empty plan, 11 refusals\n");
    return 0;
}

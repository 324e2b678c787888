// team_plan_sanitize.cpp -- the team planner and the table builders (ldpcdecoders.jl_amd/csrc/team_plan.cpp) under
// AddressSanitizer + UndefinedBehaviorSanitizer: index arithmetic over std::vector<int> with hand-computed offsets, on
// the smallest shapes that reach every branch.  CPU build only (the GPU pool offers no sanitizers); built and run by
// tests/test_team_rows_cpu.py::test_team_plan_under_sanitizers.  What the tables must SAY about the graph is that
// file's business; here only what is cheap: every call succeeds, the tables have the sizes the layout promises, the
// write-back lists name edges of the graph, the bit order is a permutation, a plan never asks for more workgroups than
// the chip hosts; the levels of the straggler hand-off (level_plan_pure()) hold what the rule says, as literals; the
// tile plans of the min-sum and relay decoders (tile_plan.hpp) stay inside the LDS budgets.  Exit code 0 and "OK ..." =
// nothing found.
#include "../../ldpcdecoders.jl_amd/csrc/team_plan.hpp"
#include "../../ldpcdecoders.jl_amd/csrc/tile_plan.hpp"

#include <algorithm>
#include <cstdio>

using namespace ldpc;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return false; } } while (0)

static uint32_t lcg_state = 12345u;
static uint32_t lcg() { lcg_state = lcg_state * 1664525u + 1013904223u; return lcg_state >> 8; }

static bool edges_ok(const std::vector<int> &v, size_t size, int nnz)
{
    CHECK(v.size() == size);
    for (int q : v) CHECK(q == -1 || (q >= 0 && q < nnz));
    return true;
}
static bool is_permutation(std::vector<int> bits)
{
    std::sort(bits.begin(), bits.end());
    for (size_t j = 0; j < bits.size(); ++j) CHECK(bits[j] == (int)j);
    return true;
}

// A (dc, dv)-regular graph of dv blocks: block b deals the bits, in an order of its own (a shuffle by the LCG), to
// the rows b n ... b n + n - 1 of the check-major message array -- dc in a row make a check, so where dc divides n
// block b's check i holds the bits at places dc i ... dc i + dc - 1 of that order (a Gallager code).
static bool regular(int n, int G, int dc, int dv, int regs, int quarters)
{
    const int nnz = n * dv, s = nnz / dc, W = LDPC_TEAM_THREADS / 64;
    CHECK(nnz % dc == 0);
    std::vector<int> c2r((size_t)nnz), order((size_t)n);
    for (int b = 0; b < dv; ++b) {
        for (int j = 0; j < n; ++j) order[(size_t)j] = j;
        for (int t = n - 1; t > 0; --t) std::swap(order[(size_t)t], order[(size_t)(lcg() % (uint32_t)(t + 1))]);
        for (int t = 0; t < n; ++t) c2r[(size_t)dv * order[(size_t)t] + b] = b * n + t;
    }
    const TeamRegPlan rp = team_reg_plan(n, s, G, regs, quarters, dv, dc);
    const TeamRowTables t = team_rows_tables(n, s, nnz, dc, dv, c2r, G, rp);
    CHECK(t.why == nullptr);
    CHECK(t.vt == team_vtab_words(dv) && t.R >= 1 && t.R <= kTeamRowsMax && rp.regs_per_wave <= kTeamRegRows);
    CHECK(t.vtab.size() == (size_t)n * t.vt && t.ctab.size() == (size_t)s * 4);
    if (!edges_ok(t.lds_edge, (size_t)G * t.R, nnz) || !edges_ok(t.reg_edge, (size_t)G * W * std::max(rp.regs_per_wave, 1), nnz)) return false;
    std::vector<int> bits((size_t)n);
    for (int p = 0; p < n; ++p) bits[(size_t)p] = t.vtab[(size_t)p * t.vt + 2 * dv] & 0x7fffffff;
    return is_permutation(bits);
}

// Random columns of degree 2 ... 6 (distinct checks), in both orders as ldpc_debug_team_irr derives them.
static bool irregular(int n, int s, int G, int dcb, int dvb)
{
    std::vector<int> col_ptr((size_t)n + 1, 0), rowval, row_ptr((size_t)s + 1, 0);
    for (int j = 0; j < n; ++j) {
        const int deg = 2 + (int)(lcg() % 5u);
        for (int k = 0; k < deg;) {
            const int i = (int)(lcg() % (uint32_t)s);
            if (std::find(rowval.begin() + col_ptr[(size_t)j], rowval.end(), i) != rowval.end()) continue;
            rowval.push_back(i); row_ptr[(size_t)i + 1]++; ++k;
        }
        col_ptr[(size_t)j + 1] = (int)rowval.size();
    }
    const int nnz = (int)rowval.size();
    for (int i = 0; i < s; ++i) row_ptr[(size_t)i + 1] += row_ptr[(size_t)i];
    std::vector<int> fill(row_ptr.begin(), row_ptr.end() - 1), edge_bit((size_t)nnz), c2r((size_t)nnz);
    for (int j = 0; j < n; ++j)
        for (int k = col_ptr[(size_t)j]; k < col_ptr[(size_t)j + 1]; ++k) { const int q = fill[(size_t)rowval[(size_t)k]]++; edge_bit[(size_t)q] = j; c2r[(size_t)k] = q; }
    const int bucket = team_irr_dc_bucket(row_ptr, s, nnz);
    CHECK(bucket == 0 || bucket == 8 || bucket == 16);
    const TeamIrrTables t = team_irr_tables(n, s, nnz, row_ptr, edge_bit, col_ptr, c2r, G, dcb, dvb);
    CHECK(t.why == nullptr && t.R >= 1 && t.R <= kTeamRowsMax && t.in_lds <= (size_t)nnz);
    CHECK(t.ctab2.size() == ((size_t)s + 1) * 2 && t.ptab.size() == ((size_t)n + 1) * 2 && t.ploc.size() == (size_t)nnz && t.posmap.size() == (size_t)n);
    if (!edges_ok(t.lds_edge, (size_t)G * t.R, nnz)) return false;
    std::vector<int> bits((size_t)n);
    for (int p = 0; p < n; ++p) bits[(size_t)p] = t.ptab[(size_t)2 * p + 1] & 0x7fffffff;
    return is_permutation(bits) && is_permutation(t.posmap);
}

// The plan for an MI355X's geometry, as ldpc_debug_team_plan sets it up (256 CUs, one team workgroup per CU).
static bool plans(int *count)
{
    for (int64_t nnz : {(int64_t)0, (int64_t)1, (int64_t)4096, (int64_t)65536, (int64_t)262144})
        for (int64_t batch : {(int64_t)0, (int64_t)1, (int64_t)64, (int64_t)193, (int64_t)65536, (int64_t)1 << 20})
            for (size_t cache : {(size_t)0, (size_t)240 << 20})
                for (int rows_dv : {0, 3, 4}) {
                    TeamPlanIn in;
                    in.nnz = nnz; in.max_iters = 50; in.cache = cache; in.rows_possible = rows_dv > 0; in.rows_dv = std::max(rows_dv, 1);
                    in.reg_rows = rows_dv > 0 ? kTeamRegRows * (LDPC_TEAM_THREADS / 64) : 0;
                    in.num_cus = 256; in.per_xcd = 32;
                    in.gcap = (int)std::min<int64_t>(32, std::max<int64_t>(1, nnz / 2048));
                    in.gcap_one = nnz / 1100 >= 32 ? 32 : in.gcap;
                    const TeamPlan pl = team_plan_pure(in, batch);
                    CHECK(pl.G >= 1 && pl.G <= kTeamMaxMembers && pl.grid >= 0 && pl.grid <= 8 * in.per_xcd);
                    ++*count;
                }
    return true;
}

// The levels of the straggler hand-off (level_plan_pure()) and the slot arithmetic of a tile launch.  The expected
// values are worked out by hand from the rule as ldpc_mi355x.hip stated it before it moved into team_plan.cpp:
//   T0 = 0 if defer_thresh < 0, max_iters < 4 or ntiles < 2, else defer_thresh or (0: automatic) defer_t0
//   level 1 holds min((ntiles T0 + 63) / 64 + 1, max(8, grid / 3)) tiles, level 2 (if defer_t1 > 0 and level 1 holds >= 8)
//   min((cap1 T1 + 63) / 64 + 1, max(4, cap1 / 4)); a forced capacity replaces both and admits level 2 at any size
//   node_take = min(node_take_max, 64 cap); teams (node_take > 0, max_iters <= 4096, geometry, gcap >= 3) from
//   team_fit(cap, rows = false), else 8 XCDs x per_xcd / 3 teams of 3; team_cap = 64 min(teams, cap) if that is > node_take
static LevelPlanIn level_in(int ntiles, size_t cache)
{
    LevelPlanIn in;
    in.ntiles = ntiles; in.max_iters = 50; in.grid_max = 768;
    in.node_ok = true; in.node_take_max = 512;
    in.team_ok = true; in.per_xcd = 32; in.gcap = 32;
    in.team.nnz = 65536; in.team.max_iters = 50; in.team.cache = cache; in.team.num_cus = 256;   // (32 MiB a slot)
    in.team.per_xcd = 32; in.team.gcap = 32; in.team.gcap_one = 32;
    return in;
}
static bool no_teams(const LevelPlan::Level &L) { return L.team_cap == 0u && L.t_G == 0 && L.t_nteams == 0 && L.t_grid == 0; }
static bool levels()
{
    LevelPlanIn in = level_in(1, 0);
    CHECK(level_plan_pure(in).nlevels == 0);
    in = level_in(100, 0); in.max_iters = 3;
    CHECK(level_plan_pure(in).nlevels == 0);
    in = level_in(100, 0); in.defer_thresh = -1;
    CHECK(level_plan_pure(in).nlevels == 0);
    {   // automatic thresholds, nothing fits the cache: 80 teams of 3
        const LevelPlan pl = level_plan_pure(level_in(100, 0));
        CHECK(pl.nlevels == 2 && pl.lv[1].thresh_in == 16 && pl.lv[2].thresh_in == 16);
        CHECK(pl.lv[1].cap_tiles == 26 && pl.lv[2].cap_tiles == 6);
        CHECK(pl.lv[1].node_take == 512u && pl.lv[2].node_take == 384u);
        for (int l = 1; l <= 2; ++l) CHECK(pl.lv[l].t_G == 3 && pl.lv[l].t_xcds == 8 && pl.lv[l].t_nteams == 80 && pl.lv[l].t_grid == 240);
        CHECK(pl.lv[1].team_cap == 1664u);   // 26 tiles
        CHECK(pl.lv[2].team_cap == 0u);      // 6 tiles = 384 syndromes: all the node kernel's
    }
    {   // the node kernel takes all a level can hold: teams planned, none needed
        in = level_in(100, 0); in.node_take_max = 100000;
        const LevelPlan pl = level_plan_pure(in);
        CHECK(pl.lv[1].node_take == 1664u && pl.lv[2].node_take == 384u && pl.lv[1].team_cap == 0u && pl.lv[2].team_cap == 0u);
    }
    {   // fewer teams than the level holds tiles: 8 x (6 / 3) = 16
        in = level_in(100, 0); in.per_xcd = 6;
        const LevelPlan pl = level_plan_pure(in);
        CHECK(pl.lv[1].t_G == 3 && pl.lv[1].t_xcds == 8 && pl.lv[1].t_nteams == 16 && pl.lv[1].t_grid == 48 && pl.lv[1].team_cap == 1024u);
        CHECK(pl.lv[2].team_cap == 0u);
    }
    {
        in = level_in(2, 0); in.grid_max = 2;
        const LevelPlan pl = level_plan_pure(in);
        CHECK(pl.nlevels == 1 && pl.lv[1].cap_tiles == 2 && pl.lv[1].thresh_in == 16 && pl.lv[1].node_take == 128u);
    }
    in = level_in(100, 0); in.defer_t1 = 0;
    CHECK(level_plan_pure(in).nlevels == 1 && level_plan_pure(in).lv[1].cap_tiles == 26);
    {
        in = level_in(100, 0); in.defer_thresh = 48;
        const LevelPlan pl = level_plan_pure(in);
        CHECK(pl.nlevels == 2 && pl.lv[1].thresh_in == 48 && pl.lv[2].thresh_in == 16 && pl.lv[1].cap_tiles == 76 && pl.lv[2].cap_tiles == 19);
    }
    {
        in = level_in(100, 0); in.lvl_cap_force = 2;
        const LevelPlan pl = level_plan_pure(in);
        CHECK(pl.nlevels == 2 && pl.lv[1].cap_tiles == 2 && pl.lv[2].cap_tiles == 2 && pl.lv[1].node_take == 128u && pl.lv[2].node_take == 128u);
    }
    for (int which = 0; which < 5; ++which) {   // no teams on a level
        in = level_in(100, (size_t)240 << 20);
        if (which == 0) in.max_iters = 4097;
        if (which == 1) in.gcap = 2;
        if (which == 2) in.node_take_max = 0;
        if (which == 3) in.node_ok = false;
        if (which == 4) in.team_ok = false;
        const LevelPlan pl = level_plan_pure(in);
        CHECK(pl.nlevels == 2 && pl.lv[1].cap_tiles == 26 && pl.lv[2].cap_tiles == 6 && no_teams(pl.lv[1]) && no_teams(pl.lv[2]));
        CHECK((pl.lv[1].node_take == 0u) == (which == 2 || which == 3));
    }
    {   // the slots fit the cache: what team_fit() says for the level's capacity, every row in the slot
        in = level_in(100, (size_t)240 << 20);
        const LevelPlan pl = level_plan_pure(in);
        for (int l = 1; l <= 2; ++l) {
            int x = 0, t = 0, g = 0;
            CHECK(team_fit(in.team, pl.lv[l].cap_tiles, false, &x, &t, &g));
            CHECK(pl.lv[l].t_G == g && pl.lv[l].t_xcds == x && pl.lv[l].t_nteams == x * t && pl.lv[l].t_grid == 8 * g * t);
        }
        CHECK(pl.lv[1].team_cap == 1664u && pl.lv[2].team_cap == 0u);
    }
    // the slot arithmetic of a tile launch: 16 waves a tile up to one tile per CU, else 8; slots by occupancy, budget, request
    CHECK(tile_waves(0, 256, 256) == 16 && tile_waves(0, 257, 256) == 8 && tile_waves(4, 1000, 256) == 4);
    const size_t slot = (size_t)6048 * 512;
    TileGeometry g = tile_geometry_pure(100 * slot, slot, 8, 3, 0, 256, 1000);
    CHECK(g.threads == 512 && g.grid == 100);
    g = tile_geometry_pure(1000 * slot, slot, 8, 3, 0, 256, 1000);
    CHECK(g.threads == 512 && g.grid == 768);
    g = tile_geometry_pure(0, slot, 16, 1, 0, 256, 1000);
    CHECK(g.threads == 1024 && g.grid == 1);
    g = tile_geometry_pure(1000 * slot, slot, 8, 3, 5, 256, 1000);
    CHECK(g.grid == 5);
    g = tile_geometry_pure(1000 * slot, slot, 16, 1, 0, 256, 3);
    CHECK(g.grid == 3);
    return true;
}

// The tier and the tile width of the min-sum and relay decoders (tile_plan.hpp) over sizes from nothing to the largest
// create accepts, every variant: a plan is tier 1 with a power of two S <= 64 inside 159 KiB or tier 2 with S = 64, and
// variant 1 is refused exactly where one syndrome does not fit.
static bool tile_plans(int *count)
{
    for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)72, (int64_t)96, (int64_t)6144, (int64_t)6480, (int64_t)13824, ((int64_t)1 << 28) - 1})
        for (int64_t s : {(int64_t)0, n / 2, n})
            for (int64_t rec : {(int64_t)0, 4 * s, ((int64_t)1 << 31) - 1})
                for (int relay = 0; relay < 2; ++relay)
                    for (int variant = 0; variant < 3; ++variant) {
                        TilePlan pl;
                        const size_t one = relay ? relay_state_bytes(s, n, rec, 1) : ms_state_bytes(s, n, rec, 1);
                        const bool ok = tile_plan(s, n, rec, relay != 0, variant, &pl);
                        CHECK(ok == !(variant == 1 && one > kTileLdsOne));
                        ++*count;
                        if (!ok) continue;
                        CHECK(pl.S == 1 << pl.shift && pl.S >= 1 && pl.S <= 64 && (pl.tier == 1 || (pl.tier == 2 && pl.S == 64)));
                        CHECK(pl.tier == 2 || pl.state_bytes <= kTileLdsOne);
                        CHECK(pl.state_bytes % 256 == 0 && pl.state_bytes >= one);
                    }
    return true;
}

int main()
{
    int nplans = 0, ntile = 0;
    const bool ok = regular(1024, 3, 8, 4, 32, 3) && regular(1008, 5, 6, 3, 0, 3) && regular(3990, 6, 7, 3, 12, 3) &&
                    regular(4000, 7, 10, 5, 20, 3) &&
                    regular(4096, 8, 8, 4, 32, 0) &&    // no static quarters: a wave's first chunk only (static = W)
                    regular(130, 32, 8, 4, 32, 3) &&    // shares smaller than 2 W, 32 members for 33 chunks (dc does not divide n: a check may straddle two blocks)
                    irregular(1000, 500, 3, 8, 4) && irregular(1000, 500, 3, 16, 16) && irregular(1000, 500, 32, 8, 4) &&
                    irregular(1000, 500, 32, 16, 16) &&
                    irregular(96, 64, 32, 8, 4) && irregular(96, 64, 32, 16, 16) &&   // 24 position chunks: members without a position
                    plans(&nplans) && levels() && tile_plans(&ntile);
    if (!ok) return 1;
    std::printf("OK 6 regular and 6 irregular table sets, %d plans, the level plans, %d tile plans\n", nplans, ntile);
    return 0;
}

// team_plan.cpp -- the team planner and the table builders declared in team_plan.hpp.
#include "team_plan.hpp"

#include <algorithm>

namespace ldpc {

// What a member is expected to keep on chip (a bit dealt to a member that owns one of its dv checks: 1 / dv of the edges
// are candidates; the LDS holds kTeamRowsMax of them, the waves' registers reg_rows more).
int team_rows_expected(const TeamPlanIn &in, int G)
{
    if (!in.rows_possible && in.irr_possible) return G == in.irr_G ? in.irr_on_chip / std::max(G, 1) : 0;
    return in.rows_possible ? (int)std::min<int64_t>(kTeamRowsMax + in.reg_rows, in.nnz / std::max(in.rows_dv, 1) / std::max(G, 1)) : 0;
}

// Persistent teams whose message slots in flight stay inside the cache budget (LDPC_TEAM_CACHE_MIB, default 240 of
// the Infinity Cache's 256 MiB): how many XCDs host teams (8, 7 or 6), how many teams each, how many members a
// team -- the combination that gives most workgroups a tile.  For the n = 16384 code (32 MiB a slot) with every row in
// the slot that is SEVEN teams of 32: with an eighth the slots fill the cache to the brim and every team is a fifth
// slower (full batch, 50 iterations, round 2: 1111 ms on 8 XCDs, 1011 ms on 7, 1158 ms on 6); with the rows a member
// keeps on chip counted off the slot (`rows`: 312 in LDS + 8 x 32 in registers) it is EIGHT (round 3: 712 ms).
// false: nothing fits, not even the second tier below.
bool team_fit(const TeamPlanIn &in, int64_t ntiles, bool rows, int *xcds, int *tpx, int *G)
{
    const int per_xcd = in.per_xcd, gcap = in.gcap;
    const size_t state = std::max<size_t>((size_t)in.nnz, 1) * kTile * sizeof(double);
    const size_t cache = in.cache;
    if (!cache) return false;
    // the combination that gives most workgroups a tile -- but among combinations within 15 % of that, the one that
    // uses most XCDs (their L2s and ports; fewer, larger teams per XCD): x runs downwards, so the first one that
    // qualifies wins.  ((3,6) n = 16380: eight teams of 23 on eight XCDs measured 7.1 TB/s, sixteen of 16 6.3)
    int64_t best = 0;
    // (not fewer than seven XCDs: n = 24576, 48 MiB slots -- six cached teams 382 ms for 16,384 syndromes x 50 iterations,
    //  eight partly cached ones 350 ms; n = 20480: seven cached 283 ms, eight 282 ms -- profiles/r03_midsize_plan.txt)
    const int x_hi = in.xcds_forced ? in.xcds_forced : 8, x_lo = in.xcds_forced ? in.xcds_forced : 7;
    for (int pass = 0; pass < 2; ++pass)
    for (int x = x_hi; x >= x_lo; --x)
        for (int t = 1; t <= per_xcd / 3; ++t) {
            if ((size_t)x * (size_t)t * (state + in.extra - (rows ? state / (size_t)std::max(in.rows_dv, 1) : 0)) > cache) break;   // (1 / dv at most can be in LDS)
            if (t > 1 && (int64_t)x * (t - 1) >= ntiles) break;            // no more teams than tiles
            const int g = std::min(t == 1 ? std::max(gcap, in.gcap_one) : gcap, per_xcd / t);
            if (g < 3) break;
            // rows that the members keep in LDS are not in the cache
            if ((size_t)x * (size_t)t * (state + in.extra - (rows ? (size_t)g * team_rows_expected(in, g) * kTile * sizeof(double) : 0)) > cache) continue;
            const int64_t w = std::min<int64_t>((int64_t)x * t, ntiles) * g;   // workgroups with a tile
            if (pass == 0) { if (w > best) best = w; }
            else if (w * 100 >= best * 85) { *xcds = x; *tpx = t; *G = g; return true; }
        }
    if (best > 0) return true;
    // Slots up to 3.3 x the budget: one team per XCD still pays -- the slots are partly cached or not at all, and a team
    // streams what is not as well as three tile-kernel workgroups per CU do, with 8 slots instead of 768 (round 3, 50
    // iterations, teams against the tile kernel: n = 40960, 80 MiB a slot: 16,384 syndromes 693 against 874 ms, 65,536
    // syndromes 2.76 against 2.94 s; n = 49152: 874 against 1071 ms, 3.51 against 3.70 s).  Beyond that (n = 65536,
    // 128 MiB a slot: 4.96 against 4.85 s) the tile kernel stays.  (profiles/r03_midsize_plan.txt)
    // (Graphs WITHOUT rows on chip of this kind -- irregular ones, degree pairs without an instantiation -- stay inside
    //  the budget: 16,384 syndromes x 50 iterations of an irregular n = 20480 graph, 8 x 35 MiB of slots: eight teams
    //  381-392 ms, the tile kernel 319-328 ms, seven teams with whole checks in LDS 319 ms; n = 32768, 8 x 56 MiB: 570 /
    //  626 ms against 518 ms -- profiles/r04_irregular.txt.  Regular graphs with rows on chip get wide teams long before
    //  this: team_wide_auto().)
    if (!in.xcds_forced && in.rows_possible && (size_t)8 * state <= cache / 10 * 33 && std::min(gcap, per_xcd) >= 3) {
        *xcds = 8; *tpx = 1; *G = std::min(gcap, per_xcd);
        return true;
    }
    return false;
}

// How many wide teams (TeamPlanIn::wide) a batch of ntiles gets by itself: as many as keep their slots -- less the rows
// their members keep on chip, plus a tile's LLR rows when wanted -- inside the cache budget, when that is fewer than the
// eight one-XCD teams the plan would otherwise build (eight or more fit: nothing to do, the C3 code) and the graph has a
// rows-on-chip instantiation (without rows on chip wide teams lose).  0 = none.
int team_wide_auto(const TeamPlanIn &in, int64_t ntiles)
{
    if (!in.cache || in.xcds_forced || in.team_max_set || !in.rows_possible || in.reg_rows <= 0 || in.per_xcd < 8) return 0;
    const size_t state = std::max<size_t>((size_t)in.nnz, 1) * kTile * sizeof(double);
    for (int T = 7; T >= 1; --T) {
        const int G = (int)std::min<int64_t>(kTeamMaxMembers, (int64_t)8 * in.per_xcd / T);
        if (in.nnz / G < in.scatter_rows) continue;                       // (a member keeps >= 512 message rows per sweep)
        const size_t on_chip = (size_t)G * (size_t)team_rows_expected(in, G) * kTile * sizeof(double);
        const size_t slot = state - std::min(on_chip, state) + in.extra;
        if ((size_t)T * slot > in.cache) continue;
        // eight one-XCD teams' slots would fit as well, or nearly (a quarter over the budget): that plan (no write-backs at
        // the barriers) stays
        const int G8 = std::min(std::max(in.gcap, in.gcap_one), in.per_xcd);
        const size_t slot8 = state - std::min((size_t)G8 * (size_t)team_rows_expected(in, G8) * kTile * sizeof(double), state) + in.extra;
        if ((size_t)8 * slot8 <= in.cache + in.cache / 4) return 0;
        return (int)std::min<int64_t>(T, ntiles);
    }
    return 0;
}

TeamPlan team_plan_pure(const TeamPlanIn &in, int64_t batch)
{
    TeamPlan pl;
    const int per_xcd = in.per_xcd, gcap = in.gcap;
    const int64_t ntiles = (batch + kTile - 1) / kTile;
    if (ntiles < 1 || per_xcd < 1) return pl;
    if ((size_t)ntiles * ((size_t)in.max_iters + 32) * sizeof(uint64_t) > ((size_t)64 << 20)) return pl;   // mismatch words per tile and iteration
    int64_t team = 1, nteams = 0;
    const int wide = in.wide > 0 ? in.wide : in.wide == 0 ? team_wide_auto(in, ntiles) : 0;
    if (wide > 0 && ntiles > in.scatter_tiles) {
        team = std::min<int64_t>(kTeamMaxMembers, (int64_t)8 * per_xcd / wide);
        nteams = std::min<int64_t>(wide, ntiles);
        pl.scatter = true;
        pl.wide = true;
    } else if (ntiles <= in.scatter_tiles && !in.team_max_set) {
        // dealt over all 8 XCDs (scatter mode of the kernel): larger teams pay -- one tile of the C3 code, 50
        // iterations: 32 members 5.4 ms, 48: 4.3 ms, 64: 3.4 ms, 128: 2.6 ms (a member still has >= 512 message rows per sweep)
        const int64_t cap = std::min<int64_t>(in.scatter_max, std::max<int64_t>(gcap, in.nnz / std::max(in.scatter_rows, 1)));
        team = std::min<int64_t>(cap, (int64_t)8 * per_xcd / ntiles);
        nteams = ntiles;
        pl.scatter = true;
    } else {
        const int64_t need = (ntiles + 7) / 8;
        const size_t state = std::max<size_t>((size_t)in.nnz, 1) * kTile * sizeof(double);
        int x = 8, t = (int)need, g = 0;
        const bool one_round = in.cache && !in.xcds_forced && (size_t)8 * (size_t)need * state <= in.cache + in.cache / 4;
        // (With the rows in LDS alone -- 15 % of a tile -- the budget is applied to whole slots: eight teams of the C3 code,
        // 8 x 27 MiB, measured 981 ms for the full batch, seven 957.  With rows in the waves' registers as well a quarter
        // of a tile is on chip and the rows on chip are taken off the slots: 8 x 24 MiB fit, and eight teams measured
        // 833 ms against 877 on seven -- round 3.)
        if (one_round || !team_fit(in, ntiles, (in.rows_possible && in.reg_rows > 0) || (in.irr_possible && in.irr_on_chip > 0), &x, &t, &g)) {
            if (!one_round && ntiles > in.num_cus) return pl;
            x = 8; t = (int)need;
            g = (int)std::min<int64_t>(gcap, (int64_t)per_xcd / t);
        }
        team = g;
        nteams = (int64_t)x * t;
        pl.xcds = x; pl.tpx = t;
    }
    if (team < 3) return pl;   // two workgroups per tile measured no better than the tile kernel's one of 16 waves
    pl.G = (int)std::min<int64_t>(team, kTeamMaxMembers);
    pl.rows = (!pl.scatter || pl.wide) && in.rows_possible && team_rows_expected(in, pl.G) >= 16;
    pl.irr = !pl.scatter && !in.rows_possible && in.irr_possible;
    pl.nteams = (int)nteams;
    pl.grid = pl.scatter ? pl.nteams * pl.G : 8 * pl.G * pl.tpx;
    return pl;
}

// Straggler hand-off in LEVELS: a tile whose active lanes have dwindled to <= T0 gives those syndromes up
// together with their message columns (bp_kernels.hpp: packed tiles of level 1); a pass over level 1 resumes
// them where they stood, densely packed again, and may itself hand its stragglers (<= T1 lanes) on to level 2,
// whose pass runs them to the end.  Nothing is decoded twice, results are those of an undisturbed run
// (the decoder is deterministic per syndrome).  Everything stays on the stream: every pass reads its syndrome
// count from device memory, grids are sized for the level's capacity and blocks past the count return at once.
// A level that is full refuses further tiles (they carry on by themselves), so capacities are a memory
// budget, not a correctness bound.
LevelPlan level_plan_pure(const LevelPlanIn &in)
{
    LevelPlan pl;
    const int T0 = (in.defer_thresh < 0 || in.max_iters < 4 || in.ntiles < 2) ? 0
                   : (in.defer_thresh ? in.defer_thresh : in.defer_t0);
    if (T0 > 0) {
        pl.lv[1].thresh_in = T0;
        const int worst1 = (int)(((int64_t)in.ntiles * T0 + kTile - 1) / kTile) + 1;
        pl.lv[1].cap_tiles = in.lvl_cap_force > 0 ? in.lvl_cap_force : std::min(worst1, std::max(8, in.grid_max / 3));
        pl.nlevels = 1;
        const int T1 = in.defer_t1;
        if (T1 > 0 && (pl.lv[1].cap_tiles >= 8 || in.lvl_cap_force > 0)) {
            pl.lv[2].thresh_in = T1;
            const int worst2 = (int)(((int64_t)pl.lv[1].cap_tiles * T1 + kTile - 1) / kTile) + 1;
            pl.lv[2].cap_tiles = in.lvl_cap_force > 0 ? in.lvl_cap_force : std::min(worst2, std::max(4, pl.lv[1].cap_tiles / 4));
            pl.nlevels = 2;
        }
    }
    for (int l = 1; l <= pl.nlevels; ++l) {
        LevelPlan::Level &L = pl.lv[l];
        // Few stragglers (the usual case): the node-parallel kernel finishes them, one workgroup per syndrome
        // straight from / into the caller's arrays, instead of a handful of tiles that each sweep the whole
        // graph with a few lanes alive.  Decided on the device: the launches of the paths not taken find the
        // level's count on the wrong side of node_take / team_cap and return at once.
        L.node_take = (in.node_ok && in.node_take_max > 0)
                          ? (unsigned)std::min<int64_t>(in.node_take_max, (int64_t)L.cap_tiles * kTile) : 0u;
        if (L.node_take && in.max_iters <= 4096 && in.team_ok && in.gcap >= 3) {
            // persistent teams inside the packed tiles, as many as keep the tiles in flight inside the cache budget
            // (team_fit()); they take whatever the level holds.  Nothing fits (LDPC_TEAM_CACHE_MIB=0, large graphs):
            // one tile per team, up to as many tiles as leave every team 3 members.
            int tiles_max, x = 8, t = 1, g = 3;
            if (team_fit(in.team, L.cap_tiles, false, &x, &t, &g)) {
                tiles_max = L.cap_tiles;
            } else {
                x = 8; t = in.per_xcd / 3; g = 3;           // (the members of surplus teams are idle: round 1's geometry in fixed form)
                tiles_max = std::min(x * t, L.cap_tiles);
            }
            L.t_G = g; L.t_xcds = x; L.t_nteams = x * t; L.t_grid = 8 * g * t;
            if ((unsigned)tiles_max * kTile > L.node_take) L.team_cap = (unsigned)tiles_max * kTile;
        }
    }
    return pl;
}

// Geometry of a tile launch: 8 waves per tile (three workgroups per CU) is the measured best
// whenever there are more tiles than CUs -- also against geometries that make every tile
// resident at once (6 waves x 4 per CU: -10 %); with at most one tile per CU, 16 waves per
// tile put more of the chip to work.  The caller may fix it.
int tile_waves(int wpt_fixed, int ntiles, int num_cus) { return wpt_fixed ? wpt_fixed : (ntiles <= num_cus ? 16 : 8); }

TileGeometry tile_geometry_pure(size_t ws_budget, size_t slot_bytes, int wpt, int blocks_per_cu, int resident_fixed, int num_cus, int ntiles)
{
    const int max_slots = (int)std::max<size_t>(std::min<size_t>(ws_budget / slot_bytes, 1u << 30), 1);
    int slots = resident_fixed ? resident_fixed : blocks_per_cu * num_cus;
    slots = std::max(1, std::min(slots, max_slots));
    TileGeometry g;
    g.threads = wpt * 64;
    g.grid = std::min(slots, ntiles);
    return g;
}

// the static part of a member's share under a plan: `frac_num / 4` of the smallest member's chunks, whole rounds of W
TeamRegPlan team_reg_plan(int n, int s, int G, int regs_per_wave, int quarters, int dv, int dc)
{
    TeamRegPlan rp;
    // Rows of checks that are only PARTLY on chip (a member's room beyond the whole checks of its block: 2-3 % of the
    // rows) put those checks and their bits on the general per-edge updates.  Round 4, 65,536 syndromes x 50 iterations,
    // alternating on one box, with them / whole checks only: bit degree 3 -- (3,6) n = 16380 505.2 / 491.2 ms, (3,9)
    // 503.0 / 498.5 ms: whole checks only; bit degree 4 and 5 -- C3 703.6 / 706.5 ms, (4,10) 354.5 / 358.2 ms, (5,10)
    // 488.9 / 493.4 ms: with them.  (profiles/r04_tform_ab.txt)
    rp.whole_checks = dv == 3;
    // ... and where they stay, their bits take a member's last positions (team_rows_tables()): C3 full-50 702.5 -> 700.9 ms, per
    // 0.02 49.1 -> 48.7 ms, with LLRs 739.8 -> 735.2 ms; check degree 10 lost by it ((4,10) 353.2 -> 354.5 ms, (5,10) 488.5 ->
    // 491.4 ms) and keeps them dealt by number.
    rp.strays_last = dc <= 9;
    const int W = rp.W;
    const int nch_c = (s + kTeamCheckChunk - 1) / kTeamCheckChunk, nch_v = (n + 3) / 4;
    const int min_c = nch_c / G, min_v = nch_v / G;           // the smallest member's share
    rp.static_c = std::max(W, min_c * quarters / 4 / W * W);
    rp.static_v = std::max(W, min_v * quarters / 4 / W * W);
    if (min_c < 2 * W || min_v < 2 * W || quarters <= 0) { rp.static_c = W; rp.static_v = W; }   // (round 2's dealing: a wave's first chunk is its by right)
    else rp.regs_per_wave = regs_per_wave;
    return rp;
}
TeamRowTables team_rows_tables(int n, int s, int nnz, int dc, int dv, const std::vector<int> &c2r, int G, const TeamRegPlan &rp)
{
    TeamRowTables out;
    const int vt = team_vtab_words(dv), W = rp.W, RC = rp.regs_per_wave;
    auto check_owner = [&](int i) { return (i / kTeamCheckChunk) % G; };
    // the wave that owns check i by right inside its member, or -1 (dealt dynamically)
    auto check_wave = [&](int i) { const int l = (i / kTeamCheckChunk) / G; return (RC > 0 && l < rp.static_c) ? l % W : -1; };
    auto pos_wave = [&](int p) { const int l = (p / 4) / G; return (RC > 0 && l < rp.static_v) ? l % W : -1; };
    std::vector<int> cap((size_t)G, 0), member_of_bit((size_t)n, -1);
    for (int p = 0; p < n; ++p) cap[(size_t)((p / 4) % G)]++;
    std::vector<int> room = cap;
    // A bit goes to the owner of its FIRST check while that member has room, else to the owner of another of its checks
    // (the one with most room).  First check first: in a Gallager code the first block's check i holds bits
    // wr * i ... wr * i + wr - 1, so all of them land with that check's owner and the rows that end up on chip are
    // whole checks' worth -- a quarter of the checks need no memory at all and the others none of the detours of a
    // mixed update (two clean checks of a chunk load their rows together) -- instead of one or two rows in nearly
    // every check (LDPC_TEAM_CONCENTRATE=0, experiments build: most room only, as in round 2).
    for (int j = 0; j < n; ++j) {
        int best = -1;
        for (int k = 0; k < dv; ++k) {
            const int m = check_owner(c2r[(size_t)dv * j + k] / dc);
            if (room[(size_t)m] <= 0) continue;
            if (k == 0 && rp.concentrate) { best = m; break; }
            if (best < 0 || room[(size_t)m] > room[(size_t)best]) best = m;
        }
        if (best >= 0) { member_of_bit[(size_t)j] = best; room[(size_t)best]--; }
    }
    for (int j = 0, m = 0; j < n; ++j) {
        if (member_of_bit[(size_t)j] >= 0) continue;
        while (m < G && room[(size_t)m] == 0) ++m;
        if (m >= G) { out.why = "team row tables: a bit is left without a position"; return out; }   // (cannot happen: the members' rooms add up to n positions and every bit takes one)
        member_of_bit[(size_t)j] = m; room[(size_t)m]--;
    }
    // positions of every member in ascending order, and which of them belong to a wave by right
    std::vector<std::vector<int>> pos_of((size_t)G), bits_of((size_t)G);
    for (int p = 0; p < n; ++p) pos_of[(size_t)((p / 4) % G)].push_back(p);
    for (int j = 0; j < n; ++j) bits_of[(size_t)member_of_bit[(size_t)j]].push_back(j);
    std::vector<int> bit((size_t)n, -1), reg_of((size_t)nnz, -1);
    std::vector<std::vector<char>> placed_of((size_t)G);        // per member: which of bits_of[m] already have a position (register rows)
    std::vector<std::vector<int>> reg_rows((size_t)G * W);       // per (member, wave): the CSR rows held in registers
    // (whole checks: a wave's registers take a multiple of dc rows, so that no check is split between registers and LDS --
    //  a split check is all on chip and still pays the general update: 30 of 32 rows a wave for dc = 6 and 10)
    const int RCw = rp.concentrate ? RC / dc * dc : RC;
    std::vector<std::vector<int>> reg_bits((size_t)G * W);      // ... and the bits those rows belong to (they get that wave's static positions)
    auto static_positions = [&](int m) {                         // of each wave of member m, ascending
        std::vector<std::vector<int>> spos((size_t)W);
        for (int p : pos_of[(size_t)m]) { const int w = pos_wave(p); if (w >= 0) spos[(size_t)w].push_back(p); }
        return spos;
    };
    for (int m = 0; m < G; ++m) {
        const std::vector<std::vector<int>> spos = static_positions(m);
        std::vector<char> placed(bits_of[(size_t)m].size(), 0);
        if (RC > 0)
            for (size_t b = 0; b < bits_of[(size_t)m].size(); ++b) {
                const int j = bits_of[(size_t)m][b];
                for (int k = 0; k < dv; ++k) {
                    const int q = c2r[(size_t)dv * j + k], i = q / dc;
                    if (check_owner(i) != m) continue;
                    const int w = check_wave(i);
                    if (w < 0 || (int)reg_rows[(size_t)m * W + w].size() >= RCw || reg_bits[(size_t)m * W + w].size() >= spos[(size_t)w].size()) continue;
                    reg_bits[(size_t)m * W + w].push_back(j);
                    reg_rows[(size_t)m * W + w].push_back(q);
                    placed[b] = 1;
                    break;
                }
            }
        placed_of[(size_t)m] = std::move(placed);   // (positions are given out once the LDS rows are known: below)
    }
    // LDS candidates per member (check and bit share the owner, not in registers), in check order; the first kTeamRowsMax of each get rows
    std::vector<char> is_reg((size_t)nnz, 0);
    for (auto &v : reg_rows) for (int q : v) is_reg[(size_t)q] = 1;
    std::vector<std::vector<int>> cand((size_t)G);
    for (int j = 0; j < n; ++j)
        for (int k = 0; k < dv; ++k) {
            const int q = c2r[(size_t)dv * j + k];
            if (!is_reg[(size_t)q] && check_owner(q / dc) == member_of_bit[(size_t)j]) cand[(size_t)member_of_bit[(size_t)j]].push_back(q);
        }
    for (auto &v : cand) { std::sort(v.begin(), v.end()); if ((int)v.size() > kTeamRowsMax) v.resize(kTeamRowsMax); }
    if (rp.whole_checks) {
        // only whole checks stay on chip: a check with SOME rows on chip takes the general update (pointers per edge),
        // which costs more than the few rows save -- in a Gallager code these are the stray edges beyond the first block
        std::vector<int> on_chip((size_t)s, 0);
        for (auto &v : reg_rows) for (int q : v) on_chip[(size_t)(q / dc)]++;
        for (auto &v : cand) for (int q : v) on_chip[(size_t)(q / dc)]++;
        auto partial = [&](int q) { return on_chip[(size_t)(q / dc)] < dc; };
        for (auto &v : reg_rows) v.erase(std::remove_if(v.begin(), v.end(), partial), v.end());
        for (auto &v : cand) v.erase(std::remove_if(v.begin(), v.end(), partial), v.end());
    }
    // The other bits fill the positions that are left, in ascending order -- first the bits with at most their FIRST edge on
    // chip, then the "strays" (a later edge in LDS: the room a member has beyond the whole checks of its block).  A position
    // chunk with one stray in it leaves the four-at-once update for the general one, and dealt by number the strays sat
    // in a third of all chunks (30 ... 52 of a member's 128 at the C3 size, and the members with most were the slowest of
    // every variable sweep); together they fill a tenth, at the upper end of the member's positions, which its waves deal
    // among themselves.
    {
        std::vector<char> in_cand((size_t)nnz, 0);
        for (auto &v : cand) for (int q : v) in_cand[(size_t)q] = 1;
        auto is_stray = [&](int j) {
            bool stray = false;
            if (!rp.strays_last) return false;
            for (int k = 1; k < dv; ++k) stray = stray || in_cand[(size_t)c2r[(size_t)dv * j + k]];
            return stray;
        };
        for (int m = 0; m < G; ++m) {
            // the bits with a row in a wave's registers: that wave's static positions, strays last as well
            const std::vector<std::vector<int>> spos = static_positions(m);
            for (int w = 0; w < W; ++w) {
                size_t at = 0;
                for (int pass = 0; pass < 2; ++pass)
                    for (int j : reg_bits[(size_t)m * W + w])
                        if ((int)is_stray(j) == pass) bit[(size_t)spos[(size_t)w][at++]] = j;
            }
            const std::vector<int> &bm = bits_of[(size_t)m];
            const std::vector<char> &placed = placed_of[(size_t)m];
            std::vector<int> order;
            for (int pass = 0; pass < 2; ++pass)
                for (size_t b = 0; b < bm.size(); ++b) {
                    if (placed[b]) continue;
                    if ((int)is_stray(bm[b]) == pass) order.push_back(bm[b]);
                }
            size_t b = 0;
            for (int p : pos_of[(size_t)m]) {
                if (bit[(size_t)p] >= 0) continue;
                if (b >= order.size()) { out.why = "team row tables: a member has fewer bits than positions"; return out; }   // (cannot happen: a member has as many bits as positions)
                bit[(size_t)p] = order[b++];
            }
        }
    }
    for (int mw = 0; mw < G * W; ++mw) {
        std::sort(reg_rows[(size_t)mw].begin(), reg_rows[(size_t)mw].end());
        for (int x = 0; x < (int)reg_rows[(size_t)mw].size(); ++x) reg_of[(size_t)reg_rows[(size_t)mw][(size_t)x]] = x;
        out.in_regs += reg_rows[(size_t)mw].size();
    }
    int R = 0;
    for (auto &v : cand) R = std::max(R, (int)v.size());
    R = std::max(R, 1);
    std::vector<int> lds_row_of((size_t)nnz, -1);
    std::vector<int> &lds_edge = out.lds_edge, &reg_edge = out.reg_edge;
    lds_edge.assign((size_t)G * R, -1);
    reg_edge.assign((size_t)G * W * std::max(RC, 1), -1);
    std::vector<int> &vtab = out.vtab, &ctab = out.ctab;
    vtab.assign((size_t)n * vt, 0);
    ctab.assign((size_t)s * 4, 0);
    for (int m = 0; m < G; ++m)
        for (int r = 0; r < (int)cand[(size_t)m].size(); ++r) {
            const int q = cand[(size_t)m][(size_t)r], i = q / dc;
            lds_row_of[(size_t)q] = r;
            lds_edge[(size_t)m * R + r] = q;
            if (ctab[(size_t)4 * i] == 0) ctab[(size_t)4 * i + 1] = r;   // (ascending q: the check's LDS edges follow each other)
            ctab[(size_t)4 * i] |= 1 << (q - dc * i);
        }
    for (int mw = 0; mw < G * W; ++mw)
        for (int x = 0; x < (int)reg_rows[(size_t)mw].size(); ++x) {
            const int q = reg_rows[(size_t)mw][(size_t)x], i = q / dc;
            reg_edge[(size_t)mw * RC + x] = q;
            if (ctab[(size_t)4 * i + 2] == 0) ctab[(size_t)4 * i + 3] = x;
            ctab[(size_t)4 * i + 2] |= 1 << (q - dc * i);
        }
    for (int p = 0; p < n; ++p) {
        const int j = bit[(size_t)p];
        bool any = false;
        for (int k = 0; k < dv; ++k) {
            const int q = c2r[(size_t)dv * j + k];
            vtab[(size_t)p * vt + k] = q;
            const int where = reg_of[(size_t)q] >= 0 ? -2 - reg_of[(size_t)q] : lds_row_of[(size_t)q];
            vtab[(size_t)p * vt + dv + k] = where;
            any = any || where != -1;
        }
        vtab[(size_t)p * vt + 2 * dv] = any ? (j | (int)0x80000000u) : j;
    }
    out.R = R;
    out.vt = vt;
    for (auto &v : cand) out.in_lds += v.size();
    return out;
}

TeamIrrTables team_irr_tables(int n, int s, int nnz, const std::vector<int> &row_ptr, const std::vector<int> &edge_bit,
                                     const std::vector<int> &col_ptr, const std::vector<int> &c2r, int G, int dcb, int dvb)
{
    TeamIrrTables out;
    auto owner = [&](int i) { return (i / kTeamCheckChunk) % G; };
    std::vector<int> room_pos((size_t)G, 0), next_lds((size_t)G, 0), member_of_bit((size_t)n, -1), lds_base((size_t)s, -1);
    for (int p = 0; p < n; ++p) room_pos[(size_t)((p / 4) % G)]++;
    for (int i = 0; i < s; ++i) {
        const int e0 = row_ptr[(size_t)i], deg = row_ptr[(size_t)i + 1] - e0, m = owner(i);
        if (deg <= 0 || deg > dcb || room_pos[(size_t)m] < deg || next_lds[(size_t)m] + deg > kTeamRowsMax) continue;
        bool ok = true;
        for (int k = 0; k < deg && ok; ++k) {
            const int j = edge_bit[(size_t)e0 + k];
            ok = member_of_bit[(size_t)j] < 0 && col_ptr[(size_t)j + 1] - col_ptr[(size_t)j] <= dvb;
        }
        if (!ok) continue;
        for (int k = 0; k < deg; ++k) member_of_bit[(size_t)edge_bit[(size_t)e0 + k]] = m;
        room_pos[(size_t)m] -= deg;
        lds_base[(size_t)i] = next_lds[(size_t)m];
        next_lds[(size_t)m] += deg;
        out.in_lds += (size_t)deg;
    }
    for (int j = 0, m = 0; j < n; ++j) {             // the other bits: wherever there is room
        if (member_of_bit[(size_t)j] >= 0) continue;
        while (m < G && room_pos[(size_t)m] == 0) ++m;
        if (m >= G) { out.why = "team tables of an irregular graph: a bit is left without a position"; return out; }   // (cannot happen: the rooms add up to n positions)
        member_of_bit[(size_t)j] = m; room_pos[(size_t)m]--;
    }
    // positions of every member in ascending order take its bits in ascending order
    std::vector<std::vector<int>> bits_of((size_t)G);
    for (int j = 0; j < n; ++j) bits_of[(size_t)member_of_bit[(size_t)j]].push_back(j);
    std::vector<size_t> taken((size_t)G, 0);
    std::vector<int> bit_at((size_t)n, -1);
    out.posmap.assign((size_t)std::max(n, 1), 0);
    for (int p = 0; p < n; ++p) {
        const int m = (p / 4) % G;
        const int j = bits_of[(size_t)m][taken[(size_t)m]++];
        bit_at[(size_t)p] = j;
        out.posmap[(size_t)j] = p;
    }
    for (int m = 0; m < G; ++m) out.R = std::max(out.R, next_lds[(size_t)m]);
    std::vector<int> check_of((size_t)std::max(nnz, 1), 0);
    for (int i = 0; i < s; ++i)
        for (int e = row_ptr[(size_t)i]; e < row_ptr[(size_t)i + 1]; ++e) check_of[(size_t)e] = i;
    out.ctab2.assign(((size_t)s + 1) * 2, -1);
    for (int i = 0; i <= s; ++i) out.ctab2[(size_t)2 * i] = row_ptr[(size_t)i];
    for (int i = 0; i < s; ++i) out.ctab2[(size_t)2 * i + 1] = lds_base[(size_t)i];
    out.lds_edge.assign((size_t)G * out.R, -1);
    for (int i = 0; i < s; ++i)
        if (lds_base[(size_t)i] >= 0)
            for (int e = row_ptr[(size_t)i]; e < row_ptr[(size_t)i + 1]; ++e)
                out.lds_edge[(size_t)owner(i) * out.R + lds_base[(size_t)i] + (e - row_ptr[(size_t)i])] = e;
    out.ptab.assign(((size_t)n + 1) * 2, 0);
    out.ploc.assign((size_t)std::max(nnz, 1), 0);
    int at = 0;
    for (int p = 0; p < n; ++p) {
        const int j = bit_at[(size_t)p];
        out.ptab[(size_t)2 * p] = at;
        bool any = false;
        for (int k = col_ptr[(size_t)j]; k < col_ptr[(size_t)j + 1]; ++k) {
            const int q = c2r[(size_t)k], i = check_of[(size_t)q];
            if (lds_base[(size_t)i] >= 0) { out.ploc[(size_t)at++] = -1 - (lds_base[(size_t)i] + (q - row_ptr[(size_t)i])); any = true; }
            else out.ploc[(size_t)at++] = q;
        }
        out.ptab[(size_t)2 * p + 1] = any ? (j | (int)0x80000000u) : j;
    }
    out.ptab[(size_t)2 * n] = at;
    return out;
}

int team_irr_dc_bucket(const std::vector<int> &row_ptr, int s, int64_t nnz)
{
    int max_deg = 0;
    int64_t halves = 0;   // edges of the checks of 17 ... 32 edges
    int64_t wide = 0;     // sum of deg^2 over the checks beyond 32 edges
    for (int i = 0; i < s; ++i) {
        const int deg = row_ptr[(size_t)i + 1] - row_ptr[(size_t)i];
        max_deg = std::max(max_deg, deg);
        if (deg > 32) wide += (int64_t)deg * deg;
        else if (deg > 16) halves += deg;
    }
    if (max_deg <= 8) return 8;
    if (max_deg <= 16) return 16;
    return (halves * 8 <= nnz && wide * 8 <= nnz) ? 16 : 0;      // (deg^2 / 2 against 2 nnz / 32)
}

}  // namespace ldpc

// team_plan.hpp -- how a batch is dealt to teams of workgroups and the index tables the team kernel
// (bp_team_kernels.hpp) reads: the plan (TeamPlanIn -> TeamPlan), the levels of the straggler hand-off (LevelPlanIn ->
// LevelPlan, level_plan_pure()), the slot arithmetic of a tile launch (tile_waves(), tile_geometry_pure()), the
// rows-on-chip tables of a regular graph (TeamRegPlan, TeamRowTables) and the whole-checks-in-LDS tables of an irregular
// one (TeamIrrTables).  Pure host code over team_layout.hpp and the standard library -- no HIP, no decoder handle, no
// environment -- so that it builds with a plain C++ compiler and runs under the sanitizers on the CPU
// (tests/native/team_plan_sanitize.cpp).  The host unit (ldpc_mi355x.hip: team_plan_in(), plan_tile_launch(),
// plan_levels(), team_rows_build(), team_irr_build()) fills the inputs from a decoder and uploads the tables;
// ldpc_debug_team_plan / _rows / _irr hand them to the CPU tests.
#pragma once
#include "team_layout.hpp"

#include <cstddef>
#include <cstdint>
#include <vector>

namespace ldpc {

// What the team plan depends on (pure data: ldpc_debug_team_plan() plans without a device for a CPU test)
struct TeamPlanIn {
    int64_t nnz = 0, max_iters = 0;
    size_t cache = 0;          // budget of message slots in flight (ldpc_bp_decoder::team_cache)
    int xcds_forced = 0;       // LDPC_TEAM_XCDS
    bool team_max_set = false; // LDPC_TEAM_MAX given: no teams over all XCDs for <= 3 tiles
    bool rows_possible = false;
    int rows_dv = 4;           // bit degree of the regular graph (one edge per bit is a candidate for a row in LDS)
    int reg_rows = 0;          // rows a member's waves keep in registers on top of the LDS (W x regs per wave)
    int num_cus = 256;
    int per_xcd = 0, gcap = 0; // team_geometry(): team workgroups one XCD hosts, members per team at most
    int gcap_one = 0;          // ... members at most of a persistent team that has an XCD to itself (>= gcap)
    // <= 3 tiles, members over all XCDs: members at most, message rows a member at least.  (Round 3, one tile of the C3 code,
    // a single decode! / 50 iterations: 64 members 0.294 / 3.44 ms, 96: 0.246 / 2.96, 128: 0.221 / 2.62, 192: 0.230 / 2.70,
    // 256: 0.244 / 3.00; n = 32768, 50 iterations: 64: 5.64, 128: 3.83, 192: 3.57, 256: 3.72 ms -- profiles/r03_scatter_tune.txt)
    int scatter_max = 192, scatter_rows = 512;
    // ... and up to how many tiles a batch is dealt that way (LDPC_TEAM_SCATTER_TILES).  (50 iterations, C3 code / n = 32768,
    // all-XCD teams against one team per XCD: 1 tile 2.4 / 3.4 against 5.1 / 10.2 ms, 2 tiles 3.3 / 5.2, 3 tiles 4.3 / 7.1,
    // 4 tiles 5.09 / 10.7 against 5.00 / 10.2, 5 tiles 6.1 / 13.9 against 5.1 / 12.1 -- profiles/r03_scatter_tiles.txt)
    int scatter_tiles = 3;
    // bytes a team keeps rewriting besides its message slot: with LLRs wanted the posterior odds of every bit of the tile in
    // hand, n x 512 B per iteration (they live in the cache with the slot, and count against the same budget)
    size_t extra = 0;
    // an irregular graph whose tables (team_irr_tables()) were built for teams of irr_G members keep irr_on_chip of the
    // tile's rows in LDS: counted off the slots of such teams
    bool irr_possible = false;
    int irr_G = 0, irr_on_chip = 0;
    // WIDE teams (round 4): T < 8 persistent teams of (all workgroups) / T members each, dealt over ALL XCDs, rows on
    // chip -- for graphs of which eight slots do not fit the Infinity Cache but a few do (n = 65536: 128 MiB a slot, 96 MiB
    // with a quarter of the rows on chip: two; n = 32768: four).  Every barrier then writes the XCDs' L2s back (the
    // members share no L2), and still -- 16,384 syndromes x 50 iterations, profiles/r04_wide_teams.txt -- n = 65536: 910 ms
    // against the tile kernel's 1238 and eight one-XCD teams' 1228 (T = 1: 1112, T = 4: 1133: four slots are 384 MiB);
    // n = 32768: T = 4 442 ms against eight one-XCD teams' 496 (T = 2: 533).  Without rows on chip: no (n = 65536, T = 2:
    // 1300 ms).  0 = automatic (team_wide_auto()), -1 = never, T > 0 = forced (LDPC_TEAM_WIDE, experiments).
    int wide = 0;
};

// How a batch of fresh tiles is dealt to teams (bp_team_kernels.hpp).  G = 1: no teams for it.
//   * up to 3 tiles: one team per tile, its members dealt over ALL XCDs (scatter), 128-192 of them;
//   * as many tiles as fit one round of teams with the slots at most a quarter over the cache budget: one team per
//     tile (8 tiles of the n = 16384 code: 8 teams once rather than 7 teams twice);
//   * otherwise PERSISTENT teams inside the budget (team_fit()): a team takes tile after tile in its own slot;
//   * nothing fits (larger graphs; LDPC_TEAM_CACHE_MIB=0): round 1's rule -- one team per tile, at most one tile
//     per CU -- and batches of more tiles than CUs stay with the tile kernel, which streams from HBM as well as
//     teams would.
struct TeamPlan {
    int G = 1;            // members per team
    int nteams = 0;       // teams (and message slots)
    int grid = 0;         // workgroups to launch
    int xcds = 8, tpx = 0;   // XCDs that host teams, teams per XCD (not in scatter mode)
    bool scatter = false;
    bool wide = false;       // a few persistent teams over all XCDs (TeamPlanIn::wide)
    bool irr = false;        // an irregular graph: members keep whole checks in LDS (team_irr_tables())
    bool rows = false;       // members keep the rows that only they touch in LDS (TeamRows)
};

// (the rules and the measurements behind them: at the definitions, team_plan.cpp)
int team_rows_expected(const TeamPlanIn &in, int G);
bool team_fit(const TeamPlanIn &in, int64_t ntiles, bool rows, int *xcds, int *tpx, int *G);
int team_wide_auto(const TeamPlanIn &in, int64_t ntiles);
TeamPlan team_plan_pure(const TeamPlanIn &in, int64_t batch);

// The straggler hand-off's LEVELS of packed tiles (ldpc_mi355x.hip, plan_levels()): how many there are, at how many
// lanes a pass hands off into each, how many packed tiles each holds, and which kernel finishes what it holds (the node
// kernel up to node_take syndromes, teams on the packed tiles up to team_cap, the tile kernel beyond).  What the rule
// depends on, as data: the host unit fills it from a decoder, its tile launch and team_geometry().
struct LevelPlanIn {
    int ntiles = 0;
    int64_t max_iters = 0;
    int defer_thresh = 0;      // 0 auto, -1 off, else the lanes at which a fresh tile gives up (ldpc_bp_decoder::defer_thresh)
    int defer_t0 = 16, defer_t1 = 16;   // LDPC_DEFER_T0 / _T1 (T1 0 = one level)
    int lvl_cap_force = 0;     // LDPC_DEFER_CAP_TILES: packed tiles per level (tests)
    int grid_max = 0;          // workgroups of the fresh pass: max(grid, tile_grid) of the tile launch
    bool node_ok = false;      // the node-parallel kernel may finish stragglers (node_ok && variant == 0)
    int64_t node_take_max = 0; // ... up to this many of a level
    bool team_ok = false;      // team_geometry() succeeded, with ...
    int per_xcd = 0, gcap = 0; // ... its team workgroups per XCD and members per team at most
    TeamPlanIn team;           // team_plan_in(d, per_xcd, gcap): what team_fit() is asked with
};
struct LevelPlan {
    int nlevels = 0;
    struct Level {
        int thresh_in = 0;        // lanes at which the level below hands off into this one
        int cap_tiles = 0;        // packed tiles it can hold
        unsigned node_take = 0;   // up to this many syndromes: the node-parallel kernel finishes them
        unsigned team_cap = 0;    // above node_take up to this many: teams of workgroups on the packed tiles
        int t_G = 0, t_xcds = 8, t_nteams = 0, t_grid = 0;   // teams on the packed tiles: members, XCDs, teams, workgroups
    } lv[3];                      // [1], [2]: the levels; [0] unused (level 0 is the batch)
};
LevelPlan level_plan_pure(const LevelPlanIn &in);

// Geometry of a tile-kernel launch: waves per tile (tile_waves(); the occupancy of that instantiation is the host
// unit's to ask), then threads and grid from the workspace slots the budget and the chip admit.
struct TileGeometry { int threads = 0, grid = 0; };
int tile_waves(int wpt_fixed, int ntiles, int num_cus);
TileGeometry tile_geometry_pure(size_t ws_budget, size_t slot_bytes, int wpt, int blocks_per_cu, int resident_fixed, int num_cus, int ntiles);

// The tables of TeamRows for teams of G members (kept until another G is asked for), for a regular graph whose checks
// have dc edges each and whose bits dv.  Checks are dealt as the kernel deals them -- chunk c of 2 checks to member
// c % G -- and so are the POSITIONS of the bit order, in chunks of 4; the bits are put into positions by the graph: a
// bit goes to the member, among the owners of its dv checks, that has most room left (any member once those are
// full).  Every edge whose check and bit then share the owner is a candidate for a row ON CHIP:
//   * in the REGISTERS of one wave (TeamRegPlan; regs_per_wave > 0).  Inside a member the first `static_c` check
//     chunks and the first `static_v` position chunks of every sweep belong to its waves by right (chunk l of the
//     member's share to wave l % W; the rest is dealt from a counter as the waves finish).  A bit whose owning check
//     sits in a static chunk of wave w is put into a static position of that same wave, as long as the wave has
//     register rows and static positions left: that edge is then read and written by ONE wave in both sweeps of every
//     iteration and lives in its registers, numbered per wave in check order;
//   * else in the member's LDS: up to kTeamRowsMax per member, numbered in check order.
// Tables: ctab [s][4] = per check {mask of its edges in LDS, LDS row of the first of them, mask of its edges in
// registers, register row of the first of them} (a check's rows of either kind follow each other); vtab [n][vt]
// (vt = team_vtab_words(dv)) = per position the CSR rows of the bit's dv edges, where each lives (>= 0: that LDS row,
// -1: the slot, <= -2: register row -2 - x of the wave), the bit (| 1 << 31 when one of its edges is not in the
// slot), padding; lds_edge [G][R], reg_edge [G][W][regs_per_wave] = the CSR rows held (-1: none), for the write-back
// before a hand-off.
// `why`: nullptr, or what went wrong in the bookkeeping (the tables are then not to be used)
struct TeamRegPlan {
    int regs_per_wave = 0;        // 0 = no rows in registers
    int static_c = 0, static_v = 0;   // chunks of a member's share of the check / variable sweep that belong to waves by right (multiples of W)
    int W = LDPC_TEAM_THREADS / 64;
    bool concentrate = true;       // bits go to the owner of their first check where there is room (team_rows_tables())
    bool whole_checks = false;     // ... and only checks with ALL their rows on chip keep them there
    bool strays_last = true;       // bits with a later edge on chip take a member's last positions (team_rows_tables(); LDPC_TEAM_STRAYS_LAST=0: by number)
};
struct TeamRowTables {
    int R = 0;                    // LDS rows per member (the largest count; kTeamRowsMax at most)
    int vt = 0;                   // words per position record of vtab
    size_t in_lds = 0, in_regs = 0;   // edges with a row in LDS / in registers
    std::vector<int> vtab, ctab, lds_edge, reg_edge;
    const char *why = nullptr;
};
TeamRegPlan team_reg_plan(int n, int s, int G, int regs_per_wave, int quarters, int dv, int dc);
TeamRowTables team_rows_tables(int n, int s, int nnz, int dc, int dv, const std::vector<int> &c2r, int G, const TeamRegPlan &rp);

// IRREGULAR graphs (round 4): whole checks in the LDS of their owners (bp_team_kernels.hpp, IRR).  Checks are dealt as the
// kernel deals them (chunk c of 2 checks to member c % G), positions of the bit order in chunks of 4.  A check can live
// in its owner's LDS when EVERY one of its bits can be given to that member -- then nobody else ever touches its rows
// in either sweep.  That is a set packing over the checks (two checks that share a bit exclude each other); it is
// taken greedily in check order, within each member's capacity (kTeamRowsMax LDS rows, its share of the positions),
// and only over nodes inside the kernel's register buckets (dcb / dvb).  Tables: ctab2 [s + 1][2], ptab [n + 1][2],
// ploc [nnz], lds_edge [G][R] (the CSR rows held, -1 beyond a member's count), posmap [n] (position of every bit).
// `why`: as in TeamRowTables.
struct TeamIrrTables {
    int R = 1;
    size_t in_lds = 0;
    std::vector<int> ctab2, ptab, ploc, lds_edge, posmap;
    const char *why = nullptr;
};
TeamIrrTables team_irr_tables(int n, int s, int nnz, const std::vector<int> &row_ptr, const std::vector<int> &edge_bit,
                              const std::vector<int> &col_ptr, const std::vector<int> &c2r, int G, int dcb, int dvb);

// The check-degree bucket of the IRR instantiation (bp_team_kernels.hpp) an irregular graph is decoded with: 8 or 16 --
// the 32-wide straight-line code on generic pointers does not fit the registers.  A graph with a FEW wider checks (the
// tail of a random construction; one wide check of a test) still takes the 16-wide instantiation: those checks stay in
// the slot (the packing never puts them in LDS); up to 32 edges they are updated in two halves (check_update_halves:
// the first half's rows are read twice), beyond that on the O(deg^2) path of every kernel (check_update_any: deg^2 / 2
// divisions instead of 2 deg).  Admitted while the checks of 17 ... 32 edges hold at most an eighth of the edges and the
// O(deg^2) ones cost at most 1 / 32 more divisions than the graph has anyway (2 nnz); otherwise 0: every row in the
// slot, the plain 32-wide team kernel.
int team_irr_dc_bucket(const std::vector<int> &row_ptr, int s, int64_t nnz);

}  // namespace ldpc

// team_layout.hpp -- what the team kernel (bp_team_kernels.hpp) and the host code that plans its teams and builds its
// index tables (team_plan.hpp) must agree on: chunk sizes, table widths, capacities, register buckets.  Each name is
// defined here and nowhere else.  Plain C++ as well as HIP: the planner builds without a HIP header.
#pragma once

#ifdef __HIPCC__
#define LDPC_HOST_DEVICE __host__ __device__
#else
#define LDPC_HOST_DEVICE
#endif

#ifndef LDPC_TEAM_THREADS   // threads per member (experiments: 1024 = one 16-wave member per CU)
#define LDPC_TEAM_THREADS 512
#endif

namespace ldpc {

constexpr int kTile = 64;  // syndromes per tile == wavefront width on gfx950

constexpr int kTeamMaxMembers = 256;
constexpr int kTeamCheckChunk = 2;                                  // checks per chunk of the check sweep

// words per position record of vtab (bp_team_kernels.hpp "Rows in LDS": 2 dv + 1 words, padded to 8 or 16)
LDPC_HOST_DEVICE constexpr int team_vtab_words(int dv) { return 2 * dv + 1 <= 8 ? 8 : 16; }
// the degree pairs that have a rows-in-LDS instantiation (pick_team.hip)
LDPC_HOST_DEVICE constexpr bool team_rows_degrees_ok(int dc, int dv) { return dc >= 6 && dc <= 10 && dv >= 3 && dv <= 5; }

// LDS rows a member of a persistent team can hold: 312 x 512 B = 156 KiB of the 160 KiB (the kernel's own few words beside)
constexpr int kTeamRowsMax = 312;
// rows a wave keeps in the top of its register file (bp_team_kernels.hpp "Rows in REGISTERS": v192 ... v255)
constexpr int kTeamRegRows = 32;

// the register buckets of the team kernels: nodes up to this degree are straight-line code (wider ones: the O(deg^2) path)
inline int team_bucket_dc(int dc) { return dc <= 8 ? 8 : dc <= 16 ? 16 : 32; }
inline int team_bucket_dv(int dv) { return dv <= 4 ? 4 : 16; }

}  // namespace ldpc

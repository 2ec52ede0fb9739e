// replan_teams.h -- the "team fold" of RRT.replanning_batch(teams=...) as pure functions: no HIP in here, g++ alone compiles it
// (tests/host/replan_team_check.cpp), and replan_team_kernel (replan_kernels.hip) and its host side (replan_host.h) are built
// from the same pieces.  The Python statement of the rule is rrt_dubins.team_fold / team_csr; this header matches it exactly.
//
// team_of [n]: AUVs with the same label >= 0 form a team, a label < 0 is an AUV on its own; labels need not be dense.  After a
// round, once every commit of the round is done, each team's members all get the bitwise AND of the members' keep masks -- a
// habitat one of them has visited leaves everybody's list.  A team of one member is no team.
//
// The teams as a CSR: team t's members are members[team_off[t] .. team_off[t+1]-1], ascending; the teams in ascending order of
// their labels; teams with fewer than two members are left out (the fold would change nothing).
#ifndef AUVP_REPLAN_TEAMS_H
#define AUVP_REPLAN_TEAMS_H
#include <stdint.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AUVP_RT_FN __host__ __device__ inline
#else
#define AUVP_RT_FN inline
#endif

namespace auvp {

// the AND of keep[members[i]] over i = first, first + stride, ... < hi (first >= lo).  No such i: all ones, the AND's neutral
// element.  The host folds a team with (first = team_off[t], stride = 1), lane l of the kernel's wavefront with
// (first = team_off[t] + l, stride = 64).
AUVP_RT_FN uint64_t replan_team_and(const uint64_t* keep, const int32_t* members, int first, int hi, int stride) {
  uint64_t k = ~0ull;
  for (int i = first; i < hi; i += stride) k &= keep[members[i]];
  return k;
}

// ---- host only: the CSR from a label array ------------------------------------------------------------------------------

struct ReplanTeamCsr {
  std::vector<int32_t> team_off{0};  // [n_teams + 1]
  std::vector<int32_t> members;      // [team_off[n_teams]] indices into [0, n)
  int n_teams() const { return (int)team_off.size() - 1; }
};

inline ReplanTeamCsr replan_team_csr(const int32_t* team_of, int n) {
  ReplanTeamCsr c;
  std::vector<int32_t> idx;
  for (int i = 0; i < n; i++)
    if (team_of[i] >= 0) idx.push_back((int32_t)i);
  std::stable_sort(idx.begin(), idx.end(), [&](int32_t a, int32_t b) { return team_of[a] < team_of[b]; });
  for (size_t a = 0; a < idx.size();) {
    size_t b = a + 1;
    while (b < idx.size() && team_of[idx[b]] == team_of[idx[a]]) b++;
    if (b - a >= 2) {
      c.members.insert(c.members.end(), idx.begin() + (long)a, idx.begin() + (long)b);
      c.team_off.push_back((int32_t)c.members.size());
    }
    a = b;
  }
  return c;
}

// the whole fold on the host, in place
inline void replan_team_fold(const ReplanTeamCsr& c, uint64_t* keep) {
  for (int t = 0; t < c.n_teams(); t++) {
    const uint64_t k = replan_team_and(keep, c.members.data(), c.team_off[(size_t)t], c.team_off[(size_t)t + 1], 1);
    for (int i = c.team_off[(size_t)t]; i < c.team_off[(size_t)t + 1]; i++) keep[c.members[(size_t)i]] = k;
  }
}

// ---- what the kernel and its host side share ---------------------------------------------------------------------------

struct ReplanRecord;  // (replan_commit.h)

constexpr int REPLAN_TEAM_WAVES = 4;  // teams per workgroup of replan_team_kernel (one wavefront each)

struct ReplanTeamDev {
  int32_t n_teams;
  const int32_t* team_off;  // [n_teams + 1]
  const int32_t* members;   // [team_off[n_teams]], every entry inside keep's range (the host built them)
  const int32_t* slot_of;   // [n_auvs] the AUV's record of this round, -1: none; null: no records (the probe)
  uint64_t* keep;           // [n_auvs], folded in place
  ReplanRecord* rec;        // [n_slots]; rec[slot_of[m]].keep gets the team's list too
};

}  // namespace auvp
#endif  // AUVP_REPLAN_TEAMS_H

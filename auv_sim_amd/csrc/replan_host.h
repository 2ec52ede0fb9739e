// replan_host.h -- host side of the device commit step of RRT.replanning_batch (auvp_replan_*, include/auvplan.h): the fleet's
// state on the handle (last [n,7], keep [n], the trajectory log, the teams), the launch of rrt_commit_kernel (replan_kernels.hip)
// behind auvp_rrt_group_best and of replan_team_kernel behind it where the fleet has teams, the one download at the end, and the
// probe entries that run the kernels' rules on the caller's courses and masks; and the team-aware winner selection
// (auvp_replan_team_pick: rrt_group_best_kernel, rrt_course_words_kernel, replan_team_pick_kernel -- replan_pick.h) and the one
// that keeps teammates' courses apart (auvp_replan_team_pick_apart: rrt_course_ticks_kernel, replan_team_pick_apart_kernel --
// replan_apart.h).
// Every index the kernel uses is computed here from host data: the group records' host copy (h->group_best) sizes the course
// scratch and the round's log space before the launch.
// Included at the end of auvplan.hip.
#ifndef AUVP_REPLAN_HOST_H
#define AUVP_REPLAN_HOST_H
#include "replan_commit.h"
#include "replan_teams.h"
#include "replan_pick.h"
#include "replan_apart.h"
#include "replan_measure.h"
#include "replan_ticks.h"

extern "C" hipError_t auvpi_replan_measure_launch(const auvp::ReplanMeasureDev* M, hipStream_t stream);
extern "C" hipError_t auvpi_replan_measure_ticks_launch(const auvp::ReplanMeasTicksDev* M, hipStream_t stream);
extern "C" hipError_t auvpi_replan_ticks_launch(const auvp::RrtBuffers* B, const auvp::ReplanTicksDev* A, hipStream_t stream);
extern "C" hipError_t auvpi_replan_pick_apart_launch(const auvp::ReplanPickDev* T, const auvp::ReplanApartDev* A, hipStream_t stream);
extern "C" hipError_t auvpi_replan_words_launch(const auvp::RrtBuffers* B, const auvp::ReplanWordsDev* A, hipStream_t stream);
extern "C" hipError_t auvpi_replan_pick_launch(const auvp::ReplanPickDev* T, hipStream_t stream);
extern "C" hipError_t auvpi_replan_team_launch(const auvp::ReplanTeamDev* T, hipStream_t stream);
extern "C" hipError_t auvpi_replan_commit_launch(const auvp::RrtBuffers* B, const auvp::ReplanCommitDev* A, int n_episodes, hipStream_t stream);
extern "C" hipError_t auvpi_replan_gather_launch(const auvp::ReplanSegment* seg, int n_seg, const double* log, double* out, hipStream_t stream);

static_assert(sizeof(auvp_replan_record) == sizeof(auvp::ReplanRecord), "round record layout");
// the public record's `claimed` is the first of the internal record's two reserved doubles
static_assert(offsetof(auvp_replan_record, claimed) == offsetof(auvp::ReplanRecord, _reserved), "round record layout: claimed");
static_assert(offsetof(auvp_replan_record, keep) == offsetof(auvp::ReplanRecord, keep), "round record layout: keep");
// ... and `conflicts` with its own reserved word the second
static_assert(offsetof(auvp_replan_record, conflicts) == offsetof(auvp::ReplanRecord, _reserved) + sizeof(double), "round record layout: conflicts");
static_assert(sizeof(((auvp_replan_record*)nullptr)->conflicts) + sizeof(((auvp_replan_record*)nullptr)->_reserved) == sizeof(double),
              "round record layout: conflicts");

namespace {

struct ReplanState {
  int n_auvs = 0;  // 0: auvp_replan_begin not called
  DevBuf last, keep, log, course, slots, rec, seg, traj;
  long long log_rows = 0;                  // rows of the log reserved so far (each round: the sum of its winners' path_len)
  long long rows_committed = 0;            // rows of the log in use
  int rounds = 0;
  std::vector<long long> auv_rows;         // [n_auvs] rows committed per AUV
  typedef auvp::ReplanPiece Piece;         // (with the round that committed it: replan_ticks.h)
  std::vector<Piece> pieces;               // in round order
  double last_span = 0.0;                  // round_span of the most recent auvp_replan_commit
  std::vector<auvp::ReplanRecord> rec_host;
  long long bytes_to_host = 0, bytes_traj = 0;
  double commit_ms = 0.0;                  // rrt_commit_kernel's time (with teams: and replan_team_kernel's; with auvp_replan_team_pick /
                                           // _apart: and its kernels'), summed over the rounds
  // the fleet's teams (auvp_replan_set_teams): the CSR of replan_teams.h in HBM; n_teams == 0: none, nothing more is launched
  int n_teams = 0;
  int max_team = 0;                        // members of the largest team
  DevBuf team_off, team_members, slot_of;
  // the team-aware selection (auvp_replan_team_pick) of the round being committed: the masks the members saw, [pick_best.size()]
  // in HBM, and the group records it left -- the commit copies the masks into its records only if the handle's group records
  // are still those
  DevBuf words, leaf_t, claimed, pick_auv, pick_slot_of;
  std::vector<RrtGroupBest> pick_best;
  bool pick_pending = false;
  // auvp_replan_team_pick_apart: every episode's tick table and the winners' conflict counts [pick_best.size()], which the
  // commit copies as it copies the masks
  DevBuf tick_head, tick_xy, conflicts;
  bool pick_apart = false;
  // auvp_replan_measure: the member table, the sharks' positions and the last table of measurements [meas_K][meas_F][meas_A][5];
  // with option MEAS_TICKS the row groups' segments of the last commit too (replan_ticks.h)
  DevBuf meas_members, meas_shark, meas, meas_seg;
  int meas_F = 0, meas_A = 0;              // 0: no measurement since auvp_replan_begin
  int meas_K = 1;                          // steps of the last table: MEAS_TICKS in force at that measurement, 1 without it
};

ReplanState* replan_of(auvp_handle* h) {
  if (!h->replan) {
    h->replan = new ReplanState();
    h->replan_free = [](void* p) { delete static_cast<ReplanState*>(p); };
  }
  return static_cast<ReplanState*>(h->replan);
}

// the log holds `rows` rows, with what it held before (DevBuf::reserve alone drops the contents of a buffer that grows)
int replan_log_reserve(auvp_handle* h, ReplanState& S, long long rows) {
  const size_t need = (size_t)std::max<long long>(rows, 1) * auvp::REPLAN_ROW * sizeof(double);
  if (need <= S.log.cap) return AUVP_OK;
  DevBuf grown;
  HIPCHK(h, grown.reserve(std::max(need, S.log.cap * 2)));
  const size_t used = (size_t)S.log_rows * auvp::REPLAN_ROW * sizeof(double);
  if (used) {
    HIPCHK(h, hipMemcpyAsync(grown.p, S.log.p, used, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  std::swap(S.log.p, grown.p);
  std::swap(S.log.cap, grown.cap);
  return AUVP_OK;
}

// slot_of [n_auvs]: the group that names each AUV, -1: none; every auv_of[g] inside [0, n_auvs) and named once
int replan_slot_of(auvp_handle* h, const int32_t* auv_of, int G, int n_auvs, std::vector<int32_t>& slot_of) {
  slot_of.assign((size_t)n_auvs, -1);
  for (int g = 0; g < G; g++) {
    const int a = auv_of[g];
    if (a < 0 || a >= n_auvs) return fail(h, AUVP_ERR_ARG, "group %d: AUV %d outside [0, %d)", g, a, n_auvs);
    if (slot_of[(size_t)a] >= 0) return fail(h, AUVP_ERR_ARG, "AUV %d is named twice", a);
    slot_of[(size_t)a] = (int32_t)g;
  }
  return AUVP_OK;
}

// course_off [n + 1]: row offsets from 0, ascending, no course of 2^31 rows or more
int replan_course_off_check(auvp_handle* h, const int64_t* course_off, int n) {
  if (course_off[0] != 0) return fail(h, AUVP_ERR_ARG, "course_off[0] != 0");
  for (int i = 0; i < n; i++)
    if (course_off[i + 1] < course_off[i] || course_off[i + 1] - course_off[i] > 0x7fffffffll)
      return fail(h, AUVP_ERR_ARG, "course_off is not an ascending list of row offsets");
  return AUVP_OK;
}

// members of the largest team
int replan_max_team(const auvp::ReplanTeamCsr& csr) {
  int n = 0;
  for (int t = 0; t < csr.n_teams(); t++) n = std::max(n, (int)(csr.team_off[(size_t)t + 1] - csr.team_off[(size_t)t]));
  return n;
}

// rrt_commit_kernel on the slots and, with `teams`, replan_team_kernel on the fleet's teams behind it, timed together; the
// records come back into S.rec_host
int replan_launch(auvp_handle* h, ReplanState& S, const auvp::RrtBuffers* B, auvp::ReplanCommitDev& A, const std::vector<auvp::ReplanSlot>& slots,
                  double* ms_out, bool teams = false) {
  int rc;
  if ((rc = upload(h, S.slots, slots.data(), slots.size()))) return rc;
  HIPCHK(h, S.rec.reserve(slots.size() * sizeof(auvp::ReplanRecord)));
  auvp::ReplanTeamDev T{};
  std::vector<int32_t> slot_of;  // (lives until the stream is waited for below)
  if (teams) {
    slot_of.assign((size_t)S.n_auvs, -1);
    for (size_t g = 0; g < slots.size(); g++) slot_of[(size_t)slots[g].auv] = (int32_t)g;  // (auv: checked against [0, n_auvs) by the caller)
    if ((rc = upload(h, S.slot_of, slot_of.data(), slot_of.size()))) return rc;
    T.n_teams = S.n_teams;
    T.team_off = S.team_off.as<int32_t>(); T.members = S.team_members.as<int32_t>(); T.slot_of = S.slot_of.as<int32_t>();
    T.keep = A.keep; T.rec = S.rec.as<auvp::ReplanRecord>();
  }
  A.n_slots = (int32_t)slots.size();
  A.slots = S.slots.as<auvp::ReplanSlot>();
  A.rec = S.rec.as<auvp::ReplanRecord>();
  A.H = h->W.n_habitats; A.hab = h->W.hab; A.hab_t = h->W.hab_t;
  HIPCHK(h, hipEventRecord(h->ev0, h->stream));
  HIPCHK(h, auvpi_replan_commit_launch(B, &A, h->E, h->stream));
  if (teams) HIPCHK(h, auvpi_replan_team_launch(&T, h->stream));
  if (B && S.pick_pending) {
    // the masks of auvp_replan_team_pick into the records' `claimed`, device to device, if the group records are still its
    S.pick_pending = false;
    if (S.pick_best.size() == slots.size() && h->group_best.size() == slots.size() &&
        memcmp(S.pick_best.data(), h->group_best.data(), slots.size() * sizeof(RrtGroupBest)) == 0) {
      HIPCHK(h, hipMemcpy2DAsync(reinterpret_cast<char*>(S.rec.p) + offsetof(auvp::ReplanRecord, _reserved), sizeof(auvp::ReplanRecord), S.claimed.p,
                                 sizeof(uint64_t), sizeof(uint64_t), slots.size(), hipMemcpyDeviceToDevice, h->stream));
      if (S.pick_apart)  // (the counts of auvp_replan_team_pick_apart into `conflicts`, the low half of the second reserved word)
        HIPCHK(h, hipMemcpy2DAsync(reinterpret_cast<char*>(S.rec.p) + offsetof(auvp::ReplanRecord, _reserved) + sizeof(double),
                                   sizeof(auvp::ReplanRecord), S.conflicts.p, sizeof(int32_t), sizeof(int32_t), slots.size(),
                                   hipMemcpyDeviceToDevice, h->stream));
    }
  }
  HIPCHK(h, hipEventRecord(h->ev1, h->stream));
  S.rec_host.resize(slots.size());
  HIPCHK(h, hipMemcpyAsync(S.rec_host.data(), S.rec.p, slots.size() * sizeof(auvp::ReplanRecord), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  float ms = 0.f;
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
  *ms_out = ms;
  S.bytes_to_host += (long long)(slots.size() * sizeof(auvp::ReplanRecord));
  return AUVP_OK;
}

// auvp_replan_measure with option MEAS_TICKS = k set: k measurements along the segment every AUV committed in the most recent
// auvp_replan_commit (replan_ticks.h), replan_measure_ticks_kernel.  shark_xy [k,F,2]; the table is [k,F,A,5].  A k outside
// 1 .. 64 or a segment outside the log: nothing is launched and the last table stays.
int replan_measure_ticks(auvp_handle* h, ReplanState& S, const auvp::ReplanMeasurePlan& plan, int32_t n_per_shark, const double* shark_xy,
                         const void** meas_dev_out) {
  const long long k = h->opt.opt_val[OPT_MEAS_TICKS];
  const int n = (int)plan.members.size();
  // (the bound is the log's reserved size: a piece lies where its winner's whole course was given room)
  const auvp::ReplanTicksPlan tp = auvp::replan_ticks_plan(S.pieces.data(), S.pieces.size(), S.rounds - 1, S.n_auvs, plan.members.data(), n,
                                                           S.log_rows, k);
  if (tp.status == auvp::REPLAN_TICKS_BAD_K)
    return fail(h, AUVP_ERR_ARG, "option MEAS_TICKS = %lld outside 1 .. %d", k, auvp::REPLAN_MEAS_MAX_TICKS);
  if (tp.status != auvp::REPLAN_TICKS_OK) return fail(h, AUVP_ERR_STATE, "the last commit's segments do not fit the log (%d, %lld)", (int)tp.status, tp.bad);
  HIPCHK(h, hipSetDevice(h->device));
  S.meas_F = S.meas_A = 0;
  int rc;
  if ((rc = upload(h, S.meas_members, plan.members.data(), plan.members.size()))) return rc;
  if ((rc = upload(h, S.meas_seg, tp.seg.data(), tp.seg.size()))) return rc;
  if ((rc = upload(h, S.meas_shark, shark_xy, (size_t)k * (size_t)plan.F * 2))) return rc;
  HIPCHK(h, S.meas.reserve((size_t)k * (size_t)n * auvp::REPLAN_MEAS_ROW * sizeof(double)));
  auvp::ReplanMeasTicksDev M{};
  M.n = n; M.A = n_per_shark; M.k = (int32_t)k;
  M.members = S.meas_members.as<int32_t>(); M.seg = S.meas_seg.as<auvp::ReplanMeasSeg>();
  M.last = S.last.as<double>(); M.log = S.log.as<double>(); M.shark_xy = S.meas_shark.as<double>();
  M.meas = S.meas.as<double>();
  M.round_span = S.last_span;
  HIPCHK(h, hipEventRecord(h->ev0, h->stream));
  HIPCHK(h, auvpi_replan_measure_ticks_launch(&M, h->stream));
  HIPCHK(h, hipEventRecord(h->ev1, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));  // (as auvp_replan_measure)
  float ms = 0.f;
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
  h->last_ms = ms; h->last_grid = (n + auvp::REPLAN_MEAS_TICKS_WAVES - 1) / auvp::REPLAN_MEAS_TICKS_WAVES;
  h->last_block = auvp::REPLAN_MEAS_TICKS_WAVES * 64; h->last_lds = 0;
  S.meas_F = plan.F; S.meas_A = n_per_shark; S.meas_K = (int)k;
  if (meas_dev_out) *meas_dev_out = S.meas.p;
  return AUVP_OK;
}

}  // namespace

extern "C" {

int auvp_replan_begin(auvp_handle* h, int32_t n_auvs, const double* start7, const uint64_t* keep0, int32_t keep_is_shared) {
  if (!h) return AUVP_ERR_ARG;
  if (n_auvs < 1 || !start7 || !keep0) return fail(h, AUVP_ERR_ARG, "need n_auvs >= 1, the start states and the keep masks");
  HIPCHK(h, hipSetDevice(h->device));
  ReplanState& S = *replan_of(h);
  S.n_auvs = 0;  // (no fleet until the new one's state is in place)
  std::vector<uint64_t> keep((size_t)n_auvs);
  for (int i = 0; i < n_auvs; i++) keep[(size_t)i] = keep0[keep_is_shared ? 0 : i];
  int rc;
  if ((rc = upload(h, S.last, start7, (size_t)n_auvs * auvp::REPLAN_ROW))) return rc;
  if ((rc = upload(h, S.keep, keep.data(), keep.size()))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  S.log_rows = S.rows_committed = 0;
  S.rounds = 0;
  S.auv_rows.assign((size_t)n_auvs, 0);
  S.pieces.clear();
  S.last_span = 0.0;
  S.bytes_to_host = S.bytes_traj = 0;
  S.commit_ms = 0.0;
  S.n_teams = 0;  // (the teams were the old fleet's)
  S.max_team = 0;
  S.pick_pending = false;
  S.meas_F = S.meas_A = 0;
  S.meas_K = 1;
  S.n_auvs = n_auvs;
  return AUVP_OK;
}

int auvp_replan_measure(auvp_handle* h, const int32_t* shark_of, int32_t n_per_shark, const double* shark_xy, const void** meas_dev_out) {
  if (!h) return AUVP_ERR_ARG;
  ReplanState* Sp = static_cast<ReplanState*>(h->replan);
  if (!Sp || Sp->n_auvs < 1) return fail(h, AUVP_ERR_STATE, "auvp_replan_begin not called");
  ReplanState& S = *Sp;
  if (!shark_of || !shark_xy) return fail(h, AUVP_ERR_ARG, "shark_of / shark_xy is null");
  const auvp::ReplanMeasurePlan plan = auvp::replan_measure_members(shark_of, S.n_auvs, n_per_shark);
  if (plan.status == auvp::REPLAN_MEAS_BAD_SHAPE)
    return fail(h, AUVP_ERR_ARG, "the fleet's %d AUVs are no multiple >= 1 of %d AUVs per shark", S.n_auvs, n_per_shark);
  if (plan.status == auvp::REPLAN_MEAS_BAD_SHARK)
    return fail(h, AUVP_ERR_ARG, "AUV %d: shark %d outside [0, %d)", plan.bad, shark_of[plan.bad], S.n_auvs / n_per_shark);
  if (plan.status != auvp::REPLAN_MEAS_OK) return fail(h, AUVP_ERR_ARG, "shark %d is not tracked by exactly %d AUVs", plan.bad, n_per_shark);
  if (h->opt.opt_has[OPT_MEAS_TICKS]) return replan_measure_ticks(h, S, plan, n_per_shark, shark_xy, meas_dev_out);
  HIPCHK(h, hipSetDevice(h->device));
  S.meas_F = S.meas_A = 0;
  int rc;
  if ((rc = upload(h, S.meas_members, plan.members.data(), plan.members.size()))) return rc;
  if ((rc = upload(h, S.meas_shark, shark_xy, (size_t)plan.F * 2))) return rc;
  HIPCHK(h, S.meas.reserve(plan.members.size() * auvp::REPLAN_MEAS_ROW * sizeof(double)));
  auvp::ReplanMeasureDev M{};
  M.n = (int32_t)plan.members.size(); M.A = n_per_shark;
  M.members = S.meas_members.as<int32_t>(); M.last = S.last.as<double>(); M.shark_xy = S.meas_shark.as<double>();
  M.meas = S.meas.as<double>();
  HIPCHK(h, hipEventRecord(h->ev0, h->stream));
  HIPCHK(h, auvpi_replan_measure_launch(&M, h->stream));
  HIPCHK(h, hipEventRecord(h->ev1, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));  // (the host tables go out of scope; a reader on another handle's stream is ordered behind)
  float ms = 0.f;
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
  h->last_ms = ms; h->last_grid = (M.n + 63) / 64; h->last_block = 64; h->last_lds = 0;
  S.meas_F = plan.F; S.meas_A = n_per_shark; S.meas_K = 1;
  if (meas_dev_out) *meas_dev_out = S.meas.p;
  return AUVP_OK;
}

int auvp_replan_meas(auvp_handle* h, int32_t* n_sharks, int32_t* n_per_shark, double* meas) {
  if (!h) return AUVP_ERR_ARG;
  ReplanState* Sp = static_cast<ReplanState*>(h->replan);
  if (!Sp || Sp->n_auvs < 1 || Sp->meas_F < 1) return fail(h, AUVP_ERR_STATE, "no auvp_replan_measure since auvp_replan_begin");
  ReplanState& S = *Sp;
  if (n_sharks) *n_sharks = S.meas_F;
  if (n_per_shark) *n_per_shark = S.meas_A;
  if (!meas) return AUVP_OK;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t bytes = (size_t)S.meas_K * (size_t)S.meas_F * (size_t)S.meas_A * auvp::REPLAN_MEAS_ROW * sizeof(double);
  HIPCHK(h, hipMemcpyAsync(meas, S.meas.p, bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  S.bytes_to_host += (long long)bytes;
  return AUVP_OK;
}

int auvp_replan_set_teams(auvp_handle* h, int32_t n_auvs, const int32_t* team_of) {
  if (!h) return AUVP_ERR_ARG;
  ReplanState* Sp = static_cast<ReplanState*>(h->replan);
  if (!Sp || Sp->n_auvs < 1) return fail(h, AUVP_ERR_STATE, "auvp_replan_begin not called");
  ReplanState& S = *Sp;
  if (n_auvs != S.n_auvs) return fail(h, AUVP_ERR_ARG, "n_auvs %d, the fleet has %d", n_auvs, S.n_auvs);
  if (!team_of) { S.n_teams = 0; S.max_team = 0; return AUVP_OK; }
  const auvp::ReplanTeamCsr csr = auvp::replan_team_csr(team_of, n_auvs);
  if (csr.n_teams() == 0) { S.n_teams = 0; S.max_team = 0; return AUVP_OK; }
  HIPCHK(h, hipSetDevice(h->device));
  // into buffers of their own, swapped in once both tables are there: a call that fails leaves the teams as they were
  DevBuf off, mem;
  int rc;
  if ((rc = upload(h, off, csr.team_off.data(), csr.team_off.size()))) return rc;
  if ((rc = upload(h, mem, csr.members.data(), csr.members.size()))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  std::swap(S.team_off.p, off.p); std::swap(S.team_off.cap, off.cap);
  std::swap(S.team_members.p, mem.p); std::swap(S.team_members.cap, mem.cap);
  S.n_teams = csr.n_teams();
  S.max_team = replan_max_team(csr);
  return AUVP_OK;
}

int auvp_replan_team_fold(auvp_handle* h, int32_t n, const int32_t* team_of, uint64_t* keep_io) {
  if (!h) return AUVP_ERR_ARG;
  if (n < 1 || !team_of || !keep_io) return fail(h, AUVP_ERR_ARG, "need n >= 1, the labels and the keep masks");
  const auvp::ReplanTeamCsr csr = auvp::replan_team_csr(team_of, n);
  if (csr.n_teams() == 0) return AUVP_OK;  // (nobody has a teammate: nothing to fold)
  HIPCHK(h, hipSetDevice(h->device));
  // the probe's own buffers: the fleet's state and counters (auvp_replan_begin) stay as they are
  DevBuf d_keep, d_off, d_mem;
  int rc;
  if ((rc = upload(h, d_keep, keep_io, (size_t)n))) return rc;
  if ((rc = upload(h, d_off, csr.team_off.data(), csr.team_off.size()))) return rc;
  if ((rc = upload(h, d_mem, csr.members.data(), csr.members.size()))) return rc;
  auvp::ReplanTeamDev T{};
  T.n_teams = csr.n_teams();
  T.team_off = d_off.as<int32_t>(); T.members = d_mem.as<int32_t>();
  T.keep = d_keep.as<uint64_t>();
  HIPCHK(h, hipEventRecord(h->ev0, h->stream));
  HIPCHK(h, auvpi_replan_team_launch(&T, h->stream));
  HIPCHK(h, hipEventRecord(h->ev1, h->stream));
  HIPCHK(h, hipMemcpyAsync(keep_io, d_keep.p, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  float ms = 0.f;
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
  h->last_ms = ms; h->last_grid = (T.n_teams + auvp::REPLAN_TEAM_WAVES - 1) / auvp::REPLAN_TEAM_WAVES;
  h->last_block = auvp::REPLAN_TEAM_WAVES * 64; h->last_lds = 0;
  return AUVP_OK;
}

int auvp_replan_commit(auvp_handle* h, int32_t n_active, const int32_t* auv_of, double round_span, auvp_replan_record* out) {
  if (!h) return AUVP_ERR_ARG;
  ReplanState* Sp = static_cast<ReplanState*>(h->replan);
  if (!Sp || Sp->n_auvs < 1) return fail(h, AUVP_ERR_STATE, "auvp_replan_begin not called");
  if (!h->have_batch) return fail(h, AUVP_ERR_STATE, "no batch has run");
  if (!h->have_group) return fail(h, AUVP_ERR_STATE, "auvp_rrt_group_best not called for this batch");
  ReplanState& S = *Sp;
  const int G = (int)h->group_best.size();
  if (n_active != G) return fail(h, AUVP_ERR_ARG, "n_active %d, the batch has %d groups", n_active, G);
  if (!auv_of) return fail(h, AUVP_ERR_ARG, "auv_of is null");
  if (!(round_span > 0.0)) return fail(h, AUVP_ERR_ARG, "round_span must be > 0");
  int rc;
  std::vector<int32_t> slot_of;
  if ((rc = replan_slot_of(h, auv_of, G, S.n_auvs, slot_of))) return rc;
  // the slots, from the host's copy of the group records: a group that failed or has no winner commits nothing
  std::vector<auvp::ReplanSlot> slots((size_t)G);
  long long total = 0;
  for (int g = 0; g < G; g++) {
    const RrtGroupBest& r = h->group_best[(size_t)g];
    const bool wins = r.status >= 0 && r.winner >= 0 && r.winner < h->E && r.path_len > 0;
    auvp::ReplanSlot& s = slots[(size_t)g];
    s.auv = auv_of[g]; s.winner = wins ? r.winner : -1; s.path_len = wins ? r.path_len : 0; s.status = r.status;
    s.course_off = total; s.log_off = S.log_rows + total;
    total += s.path_len;
  }
  HIPCHK(h, hipSetDevice(h->device));
  if ((rc = replan_log_reserve(h, S, S.log_rows + total))) return rc;
  HIPCHK(h, S.course.reserve((size_t)std::max<long long>(total, 1) * auvp::REPLAN_ROW * sizeof(double)));
  auvp::ReplanCommitDev A{};
  A.best = h->d_group_best.as<RrtGroupBest>();
  A.course = S.course.as<double>(); A.log = S.log.as<double>();
  A.last = S.last.as<double>(); A.keep = S.keep.as<uint64_t>();
  A.round_span = round_span;
  double ms = 0.0;
  if ((rc = replan_launch(h, S, &h->B, A, slots, &ms, S.n_teams > 0))) return rc;
  for (int g = 0; g < G; g++) {
    const auvp::ReplanRecord& r = S.rec_host[(size_t)g];
    const int n = r.n_committed > 0 && r.n_committed <= slots[(size_t)g].path_len ? r.n_committed : 0;
    if (n) S.pieces.push_back(ReplanState::Piece{slots[(size_t)g].auv, n, slots[(size_t)g].log_off, S.rounds, 0});
    S.auv_rows[(size_t)slots[(size_t)g].auv] += n;
    S.rows_committed += n;
  }
  S.log_rows += total;
  S.rounds++;
  S.last_span = round_span;
  S.commit_ms += ms;
  h->last_ms = ms; h->last_grid = G; h->last_block = 64; h->last_lds = 0;
  if (out) memcpy(out, S.rec_host.data(), (size_t)G * sizeof(auvp::ReplanRecord));
  return AUVP_OK;
}

}  // extern "C"

namespace {

// team_separation's arguments (replan_apart.h); null: the selection by the claims alone
struct ReplanApartArgs {
  int32_t use_claims, W;
  double d, tick;
};

int replan_apart_check(auvp_handle* h, const ReplanApartArgs* ap, int max_team) {
  if (!ap) return AUVP_OK;
  if (!auvp::replan_apart_args_ok(ap->d, ap->tick, ap->W))
    return fail(h, AUVP_ERR_ARG, "need a finite d > 0, a finite tick > 0 and W in 1 .. %d", auvp::REPLAN_APART_MAX_TICKS);
  if (max_team > auvp::REPLAN_APART_MAX_TEAM)
    return fail(h, AUVP_ERR_ARG, "a team of %d members, more than %d", max_team, auvp::REPLAN_APART_MAX_TEAM);
  return AUVP_OK;
}

// what the tick tables' kernel and the pick that reads them share: the window and the tables' place
void replan_apart_fill(const ReplanApartArgs& ap, int E, int K, int32_t* head, double* xy, int32_t* conflicts, auvp::ReplanTicksDev& C,
                       auvp::ReplanApartDev& D) {
  C.n_episodes = E; C.K = K; C.W = ap.W; C.tick = ap.tick;
  C.head = head; C.xy = xy;
  D.W = ap.W; D.use_claims = ap.use_claims ? 1 : 0; D.d2 = ap.d * ap.d;
  D.head = head; D.xy = xy; D.conflicts = conflicts;
}

// The pick's launches on h->stream: rrt_group_best_kernel's record for every group of T.K of T's summaries -- the pick rewrites
// those of the members of teams of two or more --, then, between ev0 and ev1, the words (A; null: nobody reads them) and, with D,
// the tick tables C and the pick that keeps courses apart, without it the pick by the claims.  B: the batch's trees; null: the
// probe's courses.
int replan_pick_enqueue(auvp_handle* h, const auvp::RrtBuffers* B, const int32_t* group_off, const auvp::ReplanWordsDev* A,
                        const auvp::ReplanTicksDev* C, const auvp::ReplanApartDev* D, const auvp::ReplanPickDev& T) {
  const int G = T.n_slots;
  hipLaunchKernelGGL(rrt_group_best_kernel, dim3((G + RRT_GROUP_WAVES - 1) / RRT_GROUP_WAVES), dim3(RRT_GROUP_WAVES * 64), 0, h->stream,
                     T.summary, group_off, T.best, G);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev0, h->stream));
  if (A) HIPCHK(h, auvpi_replan_words_launch(B, A, h->stream));
  if (D) {
    HIPCHK(h, auvpi_replan_ticks_launch(B, C, h->stream));
    HIPCHK(h, auvpi_replan_pick_apart_launch(&T, D, h->stream));
  } else {
    HIPCHK(h, auvpi_replan_pick_launch(&T, h->stream));
  }
  HIPCHK(h, hipEventRecord(h->ev1, h->stream));
  return AUVP_OK;
}

// [G + 1] offsets of groups of K episodes each
std::vector<int32_t> replan_group_off(int G, int K) {
  std::vector<int32_t> off((size_t)G + 1);
  for (int g = 0; g <= G; g++) off[(size_t)g] = (int32_t)(g * K);
  return off;
}

// auvp_replan_team_pick (ap == null) and auvp_replan_team_pick_apart
int replan_team_pick_impl(auvp_handle* h, int32_t n_active, const int32_t* auv_of, int32_t K, const ReplanApartArgs* ap,
                          struct auvp_rrt_group_best* out) {
  if (!h) return AUVP_ERR_ARG;
  ReplanState* Sp = static_cast<ReplanState*>(h->replan);
  if (!Sp || Sp->n_auvs < 1) return fail(h, AUVP_ERR_STATE, "auvp_replan_begin not called");
  ReplanState& S = *Sp;
  if (S.n_teams < 1) return fail(h, AUVP_ERR_STATE, "the fleet has no teams (auvp_replan_set_teams)");
  if (!h->have_batch) return fail(h, AUVP_ERR_STATE, "no batch has run");
  if (n_active < 1 || K < 1 || !auv_of) return fail(h, AUVP_ERR_ARG, "need n_active >= 1, K >= 1 and auv_of");
  const int E = h->E;
  if ((long long)n_active * K != (long long)E) return fail(h, AUVP_ERR_ARG, "the batch has %d episodes, not %d x %d", E, n_active, K);
  const int G = n_active;
  int rc;
  if ((rc = replan_apart_check(h, ap, S.max_team))) return rc;
  const bool words = !ap || ap->use_claims;  // (without the claims nobody reads the words: no launch, no scratch for them)
  std::vector<int32_t> slot_of;
  if ((rc = replan_slot_of(h, auv_of, G, S.n_auvs, slot_of))) return rc;
  const std::vector<int32_t> group_off = replan_group_off(G, K);
  HIPCHK(h, hipSetDevice(h->device));
  // a course has at most one element per node and per path point of its tree: the scratch is sized from the batch's capacities
  // (the summaries stay in HBM), the same place for every episode
  const int64_t stride = (int64_t)h->B.cap_nodes + (int64_t)h->B.cap_points;
  if (words) HIPCHK(h, S.words.reserve((size_t)E * (size_t)stride * sizeof(uint64_t)));
  HIPCHK(h, S.leaf_t.reserve((size_t)E * sizeof(double)));
  HIPCHK(h, S.claimed.reserve((size_t)G * sizeof(uint64_t)));
  if (ap) {
    HIPCHK(h, S.tick_head.reserve((size_t)E * 2 * sizeof(int32_t)));
    HIPCHK(h, S.tick_xy.reserve((size_t)E * (size_t)ap->W * 2 * sizeof(double)));
    HIPCHK(h, S.conflicts.reserve((size_t)G * sizeof(int32_t)));
  }
  h->have_group = false;
  S.pick_pending = false;
  if ((rc = upload(h, h->d_group_off, group_off.data(), group_off.size()))) return rc;
  if ((rc = upload(h, S.pick_auv, auv_of, (size_t)G))) return rc;
  if ((rc = upload(h, S.pick_slot_of, slot_of.data(), slot_of.size()))) return rc;
  HIPCHK(h, h->d_group_best.reserve((size_t)G * sizeof(RrtGroupBest)));
  HIPCHK(h, hipMemsetAsync(S.claimed.p, 0, (size_t)G * sizeof(uint64_t), h->stream));
  if (ap) HIPCHK(h, hipMemsetAsync(S.conflicts.p, 0, (size_t)G * sizeof(int32_t), h->stream));
  auvp::ReplanWordsDev A{};
  A.n_episodes = E; A.K = K; A.H = h->W.n_habitats; A.n_bins = h->W.n_bins;
  A.stride = stride;
  A.auv_of = S.pick_auv.as<int32_t>(); A.last = S.last.as<double>();
  A.hab = h->W.hab; A.hab_t = h->W.hab_t; A.bins = h->W.bins;
  A.words = S.words.as<uint64_t>(); A.leaf_t = S.leaf_t.as<double>();
  auvp::ReplanPickDev T{};
  T.n_teams = S.n_teams; T.K = K; T.n_slots = G;
  T.team_off = S.team_off.as<int32_t>(); T.members = S.team_members.as<int32_t>(); T.slot_of = S.pick_slot_of.as<int32_t>();
  T.keep = S.keep.as<uint64_t>();
  T.summary = h->B.summary;
  T.words = A.words; T.stride = stride; T.leaf_t = A.leaf_t;
  T.best = h->d_group_best.as<RrtGroupBest>(); T.claimed = S.claimed.as<uint64_t>();
  T.w1 = h->P.w[0]; T.w2 = h->P.w[1];
  auvp::ReplanTicksDev C{};
  auvp::ReplanApartDev D{};
  if (ap) {
    replan_apart_fill(*ap, E, K, S.tick_head.as<int32_t>(), S.tick_xy.as<double>(), S.conflicts.as<int32_t>(), C, D);
    C.auv_of = A.auv_of; C.last = A.last;
  }
  if ((rc = replan_pick_enqueue(h, &h->B, h->d_group_off.as<int32_t>(), words ? &A : nullptr, &C, ap ? &D : nullptr, T))) return rc;
  h->group_best.resize((size_t)G);
  HIPCHK(h, hipMemcpyAsync(h->group_best.data(), h->d_group_best.p, (size_t)G * sizeof(RrtGroupBest), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  float ms = 0.f;
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
  S.commit_ms += ms;
  h->last_ms = ms; h->last_grid = E; h->last_block = 64; h->last_lds = (int)(auvp::REPLAN_MAX_HAB * 4 * sizeof(double));
  S.pick_best = h->group_best;
  S.pick_pending = true;
  S.pick_apart = ap != nullptr;
  h->have_group = true;
  if (out) memcpy(out, h->group_best.data(), (size_t)G * sizeof(RrtGroupBest));
  return AUVP_OK;
}

// auvp_replan_team_pick_courses (ap == null) and auvp_replan_team_pick_apart_courses
int replan_team_pick_courses_impl(auvp_handle* h, int32_t n_auvs, const int32_t* team_of, const uint64_t* keep, int32_t n_active,
                                  const int32_t* auv_of, int32_t K, const int64_t* course_off, const double* courses_xyt,
                                  const double* cost4, const double* leaf_t, const double* length, const int32_t* bin_lo,
                                  const int32_t* bin_hi, const double* weights3, const ReplanApartArgs* ap,
                                  struct auvp_rrt_group_best* out, uint64_t* claimed_out, int32_t* conflicts_out) {
  if (!h) return AUVP_ERR_ARG;
  if (n_auvs < 1 || n_active < 1 || K < 1 || !team_of || !keep || !auv_of || !course_off || !cost4 || !leaf_t || !bin_lo || !bin_hi ||
      !weights3 || !out || !claimed_out)
    return fail(h, AUVP_ERR_ARG, "bad probe arguments");
  if (!h->have_world) return fail(h, AUVP_ERR_STATE, "auvp_world_set not called");
  if ((long long)n_active * K > 0x7fffffffll) return fail(h, AUVP_ERR_ARG, "too many candidates");
  const int G = n_active, E = n_active * K;
  int rc;
  std::vector<int32_t> slot_of;
  if ((rc = replan_slot_of(h, auv_of, G, n_auvs, slot_of))) return rc;
  if ((rc = replan_course_off_check(h, course_off, E))) return rc;
  const long long total = course_off[E];
  if (total > 0 && !courses_xyt) return fail(h, AUVP_ERR_ARG, "courses_xyt is null");
  for (int e = 0; e < E; e++)
    if (bin_lo[e] < 0 || bin_hi[e] > h->W.n_bins) return fail(h, AUVP_ERR_ARG, "candidate %d: bins %d .. %d outside the table of %d", e, bin_lo[e], bin_hi[e], h->W.n_bins);
  // the candidates as summaries: what the two selection kernels read of one
  std::vector<RrtSummary> summ((size_t)E);
  std::vector<int32_t> len((size_t)E);
  const std::vector<int32_t> group_off = replan_group_off(G, K);
  memset(summ.data(), 0, summ.size() * sizeof(RrtSummary));
  for (int e = 0; e < E; e++) {
    const int L = (int)(course_off[e + 1] - course_off[e]);
    len[(size_t)e] = L;
    RrtSummary& s = summ[(size_t)e];
    s.best_leaf = L > 0 ? 0 : -1;
    s.best_path_len = L;
    for (int k = 0; k < 4; k++) s.best_cost[k] = cost4[4 * (size_t)e + k];
    s.best_length = length ? length[e] : 0.0;
  }
  const auvp::ReplanTeamCsr csr = auvp::replan_team_csr(team_of, n_auvs);
  if ((rc = replan_apart_check(h, ap, replan_max_team(csr)))) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  // the probe's own buffers: the fleet's state, the handle's group records and the counters stay as they are
  DevBuf d_summ, d_len, d_goff, d_off, d_xyt, d_lt, d_lo, d_hi, d_keep, d_slot, d_toff, d_tmem, d_words, d_best, d_claimed, d_thead, d_txy, d_conf;
  if ((rc = upload(h, d_summ, summ.data(), summ.size()))) return rc;
  if ((rc = upload(h, d_len, len.data(), len.size()))) return rc;
  if ((rc = upload(h, d_goff, group_off.data(), group_off.size()))) return rc;
  if ((rc = upload(h, d_off, course_off, (size_t)E + 1))) return rc;
  if ((rc = upload(h, d_xyt, courses_xyt, (size_t)total * 3))) return rc;
  if ((rc = upload(h, d_lt, leaf_t, (size_t)E))) return rc;
  if ((rc = upload(h, d_lo, bin_lo, (size_t)E))) return rc;
  if ((rc = upload(h, d_hi, bin_hi, (size_t)E))) return rc;
  if ((rc = upload(h, d_keep, keep, (size_t)n_auvs))) return rc;
  if ((rc = upload(h, d_slot, slot_of.data(), slot_of.size()))) return rc;
  if ((rc = upload(h, d_toff, csr.team_off.data(), csr.team_off.size()))) return rc;
  if ((rc = upload(h, d_tmem, csr.members.data(), csr.members.size()))) return rc;
  HIPCHK(h, d_words.reserve((size_t)std::max<long long>(total, 1) * sizeof(uint64_t)));
  HIPCHK(h, d_best.reserve((size_t)G * sizeof(RrtGroupBest)));
  HIPCHK(h, d_claimed.reserve((size_t)G * sizeof(uint64_t)));
  HIPCHK(h, hipMemsetAsync(d_claimed.p, 0, (size_t)G * sizeof(uint64_t), h->stream));
  auvp::ReplanTicksDev C{};
  auvp::ReplanApartDev D{};
  if (ap) {
    HIPCHK(h, d_thead.reserve((size_t)E * 2 * sizeof(int32_t)));
    HIPCHK(h, d_txy.reserve((size_t)E * (size_t)ap->W * 2 * sizeof(double)));
    HIPCHK(h, d_conf.reserve((size_t)G * sizeof(int32_t)));
    HIPCHK(h, hipMemsetAsync(d_conf.p, 0, (size_t)G * sizeof(int32_t), h->stream));
    replan_apart_fill(*ap, E, K, d_thead.as<int32_t>(), d_txy.as<double>(), d_conf.as<int32_t>(), C, D);
    C.from_courses = 1;
    C.off = d_off.as<int64_t>(); C.xyt = d_xyt.as<double>(); C.len = d_len.as<int32_t>();
  }
  auvp::ReplanWordsDev A{};
  A.n_episodes = E; A.K = K; A.H = h->W.n_habitats; A.n_bins = h->W.n_bins;
  A.from_courses = 1;
  A.off = d_off.as<int64_t>(); A.xyt = d_xyt.as<double>(); A.len = d_len.as<int32_t>();
  A.bin_lo = d_lo.as<int32_t>(); A.bin_hi = d_hi.as<int32_t>();
  A.hab = h->W.hab; A.hab_t = h->W.hab_t; A.bins = h->W.bins;
  A.words = d_words.as<uint64_t>();
  auvp::ReplanPickDev T{};
  T.n_teams = csr.n_teams(); T.K = K; T.n_slots = G;
  T.team_off = d_toff.as<int32_t>(); T.members = d_tmem.as<int32_t>(); T.slot_of = d_slot.as<int32_t>();
  T.keep = d_keep.as<uint64_t>();
  T.summary = d_summ.as<RrtSummary>();
  T.words = A.words; T.off = A.off; T.leaf_t = d_lt.as<double>();
  T.best = d_best.as<RrtGroupBest>(); T.claimed = d_claimed.as<uint64_t>();
  T.w1 = weights3[0]; T.w2 = weights3[1];
  if ((rc = replan_pick_enqueue(h, nullptr, d_goff.as<int32_t>(), &A, &C, ap ? &D : nullptr, T))) return rc;
  HIPCHK(h, hipMemcpyAsync(out, d_best.p, (size_t)G * sizeof(RrtGroupBest), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(claimed_out, d_claimed.p, (size_t)G * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
  if (ap) HIPCHK(h, hipMemcpyAsync(conflicts_out, d_conf.p, (size_t)G * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  float ms = 0.f;
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
  h->last_ms = ms; h->last_grid = E; h->last_block = 64; h->last_lds = (int)(auvp::REPLAN_MAX_HAB * 4 * sizeof(double));
  return AUVP_OK;
}

}  // namespace

extern "C" {

int auvp_replan_team_pick(auvp_handle* h, int32_t n_active, const int32_t* auv_of, int32_t K, struct auvp_rrt_group_best* out) {
  return replan_team_pick_impl(h, n_active, auv_of, K, nullptr, out);
}

int auvp_replan_team_pick_apart(auvp_handle* h, int32_t n_active, const int32_t* auv_of, int32_t K, int32_t use_claims, double d, double tick,
                                int32_t W, struct auvp_rrt_group_best* out) {
  const ReplanApartArgs ap{use_claims, W, d, tick};
  return replan_team_pick_impl(h, n_active, auv_of, K, &ap, out);
}

int auvp_replan_team_pick_courses(auvp_handle* h, int32_t n_auvs, const int32_t* team_of, const uint64_t* keep, int32_t n_active,
                                  const int32_t* auv_of, int32_t K, const int64_t* course_off, const double* courses_xyt,
                                  const double* cost4, const double* leaf_t, const double* length, const int32_t* bin_lo,
                                  const int32_t* bin_hi, const double* weights3, struct auvp_rrt_group_best* out, uint64_t* claimed_out) {
  return replan_team_pick_courses_impl(h, n_auvs, team_of, keep, n_active, auv_of, K, course_off, courses_xyt, cost4, leaf_t, length, bin_lo,
                                       bin_hi, weights3, nullptr, out, claimed_out, nullptr);
}

int auvp_replan_team_pick_apart_courses(auvp_handle* h, int32_t n_auvs, const int32_t* team_of, const uint64_t* keep, int32_t n_active,
                                        const int32_t* auv_of, int32_t K, const int64_t* course_off, const double* courses_xyt,
                                        const double* cost4, const double* leaf_t, const double* length, const int32_t* bin_lo,
                                        const int32_t* bin_hi, const double* weights3, int32_t use_claims, double d, double tick, int32_t W,
                                        struct auvp_rrt_group_best* out, uint64_t* claimed_out, int32_t* conflicts_out) {
  if (!h) return AUVP_ERR_ARG;
  if (!conflicts_out) return fail(h, AUVP_ERR_ARG, "bad probe arguments");
  const ReplanApartArgs ap{use_claims, W, d, tick};
  return replan_team_pick_courses_impl(h, n_auvs, team_of, keep, n_active, auv_of, K, course_off, courses_xyt, cost4, leaf_t, length, bin_lo,
                                       bin_hi, weights3, &ap, out, claimed_out, conflicts_out);
}

int auvp_replan_traj(auvp_handle* h, int64_t* row_off, double* rows) {
  if (!h) return AUVP_ERR_ARG;
  ReplanState* Sp = static_cast<ReplanState*>(h->replan);
  if (!Sp || Sp->n_auvs < 1) return fail(h, AUVP_ERR_STATE, "auvp_replan_begin not called");
  if (!row_off) return fail(h, AUVP_ERR_ARG, "row_off is null");
  ReplanState& S = *Sp;
  row_off[0] = 0;
  for (int a = 0; a < S.n_auvs; a++) row_off[a + 1] = row_off[a] + S.auv_rows[(size_t)a];
  if (!rows || S.rows_committed == 0) return AUVP_OK;
  // the pieces in AUV order (each AUV's in round order: the list is in round order already)
  std::vector<int64_t> next(row_off, row_off + S.n_auvs);
  std::vector<auvp::ReplanSegment> seg(S.pieces.size());
  for (size_t i = 0; i < S.pieces.size(); i++) {
    const ReplanState::Piece& p = S.pieces[i];
    seg[i] = auvp::ReplanSegment{p.src, next[(size_t)p.auv], p.n, 0};
    next[(size_t)p.auv] += p.n;
  }
  HIPCHK(h, hipSetDevice(h->device));
  int rc;
  if ((rc = upload(h, S.seg, seg.data(), seg.size()))) return rc;
  const size_t bytes = (size_t)S.rows_committed * auvp::REPLAN_ROW * sizeof(double);
  HIPCHK(h, S.traj.reserve(bytes));
  HIPCHK(h, auvpi_replan_gather_launch(S.seg.as<auvp::ReplanSegment>(), (int)seg.size(), S.log.as<double>(), S.traj.as<double>(), h->stream));
  HIPCHK(h, hipMemcpyAsync(rows, S.traj.p, bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  S.bytes_to_host += (long long)bytes;
  S.bytes_traj += (long long)bytes;
  return AUVP_OK;
}

int auvp_replan_commit_courses(auvp_handle* h, int32_t n_states, const int64_t* course_off, const double* courses, double* last7,
                               uint64_t* keep, double round_span, auvp_replan_record* out, double* rows_out) {
  if (!h) return AUVP_ERR_ARG;
  if (n_states < 1 || !course_off || !last7 || !keep || !out) return fail(h, AUVP_ERR_ARG, "bad probe arguments");
  if (!h->have_world) return fail(h, AUVP_ERR_STATE, "auvp_world_set not called");
  if (!(round_span > 0.0)) return fail(h, AUVP_ERR_ARG, "round_span must be > 0");
  int rc;
  if ((rc = replan_course_off_check(h, course_off, n_states))) return rc;
  const long long total = course_off[n_states];
  if (total > 0 && (!courses || !rows_out)) return fail(h, AUVP_ERR_ARG, "courses / rows_out is null");
  HIPCHK(h, hipSetDevice(h->device));
  ReplanState& S = *replan_of(h);
  // the probe's own state arrays and row buffer: the fleet's (auvp_replan_begin) stay as they are
  DevBuf d_last, d_keep, d_rows;
  if ((rc = upload(h, d_last, last7, (size_t)n_states * auvp::REPLAN_ROW))) return rc;
  if ((rc = upload(h, d_keep, keep, (size_t)n_states))) return rc;
  if ((rc = upload(h, S.course, courses, (size_t)total * auvp::REPLAN_ROW))) return rc;
  HIPCHK(h, d_rows.reserve((size_t)std::max<long long>(total, 1) * auvp::REPLAN_ROW * sizeof(double)));
  HIPCHK(h, hipMemsetAsync(d_rows.p, 0, (size_t)std::max<long long>(total, 1) * auvp::REPLAN_ROW * sizeof(double), h->stream));
  std::vector<auvp::ReplanSlot> slots((size_t)n_states);
  for (int i = 0; i < n_states; i++) {
    const int L = (int)(course_off[i + 1] - course_off[i]);
    slots[(size_t)i] = auvp::ReplanSlot{(int32_t)i, (int32_t)(L > 0 ? 0 : -1), (int32_t)L,
                                        (int32_t)(L > 0 ? AUVP_OK : AUVP_NO_QUALIFYING_LEAF), course_off[i], course_off[i]};
  }
  auvp::ReplanCommitDev A{};
  A.course = S.course.as<double>(); A.log = d_rows.as<double>();
  A.last = d_last.as<double>(); A.keep = d_keep.as<uint64_t>();
  A.round_span = round_span;
  double ms = 0.0;
  if ((rc = replan_launch(h, S, nullptr, A, slots, &ms))) return rc;
  h->last_ms = ms; h->last_grid = n_states; h->last_block = 64; h->last_lds = 0;
  memcpy(out, S.rec_host.data(), (size_t)n_states * sizeof(auvp::ReplanRecord));
  HIPCHK(h, hipMemcpyAsync(last7, d_last.p, (size_t)n_states * auvp::REPLAN_ROW * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(keep, d_keep.p, (size_t)n_states * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
  if (total) HIPCHK(h, hipMemcpyAsync(rows_out, d_rows.p, (size_t)total * auvp::REPLAN_ROW * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  S.bytes_to_host += (long long)((size_t)n_states * (auvp::REPLAN_ROW * sizeof(double) + sizeof(uint64_t)) +
                                 (size_t)total * auvp::REPLAN_ROW * sizeof(double));
  return AUVP_OK;
}

int auvp_replan_info(auvp_handle* h, int32_t* n_auvs, int32_t* rounds, int64_t* rows, int64_t* bytes_to_host, int64_t* bytes_traj,
                     double* commit_ms) {
  if (!h) return AUVP_ERR_ARG;
  const ReplanState* S = static_cast<const ReplanState*>(h->replan);
  if (n_auvs) *n_auvs = S ? S->n_auvs : 0;
  if (rounds) *rounds = S ? S->rounds : 0;
  if (rows) *rows = S ? S->rows_committed : 0;
  if (bytes_to_host) *bytes_to_host = S ? S->bytes_to_host : 0;
  if (bytes_traj) *bytes_traj = S ? S->bytes_traj : 0;
  if (commit_ms) *commit_ms = S ? S->commit_ms : 0.0;
  return AUVP_OK;
}

}  // extern "C"
#endif  // AUVP_REPLAN_HOST_H

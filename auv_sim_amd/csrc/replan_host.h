// replan_host.h -- host side of the device commit step of RRT.replanning_batch (auvp_replan_*, include/auvplan.h): the fleet's
// state on the handle (last [n,7], keep [n], the trajectory log, the teams), the launch of rrt_commit_kernel (replan_kernels.hip)
// behind auvp_rrt_group_best and of replan_team_kernel behind it where the fleet has teams, the one download at the end, and the
// probe entries that run the kernels' rules on the caller's courses and masks.
// Every index the kernel uses is computed here from host data: the group records' host copy (h->group_best) sizes the course
// scratch and the round's log space before the launch.
// Included at the end of auvplan.hip.
#ifndef AUVP_REPLAN_HOST_H
#define AUVP_REPLAN_HOST_H
#include "replan_commit.h"
#include "replan_teams.h"

extern "C" hipError_t auvpi_replan_team_launch(const auvp::ReplanTeamDev* T, hipStream_t stream);
extern "C" hipError_t auvpi_replan_commit_launch(const auvp::RrtBuffers* B, const auvp::ReplanCommitDev* A, int n_episodes, hipStream_t stream);
extern "C" hipError_t auvpi_replan_gather_launch(const auvp::ReplanSegment* seg, int n_seg, const double* log, double* out, hipStream_t stream);

static_assert(sizeof(auvp_replan_record) == sizeof(auvp::ReplanRecord), "round record layout");

namespace {

struct ReplanState {
  int n_auvs = 0;  // 0: auvp_replan_begin not called
  DevBuf last, keep, log, course, slots, rec, seg, traj;
  long long log_rows = 0;                  // rows of the log reserved so far (each round: the sum of its winners' path_len)
  long long rows_committed = 0;            // rows of the log in use
  int rounds = 0;
  std::vector<long long> auv_rows;         // [n_auvs] rows committed per AUV
  struct Piece { int32_t auv, n; int64_t src; };
  std::vector<Piece> pieces;               // in round order
  std::vector<auvp::ReplanRecord> rec_host;
  long long bytes_to_host = 0, bytes_traj = 0;
  double commit_ms = 0.0;                  // rrt_commit_kernel's time (with teams: and replan_team_kernel's), summed over the rounds
  // the fleet's teams (auvp_replan_set_teams): the CSR of replan_teams.h in HBM; n_teams == 0: none, nothing more is launched
  int n_teams = 0;
  DevBuf team_off, team_members, slot_of;
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
  S.bytes_to_host = S.bytes_traj = 0;
  S.commit_ms = 0.0;
  S.n_teams = 0;  // (the teams were the old fleet's)
  S.n_auvs = n_auvs;
  return AUVP_OK;
}

int auvp_replan_set_teams(auvp_handle* h, int32_t n_auvs, const int32_t* team_of) {
  if (!h) return AUVP_ERR_ARG;
  ReplanState* Sp = static_cast<ReplanState*>(h->replan);
  if (!Sp || Sp->n_auvs < 1) return fail(h, AUVP_ERR_STATE, "auvp_replan_begin not called");
  ReplanState& S = *Sp;
  if (n_auvs != S.n_auvs) return fail(h, AUVP_ERR_ARG, "n_auvs %d, the fleet has %d", n_auvs, S.n_auvs);
  if (!team_of) { S.n_teams = 0; return AUVP_OK; }
  const auvp::ReplanTeamCsr csr = auvp::replan_team_csr(team_of, n_auvs);
  if (csr.n_teams() == 0) { S.n_teams = 0; return AUVP_OK; }
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
  std::vector<char> seen((size_t)S.n_auvs, 0);
  for (int g = 0; g < G; g++) {
    const int a = auv_of[g];
    if (a < 0 || a >= S.n_auvs) return fail(h, AUVP_ERR_ARG, "group %d: AUV %d outside [0, %d)", g, a, S.n_auvs);
    if (seen[(size_t)a]) return fail(h, AUVP_ERR_ARG, "AUV %d is named twice", a);
    seen[(size_t)a] = 1;
  }
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
  int rc;
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
    if (n) S.pieces.push_back(ReplanState::Piece{slots[(size_t)g].auv, n, slots[(size_t)g].log_off});
    S.auv_rows[(size_t)slots[(size_t)g].auv] += n;
    S.rows_committed += n;
  }
  S.log_rows += total;
  S.rounds++;
  S.commit_ms += ms;
  h->last_ms = ms; h->last_grid = G; h->last_block = 64; h->last_lds = 0;
  if (out) memcpy(out, S.rec_host.data(), (size_t)G * sizeof(auvp::ReplanRecord));
  return AUVP_OK;
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
  if (course_off[0] != 0) return fail(h, AUVP_ERR_ARG, "course_off[0] != 0");
  for (int i = 0; i < n_states; i++)
    if (course_off[i + 1] < course_off[i] || course_off[i + 1] - course_off[i] > 0x7fffffffll)
      return fail(h, AUVP_ERR_ARG, "course_off is not an ascending list of row offsets");
  const long long total = course_off[n_states];
  if (total > 0 && (!courses || !rows_out)) return fail(h, AUVP_ERR_ARG, "courses / rows_out is null");
  HIPCHK(h, hipSetDevice(h->device));
  ReplanState& S = *replan_of(h);
  // the probe's own state arrays and row buffer: the fleet's (auvp_replan_begin) stay as they are
  DevBuf d_last, d_keep, d_rows;
  int rc;
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

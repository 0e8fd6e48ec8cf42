// drain_standing.cpp -- what the seven trackers share (drain_impl.hpp; DESIGN.md
// §5.5i "The tracker lifecycle"): ps_load_track, ps_hops_track,
// ps_downstream_track, ps_cut_track, ps_report_track, ps_blame_track and
// ps_spread_track each keep one Drain::Standing, and everything that does not depend on what a
// family computes goes through here -- registering topics, a run's pinned
// staging, the front and the back of a window's pass, the take of the totals.
// A family's own file holds its kernels' pass, its input block and its key's
// own words, and nothing of the lifecycle.
#include "drain_impl.hpp"

namespace psamd {

using Standing = Drain::Standing;

namespace {

std::string standing_msg(const char* pre, const Standing& S, const char* post) { return std::string(pre) + S.name + post; }

// The last pass over the window's rows on `stream` (run.cpp: drain_fence),
// recorded behind it: the entry of this row set, else one whose row set is gone
int pass_fence(ps_engine* e, Standing& S) {
  Drain::PassFence* F = nullptr;
  for (auto& f : S.fence)
    if (f.seen == e->rows.seen.p) F = &f;
  for (auto& f : S.fence)
    if (!F && (!f.seen || f.seen != e->rows_other.seen.p)) F = &f;
  if (!F) return e->fail(PS_E_STATE, standing_msg("", S, ": no fence entry for the row set"));
  if (!F->ev) HIP_TRY(hipEventCreateWithFlags(&F->ev, kStreamEvent), "pass event");
  HIP_TRY(hipEventRecord(F->ev, e->stream), "event");
  F->seen = e->rows.seen.p;
  F->pending = true;
  return PS_OK;
}

// A run's pinned staging for a standing pass: run k takes arena[k & 1], folded
// into one chunk where the windows of its last run outgrew it
int pass_arena_open(ps_engine* e, Standing& S) {
  HIP_TRY(hipSetDevice(e->cfg.device), "hipSetDevice");
  auto& A = S.arena[S.runs++ & 1];
  // the arena's last run lies two back: its passes have left the staging, or do so soon
  if (A.pending) HIP_TRY(hipEventSynchronize(A.ev), "wait for a standing pass");
  A.pending = false;
  auto& R = A.mem;
  if (R.arena.size() > 1) {
    size_t cap = 0;
    for (auto& c : R.arena) {
      cap += c.cap;
      (void)hipHostFree(c.h);
    }
    R.arena.clear();
    uint8_t* h = nullptr;
    R.arena_used = 0;
    HIP_TRY(sink_stage(R, cap, &h), "alloc pass staging");
  }
  R.arena_used = 0;
  if (!A.ev) HIP_TRY(hipEventCreateWithFlags(&A.ev, hipEventDisableTiming), "pass event");
  S.open = &A;
  return PS_OK;
}

}  // namespace

// ---- around a run (run.cpp) ------------------------------------------------------

int standing_open(ps_engine* e, Standing& S) { return S.on ? pass_arena_open(e, S) : PS_OK; }

void standing_abort(ps_engine* e, Standing& S) {
  if (!S.open) return;
  // what the run's windows staged must have left the staging
  (void)hipStreamSynchronize(e->stream);
  S.open = nullptr;
}

void standing_settled(Standing& S) {
  for (auto& f : S.fence) f.pending = false;
  for (auto& a : S.arena) a.pending = false;
}

void standing_destroy(Standing& S) {
  for (auto& a : S.arena) {
    for (auto& c : a.mem.arena) (void)hipHostFree(c.h);
    if (a.ev) (void)hipEventDestroy(a.ev);
  }
  for (auto& f : S.fence)
    if (f.ev) (void)hipEventDestroy(f.ev);
  if (S.ev_take) (void)hipEventDestroy(S.ev_take);
}

// ---- ps_*_track ------------------------------------------------------------------

int standing_track_check(ps_engine* e, const Standing& S, const uint32_t* topic, size_t n) {
  if (e->world > 1) return e->fail(PS_E_STATE, standing_msg("ps_", S, "_track on a multi-rank engine"));
  if (e->infl_count) return e->fail(PS_E_STATE, "a run in flight: ps_wait first");
  return aud_check_topics(e, topic, n);
}

int standing_quiesce(ps_engine* e, Standing& S) {
  HIP_TRY(hipSetDevice(e->cfg.device), "hipSetDevice");
  if (S.runs) HIP_TRY(hipStreamSynchronize(e->stream), "sync");
  return PS_OK;
}

void standing_retrack(Standing& S, const uint32_t* topic, size_t n) {
  standing_settled(S);
  S.open = nullptr;
  S.strip_key.clear();
  S.windows = S.skipped = 0;
  S.topic.assign(topic, topic + n);
  S.on = n > 0;
}

int standing_totals(ps_engine* e, Standing& S, DevBuf& d_acc, size_t bytes, std::initializer_list<DevBuf*> pass) {
  if (!S.on) {
    d_acc.release();
    release_all(pass);
    return PS_OK;
  }
  HIP_TRY(d_acc.ensure(bytes), standing_msg("alloc ", S, " totals").c_str());
  HIP_TRY(hipMemsetAsync(d_acc.p, 0, bytes, e->stream), standing_msg("clear ", S, " totals").c_str());
  return PS_OK;
}

// ---- ps_*_take -------------------------------------------------------------------

int standing_take_enter(ps_engine* e, const Standing& S) {
  if (!S.on) return e->fail(PS_E_NOTREADY, standing_msg("no ", S, " pass is tracked"));
  if (e->infl_count) return e->fail(PS_E_STATE, "a run in flight: ps_wait first");
  HIP_TRY(hipSetDevice(e->cfg.device), "hipSetDevice");
  return PS_OK;
}

int standing_take_event(ps_engine* e, Standing& S) {
  if (!S.ev_take) HIP_TRY(hipEventCreateWithFlags(&S.ev_take, hipEventDisableTiming), standing_msg("", S, " event").c_str());
  return PS_OK;
}

int standing_take_totals(ps_engine* e, Standing& S, DevBuf& d_acc, Drain::Answer& A, size_t bytes) {
  if (const int rc = standing_take_enter(e, S)) return rc;
  HIP_TRY(pinned_ensure(&A.h_out, nullptr, &A.out_cap, bytes), standing_msg("alloc ", S, " view").c_str());
  if (const int rc = standing_take_event(e, S)) return rc;
  // every pass ran on `stream`: the copy behind them, the clearing behind the
  // copy and in front of whatever runs next, one wait
  hipStream_t s = e->stream;
  HIP_TRY(hipMemcpyAsync(A.h_out, d_acc.p, bytes, hipMemcpyDeviceToHost, s), standing_msg("read ", S, " totals").c_str());
  HIP_TRY(hipMemsetAsync(d_acc.p, 0, bytes, s), standing_msg("clear ", S, " totals").c_str());
  HIP_TRY(hipEventRecord(S.ev_take, s), "event");
  HIP_TRY(hipEventSynchronize(S.ev_take), standing_msg("wait for the ", S, " totals").c_str());
  standing_settled(S);
  return PS_OK;
}

// ---- a window's pass (the families' *_window hooks) -------------------------------

int standing_window_begin(ps_engine* e, Standing& S, Drain::Sink::Res** R) {
  *R = &S.open->mem;
  if (const int rj = twin_join(e)) return rj;
  // (no drain_ready: the passes read no host mirror of the node space, so a
  // GPU-built one is not read back for them)
  size_t used = 0;
  uint8_t* h = nullptr;
  return drain_tables_async(e, Staging{nullptr, *R}, 0, false, &used, &h);
}

uint32_t standing_key_topic(ps_engine* e, uint32_t t, std::vector<uint64_t>* key) {
  const DrainTopic& T = e->drain.tab.topics[t];
  uint32_t u0 = 0;
  const uint32_t nn = aud_nodes(e, t, &u0);
  key->push_back(static_cast<uint64_t>(T.flags) << 32 | T.n_pos);
  key->push_back(static_cast<uint64_t>(nn) << 32 | e->last_topics[t].nbase);
  return u0;
}

int standing_window_done(ps_engine* e, Standing& S, size_t n_skipped) {
  // classify and the counted rows read the window's row set: the events are
  // recorded whether or not a row was read
  if (const int rc = pass_fence(e, S)) return rc;
  HIP_TRY(hipEventRecord(S.open->ev, e->stream), "event");
  S.open->pending = true;
  S.windows += 1;
  S.skipped += n_skipped;
  return PS_OK;
}

}  // namespace psamd

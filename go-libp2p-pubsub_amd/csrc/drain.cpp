// drain.cpp -- the plain drain (drain_impl.hpp):
// ps_drain, ps_drain_begin / ps_drain_end, and the two slots the asynchronous
// calls of every kind (this one, ps_drain_shared_begin, ps_drain_topics_begin)
// wait in.
#include "drain_impl.hpp"

using namespace psamd;

namespace {

// The slot the next asynchronous drain takes, its events made
int drain_next_slot(ps_engine* e, Drain::Slot** out) {
  auto& D = e->drain;
  auto& S = D.slot[(D.slot_head + D.slot_count) & 1];
  if (!S.ev_emit) {
    HIP_TRY(hipEventCreateWithFlags(&S.ev_emit, kStreamEvent), "drain event");
    // (the host reads the view after ev_done: it keeps the system-scope release)
    HIP_TRY(hipEventCreateWithFlags(&S.ev_done, hipEventDisableTiming), "drain event");
  }
  *out = &S;
  return PS_OK;
}

}  // namespace

// ---- what the two asynchronous forms share around their slots ------------------

namespace psamd {

// A begin call behind its state checks: it joins the twin (behind the last
// launch of the window: `stream` follows a twin's tstream), takes the next
// slot and has the window's tables on the device, with `tail` bytes of the
// slot's staging at *tail_out for its own input (drain_tables_async).  From
// here to the slot's taking a failure gives the slot up (drain_give_up).
int drain_begin_slot(ps_engine* e, size_t tail, bool timed, Drain::Slot** slot, size_t* used, uint8_t** tail_out) {
  if (const int rj = twin_join(e)) return rj;
  if (const int rc = drain_ready(e)) return rc;
  if (const int rc = drain_next_slot(e, slot)) return rc;
  return drain_tables_async(e, Staging{*slot, nullptr}, tail, timed, used, tail_out);
}

// A begin call fails between drain_tables_async and the taking of its slot:
// a table block staged in the slot's memory (`staged`) must have left it
// before the next begin writes there
int drain_give_up(ps_engine* e, bool staged, int code, const char* what) {
  if (staged) HIP_TRY(hipStreamSynchronize(e->stream), "sync");
  return e->fail(code, what);
}

// The slot is taken with a view the host wrote.  Nothing of it is on the GPU
// but a table block it staged: the end call then waits for that upload.
int drain_slot_host_view(ps_engine* e, Drain::Slot& S, bool staged) {
  if (staged) {
    HIP_TRY(hipEventRecord(S.ev_done, e->stream), "event");
    S.enqueued = true;
  }
  ++e->drain.slot_count;
  return PS_OK;
}

// What an end call returns for the error and overflow words of its view
int drain_view_status(ps_engine* e, uint64_t err, uint32_t over) {
  if (err)
    return e->fail(PS_E_STATE, err & kDrainErrBit ? "drain tables: a window message bit past the row or shared"
                                                  : "drain tables: row bits do not ascend in arrival order");
  if (over)
    return e->fail(PS_E_RANGE, over & kDrainOverExc     ? "more exceptions than exc_cap"
                               : over & kDrainOverLists ? "more lists than list_cap"
                                                        : "more ids than id_cap");
  return PS_OK;
}

// An asynchronous drain's last steps, behind its last kernel on `stream`:
// that kernel is the last reader of the window's rows (run.cpp: drain_fence);
// the slot is taken; the view leaves on the copy stream, beside whatever
// `stream` runs next (to_host), or was written in place (mapped memory).
int drain_slot_enqueued(ps_engine* e, Drain::Slot& S, size_t res_bytes, bool to_host) {
  auto& D = e->drain;
  hipStream_t s = e->stream;
  HIP_TRY(hipEventRecord(S.ev_emit, s), "event");
  S.seen = e->rows.seen.p;
  S.emit_pending = true;
  S.enqueued = true;
  ++D.slot_count;
  if (!to_host) {
    HIP_TRY(hipEventRecord(S.ev_done, s), "event");
  } else {
    HIP_TRY(hipStreamWaitEvent(D.copy_stream, S.ev_emit, 0), "wait");
    HIP_TRY(hipMemcpyAsync(S.h_res, S.d_res.p, res_bytes, hipMemcpyDeviceToHost, D.copy_stream), "read drain view");
    HIP_TRY(hipEventRecord(S.ev_done, D.copy_stream), "event");
  }
  return PS_OK;
}

// The oldest slot leaves the queue; its view is complete on return
int drain_slot_complete(ps_engine* e, Drain::Slot& S) {
  auto& D = e->drain;
  D.slot_head ^= 1;
  --D.slot_count;
  if (S.enqueued) {
    HIP_TRY(hipEventSynchronize(S.ev_done), "wait for the drain");
    S.emit_pending = false;
    S.enqueued = false;
  }
  return PS_OK;
}

}  // namespace psamd

extern "C" {

// ---- ps_drain -----------------------------------------------

int ps_drain(ps_engine* e, const uint32_t* topic, const uint32_t* peer, size_t n, uint64_t* off_out, uint32_t* msg_out,
             size_t cap, uint64_t* total_out) {
  if (!e || !off_out || !total_out || (n && (!topic || !peer)) || (cap && !msg_out)) return PS_E_INVAL;
  if (const int rc = drain_enter(e, {nullptr, "no completed run", nullptr, true}, topic, peer, n)) return rc;
  off_out[0] = 0;
  *total_out = 0;
  if (n == 0) return PS_OK;
  if (n >= 0xFFFFFFFFull) return e->fail(PS_E_RANGE, "too many queries");
  auto& D = e->drain;
  // (PSAMD_DRAIN_TIMING: the host phases of the call, the first after a window above all)
  double host_ms[3] = {0, 0, 0};  // node-space mirrors, table build + upload, queries (peer maps)
  auto h0 = hclock::now();
  int rc = drain_ready(e);
  host_ms[0] = ms_since(h0);
  h0 = hclock::now();
  const bool tables_built = D.tab.seq != e->window_seq;
  if (!rc) rc = drain_tables(e);
  host_ms[1] = ms_since(h0);
  if (rc) return rc;
  hipStream_t s = e->stream;
  h0 = hclock::now();
  D.sync.queries.resize(n);
  const uint64_t n_segs64 = drain_resolve(e, topic, peer, n, D.sync.queries.data(), nullptr);
  if (n_segs64 >= kDrainRowLimit) return e->fail(PS_E_RANGE, "too many rows in one drain");
  const uint32_t n_segs = static_cast<uint32_t>(n_segs64);
  host_ms[2] = ms_since(h0);
  D.sync.off.assign(static_cast<size_t>(n_segs) + 1, 0);
  float ms[4] = {0, 0, 0, 0};  // count, scan, emit, copy (PSAMD_DRAIN_TIMING)
  const PhaseTimer tm{D.ev_t, s, D.env.timing};
  DrainArgs a = drain_args(e, D.tab);
  auto& B = D.sync.scratch;
  if (n_segs) {
    if ((rc = drain_count_scan(e, a, n_segs, B, D.sync.queries.data(), n, s, tm, ms[0]))) return rc;
    HIP_TRY(tm.end(ms[1]), "event");
    HIP_TRY(hipMemcpyAsync(D.sync.off.data(), B.d_off.p, (static_cast<size_t>(n_segs) + 1) * 8, hipMemcpyDeviceToHost, s),
            "read drain offsets");
    HIP_TRY(hipStreamSynchronize(s), "sync");
  }
  const uint64_t total = D.sync.off[n_segs];
  for (size_t q = 0; q < n; ++q) off_out[q] = D.sync.off[D.sync.queries[q].seg0];
  off_out[n] = total;
  *total_out = total;
  if (total > cap) {
    if (D.env.timing)
      std::fprintf(stderr, "psamd drain: queries %zu sizing host_mirrors_ms %.4f host_tables_ms %.4f (%s) host_queries_ms %.4f\n",
                   n, host_ms[0], host_ms[1], tables_built ? "built" : "kept", host_ms[2]);
    return e->fail(PS_E_RANGE, "output buffer too small");
  }

  // emit, slab by slab: the segments [lo, hi) whose ids fit one slab; slab k
  // is copied out on the copy stream while slab k + 1 is emitted
  const uint64_t slab = std::min<uint64_t>(D.env.slab_ids, std::max<uint64_t>(total, 1));
  // both slabs, sized once (behind the copies of an earlier drain: all complete)
  for (DevBuf& buf : D.sync.d_slab) HIP_TRY(buf.ensure(slab * 4), "alloc drain slab");
  uint64_t pend_base = 0, pend_len = 0;  // the slab emitted last, not yet copied
  uint32_t lo = 0, k = 0;  // k: slabs emitted; slab j lives in d_slab[j & 1]
  // slab j's copy: behind its emit, on the copy stream (timing: in line)
  auto copy_out = [&](uint32_t j) -> int {
    hipStream_t cs = D.env.timing ? s : D.copy_stream;
    if (!D.env.timing) HIP_TRY(hipStreamWaitEvent(cs, D.sync.ev_emit[j & 1], 0), "wait");
    HIP_TRY(tm.begin(), "event");
    HIP_TRY(hipMemcpyAsync(msg_out + pend_base, D.sync.d_slab[j & 1].p, pend_len * 4, hipMemcpyDeviceToHost, cs),
            "read drain slab");
    HIP_TRY(tm.end(ms[3]), "event");
    HIP_TRY(hipEventRecord(D.sync.ev_copy[j & 1], cs), "event");
    return PS_OK;
  };
  while (lo < n_segs && D.sync.off[lo] < total) {
    const uint64_t base = D.sync.off[lo];
    const uint32_t hi =
        static_cast<uint32_t>(std::upper_bound(D.sync.off.begin() + lo, D.sync.off.end(), base + slab) - D.sync.off.begin()) - 1;
    // (a segment holds at most kDrainSegBits <= slab ids, or all that is left: hi > lo)
    if (hi <= lo) return e->fail(PS_E_STATE, "drain slab smaller than a segment");
    const uint64_t len = D.sync.off[hi] - base;
    HIP_TRY(hipStreamWaitEvent(s, D.sync.ev_copy[k & 1], 0), "wait");  // (slab k - 2 has left the buffer)
    HIP_TRY(tm.begin(), "event");
    HIP_TRY(launch_drain_emit(a, lo, hi, B.d_off.as<uint64_t>(), base, D.sync.d_slab[k & 1].as<uint32_t>(), len, D.env.staged, s),
            "k_drain_emit");
    HIP_TRY(tm.end(ms[2]), "event");
    HIP_TRY(hipEventRecord(D.sync.ev_emit[k & 1], s), "event");
    if (k)  // the slab before goes out while this one is emitted
      if (const int rcc = copy_out(k - 1)) return rcc;
    pend_base = base;
    pend_len = len;
    ++k;
    lo = hi;
  }
  if (k)
    if (const int rcc = copy_out(k - 1)) return rcc;
  HIP_TRY(hipStreamSynchronize(D.copy_stream), "sync");
  HIP_TRY(hipStreamSynchronize(s), "sync");
  if (D.env.timing)
    std::fprintf(stderr,
                 "psamd drain: queries %zu segments %u ids %llu slabs %u emit %s count_ms %.4f scan_ms %.4f emit_ms %.4f "
                 "copy_ms %.4f host_mirrors_ms %.4f host_tables_ms %.4f (%s) host_queries_ms %.4f\n",
                 n, n_segs, static_cast<unsigned long long>(total), k, D.env.staged ? "lds" : "direct", ms[0], ms[1], ms[2],
                 ms[3], host_ms[0], host_ms[1], tables_built ? "built" : "kept", host_ms[2]);
  return PS_OK;
}

// ---- ps_drain_begin / ps_drain_end -------------------------

int ps_drain_begin(ps_engine* e, const uint32_t* topic, const uint32_t* peer, size_t n) {
  if (!e || (n && (!topic || !peer))) return PS_E_INVAL;
  if (const int rc = drain_enter(e, {"ps_drain_begin on a multi-rank engine: use ps_drain", "no run enqueued",
                                    "two drains outstanding: ps_drain_end first", false},
                                topic, peer, n))
    return rc;
  if (n >= 0x7FFFFFFFull) return e->fail(PS_E_RANGE, "too many queries");
  auto& D = e->drain;
  const auto t_host0 = hclock::now();
  Drain::Slot* slot = nullptr;
  size_t used = 0;
  uint8_t* h = nullptr;
  int rc = drain_begin_slot(e, align256(n * sizeof(DrainQuery)), D.env.timing, &slot, &used, &h);
  if (rc) return rc;
  auto& S = *slot;
  hipStream_t s = e->stream;
  // (written once the tables stand, not before their build: nothing reads a slot that is not taken)
  S.n = n;
  S.kind = Drain::Slot::kPlain;

  // the queries, resolved straight into the slot's staging behind the tables
  DrainQuery* hq = reinterpret_cast<DrainQuery*>(h);
  uint64_t bound = 0;
  const uint64_t n_segs64 = drain_resolve(e, topic, peer, n, hq, &bound);
  if (n_segs64 >= kDrainRowLimit || bound > kDrainAsyncMaxIds)
    return drain_give_up(e, used, PS_E_RANGE, n_segs64 >= kDrainRowLimit ? "too many rows in one drain"
                                                                         : "drain may exceed 2^30 ids: use ps_drain");
  const uint32_t n_segs = static_cast<uint32_t>(n_segs64);
  S.hdr_bytes = align256((n + 2) * 8);
  S.bound = bound;
  const size_t res_bytes = S.hdr_bytes + bound * 4;
  HIP_TRY(pinned_ensure(&S.h_res, &S.h_res_dev, &S.res_cap, res_bytes), "alloc drain view");
  S.enqueued = false;
  if (n_segs == 0) {  // nothing to read: the view is n + 1 zeros
    std::memset(S.h_res, 0, (n + 2) * 8);
    return drain_slot_host_view(e, S, used);
  }
  if (!D.env.mapped_out) HIP_TRY(S.d_res.ensure(res_bytes), "alloc drain result");
  DrainArgs a = drain_args(e, D.tab);
  const PhaseTimer untimed{D.ev_t, s, false};  // (nothing here may wait for the stream)
  float none = 0;
  if ((rc = drain_count_scan(e, a, n_segs, S.lb.scratch, hq, n, s, untimed, none))) return rc;
  uint8_t* res = D.env.mapped_out ? S.h_res_dev : S.d_res.as<uint8_t>();
  if ((rc = drain_err_word(e, s))) return rc;
  const uint64_t* seg_off = S.lb.scratch.d_off.as<uint64_t>();
  HIP_TRY(launch_drain_offsets(a.queries, a.n_queries, seg_off, n_segs, D.tab.d_err, reinterpret_cast<uint64_t*>(res), s),
          "k_drain_offsets");
  HIP_TRY(launch_drain_emit(a, 0, n_segs, seg_off, 0, reinterpret_cast<uint32_t*>(res + S.hdr_bytes), bound, true, s),
          "k_drain_emit");
  if ((rc = drain_slot_enqueued(e, S, res_bytes, !D.env.mapped_out))) return rc;
  if (D.env.timing)
    std::fprintf(stderr, "psamd drain_begin: queries %zu segments %u bound %llu tables %s out %s host_us %.1f\n", n, n_segs,
                 static_cast<unsigned long long>(bound), used ? "built" : "kept", D.env.mapped_out ? "mapped" : "copy",
                 1e3 * ms_since(t_host0));
  return PS_OK;
}

int ps_drain_end(ps_engine* e, const uint64_t** off_out, const uint32_t** msg_out, uint64_t* total_out) {
  if (!e || !off_out || !msg_out || !total_out) return PS_E_INVAL;
  auto& D = e->drain;
  if (D.slot_count == 0) return e->fail(PS_E_NOTREADY, "no drain outstanding");
  auto& S = D.slot[D.slot_head];
  if (S.kind != Drain::Slot::kPlain)
    return e->fail(PS_E_STATE, S.kind == Drain::Slot::kShared ? "the oldest drain is a shared one: ps_drain_shared_end"
                                                               : "the oldest drain is a topics one: ps_drain_topics_end");
  if (const int rc = drain_slot_complete(e, S)) return rc;
  const uint64_t* hdr = reinterpret_cast<const uint64_t*>(S.h_res);
  *off_out = hdr;
  *msg_out = reinterpret_cast<const uint32_t*>(S.h_res + S.hdr_bytes);
  *total_out = hdr[S.n];
  if (const int rc = drain_view_status(e, hdr[S.n + 1], 0)) return rc;
  if (hdr[S.n] > S.bound) return e->fail(PS_E_STATE, "drain total above its bound");
  return PS_OK;
}

}  // extern "C"

// drain_blame_track.cpp -- blame records behind every window (drain_impl.hpp;
// DESIGN.md §5.5s): ps_blame_track registers standing tree topics whose blame
// pass run.cpp's hooks enqueue behind every window of a run; ps_blame_take
// lends everything since the last take.  A window's pass is ps_topic_blame's
// (drain_blame.cpp) as far as the scan -- the downstream pass's plan and front
// (down_window_stage, down_front), k_blame_top and one k_blame_level launch per
// level backwards, k_blame_count, the scan -- and then places its records where
// a cursor on the device stands: k_blame_track_commit writes the window's row
// of the run's rec_off and moves the cursor on, k_blame_track_emit stores the
// records from the window's base.  Stream order is the only order between the
// launches; nothing waits.  Buffers of its own.
#include "drain_impl.hpp"

using namespace psamd;

namespace {

using Track = Drain::BlameTrack;

// A device buffer of the run's records grown with its contents kept: the
// windows before have written there, on s.  (Not the steady state: the next
// take-to-take interval of the same shape finds the room.)
int blame_grow(ps_engine* e, DevBuf& buf, size_t need, hipStream_t s) {
  if (need <= buf.bytes) return PS_OK;
  DevBuf nb;
  HIP_TRY(nb.ensure(std::max(need, 2 * buf.bytes)), "alloc blame records");
  if (buf.bytes) {
    HIP_TRY(hipMemcpyAsync(nb.p, buf.p, buf.bytes, hipMemcpyDeviceToDevice, s), "move blame records");
    HIP_TRY(hipStreamSynchronize(s), "sync");
  }
  buf.swap(nb);
  return PS_OK;
}

void blame_release(Track& T) {
  auto& P = T.track;
  release_all({&P.d_in, &P.d_verdict, &P.d_exc, &P.d_full, &P.d_scratch, &T.d_cut, &T.d_cnt, &T.d_off, &T.d_scan, &T.d_map,
               &T.d_cur, &T.d_rec_off, &T.d_rec[0], &T.d_rec[1], &T.d_rec[2], &T.d_rec[3], &T.d_rec[4]});
}

}  // namespace

// ---- the standing pass's window hook (run.cpp calls it) --------------------------

// The window just remembered, its records appended: the block as cut_window
// stages its own, the map from request position to the entry behind it, the
// room for the window's row of offsets and for the records the cap in effect
// allows, then the pass.  All on `stream`; nothing waits but a buffer that grows.
int psamd::blame_window(ps_engine* e) {
  auto& D = e->drain;
  auto& T = D.blame_trk;
  auto& H = T.st;
  if (!H.on || !H.open) return PS_OK;
  const auto t_host0 = hclock::now();
  Down::Shape K;
  size_t n_tree = 0;
  int rc = down_window_stage(e, H, T.track, T.kept, &K, &n_tree);
  if (rc) return rc;
  hipStream_t s = e->stream;
  const size_t n = H.topic.size();
  const uint64_t w = H.windows;
  if ((w + 1) * n + 1 >= (1ull << 32)) return e->fail(PS_E_RANGE, "too many rows between two ps_blame_take");

  // a window's row is indexed by request position, the entry table by tree
  // topic: the tree topics among the positions [0, i]
  uint8_t* hm = nullptr;
  HIP_TRY(sink_stage(H.open->mem, n * 4, &hm), "alloc blame staging");
  uint32_t* const ent = reinterpret_cast<uint32_t*>(hm);
  uint32_t behind = 0;
  for (size_t i = 0; i < n; ++i) {
    behind += !hops_is_mesh(e, H.topic[i]);
    ent[i] = behind;
  }
  if (behind != n_tree) return e->fail(PS_E_STATE, "blame: the entries are not the window's tree topics");
  HIP_TRY(hipMemcpyAsync(T.d_map.p, hm, n * 4, hipMemcpyHostToDevice, s), "upload blame positions");

  // the engine's own cap: every node with a row to classify may lack a
  // message, kAudPrefix a window at most, summed as the windows come
  if (!T.rec_cap) {
    T.cap += K.ns ? std::min<uint64_t>(K.n_verdicts, kAudPrefix) : 0;
    if (T.cap > (1ull << 30)) return e->fail(PS_E_RANGE, "more than 2^30 blame records between two ps_blame_take");
    for (auto& b : T.d_rec)
      if ((rc = blame_grow(e, b, T.cap * 4, s))) return rc;
  }
  if ((rc = blame_grow(e, T.d_rec_off, ((w + 1) * n + 1) * 8, s))) return rc;

  float ms[5] = {0, 0, 0, 0, 0};  // classify, weights, sweep, count + scan, commit + emit (PSAMD_DRAIN_TIMING)
  // (the events are the pass's own: no blocking call need have created the drain's)
  for (auto& ev : T.ev_t)
    if (D.env.timing && !ev) HIP_TRY(hipEventCreate(&ev), "blame event");
  const PhaseTimer tm{T.ev_t, s, D.env.timing};
  const double host_ms = ms_since(t_host0);
  BlameArgs g{};
  BlameTrack t{};
  t.cur = T.d_cur.as<BlameCursor>();
  t.ent = T.d_map.as<uint32_t>();
  t.rec_off = T.d_rec_off.as<uint64_t>();
  t.w = w;
  t.cap = T.cap;
  t.n_req = static_cast<uint32_t>(n);
  if (K.ns) {
    const size_t n_off = static_cast<size_t>(K.ns) + 1;
    HIP_TRY(T.d_cnt.ensure(n_off * 8), "alloc blame counts");
    HIP_TRY(T.d_off.ensure(n_off * 8), "alloc blame offsets");
    HIP_TRY(T.d_cut.ensure(K.n_nodes * 8), "alloc blame words");
    size_t scan_bytes = 0;
    HIP_TRY(drain_scan(nullptr, &scan_bytes, T.d_cnt.as<uint64_t>(), T.d_off.as<uint64_t>(), K.ns + 1, s), "size blame scan");
    HIP_TRY(T.d_scan.ensure(scan_bytes), "alloc blame scan");
    if ((rc = down_front(e, T.track, T.track.d_in.as<uint8_t>(), K, tm, ms, &g.d))) return rc;
    g.cut_node = T.d_cut.as<uint32_t>();
    g.cut_level = g.cut_node + K.n_nodes;
    g.n_rec = T.d_cnt.as<uint64_t>();
    g.off = T.d_off.as<uint64_t>();
    g.rec_peer = T.d_rec[0].as<uint32_t>();
    g.rec_cut_peer = T.d_rec[1].as<uint32_t>();
    g.rec_hop = T.d_rec[2].as<uint32_t>();
    g.rec_cut_hop = T.d_rec[3].as<uint32_t>();
    g.rec_missed = T.d_rec[4].as<uint32_t>();
    HIP_TRY(tm.begin(), "event");
    HIP_TRY(launch_blame_top(g, s), "k_blame_top");
    // (the bottom-up order backwards: every entry's level `top` first)
    for (size_t j = K.launch.size(); j-- > 1;) HIP_TRY(launch_blame_level(g, K.launch[j - 1], K.launch[j], s), "k_blame_level");
    HIP_TRY(tm.end(ms[2]), "event");
    HIP_TRY(tm.begin(), "event");
    HIP_TRY(launch_blame_count(g, s), "k_blame_count");
    scan_bytes = T.d_scan.bytes;
    HIP_TRY(drain_scan(T.d_scan.p, &scan_bytes, g.n_rec, T.d_off.as<uint64_t>(), K.ns + 1, s), "blame scan");
    HIP_TRY(tm.end(ms[3]), "event");
  }
  // (no row to read: g.d.n_strips is 0, the row repeats the base and the cursor moves on by a window)
  HIP_TRY(tm.begin(), "event");
  HIP_TRY(launch_blame_track_commit(g, t, s), "k_blame_track_commit");
  HIP_TRY(launch_blame_track_emit(g, t, s), "k_blame_track_emit");
  HIP_TRY(tm.end(ms[4]), "event");
  if (D.env.timing)
    std::fprintf(stderr,
                 "psamd blame_track: window %llu topics %zu strips %u nodes %llu row_bytes %llu work %u launches %zu cap %llu "
                 "classify_ms %.4f weights_ms %.4f sweep_ms %.4f count_scan_ms %.4f commit_emit_ms %.4f host_ms %.4f\n",
                 static_cast<unsigned long long>(w), n, K.ns, static_cast<unsigned long long>(K.n_nodes),
                 static_cast<unsigned long long>(K.row_bytes), K.launch.empty() ? 0u : K.launch.back(),
                 K.ns ? K.launch.size() + 6 : size_t(1), static_cast<unsigned long long>(T.cap), ms[0], ms[1], ms[2], ms[3],
                 ms[4], host_ms);
  return standing_window_done(e, H, n - n_tree);  // the mesh topics of this window
}

extern "C" {

// ---- ps_blame_track / ps_blame_take ------------------------------

int ps_blame_track(ps_engine* e, const uint32_t* topic, size_t n, size_t rec_cap) {
  if (!e || (n && !topic)) return PS_E_INVAL;
  auto& T = e->drain.blame_trk;
  auto& H = T.st;
  if (const int rc = standing_track_check(e, H, topic, n)) return rc;
  if (n && rec_cap > (size_t(1) << 30)) return e->fail(PS_E_RANGE, "ps_blame_track: rec_cap above 2^30");
  for (size_t i = 0; i < n; ++i)
    if (hops_child_lists_mesh(e->topics[topic[i]])) return e->fail(PS_E_STATE, "ps_blame_track: a mesh topic has no cut points");
  // whatever still appends records ends first
  if (const int rc = standing_quiesce(e, H)) return rc;
  // the new tracking's buffers before the old one's go: a failed allocation
  // leaves the previous tracking as it stands
  DevBuf rec[5], map, cur, rec_off;
  if (n) {
    hipError_t rc = map.ensure(n * 4);
    if (rc == hipSuccess) rc = cur.ensure(2 * sizeof(BlameCursor));
    if (rc == hipSuccess) rc = rec_off.ensure((n + 1) * 8);
    for (auto& b : rec)
      if (rc == hipSuccess && rec_cap) rc = b.ensure(rec_cap * 4);
    if (rc != hipSuccess) {
      (void)hipGetLastError();
      return e->fail(PS_E_NOMEM, std::string("ps_blame_track: ") + hipGetErrorString(rc));
    }
  }
  standing_retrack(H, topic, n);
  T.rec_cap = n ? rec_cap : 0;
  T.cap = T.rec_cap;
  blame_release(T);
  if (!H.on) return PS_OK;
  T.d_map.swap(map);
  T.d_cur.swap(cur);
  T.d_rec_off.swap(rec_off);
  for (size_t i = 0; i < 5; ++i) T.d_rec[i].swap(rec[i]);
  HIP_TRY(hipMemsetAsync(T.d_cur.p, 0, 2 * sizeof(BlameCursor), e->stream), "clear blame cursor");
  return PS_OK;
}

int ps_blame_take(ps_engine* e, const uint64_t** rec_off_out, const uint32_t** rec_peer_out, const uint32_t** rec_cut_peer_out,
                  const uint32_t** rec_hop_out, const uint32_t** rec_cut_hop_out, const uint32_t** rec_missed_out,
                  uint64_t* n_windows_out, uint64_t* n_skipped_out, uint64_t* total_out, uint64_t* stored_out) {
  const uint32_t** const outs[5] = {rec_peer_out, rec_cut_peer_out, rec_hop_out, rec_cut_hop_out, rec_missed_out};
  if (!e || !rec_off_out || !n_windows_out || !n_skipped_out || !total_out || !stored_out) return PS_E_INVAL;
  auto& D = e->drain;
  auto& T = D.blame_trk;
  auto& H = T.st;
  if (const int rc = standing_take_enter(e, H)) return rc;
  const auto t0 = hclock::now();
  const size_t n = H.topic.size();
  const uint64_t W = H.windows;
  const size_t n_off = static_cast<size_t>(W) * n + 1;
  size_t asked = 0;
  for (auto* o : outs) asked += o != nullptr;
  HIP_TRY(pinned_ensure(&T.h_off, nullptr, &T.off_cap, n_off * 8), "alloc blame offsets");
  HIP_TRY(pinned_ensure(&T.h_cur, nullptr, &T.cur_cap, sizeof(BlameCursor)), "alloc blame cursor");
  if (const int rc = standing_take_event(e, H)) return rc;
  uint64_t* const h_off = reinterpret_cast<uint64_t*>(T.h_off);
  BlameCursor C{};
  size_t h_stride = 0;
  hipStream_t s = e->stream;
  if (W == 0) {
    // no window since the last take: the cursor stands cleared
    h_off[0] = 0;
    HIP_TRY(pinned_ensure(&T.h_rec, nullptr, &T.view_cap, 1), "alloc blame view");
  } else {
    // every pass ran on `stream`: one wait for the cursor behind them, with
    // the offsets, whose number the host knows; then one copy per array asked
    // for, sized by what was stored, and the clearing behind the copies and in
    // front of whatever runs next
    HIP_TRY(hipMemcpyAsync(T.h_cur, T.d_cur.as<BlameCursor>() + (W & 1), sizeof(BlameCursor), hipMemcpyDeviceToHost, s),
            "read blame cursor");
    HIP_TRY(hipMemcpyAsync(h_off, T.d_rec_off.p, n_off * 8, hipMemcpyDeviceToHost, s), "read blame offsets");
    HIP_TRY(hipEventRecord(H.ev_take, s), "event");
    HIP_TRY(hipEventSynchronize(H.ev_take), "wait for the blame cursor");
    std::memcpy(&C, T.h_cur, sizeof(C));
    // (after a failed run the content is unspecified: no copy past the arrays)
    C.stored = std::min<uint64_t>(C.stored, T.d_rec[0].bytes / 4);
    h_stride = align256(C.stored * 4);
    HIP_TRY(pinned_ensure(&T.h_rec, nullptr, &T.view_cap, std::max<size_t>(asked * h_stride, 1)), "alloc blame view");
    for (size_t i = 0, j = 0; i < 5; ++i)
      if (outs[i]) {
        if (C.stored)
          HIP_TRY(hipMemcpyAsync(T.h_rec + j * h_stride, T.d_rec[i].p, C.stored * 4, hipMemcpyDeviceToHost, s),
                  "read blame records");
        ++j;
      }
    HIP_TRY(hipMemsetAsync(T.d_cur.p, 0, 2 * sizeof(BlameCursor), s), "clear blame cursor");
    HIP_TRY(hipEventRecord(H.ev_take, s), "event");
    HIP_TRY(hipEventSynchronize(H.ev_take), "wait for the blame records");
  }
  standing_settled(H);
  *rec_off_out = h_off;
  for (size_t i = 0, j = 0; i < 5; ++i)
    if (outs[i]) *outs[i] = reinterpret_cast<const uint32_t*>(T.h_rec + j++ * h_stride);
  *n_windows_out = W;
  *n_skipped_out = H.skipped;
  *total_out = C.total;
  *stored_out = C.stored;
  H.windows = H.skipped = 0;
  T.cap = T.rec_cap;
  if (D.env.timing)
    std::fprintf(stderr, "psamd blame_take: windows %llu topics %zu records %llu stored %llu copied_bytes %llu take_ms %.4f\n",
                 static_cast<unsigned long long>(W), n, static_cast<unsigned long long>(C.total),
                 static_cast<unsigned long long>(C.stored), static_cast<unsigned long long>(n_off * 8 + asked * C.stored * 4),
                 ms_since(t0));
  if (C.over) return e->fail(PS_E_RANGE, "ps_blame_take: more records than the cap; the first `stored` are kept");
  return PS_OK;
}

}  // extern "C"

// drain.hip -- the batched drain (ps_drain): the seen rows of
// many (topic, peer) queries turned into message id lists on the device.
//   k_drain_count  delivered positions per (query, segment)
//   drain_scan     hipcub's exclusive sum over the segments
//   k_drain_emit   one wave per segment: set positions -> ids, in order
// and, for ps_drain_begin (§5.5b), which may not wait for the GPU:
//   k_drain_tables        the window's bit -> id table and message mask
//   k_drain_tables_check  arrival keys ascend with the row bit, per topic
//   k_drain_offsets       per-query offsets, total and error word of a view
// and, for ps_drain_shared (§5.5c):
//   k_drain_classify      per query: which of its topic's message bits the row holds
// and, for ps_drain_shared_begin (§5.5d), which may not wait either:
//   k_drain_first / _keys / _lists  the lists numbered by first use and their
//                         segments laid out, around one scan (the host loop
//                         of ps_drain_shared on the device)
//   k_drain_count_dev / _offsets_dev / _emit_dev  count, offsets and emit over
//                         those lists, the counts read from a control block
// and, for the sink (ps_sink_set, §5.5e), every window of a run into one result:
//   k_sink_commit         a window's list offsets and list numbers at the
//                         run's cursor, and the cursor moved on
//   k_sink_emit           k_drain_emit_dev at the cursor's id count
// and, for ps_drain_topics (§5.5f), a topic's whole audience with no query list:
//   k_audience_classify   one streaming pass over a topic's rows: a verdict
//                         byte per node, the full and other nodes per strip
//   k_audience_emit       the nodes that are not full, in node order
// and, for ps_drain_topics_begin (§5.5g), which may not wait:
//   k_audience_totals / _keys / _lists  per-topic totals from the strips'
//                         counts, the lists numbered in request order and
//                         their segments laid out, around two scans (the host
//                         loop of ps_drain_topics on the device)
// and, for ps_peer_load / ps_load_track (§5.5i), per-peer traffic:
//   k_audience_load       behind k_audience_classify: a node's verdict, peer and
//                         CSR children into recv / sent sums in peer space
// and, for ps_topic_hops / ps_hops_track (§5.5j), deliveries by hop per topic:
//   k_audience_hops       behind k_audience_classify: per (strip, level) the
//                         nodes reached and the messages they hold
//   k_audience_hops_sum   each (topic, column)'s partials into its row: one
//                         writer per word, no atomics
// and, for ps_peer_downstream / ps_downstream_track (§5.5k), the audience behind each peer:
//   k_audience_weights    behind k_audience_classify: the messages a node's row holds
//   k_downstream_level    one launch per BFS level, bottom-up: a node's subtree
//                         size and subtree messages from its children's, and
//                         what lies below it into its peer's two sums
//   k_downstream_top      the narrow levels under a root in one block
// and, for ps_peer_cut / ps_cut_track (§5.5l), the losses blamed on their cut points:
//   k_audience_missed     behind k_audience_weights: what a node's row lacks
//                         into its peer's sum
//   k_cut_level           k_downstream_level's pass, a full node looking at its
//                         children: one that lacks messages is a cut point, its
//                         subtree's words into its peer's three sums
//   k_cut_top             the narrow levels under a root in one block
// and, for ps_topic_blame / ps_blame (§5.5q), each missed subscriber and its cut point:
//   k_blame_top           the narrow levels under a root in one block, downwards:
//                         a node hands its children their cut point and its level
//   k_blame_level         one launch per BFS level, top-down, behind it
//   k_blame_count / _emit the nodes that lack messages, strip by strip, into
//                         records in node order
//   k_blame_gather        a (topic, node) query's four facts from the words
//   k_blame_track_commit  ps_blame_track (§5.5s): a window's row of offsets at
//                         the run's cursor on the device, and the cursor moved on
//   k_blame_track_emit    k_blame_emit's records from the window's base on,
//                         below the cap in effect
// and, for ps_peer_report / ps_report_track (§5.5m), those four answers from one pass:
//   k_report_nodes        behind one k_audience_classify: a node's k once, into
//                         the sections selected per launch (load's sums, the hop
//                         partials, the k word, the misses)
//   k_report_level        the bottom-up pass once: k_cut_level's walk with
//                         k_downstream_level's two sums
//   k_report_top          the narrow levels under a root in one block
// and, for ps_dist_report (§5.5n), a rank's share of load, hops and downstream on
// a sharded engine's numbering (one rank's too):
//   k_dist_nodes          k_report_nodes where node 0 need not be a root and a
//                         level may be empty; the roots' share of `sent`
//   k_dist_hops_sum       k_audience_hops_sum over such a level table
//   k_dist_sweep_level    one launch per level, bottom-up: a node's accumulator
//                         into its peer's two sums, and pushed to its parent --
//                         the parent's accumulator, or a record for its owner
//   k_dist_apply          behind a level's exchange: the records received into
//                         the parents' accumulators
// and, for ps_dist_cut (§5.5o), a rank's share of the cut, decided at the child:
//   k_dist_cut_nodes      k_dist_nodes' k word, and what the node lacks into
//                         `missed`
//   k_dist_cut_fill       the k of the parents this rank owns into the words
//                         their children's ranks receive ahead of the sweep
//   k_dist_cut_level      k_dist_sweep_level's push; a node that lacks messages
//                         under a full parent adds its subtree's losses
// and, for ps_topic_spread (§5.5p), hops and duplicate copies of meshes and trees:
//   k_spread_nodes        behind k_audience_classify: a node's k into its word
//                         and its peer's recv; holders and a tree's unreached per entry
//   k_spread_unreached    a mesh's unreached nodes, each peer once
//   k_spread_level        one launch per BFS level over the child lists, top-down,
//                         from a frontier queue into the other: copies per peer,
//                         a hop per forwarder
//   k_spread_sum          the hop words into reached / deliv per (entry, column)
//   k_spread_dup          copies - recv per peer
// and, for ps_spread_track (§5.5t), that pass behind every window of a run:
//   k_spread_track_close  behind the window's level launches: a frontier left
//                         over counts the window as truncated; the counts zeroed
// A segment is kDrainSegBits positions of one query's row (kernels.hpp,
// DrainTopic): lane l of its wave owns lane word l.
#include <hipcub/hipcub.hpp>

#include "devutil.hpp"

namespace psamd {
namespace {

constexpr uint32_t kWave = 64;
constexpr uint32_t kCountBlock = 256;
constexpr uint64_t kNoWord = ~0ull;

// word w of the row of node u: node-major, or the start group's block
__device__ __forceinline__ uint64_t row_word_at(const DrainArgs& a, const DrainTopic& T, uint32_t u, uint32_t w) {
  if (w >= T.W) return kNoWord;
  if (!(T.flags & kTopicGroups)) return T.wbase + static_cast<uint64_t>(u) * T.W + w;
  for (uint32_t g = 0; g < T.group_n; ++g) {
    const DrainGroup G = a.groups[T.group_lo + g];
    if (w < G.w0 + G.wn)
      return w < G.w0 ? kNoWord
                      : T.wbase + static_cast<uint64_t>(T.n_nodes) * G.w0 + static_cast<uint64_t>(u) * G.wn + (w - G.w0);
  }
  return kNoWord;
}

// the 64 positions from p0 of node u's row, bit i = position p0 + i delivered
__device__ __forceinline__ uint64_t lane_word(const DrainArgs& a, const DrainTopic& T, uint32_t u, uint32_t p0) {
  if (p0 >= T.n_pos) return 0;
  if (u == kDrainMaskRow) return a.mask[T.aux0 + (p0 >> 6)];  // (a shared list: every message bit)
  if (!(T.flags & kDrainGather)) {
    const uint64_t at = row_word_at(a, T, u, p0 >> 6);
    return at == kNoWord ? 0ull : a.seen[at] & a.mask[T.aux0 + (p0 >> 6)];
  }
  const uint32_t n = min(64u, T.n_pos - p0);
  uint64_t x = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t b = a.order[T.aux0 + p0 + i];
    const uint64_t at = row_word_at(a, T, u, b >> 6);
    if (at != kNoWord && (a.seen[at] >> (b & 63) & 1ull)) x |= 1ull << i;
  }
  return x;
}

// Segment s -> its query (the last one whose first segment is <= s) and its
// index k within the query; false: the query's row holds nothing to read
// (k past its positions, or a tree node the window did not reach).
__device__ __forceinline__ bool locate(const DrainArgs& a, uint32_t s, DrainQuery* Q, DrainTopic* T, uint32_t* k) {
  uint32_t lo = 0, hi = a.n_queries;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (a.queries[mid].seg0 <= s) lo = mid + 1;
    else hi = mid;
  }
  if (lo == 0) return false;
  *Q = a.queries[lo - 1];
  *T = a.topics[Q->topic];
  *k = s - Q->seg0;
  if (static_cast<uint64_t>(*k) * kDrainSegBits >= T->n_pos) return false;
  if (Q->node == kDrainMaskRow) return true;
  if (Q->node >= T->n_nodes) return false;
  return (T->flags & kTopicMesh) || a.gen[T->nbase + Q->node] == static_cast<uint8_t>(a.gen_cur);
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int src) {
  const uint32_t lo = __shfl(static_cast<uint32_t>(v), src, 64);
  const uint32_t hi = __shfl(static_cast<uint32_t>(v >> 32), src, 64);
  return static_cast<uint64_t>(hi) << 32 | lo;
}

__global__ __launch_bounds__(kCountBlock) void k_drain_count(DrainArgs a, uint32_t n_segs, uint64_t* __restrict__ cnt) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t s = __builtin_amdgcn_readfirstlane(blockIdx.x * (kCountBlock / kWave) + threadIdx.x / kWave);
  if (s > n_segs) return;
  uint32_t c = 0;
  if (s < n_segs) {
    DrainQuery Q;
    DrainTopic T;
    uint32_t k;
    if (locate(a, s, &Q, &T, &k)) c = __popcll(lane_word(a, T, Q.node, k * kDrainSegBits + lane * 64));
  }
  c = wave_sum_u32(c);
  if (lane == 0) cnt[s] = c;
}

// One wave: the ids of segment s to out[off[s] - off0 ..), below out_cap
template <bool kStaged>
__device__ __forceinline__ void emit_segment(const DrainArgs& a, uint32_t s, const uint64_t* __restrict__ off,
                                             uint64_t off0, uint32_t* __restrict__ out, uint64_t out_cap,
                                             uint32_t* stage) {
  const uint32_t lane = threadIdx.x;
  DrainQuery Q;
  DrainTopic T;
  uint32_t k;
  if (!locate(a, s, &Q, &T, &k)) return;  // (block-uniform)
  const uint32_t p0 = k * kDrainSegBits + lane * 64;
  uint64_t x = lane_word(a, T, Q.node, p0);
  const uint32_t c = __popcll(x);
  uint32_t incl = c;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(incl, d, 64);
    if (lane >= static_cast<uint32_t>(d)) incl += t;
  }
  const uint32_t pre = incl - c;
  const uint32_t total = __shfl(incl, 63, 64);
  if (total == 0) return;
  const uint64_t base = off[s] - off0;
  const uint32_t* ids = a.ids + T.tab0;
  if (kStaged) {
    // lane word w at a time: lane l places position 64 w + l behind the set
    // bits below it (consecutive LDS words), then whole-wave stores
    for (uint32_t w = 0; w < kWave; ++w) {
      const uint64_t xw = shfl_u64(x, static_cast<int>(w));
      const uint32_t pw = __shfl(pre, static_cast<int>(w), 64);
      if (xw == 0) continue;
      if (xw >> lane & 1ull) stage[pw + __popcll(xw & ((1ull << lane) - 1))] = k * kDrainSegBits + w * 64 + lane;
    }
    __syncthreads();
    for (uint32_t i = lane; i < total; i += kWave) {
      const uint64_t o = base + i;
      if (o < out_cap) out[o] = ids[stage[i]];
    }
  } else {
    uint32_t p = pre;
    while (x) {
      const uint32_t b = __ffsll(static_cast<long long>(x)) - 1;
      const uint64_t o = base + p++;
      if (o < out_cap) out[o] = ids[p0 + b];
      x &= x - 1;
    }
  }
}

template <bool kStaged>
__global__ __launch_bounds__(kWave) void k_drain_emit(DrainArgs a, uint32_t seg_lo, const uint64_t* __restrict__ off,
                                                      uint64_t off0, uint32_t* __restrict__ out, uint64_t out_cap) {
  __shared__ uint32_t stage[kStaged ? kDrainSegBits : 1];
  emit_segment<kStaged>(a, seg_lo + blockIdx.x, off, off0, out, out_cap, stage);
}

// ---- the shared drain's classify pass (ps_drain_shared) ----------------------

constexpr uint32_t kClassBlock = 256;

// One lane per (query, mask word): the row word under the mask against the
// mask word, reduced over the query's lanes with two ballots.  A row of up to
// 64 words lies in one aligned group of 1 << lanes_log2 lanes and its first
// lane stores the verdict; a wider row spans `waves` steps, each of which ORs
// its part into the (cleared) verdict word.  A wave takes kDrainClassPer steps
// of one bin: the bin search and the topic are paid once, and the steps'
// loads are issued together before the first is used.
__global__ __launch_bounds__(kClassBlock) void k_drain_classify(DrainArgs a, const DrainClassBin* __restrict__ bins,
                                                                uint32_t n_bins,
                                                                const DrainClassQuery* __restrict__ queries,
                                                                uint32_t n_waves, uint32_t* __restrict__ verdict) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * (kClassBlock / kWave) + threadIdx.x / kWave);
  if (w >= n_waves) return;
  uint32_t lo = 0, hi = n_bins;  // the last bin whose first wave is <= w (bins[0].wave0 = 0)
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (bins[mid].wave0 <= w) lo = mid + 1;
    else hi = mid;
  }
  const DrainClassBin B = bins[lo - 1];
  const DrainTopic T = a.topics[B.topic];
  const bool wide = B.waves != 0;
  const bool mesh = T.flags & kTopicMesh;
  const uint32_t step0 = (w - B.wave0) * kDrainClassPer;
  uint32_t slot[kDrainClassPer];
  uint64_t x[kDrainClassPer], m[kDrainClassPer];
  bool head[kDrainClassPer];  // the lane that reports the step's (group's) verdict
#pragma unroll
  for (uint32_t i = 0; i < kDrainClassPer; ++i) {
    const uint32_t s = step0 + i;
    const uint32_t qi = wide ? s / B.waves : (s << (6 - B.lanes_log2)) + (lane >> B.lanes_log2);
    const uint32_t word = wide ? (s % B.waves) * kWave + lane : lane & ((1u << B.lanes_log2) - 1);
    head[i] = qi < B.n_q && (wide ? lane == 0 : word == 0);
    // (indices clamped into range, so that every load below is unconditional)
    const DrainClassQuery Q = queries[B.q0 + min(qi, B.n_q - 1)];
    slot[i] = Q.slot;
    const uint32_t wc = min(word, B.words - 1);
    const bool in = Q.node < T.n_nodes;
    const uint32_t u = in ? Q.node : 0;
    const uint64_t at = row_word_at(a, T, u, wc);
    const bool fresh = mesh || a.gen[T.nbase + u] == static_cast<uint8_t>(a.gen_cur);
    const bool live = qi < B.n_q && word < B.words;
    m[i] = live ? a.mask[T.aux0 + wc] : 0ull;
    x[i] = (at != kNoWord ? a.seen[at] : 0ull) & (live && in && fresh ? m[i] : 0ull);
  }
#pragma unroll
  for (uint32_t i = 0; i < kDrainClassPer; ++i) {
    const uint64_t bm = __ballot(x[i] != m[i]), ba = __ballot(x[i] != 0);
    if (wide) {
      const uint32_t v = (bm ? kDrainRowMissing : 0u) | (ba ? kDrainRowAny : 0u);
      if (head[i] && v) atomicOr(verdict + slot[i], v);
    } else {
      const uint32_t g = 1u << B.lanes_log2;
      const uint64_t gm = (g == kWave ? ~0ull : (1ull << g) - 1) << (lane & ~(g - 1));
      if (head[i]) verdict[slot[i]] = ((bm & gm) ? kDrainRowMissing : 0u) | ((ba & gm) ? kDrainRowAny : 0u);
    }
  }
}

// ---- a topic's audience (ps_drain_topics) -------------------------------------

constexpr uint32_t kAudBlock = 256;
constexpr uint32_t kAudPer = 4;  // row loads a lane has in flight (twice that for rows wider than a wave)
static_assert(kAudStripBytes / ((kWave + 1) * 8) <= kWave, "a strip of rows wider than a wave: a bit per node");

// a node that is not on its topic's shared list
__device__ __forceinline__ bool aud_exception(uint32_t v, uint32_t share) { return !share || v != kDrainRowAny; }

// One wave per strip, front to back.  Rows of up to 64 mask words: an aligned
// group of lanes per row as in k_drain_classify, 64 >> lanes_log2 rows to a
// load and kAudPer loads in flight; the lane's mask word is read once for the
// strip.  Wider rows: 64 words to a load, two nodes at a time with kAudPer
// loads each in flight.  The generation bytes are read first: a stale row is
// not loaded.
// Group-major rows are addressed word by word through row_word_at, so a node's
// blocks are all walked here and its verdict is written once.
__global__ __launch_bounds__(kAudBlock) void k_audience_classify(DrainArgs a, AudArgs g) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t s = __builtin_amdgcn_readfirstlane(blockIdx.x * (kAudBlock / kWave) + threadIdx.x / kWave);
  if (s > g.n_strips) return;
  if (s == g.n_strips) {  // (the scan's last input)
    if (lane == 0) g.n_exc[s] = 0;
    return;
  }
  const AudStrip S = g.strips[s];
  const DrainTopic T = a.topics[S.topic];
  const bool mesh = T.flags & kTopicMesh;
  const uint8_t cur = static_cast<uint8_t>(a.gen_cur);
  const uint8_t* __restrict__ gen = a.gen + T.nbase;
  uint8_t* __restrict__ out = g.verdict + S.v0;
  const uint32_t words = T.n_pos / 64;
  uint32_t n_exc = 0, n_full = 0;  // (wave-uniform)
  if (T.flags & kDrainGather) {
    for (uint32_t i = lane; i < S.n; i += kWave) out[i] = kDrainRowAny | kDrainRowMissing;
    n_exc = S.n;
  } else if (words <= kWave) {
    uint32_t l2 = 0;
    while ((1u << l2) < words) ++l2;
    const uint32_t gl = 1u << l2, per = kWave >> l2;
    const uint32_t word = lane & (gl - 1), sub = lane >> l2;
    const bool has_word = word < words;
    const uint64_t m = has_word ? a.mask[T.aux0 + word] : 0ull;
    const uint64_t gm = (gl == kWave ? ~0ull : (1ull << gl) - 1) << (lane & ~(gl - 1));
    for (uint32_t i0 = 0; i0 < S.n; i0 += per * kAudPer) {
      bool read[kAudPer];
      uint64_t x[kAudPer];
#pragma unroll
      for (uint32_t k = 0; k < kAudPer; ++k) {
        const uint32_t i = i0 + k * per + sub;
        read[k] = has_word && i < S.n && (mesh || gen[S.u0 + min(i, S.n - 1)] == cur);
      }
#pragma unroll
      for (uint32_t k = 0; k < kAudPer; ++k) {
        x[k] = 0;
        if (read[k]) {
          const uint64_t at = row_word_at(a, T, S.u0 + i0 + k * per + sub, word);
          if (at != kNoWord) x[k] = a.seen[at] & m;
        }
      }
#pragma unroll
      for (uint32_t k = 0; k < kAudPer; ++k) {
        const uint32_t i = i0 + k * per + sub;
        const bool in = i < S.n;
        const uint64_t bm = __ballot(in && x[k] != m), ba = __ballot(x[k] != 0);
        const uint32_t v = ((bm & gm) ? kDrainRowMissing : 0u) | ((ba & gm) ? kDrainRowAny : 0u);
        const bool head = in && word == 0;
        if (head) out[i] = static_cast<uint8_t>(v);
        const uint32_t heads = __popcll(__ballot(head));
        const uint32_t exc = __popcll(__ballot(head && aud_exception(v, g.share)));
        n_exc += exc;
        n_full += heads - exc;
      }
    }
  } else {
    // At most 31 nodes (kAudStripBytes of rows 65 words wide or more): a bit
    // per node in wave-uniform words.  The generation bytes are read once,
    // lane i node i's; the mask words of a step of 64 * kAudPer words are
    // read once for all nodes; the fresh nodes go two at a time, so that
    // 2 * kAudPer row loads are in flight and no load waits for a verdict.
    const uint32_t n = min(S.n, kWave);
    const uint64_t fresh = __ballot(lane < n && (mesh || gen[S.u0 + min(lane, n - 1)] == cur));
    uint64_t any_bits = 0, miss_bits = 0;
    for (uint32_t w0 = 0; w0 < words; w0 += kWave * kAudPer) {
      uint64_t m[kAudPer];
#pragma unroll
      for (uint32_t k = 0; k < kAudPer; ++k) {
        const uint32_t w = w0 + k * kWave + lane;
        m[k] = w < words ? a.mask[T.aux0 + w] : 0ull;
      }
      uint64_t todo = fresh;
      while (todo) {
        const uint32_t i0 = __builtin_ctzll(todo);
        todo &= todo - 1;
        const uint32_t i1 = todo ? __builtin_ctzll(todo) : i0;  // (an odd node out is read twice)
        todo &= todo - 1;
        uint64_t x0[kAudPer], x1[kAudPer];
#pragma unroll
        for (uint32_t k = 0; k < kAudPer; ++k) {
          const uint32_t w = w0 + k * kWave + lane;
          x0[k] = 0;
          x1[k] = 0;
          if (w < words) {
            const uint64_t at0 = row_word_at(a, T, S.u0 + i0, w), at1 = row_word_at(a, T, S.u0 + i1, w);
            if (at0 != kNoWord) x0[k] = a.seen[at0] & m[k];
            if (at1 != kNoWord) x1[k] = a.seen[at1] & m[k];
          }
        }
        bool miss0 = false, any0 = false, miss1 = false, any1 = false;
#pragma unroll
        for (uint32_t k = 0; k < kAudPer; ++k) {
          miss0 |= x0[k] != m[k];
          any0 |= x0[k] != 0;
          miss1 |= x1[k] != m[k];
          any1 |= x1[k] != 0;
        }
        miss_bits |= (__ballot(miss0) ? 1ull << i0 : 0ull) | (__ballot(miss1) ? 1ull << i1 : 0ull);
        any_bits |= (__ballot(any0) ? 1ull << i0 : 0ull) | (__ballot(any1) ? 1ull << i1 : 0ull);
      }
    }
    uint32_t v = kDrainRowMissing;  // (a stale row: none)
    if (fresh >> lane & 1ull) v = ((miss_bits >> lane & 1ull) ? kDrainRowMissing : 0u) | ((any_bits >> lane & 1ull) ? kDrainRowAny : 0u);
    if (lane < n) out[lane] = static_cast<uint8_t>(v);
    n_exc = __popcll(__ballot(lane < n && aud_exception(v, g.share)));
    n_full = n - n_exc;
  }
  if (lane == 0) {
    g.n_exc[s] = n_exc;
    g.n_full[s] = n_full;
  }
}

// One wave per strip: the nodes that are not full, in node order (ballot and
// lane prefix), from the strip's offset on
__global__ __launch_bounds__(kAudBlock) void k_audience_emit(AudArgs g, AudEmit o) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t s = __builtin_amdgcn_readfirstlane(blockIdx.x * (kAudBlock / kWave) + threadIdx.x / kWave);
  if (s >= g.n_strips) return;
  const AudStrip S = g.strips[s];
  if (g.n_exc[s] == 0) return;
  const uint8_t* __restrict__ vin = g.verdict + S.v0;
  uint64_t at = o.off[s];
  for (uint32_t i0 = 0; i0 < S.n; i0 += kWave) {
    const uint32_t i = i0 + lane;
    const uint32_t v = i < S.n ? vin[i] : 0u;
    const bool exc = i < S.n && aud_exception(v, g.share);
    const uint64_t b = __ballot(exc);
    const uint64_t to = at + __popcll(b & ((1ull << lane) - 1));
    if (exc && to < o.cap) {
      o.peer[to] = o.node_peer[S.nbase + S.u0 + i];
      o.node[to] = S.u0 + i;
      o.verdict[to] = static_cast<uint8_t>(v);
    }
    at += __popcll(b);
  }
}

// ---- per-peer load (ps_peer_load, ps_load_track) -------------------------------

// the topic's window messages the row of node u holds (wave-uniform): the row
// words under the message mask, lanes across words; an arrival-order topic's
// bits through its order table, lanes across positions
__device__ __forceinline__ uint32_t load_count_row(const DrainArgs& a, const DrainTopic& T, uint32_t u, uint32_t lane) {
  if (!(T.flags & kTopicMesh) && a.gen[T.nbase + u] != static_cast<uint8_t>(a.gen_cur)) return 0;
  uint32_t c = 0;
  if (!(T.flags & kDrainGather)) {
    const uint32_t words = T.n_pos / 64;
    for (uint32_t w0 = 0; w0 < words; w0 += kWave) {
      const uint32_t w = w0 + lane;
      if (w < words) {
        const uint64_t at = row_word_at(a, T, u, w);
        if (at != kNoWord) c += __popcll(a.seen[at] & a.mask[T.aux0 + w]);
      }
    }
    return wave_sum_u32(c);
  }
  for (uint32_t p0 = 0; p0 < T.n_pos; p0 += kWave) {
    const uint32_t p = p0 + lane;
    bool set = false;
    if (p < T.n_pos) {
      const uint32_t b = a.order[T.aux0 + p];
      const uint64_t at = row_word_at(a, T, u, b >> 6);
      set = at != kNoWord && (a.seen[at] >> (b & 63) & 1ull);
    }
    c += __popcll(__ballot(set));
  }
  return c;
}

// One wave per strip, one node per lane: the verdict byte, the node's peer and
// its two CSR bounds, then at most two 64-bit atomic adds in peer space.  The
// rows the verdict does not settle go through load_count_row one at a time.
// The wave of an entry's first strip adds the root's share.
__global__ __launch_bounds__(kAudBlock) void k_audience_load(DrainArgs a, LoadArgs g) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t s = __builtin_amdgcn_readfirstlane(blockIdx.x * (kAudBlock / kWave) + threadIdx.x / kWave);
  if (s >= g.n_strips) return;
  const AudStrip S = g.strips[s];
  uint32_t lo = 0, hi = g.n;  // the last entry whose first strip is <= s: the one that holds it
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (g.entries[mid].strip0 <= s) lo = mid + 1;
    else hi = mid;
  }
  if (lo == 0) return;
  const LoadEntry E = g.entries[lo - 1];
  const DrainTopic T = a.topics[S.topic];
  const bool gather = T.flags & kDrainGather;
  const uint8_t* __restrict__ vin = g.verdict + S.v0;
  unsigned long long* const recv = reinterpret_cast<unsigned long long*>(g.recv);
  unsigned long long* const sent = reinterpret_cast<unsigned long long*>(g.sent);
  for (uint32_t i0 = 0; i0 < S.n; i0 += kWave) {
    const uint32_t i = i0 + lane;
    const bool in = i < S.n;
    const uint32_t u = S.nbase + S.u0 + min(i, S.n - 1);
    const uint32_t v = vin[min(i, S.n - 1)];
    const uint32_t peer = g.node_peer[u];
    const uint32_t deg = g.row_ptr[u + 1] - g.row_ptr[u];
    const bool full = !gather && v == kDrainRowAny;
    const bool count = in && (gather || ((v & kDrainRowAny) && (!full || g.count_rows)));
    uint32_t k = in && full && !count ? E.c_t : 0u;
    uint64_t todo = __ballot(count);
    while (todo) {
      const uint32_t j = __builtin_ctzll(todo);
      todo &= todo - 1;
      const uint32_t c = load_count_row(a, T, S.u0 + i0 + j, lane);
      if (lane == j) k = c;
    }
    if (k) {
      atomicAdd(recv + peer, static_cast<unsigned long long>(k));
      if (deg) atomicAdd(sent + peer, static_cast<unsigned long long>(k) * deg);
    }
  }
  if (E.strip0 == s && lane == 0 && E.root != kLoadNoRoot && E.c_t) {
    const uint32_t deg = g.row_ptr[E.root + 1] - g.row_ptr[E.root];
    if (deg) atomicAdd(sent + g.node_peer[E.root], static_cast<unsigned long long>(E.c_t) * deg);
  }
}

// ---- deliveries by hop per topic (ps_topic_hops, ps_hops_track) ----------------

constexpr uint32_t kHopsSumBlock = 1024;
constexpr uint32_t kHopsSumPer = 4;  // partial pairs a thread has in flight

// One wave per strip: the level of the strip's first node by bisection of the
// topic's level table, then level by level to the strip's end -- the level's
// nodes of the strip a lane each, their verdict bytes (full: c_t, none: 0,
// anything else, and under the seam every full row, through load_count_row),
// a wave sum, one partial pair per (strip, level).  Where classify counted no
// exception in the strip, every node is full: the partials follow from the
// level bounds and no verdict byte is read.
__global__ __launch_bounds__(kAudBlock) void k_audience_hops(DrainArgs a, HopsArgs g) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t s = __builtin_amdgcn_readfirstlane(blockIdx.x * (kAudBlock / kWave) + threadIdx.x / kWave);
  if (s >= g.n_strips) return;
  const AudStrip S = g.strips[s];
  uint32_t lo = 0, hi = g.n;  // the last entry whose first strip is <= s: the one that holds it
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (g.entries[mid].strip0 <= s) lo = mid + 1;
    else hi = mid;
  }
  if (lo == 0) return;
  const HopsEntry E = g.entries[lo - 1];
  const DrainTopic T = a.topics[S.topic];
  const bool gather = T.flags & kDrainGather;
  const uint32_t* __restrict__ lv = g.levels + E.lvl0;
  const uint8_t* __restrict__ vin = g.verdict + S.v0;
  lo = 1, hi = E.depth + 1;  // the last level whose first node is <= u0: the first node's
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (lv[mid] <= S.u0) lo = mid + 1;
    else hi = mid;
  }
  uint32_t d = lo - 1;
  if (d == 0) return;  // (a strip holds no root)
  const bool all_full = !g.count_rows && g.n_exc[s] == 0;
  const uint32_t end = S.u0 + S.n;
  uint32_t slot = E.part0 + (s - E.strip0) + (d - 1);
  for (uint32_t u = S.u0; u < end && d <= E.depth; ++d, ++slot) {
    const uint32_t ue = min(end, max(lv[d + 1], u + 1));
    uint32_t reached = 0;  // (wave-uniform)
    uint64_t deliv = 0;
    if (all_full) {
      reached = ue - u;
      deliv = static_cast<uint64_t>(reached) * E.c_t;
    } else {
      for (uint32_t i0 = u; i0 < ue; i0 += kWave) {
        const uint32_t i = i0 + lane;
        const bool in = i < ue;
        const uint32_t v = vin[min(i, ue - 1) - S.u0];
        const bool full = !gather && v == kDrainRowAny;
        const bool count = in && (gather || ((v & kDrainRowAny) && (!full || g.count_rows)));
        uint32_t k = in && full && !count ? E.c_t : 0u;
        uint64_t todo = __ballot(count);
        while (todo) {
          const uint32_t j = __builtin_ctzll(todo);
          todo &= todo - 1;
          const uint32_t c = load_count_row(a, T, i0 + j, lane);
          if (lane == j) k = c;
        }
        reached += __popcll(__ballot(k != 0));
        deliv += wave_sum_u32(k);
      }
    }
    if (lane == 0) {
      g.part_reached[slot] = reached;
      g.part_deliv[slot] = deliv;
    }
    u = ue;
  }
}

// One block per (entry, column): the strips that meet level d are those of its
// first to its last node, their slots a run with stride one; the last column
// takes every level from its own on.  The block's two sums and the levels'
// nodes are added to the entry's row by one thread: nobody else writes there
// in this pass, and the passes follow each other on one stream.
__global__ __launch_bounds__(kHopsSumBlock) void k_audience_hops_sum(HopsArgs g) {
  __shared__ uint64_t part[2][kHopsSumBlock / kWave];
  const uint32_t h = blockIdx.y + 1;
  const HopsEntry E = g.entries[blockIdx.x];
  if (!E.c_t || h > min(E.depth, kHopsCols - 1) || g.entries[blockIdx.x + 1].strip0 == E.strip0) return;
  const uint32_t* __restrict__ lv = g.levels + E.lvl0;
  const uint32_t d_hi = h == kHopsCols - 1 ? E.depth : h;
  uint64_t r = 0, dl = 0;
  for (uint32_t d = h; d <= d_hi; ++d) {
    const uint32_t sa = (lv[d] - lv[1]) / E.per, sb = (lv[d + 1] - 1 - lv[1]) / E.per;  // (relative to strip0)
    const uint32_t p0 = E.part0 + (d - 1);
    for (uint32_t s0 = sa + threadIdx.x; s0 <= sb; s0 += kHopsSumBlock * kHopsSumPer) {
      uint32_t vr[kHopsSumPer];
      uint64_t vd[kHopsSumPer];
#pragma unroll
      for (uint32_t k = 0; k < kHopsSumPer; ++k) {
        const uint32_t sk = s0 + k * kHopsSumBlock;
        vr[k] = sk <= sb ? g.part_reached[p0 + sk] : 0u;
        vd[k] = sk <= sb ? g.part_deliv[p0 + sk] : 0ull;
      }
#pragma unroll
      for (uint32_t k = 0; k < kHopsSumPer; ++k) {
        r += vr[k];
        dl += vd[k];
      }
    }
  }
  r = dev::wave_sum_u64(r);
  dl = dev::wave_sum_u64(dl);
  if ((threadIdx.x & (kWave - 1)) == 0) {
    part[0][threadIdx.x / kWave] = r;
    part[1][threadIdx.x / kWave] = dl;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    r = dl = 0;
    for (uint32_t w = 0; w < kHopsSumBlock / kWave; ++w) {
      r += part[0][w];
      dl += part[1][w];
    }
    const size_t at = static_cast<size_t>(E.row) * kHopsCols + h;
    g.nodes[at] += lv[d_hi + 1] - lv[h];
    g.reached[at] += r;
    g.deliv[at] += dl;
  }
}

// ---- audience behind each peer (ps_peer_downstream, ps_downstream_track) -------

// One wave per strip, one node per lane: the messages the node's row holds
// into k -- full: c_t, none: 0, anything else, and under the seam every full
// row, through load_count_row.  Where classify counted no exception in the
// strip every node is full and no verdict byte is read.  The wave of an
// entry's first strip writes the root's 0.
__global__ __launch_bounds__(kAudBlock) void k_audience_weights(DrainArgs a, DownArgs g) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t s = __builtin_amdgcn_readfirstlane(blockIdx.x * (kAudBlock / kWave) + threadIdx.x / kWave);
  if (s >= g.n_strips) return;
  const AudStrip S = g.strips[s];
  uint32_t lo = 0, hi = g.n;  // the last entry whose first strip is <= s: the one that holds it
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (g.entries[mid].strip0 <= s) lo = mid + 1;
    else hi = mid;
  }
  if (lo == 0) return;
  const DownEntry E = g.entries[lo - 1];
  const DrainTopic T = a.topics[S.topic];
  const bool gather = T.flags & kDrainGather;
  const uint8_t* __restrict__ vin = g.verdict + S.v0;
  uint32_t* __restrict__ kout = g.k + E.n0;
  const bool all_full = !g.count_rows && g.n_exc[s] == 0;
  for (uint32_t i0 = 0; i0 < S.n; i0 += kWave) {
    const uint32_t i = i0 + lane;
    const bool in = i < S.n;
    uint32_t k = E.c_t;
    if (!all_full) {
      const uint32_t v = vin[min(i, S.n - 1)];
      const bool full = !gather && v == kDrainRowAny;
      const bool count = in && (gather || ((v & kDrainRowAny) && (!full || g.count_rows)));
      k = full && !count ? E.c_t : 0u;
      uint64_t todo = __ballot(count);
      while (todo) {
        const uint32_t j = __builtin_ctzll(todo);
        todo &= todo - 1;
        const uint32_t c = load_count_row(a, T, S.u0 + i0 + j, lane);
        if (lane == j) k = c;
      }
    }
    if (in) kout[S.u0 + i] = k;
  }
  if (E.strip0 == s && lane == 0) kout[0] = 0;
}

// The nodes [lo, hi) of level d < depth of entry E, thread tid of nt (whole
// waves) a node each: the node's children are the CSR range's length of nodes
// of level d + 1, from that level's first node plus what the level's nodes
// before it have.  A lane sums its node's children; a node with more than a
// wave's worth is summed by the wave, lanes across its children.  Children of
// the deepest level are leaves: (1, k).  Then the node's two words, and what
// lies strictly below it into its peer's sums.
__device__ __forceinline__ void down_nodes(const DownArgs& g, const DownEntry& E, const uint32_t* __restrict__ lv,
                                           uint32_t d, uint32_t lo, uint32_t hi, uint32_t tid, uint32_t nt) {
  const uint32_t lane = tid & (kWave - 1);
  const uint32_t c0 = lv[d + 1], c1 = lv[d + 2];
  const uint32_t rp0 = g.row_ptr[E.nbase + lv[d]];
  const bool leaf_kids = d + 1 == E.depth;
  const uint32_t* const k = g.k + E.n0;
  uint32_t* const w_n = g.w_n + E.n0;
  uint64_t* const w_k = g.w_k + E.n0;
  unsigned long long* const below = reinterpret_cast<unsigned long long*>(g.below);
  unsigned long long* const carried = reinterpret_cast<unsigned long long*>(g.carried);
  for (uint32_t u0 = lo + (tid & ~(kWave - 1)); u0 < hi; u0 += nt) {  // (wave-uniform)
    const bool in = u0 + lane < hi;
    const uint32_t u = min(u0 + lane, hi - 1);
    const uint32_t r0 = g.row_ptr[E.nbase + u], r1 = g.row_ptr[E.nbase + u + 1];
    // (clamped into level d + 1, whatever the CSR says)
    const uint32_t cb = min(c0 + (r0 - rp0), c1);
    const uint32_t deg = in ? min(r1 - r0, c1 - cb) : 0u;
    const bool wide = deg > kWave;
    uint32_t sn = 0;
    uint64_t sk = 0;
    if (!wide) {
      for (uint32_t j = 0; j < deg; ++j) {
        sn += leaf_kids ? 1u : w_n[cb + j];
        sk += leaf_kids ? k[cb + j] : w_k[cb + j];
      }
    }
    uint64_t todo = __ballot(wide);
    while (todo) {
      const uint32_t j = __builtin_ctzll(todo);
      todo &= todo - 1;
      const uint32_t b = __shfl(cb, static_cast<int>(j), 64), n = __shfl(deg, static_cast<int>(j), 64);
      uint32_t pn = 0;
      uint64_t pk = 0;
      for (uint32_t i = lane; i < n; i += kWave) {
        pn += leaf_kids ? 1u : w_n[b + i];
        pk += leaf_kids ? k[b + i] : w_k[b + i];
      }
      pn = wave_sum_u32(pn);
      pk = dev::wave_sum_u64(pk);
      if (lane == j) {
        sn = pn;
        sk = pk;
      }
    }
    if (in) {
      w_n[u] = 1 + sn;
      w_k[u] = k[u] + sk;
      const uint32_t peer = g.node_peer[E.nbase + u];
      if (sn) atomicAdd(below + peer, static_cast<unsigned long long>(sn));
      if (sk) atomicAdd(carried + peer, static_cast<unsigned long long>(sk));
    }
  }
}

// One block per work item of this launch: a run of nodes of the level that
// lies as far above its entry's deepest as the launch is behind the first.
// The words it reads were written by the launch before (or are the deepest
// level's k): stream order is the only order between the launches' waves.
__global__ __launch_bounds__(kDownBlock) void k_downstream_level(DownArgs g, uint32_t w0) {
  const DownWork W = g.work[w0 + blockIdx.x];
  const DownEntry E = g.entries[W.entry];
  if (W.level >= E.depth) return;  // (block-uniform; leaves take no work)
  const uint32_t* __restrict__ lv = g.levels + E.lvl0;
  down_nodes(g, E, lv, W.level, max(W.lo, lv[W.level]), min(W.hi, lv[W.level + 1]), threadIdx.x, kDownBlock);
}

// One block per entry, behind the last level launch: the levels [0, top),
// none wider than the block by the host's choice, walked upwards; the barrier
// between two levels orders the block's own stores and loads.
__global__ __launch_bounds__(kDownBlock) void k_downstream_top(DownArgs g) {
  const DownEntry E = g.entries[blockIdx.x];
  if (!E.c_t || g.entries[blockIdx.x + 1].strip0 == E.strip0) return;  // (block-uniform)
  const uint32_t* __restrict__ lv = g.levels + E.lvl0;
  for (uint32_t d = min(E.top, E.depth); d-- > 0;) {
    down_nodes(g, E, lv, d, lv[d], lv[d + 1], threadIdx.x, kDownBlock);
    __syncthreads();
  }
}

// ---- losses blamed on their cut points (ps_peer_cut, ps_cut_track) -------------

// One wave per strip, one node per lane, behind k_audience_weights: what the
// node's row lacks of its topic's window messages into missed[its peer].  A
// strip holds no root; a full node adds nothing and reads no peer.
__global__ __launch_bounds__(kAudBlock) void k_audience_missed(CutArgs g) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t s = __builtin_amdgcn_readfirstlane(blockIdx.x * (kAudBlock / kWave) + threadIdx.x / kWave);
  if (s >= g.d.n_strips) return;
  const AudStrip S = g.d.strips[s];
  uint32_t lo = 0, hi = g.d.n;  // the last entry whose first strip is <= s: the one that holds it
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (g.d.entries[mid].strip0 <= s) lo = mid + 1;
    else hi = mid;
  }
  if (lo == 0) return;
  const DownEntry E = g.d.entries[lo - 1];
  const uint32_t* __restrict__ k = g.d.k + E.n0;
  unsigned long long* const missed = reinterpret_cast<unsigned long long*>(g.missed);
  for (uint32_t i = lane; i < S.n; i += kWave) {
    const uint32_t u = S.u0 + i;
    const uint32_t have = k[u];
    if (have < E.c_t) atomicAdd(missed + g.d.node_peer[E.nbase + u], static_cast<unsigned long long>(E.c_t - have));
  }
}

// Child c of a full node lacks messages: the tree is cut at c.  Its subtree's
// two words (n nodes, k messages held) into the three sums of c's peer.
__device__ __forceinline__ void cut_point(const CutArgs& g, const DownEntry& E, uint32_t c, uint32_t n, uint64_t k) {
  const uint32_t peer = g.d.node_peer[E.nbase + c];
  atomicAdd(reinterpret_cast<unsigned long long*>(g.cuts) + peer, 1ull);
  if (n > 1) atomicAdd(reinterpret_cast<unsigned long long*>(g.orphaned) + peer, static_cast<unsigned long long>(n - 1));
  atomicAdd(reinterpret_cast<unsigned long long*>(g.lost) + peer,
            static_cast<unsigned long long>(static_cast<uint64_t>(E.c_t) * n - k));
}

// down_nodes' walk over the nodes [lo, hi) of level d < depth, without the
// peer sums of its own: a node's two words from its children's, and, at a node
// that is full -- the root counts as full, whatever k holds for it --, every
// child that is not is a cut point, found here with its subtree's words at
// hand.  A wide node's lanes each look at their own children.
__device__ __forceinline__ void cut_nodes(const CutArgs& g, const DownEntry& E, const uint32_t* __restrict__ lv, uint32_t d,
                                          uint32_t lo, uint32_t hi, uint32_t tid, uint32_t nt) {
  const uint32_t lane = tid & (kWave - 1);
  const uint32_t c0 = lv[d + 1], c1 = lv[d + 2];
  const uint32_t rp0 = g.d.row_ptr[E.nbase + lv[d]];
  const bool leaf_kids = d + 1 == E.depth;
  const uint32_t* const k = g.d.k + E.n0;
  uint32_t* const w_n = g.d.w_n + E.n0;
  uint64_t* const w_k = g.d.w_k + E.n0;
  for (uint32_t u0 = lo + (tid & ~(kWave - 1)); u0 < hi; u0 += nt) {  // (wave-uniform)
    const bool in = u0 + lane < hi;
    const uint32_t u = min(u0 + lane, hi - 1);
    const uint32_t r0 = g.d.row_ptr[E.nbase + u], r1 = g.d.row_ptr[E.nbase + u + 1];
    // (clamped into level d + 1, whatever the CSR says)
    const uint32_t cb = min(c0 + (r0 - rp0), c1);
    const uint32_t deg = in ? min(r1 - r0, c1 - cb) : 0u;
    const bool wide = deg > kWave;
    const uint32_t ku = k[u];
    const bool full = d == 0 || ku == E.c_t;
    uint32_t sn = 0;
    uint64_t sk = 0;
    if (!wide) {
      for (uint32_t j = 0; j < deg; ++j) {
        const uint32_t kc = k[cb + j];
        const uint32_t cn = leaf_kids ? 1u : w_n[cb + j];
        const uint64_t ck = leaf_kids ? kc : w_k[cb + j];
        sn += cn;
        sk += ck;
        if (full && kc < E.c_t) cut_point(g, E, cb + j, cn, ck);
      }
    }
    uint64_t todo = __ballot(wide);
    while (todo) {
      const uint32_t j = __builtin_ctzll(todo);
      todo &= todo - 1;
      const uint32_t b = __shfl(cb, static_cast<int>(j), 64), n = __shfl(deg, static_cast<int>(j), 64);
      const bool pfull = __shfl(static_cast<int>(full), static_cast<int>(j), 64) != 0;
      uint32_t pn = 0;
      uint64_t pk = 0;
      for (uint32_t i = lane; i < n; i += kWave) {
        const uint32_t kc = k[b + i];
        const uint32_t cn = leaf_kids ? 1u : w_n[b + i];
        const uint64_t ck = leaf_kids ? kc : w_k[b + i];
        pn += cn;
        pk += ck;
        if (pfull && kc < E.c_t) cut_point(g, E, b + i, cn, ck);
      }
      pn = wave_sum_u32(pn);
      pk = dev::wave_sum_u64(pk);
      if (lane == j) {
        sn = pn;
        sk = pk;
      }
    }
    if (in) {
      w_n[u] = 1 + sn;
      w_k[u] = ku + sk;
    }
  }
}

// k_downstream_level's launch: one block per work item, stream order the only
// order between the launches' waves.
__global__ __launch_bounds__(kDownBlock) void k_cut_level(CutArgs g, uint32_t w0) {
  const DownWork W = g.d.work[w0 + blockIdx.x];
  const DownEntry E = g.d.entries[W.entry];
  if (W.level >= E.depth) return;  // (block-uniform; leaves take no work)
  const uint32_t* __restrict__ lv = g.d.levels + E.lvl0;
  cut_nodes(g, E, lv, W.level, max(W.lo, lv[W.level]), min(W.hi, lv[W.level + 1]), threadIdx.x, kDownBlock);
}

// k_downstream_top's: one block per entry walks the levels [0, top) upwards,
// a barrier between two levels.
__global__ __launch_bounds__(kDownBlock) void k_cut_top(CutArgs g) {
  const DownEntry E = g.d.entries[blockIdx.x];
  if (!E.c_t || g.d.entries[blockIdx.x + 1].strip0 == E.strip0) return;  // (block-uniform)
  const uint32_t* __restrict__ lv = g.d.levels + E.lvl0;
  for (uint32_t d = min(E.top, E.depth); d-- > 0;) {
    cut_nodes(g, E, lv, d, lv[d], lv[d + 1], threadIdx.x, kDownBlock);
    __syncthreads();
  }
}

// ---- each missed subscriber and its cut point (ps_topic_blame, ps_blame) --------

// cut_nodes' visit of the nodes [lo, hi) of level d < depth, downwards: every
// child of level d + 1 gets its two words from its one parent -- none where
// the child is full; itself and d + 1 where the parent is full (level 0
// counts as full, whatever k holds for it); else the parent's own two, which
// the level above left.  One writer per word: plain stores.
__device__ __forceinline__ void blame_nodes(const BlameArgs& g, const DownEntry& E, const uint32_t* __restrict__ lv, uint32_t d,
                                            uint32_t lo, uint32_t hi, uint32_t tid, uint32_t nt) {
  const uint32_t lane = tid & (kWave - 1);
  const uint32_t c0 = lv[d + 1], c1 = lv[d + 2];
  const uint32_t rp0 = g.d.row_ptr[E.nbase + lv[d]];
  const uint32_t* const k = g.d.k + E.n0;
  uint32_t* const cut_node = g.cut_node + E.n0;
  uint32_t* const cut_level = g.cut_level + E.n0;
  for (uint32_t u0 = lo + (tid & ~(kWave - 1)); u0 < hi; u0 += nt) {  // (wave-uniform)
    const bool in = u0 + lane < hi;
    const uint32_t u = min(u0 + lane, hi - 1);
    const uint32_t r0 = g.d.row_ptr[E.nbase + u], r1 = g.d.row_ptr[E.nbase + u + 1];
    // (clamped into level d + 1, whatever the CSR says)
    const uint32_t cb = min(c0 + (r0 - rp0), c1);
    const uint32_t deg = in ? min(r1 - r0, c1 - cb) : 0u;
    const bool wide = deg > kWave;
    const bool full = d == 0 || k[u] == E.c_t;
    // what a child that lacks messages inherits under a node that does too
    const uint32_t pn = full ? 0u : cut_node[u], pl = full ? d + 1 : cut_level[u];
    if (!wide) {
      for (uint32_t j = 0; j < deg; ++j) {
        const uint32_t c = cb + j;
        const bool cfull = k[c] == E.c_t;
        cut_node[c] = cfull ? kBlameNone : full ? c : pn;
        cut_level[c] = cfull ? kBlameNone : pl;
      }
    }
    uint64_t todo = __ballot(wide);
    while (todo) {
      const uint32_t j = __builtin_ctzll(todo);
      todo &= todo - 1;
      const uint32_t b = __shfl(cb, static_cast<int>(j), 64), n = __shfl(deg, static_cast<int>(j), 64);
      const bool pfull = __shfl(static_cast<int>(full), static_cast<int>(j), 64) != 0;
      const uint32_t qn = __shfl(pn, static_cast<int>(j), 64), ql = __shfl(pl, static_cast<int>(j), 64);
      for (uint32_t i = lane; i < n; i += kWave) {
        const uint32_t c = b + i;
        const bool cfull = k[c] == E.c_t;
        cut_node[c] = cfull ? kBlameNone : pfull ? c : qn;
        cut_level[c] = cfull ? kBlameNone : ql;
      }
    }
  }
}

// One block per entry, first: the levels [0, top), none wider than the block,
// walked downwards; the barrier between two levels orders the block's own
// stores and loads.  It leaves the words of the levels 1 .. top.
__global__ __launch_bounds__(kDownBlock) void k_blame_top(BlameArgs g) {
  const DownEntry E = g.d.entries[blockIdx.x];
  if (!E.c_t || g.d.entries[blockIdx.x + 1].strip0 == E.strip0) return;  // (block-uniform)
  const uint32_t* __restrict__ lv = g.d.levels + E.lvl0;
  const uint32_t top = min(E.top, E.depth);
  for (uint32_t d = 0; d < top; ++d) {
    blame_nodes(g, E, lv, d, lv[d], lv[d + 1], threadIdx.x, kDownBlock);
    __syncthreads();
  }
}

// One block per work item of this launch: a run of nodes of a level >= top,
// whose own words the launch before wrote (level top's: k_blame_top).  Stream
// order is the only order between the launches' waves.
__global__ __launch_bounds__(kDownBlock) void k_blame_level(BlameArgs g, uint32_t w0) {
  const DownWork W = g.d.work[w0 + blockIdx.x];
  const DownEntry E = g.d.entries[W.entry];
  if (W.level >= E.depth) return;  // (block-uniform; leaves have no children)
  const uint32_t* __restrict__ lv = g.d.levels + E.lvl0;
  blame_nodes(g, E, lv, W.level, max(W.lo, lv[W.level]), min(W.hi, lv[W.level + 1]), threadIdx.x, kDownBlock);
}

// the last level d in [0, depth] with lv[d] <= u (lv[0] = 0)
__device__ __forceinline__ uint32_t blame_level_of(const uint32_t* __restrict__ lv, uint32_t depth, uint32_t u) {
  uint32_t lo = 0, hi = depth + 1;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (lv[mid] <= u) lo = mid;
    else hi = mid;
  }
  return lo;
}

// the entry that holds strip s: the last one whose first strip is <= s (false: none)
__device__ __forceinline__ bool blame_entry_of(const DownArgs& d, uint32_t s, DownEntry* E) {
  uint32_t lo = 0, hi = d.n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (d.entries[mid].strip0 <= s) lo = mid + 1;
    else hi = mid;
  }
  if (lo == 0) return false;
  *E = d.entries[lo - 1];
  return true;
}

// One wave per strip, one node per lane: the strip's nodes that lack messages.
// The wave behind the last strip writes the closing 0.
__global__ __launch_bounds__(kAudBlock) void k_blame_count(BlameArgs g) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t s = __builtin_amdgcn_readfirstlane(blockIdx.x * (kAudBlock / kWave) + threadIdx.x / kWave);
  if (s > g.d.n_strips) return;
  uint32_t c = 0;
  DownEntry E;
  if (s < g.d.n_strips && blame_entry_of(g.d, s, &E)) {
    const AudStrip S = g.d.strips[s];
    const uint32_t* __restrict__ k = g.d.k + E.n0;
    for (uint32_t i = lane; i < S.n; i += kWave) c += k[S.u0 + i] < E.c_t;
  }
  c = wave_sum_u32(c);
  if (lane == 0) g.n_rec[s] = c;
}

// One wave per strip: the nodes that lack messages, in node order (ballot and
// lane prefix), from the strip's offset on.  The first n + 1 threads of the
// grid leave the entries' record offsets.
__global__ __launch_bounds__(kAudBlock) void k_blame_emit(BlameArgs g) {
  const uint32_t tid = blockIdx.x * kAudBlock + threadIdx.x;
  if (tid <= g.d.n) g.rec_off[tid] = g.off[min(g.d.entries[tid].strip0, g.d.n_strips)];
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t s = __builtin_amdgcn_readfirstlane(blockIdx.x * (kAudBlock / kWave) + threadIdx.x / kWave);
  if (s >= g.d.n_strips || g.n_rec[s] == 0) return;
  DownEntry E;
  if (!blame_entry_of(g.d, s, &E)) return;
  const AudStrip S = g.d.strips[s];
  const uint32_t* __restrict__ lv = g.d.levels + E.lvl0;
  const uint32_t nn = lv[E.depth + 1];
  const uint32_t* __restrict__ k = g.d.k + E.n0;
  const uint32_t* __restrict__ cut_node = g.cut_node + E.n0;
  const uint32_t* __restrict__ cut_level = g.cut_level + E.n0;
  uint64_t at = g.off[s];
  for (uint32_t i0 = 0; i0 < S.n; i0 += kWave) {
    const uint32_t i = i0 + lane;
    const uint32_t u = S.u0 + min(i, S.n - 1);
    const uint32_t have = k[u];
    const bool rec = i < S.n && have < E.c_t;
    const uint64_t b = __ballot(rec);
    const uint64_t to = at + __popcll(b & ((1ull << lane) - 1));
    if (rec && to < g.cap) {
      const uint32_t cn = cut_node[u];
      if (g.rec_peer) g.rec_peer[to] = g.d.node_peer[E.nbase + u];
      if (g.rec_cut_peer) g.rec_cut_peer[to] = cn < nn ? g.d.node_peer[E.nbase + cn] : kBlameNone;
      if (g.rec_hop) g.rec_hop[to] = blame_level_of(lv, E.depth, u);
      if (g.rec_cut_hop) g.rec_cut_hop[to] = cut_level[u];
      if (g.rec_missed) g.rec_missed[to] = E.c_t - have;
    }
    at += __popcll(b);
  }
}

// ps_blame_track's window w behind the scan, a thread per request position:
// the window's row of the run's rec_off from the cursor the window before
// left (cur[w & 1]: the window's base, which k_blame_track_emit reads there
// too), and, by the grid's first thread, the cursor of the window behind
// (cur[(w + 1) & 1]).  One writer per word: plain loads and stores.
__global__ __launch_bounds__(kAudBlock) void k_blame_track_commit(BlameArgs g, BlameTrack t) {
  const uint32_t i = blockIdx.x * kAudBlock + threadIdx.x;
  const BlameCursor C = t.cur[t.w & 1];
  const uint32_t ns = g.d.n_strips;
  if (i < t.n_req) {
    // the records in front of the entry behind position i: an idle or a
    // skipped position repeats its predecessor
    const uint64_t o = ns ? g.off[min(g.d.entries[min(t.ent[i], g.d.n)].strip0, ns)] : 0;
    t.rec_off[t.w * t.n_req + 1 + i] = C.total + o;
  }
  if (i != 0) return;
  if (t.w == 0) t.rec_off[0] = 0;
  const uint64_t total = C.total + (ns ? g.off[ns] : 0);
  BlameCursor N;
  N.total = total;
  N.over = C.over || total > t.cap;
  // (no overflow so far: everything below C.total is stored, and C.total <= cap)
  N.stored = C.over ? C.stored : total < t.cap ? total : t.cap;
  N.pad = 0;
  t.cur[(t.w + 1) & 1] = N;
}

// k_blame_emit's strips into the run's record arrays: from the window's base
// on, below the cap in effect, and nothing once a window before overflowed.
__global__ __launch_bounds__(kAudBlock) void k_blame_track_emit(BlameArgs g, BlameTrack t) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t s = __builtin_amdgcn_readfirstlane(blockIdx.x * (kAudBlock / kWave) + threadIdx.x / kWave);
  if (s >= g.d.n_strips || g.n_rec[s] == 0) return;
  const BlameCursor C = t.cur[t.w & 1];
  if (C.over) return;
  DownEntry E;
  if (!blame_entry_of(g.d, s, &E)) return;
  const AudStrip S = g.d.strips[s];
  const uint32_t* __restrict__ lv = g.d.levels + E.lvl0;
  const uint32_t nn = lv[E.depth + 1];
  const uint32_t* __restrict__ k = g.d.k + E.n0;
  const uint32_t* __restrict__ cut_node = g.cut_node + E.n0;
  const uint32_t* __restrict__ cut_level = g.cut_level + E.n0;
  uint64_t at = C.total + g.off[s];
  for (uint32_t i0 = 0; i0 < S.n && at < t.cap; i0 += kWave) {  // (wave-uniform)
    const uint32_t i = i0 + lane;
    const uint32_t u = S.u0 + min(i, S.n - 1);
    const uint32_t have = k[u];
    const bool rec = i < S.n && have < E.c_t;
    const uint64_t b = __ballot(rec);
    const uint64_t to = at + __popcll(b & ((1ull << lane) - 1));
    if (rec && to < t.cap) {
      const uint32_t cn = cut_node[u];
      g.rec_peer[to] = g.d.node_peer[E.nbase + u];
      g.rec_cut_peer[to] = cn < nn ? g.d.node_peer[E.nbase + cn] : kBlameNone;
      g.rec_hop[to] = blame_level_of(lv, E.depth, u);
      g.rec_cut_hop[to] = cut_level[u];
      g.rec_missed[to] = E.c_t - have;
    }
    at += __popcll(b);
  }
}

// One thread per query.  A peer without a node of the topic: none, none, none,
// 0.  The root, a full row and every node of a topic idle in the window: none,
// its level, none, 0 -- the latter without a read of the sweep's words.
__global__ __launch_bounds__(kAudBlock) void k_blame_gather(BlameArgs g, BlameGather q) {
  const uint32_t i = blockIdx.x * kAudBlock + threadIdx.x;
  if (i >= q.n) return;
  const DrainQuery Q = q.queries[i];
  uint32_t cut_peer = kBlameNone, hop = kBlameNone, cut_hop = kBlameNone, missed = 0;
  if (Q.node != kBlameNone) {
    const BlameTopic T = q.topics[Q.topic];
    hop = blame_level_of(q.levels + T.lvl0, T.depth, Q.node);
    if (T.entry != kBlameNone && Q.node != 0) {
      const DownEntry E = g.d.entries[T.entry];
      const uint32_t nn = g.d.levels[E.lvl0 + E.depth + 1];
      const uint32_t have = Q.node < nn ? g.d.k[E.n0 + Q.node] : E.c_t;
      if (have < E.c_t) {
        const uint32_t cn = g.cut_node[E.n0 + Q.node];
        missed = E.c_t - have;
        cut_hop = g.cut_level[E.n0 + Q.node];
        cut_peer = cn < nn ? g.d.node_peer[E.nbase + cn] : kBlameNone;
      }
    }
  }
  if (q.cut_peer) q.cut_peer[i] = cut_peer;
  if (q.hop) q.hop[i] = hop;
  if (q.cut_hop) q.cut_hop[i] = cut_hop;
  if (q.missed) q.missed[i] = missed;
}

// ---- the four answers from one pass (ps_peer_report, ps_report_track) ----------

// One wave per strip behind k_audience_classify, a node per lane: a node's k
// once -- the verdict byte (full: c_t, none: 0), anything else, and under the
// seam every full row, through load_count_row; no verdict byte where classify
// counted no exception in the strip -- and from it what each section selected
// at compile time takes: k_audience_load's two adds (and the root's share from
// the entry's first strip), k_audience_hops' partial pair per (strip, level),
// k_audience_weights' word (the root's 0), k_audience_missed's add.  With hops
// selected a tree strip is walked level by level as k_audience_hops walks it,
// else in one run; the sums are integers, so the order changes nothing.  An
// entry that is no tree feeds the load section alone.
template <bool kLoad, bool kHops, bool kWords, bool kMissed>
__global__ __launch_bounds__(kAudBlock) void k_report_nodes(DrainArgs a, ReportArgs g) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t s = __builtin_amdgcn_readfirstlane(blockIdx.x * (kAudBlock / kWave) + threadIdx.x / kWave);
  if (s >= g.n_strips) return;
  const AudStrip S = g.strips[s];
  uint32_t lo = 0, hi = g.n;  // the last entry whose first strip is <= s: the one that holds it
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (g.entries[mid].strip0 <= s) lo = mid + 1;
    else hi = mid;
  }
  if (lo == 0) return;
  const ReportEntry E = g.entries[lo - 1];
  const bool tree = E.tree != 0;  // (wave-uniform, as everything read from E and S)
  if (!kLoad && !tree) return;
  const DrainTopic T = a.topics[S.topic];
  const bool gather = T.flags & kDrainGather;
  const uint8_t* __restrict__ vin = g.verdict + S.v0;
  const bool all_full = !g.count_rows && g.n_exc[s] == 0;
  const uint32_t end = S.u0 + S.n;
  unsigned long long* const recv = reinterpret_cast<unsigned long long*>(g.recv);
  unsigned long long* const sent = reinterpret_cast<unsigned long long*>(g.sent);
  unsigned long long* const missed = reinterpret_cast<unsigned long long*>(g.missed);
  uint32_t* const kout = kWords ? g.k + E.n0 : nullptr;
  // the level of the strip's first node (a strip holds no root: d >= 1)
  const uint32_t* __restrict__ lv = g.levels + E.lvl0;
  uint32_t d = 0, slot = 0;
  if (kHops && tree) {
    lo = 1, hi = E.depth + 1;
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (lv[mid] <= S.u0) lo = mid + 1;
      else hi = mid;
    }
    d = lo - 1;
    slot = E.part0 + (s - E.strip0) + (d - 1);
  }
  for (uint32_t u = S.u0; u < end;) {
    const bool hop = kHops && tree && d >= 1 && d <= E.depth;
    const uint32_t ue = hop ? min(end, max(lv[d + 1], u + 1)) : end;
    uint32_t reached = 0;  // (wave-uniform)
    uint64_t deliv = 0;
    if (all_full && !kLoad && !kWords) {
      // every node holds c_t: nothing is missed, the partials follow from the bounds
      reached = ue - u;
      deliv = static_cast<uint64_t>(reached) * E.c_t;
    } else {
      for (uint32_t i0 = u; i0 < ue; i0 += kWave) {
        const uint32_t i = min(i0 + lane, ue - 1);
        const bool in = i0 + lane < ue;
        uint32_t peer = 0, deg = 0;
        if (kLoad) {
          peer = g.node_peer[S.nbase + i];
          deg = g.row_ptr[S.nbase + i + 1] - g.row_ptr[S.nbase + i];
        }
        uint32_t k = in ? E.c_t : 0u;
        if (!all_full) {
          const uint32_t v = vin[i - S.u0];
          const bool full = !gather && v == kDrainRowAny;
          const bool count = in && (gather || ((v & kDrainRowAny) && (!full || g.count_rows)));
          k = in && full && !count ? E.c_t : 0u;
          uint64_t todo = __ballot(count);
          while (todo) {
            const uint32_t j = __builtin_ctzll(todo);
            todo &= todo - 1;
            const uint32_t c = load_count_row(a, T, i0 + j, lane);
            if (lane == j) k = c;
          }
        }
        if (kLoad && k) {
          atomicAdd(recv + peer, static_cast<unsigned long long>(k));
          if (deg) atomicAdd(sent + peer, static_cast<unsigned long long>(k) * deg);
        }
        if (kWords && in && tree) kout[i] = k;
        if (kMissed && in && tree && k < E.c_t) {
          if (!kLoad) peer = g.node_peer[S.nbase + i];
          atomicAdd(missed + peer, static_cast<unsigned long long>(E.c_t - k));
        }
        if (kHops && hop) {
          reached += __popcll(__ballot(k != 0));
          deliv += wave_sum_u32(k);
        }
      }
    }
    if (kHops && hop) {
      if (lane == 0) {
        g.part_reached[slot] = reached;
        g.part_deliv[slot] = deliv;
      }
      ++d, ++slot;
    }
    u = ue;
  }
  if (E.strip0 == s && lane == 0) {
    if (kLoad && E.root != kLoadNoRoot && E.c_t) {
      const uint32_t deg = g.row_ptr[E.root + 1] - g.row_ptr[E.root];
      if (deg) atomicAdd(sent + g.node_peer[E.root], static_cast<unsigned long long>(E.c_t) * deg);
    }
    if (kWords && tree) kout[0] = 0;
  }
}

// cut_nodes' walk over the nodes [lo, hi) of level d < depth with down_nodes'
// two adds: a node's two words from its children's, written once; every child
// of a full node -- the root counts as full -- that lacks messages is a cut
// point; and what lies strictly below the node into its peer's below / carried.
__device__ __forceinline__ void report_nodes(const CutArgs& g, const DownEntry& E, const uint32_t* __restrict__ lv, uint32_t d,
                                             uint32_t lo, uint32_t hi, uint32_t tid, uint32_t nt) {
  const uint32_t lane = tid & (kWave - 1);
  const uint32_t c0 = lv[d + 1], c1 = lv[d + 2];
  const uint32_t rp0 = g.d.row_ptr[E.nbase + lv[d]];
  const bool leaf_kids = d + 1 == E.depth;
  const uint32_t* const k = g.d.k + E.n0;
  uint32_t* const w_n = g.d.w_n + E.n0;
  uint64_t* const w_k = g.d.w_k + E.n0;
  unsigned long long* const below = reinterpret_cast<unsigned long long*>(g.d.below);
  unsigned long long* const carried = reinterpret_cast<unsigned long long*>(g.d.carried);
  for (uint32_t u0 = lo + (tid & ~(kWave - 1)); u0 < hi; u0 += nt) {  // (wave-uniform)
    const bool in = u0 + lane < hi;
    const uint32_t u = min(u0 + lane, hi - 1);
    const uint32_t r0 = g.d.row_ptr[E.nbase + u], r1 = g.d.row_ptr[E.nbase + u + 1];
    // (clamped into level d + 1, whatever the CSR says)
    const uint32_t cb = min(c0 + (r0 - rp0), c1);
    const uint32_t deg = in ? min(r1 - r0, c1 - cb) : 0u;
    const bool wide = deg > kWave;
    const uint32_t ku = k[u];
    const bool full = d == 0 || ku == E.c_t;
    uint32_t sn = 0;
    uint64_t sk = 0;
    if (!wide) {
      for (uint32_t j = 0; j < deg; ++j) {
        const uint32_t kc = k[cb + j];
        const uint32_t cn = leaf_kids ? 1u : w_n[cb + j];
        const uint64_t ck = leaf_kids ? kc : w_k[cb + j];
        sn += cn;
        sk += ck;
        if (full && kc < E.c_t) cut_point(g, E, cb + j, cn, ck);
      }
    }
    uint64_t todo = __ballot(wide);
    while (todo) {
      const uint32_t j = __builtin_ctzll(todo);
      todo &= todo - 1;
      const uint32_t b = __shfl(cb, static_cast<int>(j), 64), n = __shfl(deg, static_cast<int>(j), 64);
      const bool pfull = __shfl(static_cast<int>(full), static_cast<int>(j), 64) != 0;
      uint32_t pn = 0;
      uint64_t pk = 0;
      for (uint32_t i = lane; i < n; i += kWave) {
        const uint32_t kc = k[b + i];
        const uint32_t cn = leaf_kids ? 1u : w_n[b + i];
        const uint64_t ck = leaf_kids ? kc : w_k[b + i];
        pn += cn;
        pk += ck;
        if (pfull && kc < E.c_t) cut_point(g, E, b + i, cn, ck);
      }
      pn = wave_sum_u32(pn);
      pk = dev::wave_sum_u64(pk);
      if (lane == j) {
        sn = pn;
        sk = pk;
      }
    }
    if (in) {
      w_n[u] = 1 + sn;
      w_k[u] = ku + sk;
      const uint32_t peer = g.d.node_peer[E.nbase + u];
      if (sn) atomicAdd(below + peer, static_cast<unsigned long long>(sn));
      if (sk) atomicAdd(carried + peer, static_cast<unsigned long long>(sk));
    }
  }
}

// k_downstream_level's launch: one block per work item, stream order the only
// order between the launches' waves.
__global__ __launch_bounds__(kDownBlock) void k_report_level(CutArgs g, uint32_t w0) {
  const DownWork W = g.d.work[w0 + blockIdx.x];
  const DownEntry E = g.d.entries[W.entry];
  if (W.level >= E.depth) return;  // (block-uniform; leaves take no work)
  const uint32_t* __restrict__ lv = g.d.levels + E.lvl0;
  report_nodes(g, E, lv, W.level, max(W.lo, lv[W.level]), min(W.hi, lv[W.level + 1]), threadIdx.x, kDownBlock);
}

// k_downstream_top's: one block per entry walks the levels [0, top) upwards,
// a barrier between two levels.
__global__ __launch_bounds__(kDownBlock) void k_report_top(CutArgs g) {
  const DownEntry E = g.d.entries[blockIdx.x];
  if (!E.c_t || g.d.entries[blockIdx.x + 1].strip0 == E.strip0) return;  // (block-uniform)
  const uint32_t* __restrict__ lv = g.d.levels + E.lvl0;
  for (uint32_t d = min(E.top, E.depth); d-- > 0;) {
    report_nodes(g, E, lv, d, lv[d], lv[d + 1], threadIdx.x, kDownBlock);
    __syncthreads();
  }
}

// ---- a rank's share of the report (ps_dist_report) -------------------------------

// k_report_nodes for a rank's own numbering (kernels.hpp, DistArgs): the same k
// per node and the same two load adds; a partial pair per (strip, level) in
// k_audience_hops' slots -- part0 + (s - strip0) + (d - 1): levels a strip
// does not meet, empty ones among them, leave gaps and no two pairs share a
// slot --; the k word at the node's own place, none for a root.  The waves
// behind the strips' take an entry each and add its root's share of `sent`: a
// root's owner may own no other node of the topic, and then no strip of it.
template <bool kLoad, bool kHops, bool kWords>
__global__ __launch_bounds__(kAudBlock) void k_dist_nodes(DrainArgs a, DistArgs g) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t s = __builtin_amdgcn_readfirstlane(blockIdx.x * (kAudBlock / kWave) + threadIdx.x / kWave);
  unsigned long long* const sent = reinterpret_cast<unsigned long long*>(g.sent);
  if (s >= g.n_strips) {
    if (!kLoad || s - g.n_strips >= g.n || lane != 0) return;
    const DistEntry E = g.entries[s - g.n_strips];
    if (E.root == kLoadNoRoot || !E.c_t) return;
    const uint32_t deg = g.row_ptr[E.root + 1] - g.row_ptr[E.root];
    if (deg) atomicAdd(sent + g.node_peer[E.root], static_cast<unsigned long long>(E.c_t) * deg);
    return;
  }
  const AudStrip S = g.strips[s];
  uint32_t lo = 0, hi = g.n;  // the last entry whose first strip is <= s: the one that holds it
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (g.entries[mid].strip0 <= s) lo = mid + 1;
    else hi = mid;
  }
  if (lo == 0) return;
  const DistEntry E = g.entries[lo - 1];
  const bool tree = E.tree != 0;  // (wave-uniform, as everything read from E and S)
  if (!kLoad && !tree) return;
  const DrainTopic T = a.topics[S.topic];
  const bool gather = T.flags & kDrainGather;
  const uint8_t* __restrict__ vin = g.verdict + S.v0;
  const bool all_full = !g.count_rows && g.n_exc[s] == 0;
  const uint32_t end = S.u0 + S.n;
  unsigned long long* const recv = reinterpret_cast<unsigned long long*>(g.recv);
  uint32_t* const kout = kWords ? g.k + E.n0 : nullptr;
  // the level of the strip's first node: the last one that starts at or before
  // it (an empty level starts where the next one does)
  const uint32_t* __restrict__ lv = g.levels + E.lvl0;
  uint32_t d = 0;
  if (kHops && tree) {
    lo = 0, hi = E.depth + 1;
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (lv[mid] <= S.u0) lo = mid + 1;
      else hi = mid;
    }
    d = lo ? lo - 1 : 0;
  }
  for (uint32_t u = S.u0; u < end;) {
    bool hop = false;
    uint32_t ue = end;
    if (kHops && tree) {
      while (d <= E.depth && lv[d + 1] <= u) ++d;
      hop = d >= 1 && d <= E.depth;  // (a strip holds no root)
      if (hop) ue = min(end, lv[d + 1]);
    }
    uint32_t reached = 0;  // (wave-uniform)
    uint64_t deliv = 0;
    if (all_full && !kLoad && !kWords) {
      // every node holds c_t: the sums follow from the bounds
      reached = ue - u;
      deliv = static_cast<uint64_t>(reached) * E.c_t;
    } else {
      for (uint32_t i0 = u; i0 < ue; i0 += kWave) {
        const uint32_t i = min(i0 + lane, ue - 1);
        const bool in = i0 + lane < ue;
        uint32_t peer = 0, deg = 0;
        if (kLoad) {
          peer = g.node_peer[S.nbase + i];
          deg = g.row_ptr[S.nbase + i + 1] - g.row_ptr[S.nbase + i];
        }
        uint32_t k = in ? E.c_t : 0u;
        if (!all_full) {
          const uint32_t v = vin[i - S.u0];
          const bool full = !gather && v == kDrainRowAny;
          const bool count = in && (gather || ((v & kDrainRowAny) && (!full || g.count_rows)));
          k = in && full && !count ? E.c_t : 0u;
          uint64_t todo = __ballot(count);
          while (todo) {
            const uint32_t j = __builtin_ctzll(todo);
            todo &= todo - 1;
            const uint32_t c = load_count_row(a, T, i0 + j, lane);
            if (lane == j) k = c;
          }
        }
        if (kLoad && k) {
          atomicAdd(recv + peer, static_cast<unsigned long long>(k));
          if (deg) atomicAdd(sent + peer, static_cast<unsigned long long>(k) * deg);
        }
        if (kWords && in && tree && i < E.nn) kout[i] = k;
        if (kHops && hop) {
          reached += __popcll(__ballot(k != 0));
          deliv += wave_sum_u32(k);
        }
      }
    }
    if (kHops && hop && lane == 0) {
      const uint32_t slot = min(E.part0 + (s - E.strip0) + (d - 1), g.n_parts - 1);
      g.part_reached[slot] = reached;
      g.part_deliv[slot] = deliv;
    }
    u = ue;
  }
}

// k_audience_hops_sum for a rank's own level table: one block per (entry,
// column) adds the partials of the strips that meet the column's levels -- a
// level's first to its last node; an empty level has none -- and the level's
// size into the entry's row: one writer per word, plain loads and stores.
__global__ __launch_bounds__(kHopsSumBlock) void k_dist_hops_sum(DistArgs g) {
  __shared__ uint64_t part[2][kHopsSumBlock / kWave];
  const uint32_t h = blockIdx.y + 1;
  const DistEntry E = g.entries[blockIdx.x];
  if (!E.tree || !E.c_t || h > min(E.depth, kHopsCols - 1) || g.entries[blockIdx.x + 1].strip0 == E.strip0) return;
  const uint32_t* __restrict__ lv = g.levels + E.lvl0;
  const uint32_t d_hi = h == kHopsCols - 1 ? E.depth : h;
  const uint32_t u0 = lv[1];  // (the entry's strips start at its first node that is no root)
  uint64_t r = 0, dl = 0;
  for (uint32_t d = h; d <= d_hi; ++d) {
    if (lv[d + 1] <= lv[d]) continue;  // (block-uniform)
    const uint32_t sa = (lv[d] - u0) / E.per, sb = (lv[d + 1] - 1 - u0) / E.per;  // (relative to strip0)
    const uint32_t p0 = E.part0 + (d - 1);
    for (uint32_t s0 = sa + threadIdx.x; s0 <= sb; s0 += kHopsSumBlock) {
      const uint32_t slot = min(p0 + s0, g.n_parts - 1);
      r += g.part_reached[slot];
      dl += g.part_deliv[slot];
    }
  }
  r = dev::wave_sum_u64(r);
  dl = dev::wave_sum_u64(dl);
  if ((threadIdx.x & (kWave - 1)) == 0) {
    part[0][threadIdx.x / kWave] = r;
    part[1][threadIdx.x / kWave] = dl;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    r = dl = 0;
    for (uint32_t w = 0; w < kHopsSumBlock / kWave; ++w) {
      r += part[0][w];
      dl += part[1][w];
    }
    const size_t at = static_cast<size_t>(blockIdx.x) * kHopsCols + h;
    g.nodes[at] += lv[d_hi + 1] - lv[h];
    g.reached[at] += r;
    g.deliv[at] += dl;
  }
}

// One add of (vn, vk) into the pair of words at (pn, pk), the active lanes of
// a wave a push each.  Where every active lane of the wave pushes to one pair
// -- siblings of one wide parent lie side by side -- the wave sums first and
// one lane adds.
__device__ __forceinline__ void dist_push(unsigned long long* pn, unsigned long long* pk, uint64_t vn, uint64_t vk,
                                          bool on) {
  const uint64_t act = __ballot(on);
  if (!act) return;
  const uint32_t first = __builtin_ctzll(act);
  const uint64_t key = reinterpret_cast<uint64_t>(pn);
  const uint64_t key0 = static_cast<uint64_t>(__shfl(static_cast<uint32_t>(key >> 32), static_cast<int>(first), 64)) << 32 |
                        __shfl(static_cast<uint32_t>(key), static_cast<int>(first), 64);
  if (__popcll(act) > 1 && __ballot(on && key != key0) == 0) {
    const uint64_t sn = dev::wave_sum_u64(on ? vn : 0ull), sk = dev::wave_sum_u64(on ? vk : 0ull);
    if ((threadIdx.x & (kWave - 1)) == first) {
      if (sn) atomicAdd(pn, static_cast<unsigned long long>(sn));
      if (sk) atomicAdd(pk, static_cast<unsigned long long>(sk));
    }
    return;
  }
  if (on) {
    if (vn) atomicAdd(pn, static_cast<unsigned long long>(vn));
    if (vk) atomicAdd(pk, static_cast<unsigned long long>(vk));
  }
}

// One block per work item of this launch, a thread per node of level `level`
// (kernels.hpp, DistArgs).  What the node's accumulator holds was added by the
// launches of the levels below, on this rank and -- through the exchanges and
// k_dist_apply between them -- on the others: stream order and the
// transport's are the only order.
__global__ __launch_bounds__(kDownBlock) void k_dist_sweep_level(DistArgs g, uint32_t level, uint32_t w0) {
  const DistWork W = g.work[w0 + blockIdx.x];
  const DistEntry E = g.entries[W.entry];
  const uint32_t* __restrict__ lv = g.levels + E.lvl0;
  if (!E.tree || !E.c_t || level > E.depth || !E.nn) return;  // (block-uniform)
  const uint32_t lo = max(W.lo, lv[level]), hi = min(min(W.hi, lv[level + 1]), E.nn);
  const uint32_t u = lo + threadIdx.x;
  const bool in = u < hi;
  const uint32_t uc = in ? u : E.nn - 1;  // (clamped into the entry's words)
  unsigned long long* const acc_n = reinterpret_cast<unsigned long long*>(g.acc_n) + E.n0;
  unsigned long long* const acc_k = reinterpret_cast<unsigned long long*>(g.acc_k) + E.n0;
  unsigned long long* const below = reinterpret_cast<unsigned long long*>(g.below);
  unsigned long long* const carried = reinterpret_cast<unsigned long long*>(g.carried);
  const uint64_t an = in ? acc_n[uc] : 0ull, ak = in ? acc_k[uc] : 0ull;
  if (in) {
    const uint32_t peer = g.node_peer[E.nbase + uc];
    if (an) atomicAdd(below + peer, static_cast<unsigned long long>(an));
    if (ak) atomicAdd(carried + peer, static_cast<unsigned long long>(ak));
  }
  if (level == 0) return;  // (block-uniform: a root pushes nothing)
  const uint64_t wn = 1 + an, wk = g.k[E.n0 + uc] + ak;
  const uint32_t par = g.node_parent[E.nbase + uc];
  unsigned long long *pn = nullptr, *pk = nullptr;
  bool on = false;
  if (in && par != kNoneNode) {
    const uint32_t p = min(par - E.nbase, E.nn - 1);  // (par >= nbase: the parent is a node of this topic)
    on = par >= E.nbase;
    pn = acc_n + p;
    pk = acc_k + p;
  } else if (in && g.gslot) {
    const uint32_t gs = g.gslot[E.nbase + uc];
    const uint32_t owner = gs >> kRemoteRankShift;
    if (gs != kNoneNode && owner < g.world && g.n_send) {
      const uint32_t rec = min(g.send_base[E.sb0 + level * g.world + owner] + (gs & kRemoteIdMask), g.n_send - 1);
      on = true;
      pn = reinterpret_cast<unsigned long long*>(&g.send[rec].n);
      pk = reinterpret_cast<unsigned long long*>(&g.send[rec].k);
    }
  }
  dist_push(pn, pk, wn, wk, on);
}

// One block per apply item, a thread per received record: into the
// accumulator of the parent the record belongs to.  Two ranks may hold
// children of one parent: atomics here too.
__global__ __launch_bounds__(kDownBlock) void k_dist_apply(DistArgs g, uint32_t a0) {
  const DistApply A = g.apply[a0 + blockIdx.x];
  const DistEntry E = g.entries[A.entry];
  if (threadIdx.x >= A.n || !E.nn) return;
  const uint32_t r = min(A.rec0 + threadIdx.x, g.n_recv - 1), pl = min(A.pl0 + threadIdx.x, g.n_plist - 1);
  const DistRec R = g.rcv[r];
  const uint32_t par = g.plist[pl];
  if (par < E.nbase) return;
  const uint32_t p = min(par - E.nbase, E.nn - 1);
  if (R.n) atomicAdd(reinterpret_cast<unsigned long long*>(g.acc_n) + E.n0 + p, static_cast<unsigned long long>(R.n));
  if (R.k) atomicAdd(reinterpret_cast<unsigned long long*>(g.acc_k) + E.n0 + p, static_cast<unsigned long long>(R.k));
}

// ---- a rank's share of the cut (ps_dist_cut) --------------------------------------

// k_dist_nodes<false, false, true> (kernels.hpp, DistCutArgs): the same k per
// node into the k word, none for a root, and what the node lacks of the
// window's messages into missed of its peer.
__global__ __launch_bounds__(kAudBlock) void k_dist_cut_nodes(DrainArgs a, DistCutArgs g) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t s = __builtin_amdgcn_readfirstlane(blockIdx.x * (kAudBlock / kWave) + threadIdx.x / kWave);
  if (s >= g.d.n_strips) return;
  const AudStrip S = g.d.strips[s];
  uint32_t lo = 0, hi = g.d.n;  // the last entry whose first strip is <= s: the one that holds it
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (g.d.entries[mid].strip0 <= s) lo = mid + 1;
    else hi = mid;
  }
  if (lo == 0) return;
  const DistEntry E = g.d.entries[lo - 1];
  if (!E.tree) return;  // (wave-uniform, as everything read from E and S)
  const DrainTopic T = a.topics[S.topic];
  const bool gather = T.flags & kDrainGather;
  const uint8_t* __restrict__ vin = g.d.verdict + S.v0;
  const bool all_full = !g.d.count_rows && g.d.n_exc[s] == 0;
  const uint32_t end = S.u0 + S.n;
  unsigned long long* const missed = reinterpret_cast<unsigned long long*>(g.missed);
  uint32_t* const kout = g.d.k + E.n0;
  for (uint32_t i0 = S.u0; i0 < end; i0 += kWave) {
    const uint32_t i = min(i0 + lane, end - 1);
    const bool in = i0 + lane < end;
    uint32_t k = in ? E.c_t : 0u;
    if (!all_full) {
      const uint32_t v = vin[i - S.u0];
      const bool full = !gather && v == kDrainRowAny;
      const bool count = in && (gather || ((v & kDrainRowAny) && (!full || g.d.count_rows)));
      k = in && full && !count ? E.c_t : 0u;
      uint64_t todo = __ballot(count);
      while (todo) {
        const uint32_t j = __builtin_ctzll(todo);
        todo &= todo - 1;
        const uint32_t c = load_count_row(a, T, i0 + j, lane);
        if (lane == j) k = c;
      }
    }
    if (in && i < E.nn) {
      kout[i] = k;
      if (k < E.c_t) atomicAdd(missed + g.d.node_peer[S.nbase + i], static_cast<unsigned long long>(E.c_t - k));
    }
  }
}

// One block per fill item, a thread per plist record this rank holds as the
// parents' owner: the parent's k into the word its children's rank reads it
// from.  A root's k word stays 0: it counts as full.
__global__ __launch_bounds__(kDownBlock) void k_dist_cut_fill(DistCutArgs g) {
  const DistApply A = g.fill[blockIdx.x];
  const DistEntry E = g.d.entries[A.entry];
  if (threadIdx.x >= A.n || !E.nn || !g.n_down_send || !g.d.n_plist) return;
  const uint32_t w = min(A.rec0 + threadIdx.x, g.n_down_send - 1), pl = min(A.pl0 + threadIdx.x, g.d.n_plist - 1);
  const uint32_t par = g.d.plist[pl];
  if (par < E.nbase) return;
  const uint32_t p = min(par - E.nbase, E.nn - 1);
  g.down_send[w] = par == E.root ? E.c_t : g.d.k[E.n0 + p];
}

// k_dist_sweep_level's launch (kernels.hpp, DistCutArgs): the same accumulator
// and the same push; where the node lacks messages under a full parent, its
// subtree is what the cut lost.  The parent's k is a word this rank wrote
// (k_dist_cut_nodes) or received ahead of the sweep (the downward exchange).
__global__ __launch_bounds__(kDownBlock) void k_dist_cut_level(DistCutArgs g, uint32_t level, uint32_t w0) {
  const DistWork W = g.d.work[w0 + blockIdx.x];
  const DistEntry E = g.d.entries[W.entry];
  const uint32_t* __restrict__ lv = g.d.levels + E.lvl0;
  if (!E.tree || !E.c_t || level == 0 || level > E.depth || !E.nn) return;  // (block-uniform: a root adds and pushes nothing)
  const uint32_t lo = max(W.lo, lv[level]), hi = min(min(W.hi, lv[level + 1]), E.nn);
  const uint32_t u = lo + threadIdx.x;
  const bool in = u < hi;
  const uint32_t uc = in ? u : E.nn - 1;  // (clamped into the entry's words)
  unsigned long long* const acc_n = reinterpret_cast<unsigned long long*>(g.d.acc_n) + E.n0;
  unsigned long long* const acc_k = reinterpret_cast<unsigned long long*>(g.d.acc_k) + E.n0;
  const uint64_t an = in ? acc_n[uc] : 0ull, ak = in ? acc_k[uc] : 0ull;
  const uint32_t k = g.d.k[E.n0 + uc];
  const uint32_t par = g.d.node_parent[E.nbase + uc];
  unsigned long long *pn = nullptr, *pk = nullptr;
  bool on = false;
  uint32_t kp = 0;  // the parent's k
  if (in && par != kNoneNode) {
    const uint32_t p = min(par - E.nbase, E.nn - 1);  // (par >= nbase: the parent is a node of this topic)
    on = par >= E.nbase;
    pn = acc_n + p;
    pk = acc_k + p;
    kp = par == E.root ? E.c_t : g.d.k[E.n0 + p];
  } else if (in && g.d.gslot) {
    const uint32_t gs = g.d.gslot[E.nbase + uc];
    const uint32_t owner = gs >> kRemoteRankShift;
    if (gs != kNoneNode && owner < g.d.world && g.d.n_send && g.n_down_recv) {
      const uint32_t at = E.sb0 + level * g.d.world + owner, j = gs & kRemoteIdMask;
      const uint32_t rec = min(g.d.send_base[at] + j, g.d.n_send - 1);
      on = true;
      pn = reinterpret_cast<unsigned long long*>(&g.d.send[rec].n);
      pk = reinterpret_cast<unsigned long long*>(&g.d.send[rec].k);
      kp = g.down_recv[min(g.down_base[at] + j, g.n_down_recv - 1)];
    }
  }
  if (on && k < E.c_t && kp == E.c_t) {
    const uint32_t peer = g.d.node_peer[E.nbase + uc];
    atomicAdd(reinterpret_cast<unsigned long long*>(g.cuts) + peer, 1ull);
    if (an) atomicAdd(reinterpret_cast<unsigned long long*>(g.orphaned) + peer, static_cast<unsigned long long>(an));
    atomicAdd(reinterpret_cast<unsigned long long*>(g.lost) + peer,
              static_cast<unsigned long long>(static_cast<uint64_t>(E.c_t) * (1 + an) - (k + ak)));
  }
  dist_push(pn, pk, 1 + an, k + ak, on);
}

// ---- a rank's share of the blame (ps_dist_blame) -----------------------------------

// One block per fill item of the level about to run, a thread per plist record
// this rank holds as the parents' owner: the parent's pair into the 8 bytes
// its children's rank reads it from.  A full parent and the entry's root --
// whose words nothing writes -- read as (none, none).
__global__ __launch_bounds__(kDownBlock) void k_dist_blame_fill(DistBlameArgs g, uint32_t f0) {
  const DistApply A = g.fill[f0 + blockIdx.x];
  const DistEntry E = g.d.entries[A.entry];
  if (threadIdx.x >= A.n || !E.nn || !g.n_down_send || !g.d.n_plist) return;
  const uint32_t w = min(A.rec0 + threadIdx.x, g.n_down_send - 1), pl = min(A.pl0 + threadIdx.x, g.d.n_plist - 1);
  const uint32_t par = g.d.plist[pl];
  if (par < E.nbase) return;
  const uint32_t p = E.n0 + min(par - E.nbase, E.nn - 1);
  const bool full = par == E.root || g.d.k[p] >= E.c_t;
  g.down_send[w] = full ? make_uint2(kBlameNone, kBlameNone) : make_uint2(g.cut_peer[p], g.cut_hop[p]);
}

// k_dist_sweep_level's launch, walked the other way (kernels.hpp,
// DistBlameArgs): a thread per node of level `level` >= 1.  The parent's pair
// is two words the launch of the level above wrote on this rank, or 8 bytes
// that level's owner filled and this level's exchange brought.
__global__ __launch_bounds__(kDownBlock) void k_dist_blame_level(DistBlameArgs g, uint32_t level, uint32_t w0) {
  const DistWork W = g.d.work[w0 + blockIdx.x];
  const DistEntry E = g.d.entries[W.entry];
  const uint32_t* __restrict__ lv = g.d.levels + E.lvl0;
  if (!E.tree || !E.c_t || level == 0 || level > E.depth || !E.nn) return;  // (block-uniform: a root has no record)
  const uint32_t lo = max(W.lo, lv[level]), hi = min(min(W.hi, lv[level + 1]), E.nn);
  const uint32_t u = lo + threadIdx.x;
  if (u >= hi) return;
  uint2 cut = make_uint2(kBlameNone, kBlameNone);
  if (g.d.k[E.n0 + u] < E.c_t) {
    uint2 up = cut;  // the parent's pair; none: it is full
    const uint32_t par = g.d.node_parent[E.nbase + u];
    if (par != kNoneNode) {
      if (par >= E.nbase && par != E.root) {
        const uint32_t p = E.n0 + min(par - E.nbase, E.nn - 1);
        if (g.d.k[p] < E.c_t) up = make_uint2(g.cut_peer[p], g.cut_hop[p]);
      }
    } else if (g.d.gslot) {
      const uint32_t gs = g.d.gslot[E.nbase + u];
      const uint32_t owner = gs >> kRemoteRankShift;
      if (gs != kNoneNode && owner < g.d.world && g.n_down_recv)
        up = g.down_recv[min(g.down_base[E.sb0 + level * g.d.world + owner] + (gs & kRemoteIdMask), g.n_down_recv - 1)];
    }
    cut = up.x == kBlameNone ? make_uint2(g.d.node_peer[E.nbase + u], level) : up;
  }
  g.cut_peer[E.n0 + u] = cut.x;
  g.cut_hop[E.n0 + u] = cut.y;
}

// the entry that holds strip s: the last one whose first strip is <= s (false: none)
__device__ __forceinline__ bool dist_entry_of(const DistArgs& d, uint32_t s, DistEntry* E) {
  uint32_t lo = 0, hi = d.n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (d.entries[mid].strip0 <= s) lo = mid + 1;
    else hi = mid;
  }
  if (lo == 0) return false;
  *E = d.entries[lo - 1];
  return true;
}

// k_blame_count over a rank's strips: one wave per strip, one node per lane.
// The wave behind the last strip writes the closing 0.
__global__ __launch_bounds__(kAudBlock) void k_dist_blame_count(DistBlameArgs g) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t s = __builtin_amdgcn_readfirstlane(blockIdx.x * (kAudBlock / kWave) + threadIdx.x / kWave);
  if (s > g.d.n_strips) return;
  uint32_t c = 0;
  DistEntry E;
  if (s < g.d.n_strips && dist_entry_of(g.d, s, &E) && E.tree) {
    const AudStrip S = g.d.strips[s];
    const uint32_t* __restrict__ k = g.d.k + E.n0;
    const uint32_t end = min(S.u0 + S.n, E.nn);
    for (uint32_t u = S.u0 + lane; u < end; u += kWave) c += k[u] < E.c_t;
  }
  c = wave_sum_u32(c);
  if (lane == 0) g.n_rec[s] = c;
}

// k_blame_emit over a rank's strips: the nodes that lack messages, in the
// rank's own node order (ballot and lane prefix), from the strip's offset on.
// The first n + 1 threads of the grid leave the entries' record offsets.
__global__ __launch_bounds__(kAudBlock) void k_dist_blame_emit(DistBlameArgs g) {
  const uint32_t tid = blockIdx.x * kAudBlock + threadIdx.x;
  if (tid <= g.d.n) g.rec_off[tid] = g.off[min(g.d.entries[tid].strip0, g.d.n_strips)];
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t s = __builtin_amdgcn_readfirstlane(blockIdx.x * (kAudBlock / kWave) + threadIdx.x / kWave);
  if (s >= g.d.n_strips || g.n_rec[s] == 0) return;
  DistEntry E;
  if (!dist_entry_of(g.d, s, &E) || !E.tree || !E.nn) return;
  const AudStrip S = g.d.strips[s];
  const uint32_t* __restrict__ lv = g.d.levels + E.lvl0;
  const uint32_t* __restrict__ k = g.d.k + E.n0;
  const uint32_t* __restrict__ cut_peer = g.cut_peer + E.n0;
  const uint32_t* __restrict__ cut_hop = g.cut_hop + E.n0;
  const uint32_t end = min(S.u0 + S.n, E.nn);
  uint64_t at = g.off[s];
  for (uint32_t u0 = S.u0; u0 < end; u0 += kWave) {
    const uint32_t u = min(u0 + lane, end - 1);
    const uint32_t have = k[u];
    const bool rec = u0 + lane < end && have < E.c_t;
    const uint64_t b = __ballot(rec);
    const uint64_t to = at + __popcll(b & ((1ull << lane) - 1));
    if (rec && to < g.cap) {
      if (g.rec_peer) g.rec_peer[to] = g.d.node_peer[E.nbase + u];
      if (g.rec_cut_peer) g.rec_cut_peer[to] = cut_peer[u];
      if (g.rec_hop) g.rec_hop[to] = blame_level_of(lv, E.depth, u);
      if (g.rec_cut_hop) g.rec_cut_hop[to] = cut_hop[u];
      if (g.rec_missed) g.rec_missed[to] = E.c_t - have;
    }
    at += __popcll(b);
  }
}

// ---- hops and duplicate copies, meshes too (ps_topic_spread) ---------------------

constexpr uint32_t kSpreadBlock = 256;

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = max(v, static_cast<uint32_t>(__shfl_xor(v, m, 64)));
  return v;
}

// One wave per strip, one node per lane: k_audience_weights' k into the node's
// word, and into recv of its peer; the strip's nodes with k > 0 and, for a
// tree, those with k == 0 into the entry's two counts, an add per wave each.
__global__ __launch_bounds__(kAudBlock) void k_spread_nodes(DrainArgs a, SpreadArgs g) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t s = __builtin_amdgcn_readfirstlane(blockIdx.x * (kAudBlock / kWave) + threadIdx.x / kWave);
  if (s >= g.n_strips) return;
  const AudStrip S = g.strips[s];
  uint32_t lo = 0, hi = g.n;  // the last entry whose first strip is <= s: the one that holds it
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (g.entries[mid].strip0 <= s) lo = mid + 1;
    else hi = mid;
  }
  if (lo == 0) return;
  const uint32_t ei = lo - 1;
  const SpreadEntry E = g.entries[ei];
  if (!E.c_t || S.n == 0 || S.u0 + S.n > E.nn) return;  // (the strip lies within the entry's words)
  const DrainTopic T = a.topics[S.topic];
  const bool gather = T.flags & kDrainGather;
  const uint8_t* __restrict__ vin = g.verdict + S.v0;
  uint32_t* __restrict__ kout = g.k + E.n0;
  const bool all_full = !g.count_rows && g.n_exc[s] == 0;
  uint32_t n_zero = 0, n_held = 0;  // (wave-uniform)
  for (uint32_t i0 = 0; i0 < S.n; i0 += kWave) {
    const uint32_t i = i0 + lane;
    const bool in = i < S.n;
    uint32_t k = E.c_t;
    if (!all_full) {
      const uint32_t v = vin[min(i, S.n - 1)];
      const bool full = !gather && v == kDrainRowAny;
      const bool count = in && (gather || ((v & kDrainRowAny) && (!full || g.count_rows)));
      k = full && !count ? E.c_t : 0u;
      uint64_t todo = __ballot(count);
      while (todo) {
        const uint32_t j = __builtin_ctzll(todo);
        todo &= todo - 1;
        const uint32_t c = load_count_row(a, T, S.u0 + i0 + j, lane);
        if (lane == j) k = c;
      }
    }
    if (in) {
      kout[S.u0 + i] = k;
      const uint32_t peer = g.node_peer[E.nbase + S.u0 + i];
      if (k && peer < g.n_peers) atomicAdd(reinterpret_cast<unsigned long long*>(g.recv) + peer, static_cast<unsigned long long>(k));
    }
    const uint32_t held = __popcll(__ballot(in && k != 0));
    n_held += held;
    n_zero += min(S.n - i0, kWave) - held;
  }
  if (lane == 0) {
    // (a tree's nodes are its peers; a mesh's are counted by k_spread_unreached)
    if (n_zero && !E.mesh)
      atomicAdd(reinterpret_cast<unsigned long long*>(g.unreached) + ei, static_cast<unsigned long long>(n_zero));
    if (n_held) atomicAdd(reinterpret_cast<unsigned long long*>(g.holders) + ei, static_cast<unsigned long long>(n_held));
  }
}

// the child entry that names node v of entry E: 1 where v is a non-root node
// without messages and this entry is the one that marks its hop word
__device__ __forceinline__ uint32_t spread_name(const SpreadArgs& g, const SpreadEntry& E, uint32_t v) {
  const uint32_t r = v - E.nbase;
  if (r == 0 || r >= E.nn || g.k[E.n0 + r] != 0) return 0;
  uint32_t* const h = g.hop + E.n0 + r;
  return *h == kSpreadNone && atomicCAS(h, kSpreadNone, kSpreadNamed) == kSpreadNone ? 1u : 0u;
}

// One wave per strip of a mesh entry, one node per lane, the wave of the
// entry's first strip the root too: the node's child entries one by one, or
// by the whole wave where it has more than g.wide; a non-root target without
// messages is counted once, by the entry that marks its hop word (kernels.hpp).
__global__ __launch_bounds__(kAudBlock) void k_spread_unreached(SpreadArgs g) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t s = __builtin_amdgcn_readfirstlane(blockIdx.x * (kAudBlock / kWave) + threadIdx.x / kWave);
  if (s >= g.n_strips) return;
  const AudStrip S = g.strips[s];
  uint32_t lo = 0, hi = g.n;  // the last entry whose first strip is <= s: the one that holds it
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (g.entries[mid].strip0 <= s) lo = mid + 1;
    else hi = mid;
  }
  if (lo == 0) return;
  const uint32_t ei = lo - 1;
  const SpreadEntry E = g.entries[ei];
  if (!E.c_t || !E.mesh || S.n == 0 || S.u0 + S.n > E.nn) return;
  const uint32_t n_items = S.n + (E.strip0 == s ? 1u : 0u);  // (item S.n: the root)
  uint32_t cnt = 0;
  for (uint32_t i0 = 0; i0 < n_items; i0 += kWave) {  // (wave-uniform)
    const uint32_t i = i0 + lane;
    uint32_t r0 = 0, deg = 0;
    if (i < n_items) {
      const uint32_t u = i < S.n ? S.u0 + i : 0u;
      r0 = min(g.row_ptr[E.nbase + u], g.n_edges);
      const uint32_t r1 = min(g.row_ptr[E.nbase + u + 1], g.n_edges);
      deg = r1 > r0 ? r1 - r0 : 0u;
    }
    const uint32_t dn = deg <= g.wide ? deg : 0u;
    for (uint32_t j = 0; j < dn; ++j) cnt += spread_name(g, E, g.col[r0 + j]);
    uint64_t todo = __ballot(deg > g.wide);
    while (todo) {  // (a node of many entries: lanes across them)
      const int src = __builtin_ctzll(todo);
      todo &= todo - 1;
      const uint32_t w0 = __shfl(r0, src, 64), w1 = w0 + __shfl(deg, src, 64);
      for (uint32_t j = w0 + lane; j < w1; j += kWave) cnt += spread_name(g, E, g.col[j]);
    }
  }
  cnt = wave_sum_u32(cnt);
  if (lane == 0 && cnt) atomicAdd(reinterpret_cast<unsigned long long*>(g.unreached) + ei, static_cast<unsigned long long>(cnt));
}

// The child entry of a frontier item of entry E that names node v: where the
// target forwards (the root, or a node whose row holds messages), the item's
// kq into copies of the target's peer; true: this entry is the one that gave
// the (non-root) target *vr its hop `next`, so it joins the next frontier.
__device__ __forceinline__ bool spread_edge(const SpreadArgs& g, const SpreadEntry& E, uint32_t v, uint32_t kq,
                                            uint32_t next, uint32_t* vr) {
  const uint32_t r = v - E.nbase;  // (a node of another topic, or no node at all: past nn either way)
  *vr = r;
  if (r >= E.nn) return false;
  if (r != 0 && g.k[E.n0 + r] == 0) return false;
  const uint32_t peer = g.node_peer[E.nbase + r];
  if (peer < g.n_peers) atomicAdd(reinterpret_cast<unsigned long long*>(g.copies) + peer, static_cast<unsigned long long>(kq));
  if (r == 0) return false;
  uint32_t* const h = g.hop + E.n0 + r;
  // (a stale kSpreadNone costs a compare-and-swap that fails; the word never returns to it)
  return *h == kSpreadNone && atomicCAS(h, kSpreadNone, next) == kSpreadNone;
}

// the lanes with `push` append (ei, vr) to the next queue: one add per wave
__device__ __forceinline__ void spread_append(const SpreadArgs& g, SpreadItem* __restrict__ qout, uint32_t* n_out, bool push,
                                              uint32_t ei, uint32_t vr, uint32_t lane) {
  const uint64_t b = __ballot(push);
  if (!b) return;  // (wave-uniform)
  const uint32_t leader = __builtin_ctzll(b);
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(n_out, static_cast<uint32_t>(__popcll(b)));
  base = __shfl(base, static_cast<int>(leader), 64);
  const uint32_t at = base + __popcll(b & ((1ull << lane) - 1));
  if (push && at < g.q_cap) qout[at] = SpreadItem{ei, vr};
}

// Launch L of the BFS (kernels.hpp): the waves stride over the frontier, a
// lane per item; items of at most g.wide child entries walk them lane by lane,
// in step up to the wave's longest, the others are walked one after the other
// by the whole wave.
__global__ __launch_bounds__(kSpreadBlock) void k_spread_level(SpreadArgs g, uint32_t L) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (kSpreadBlock / kWave) + threadIdx.x / kWave);
  const uint32_t n_waves = gridDim.x * (kSpreadBlock / kWave);
  if (blockIdx.x == 0 && threadIdx.x == 0) g.cnt[(L + 2) % 3] = 0;
  const uint32_t n_in = min(g.cnt[L % 3], g.q_cap);
  const SpreadItem* __restrict__ qin = g.queue + static_cast<size_t>(L & 1) * g.q_cap;
  SpreadItem* __restrict__ qout = g.queue + static_cast<size_t>((L + 1) & 1) * g.q_cap;
  uint32_t* const n_out = g.cnt + (L + 1) % 3;
  for (uint64_t i0 = static_cast<uint64_t>(wave) * kWave; i0 < n_in; i0 += static_cast<uint64_t>(n_waves) * kWave) {  // (wave-uniform)
    const bool in = i0 + lane < n_in;
    const SpreadItem q = qin[min(static_cast<uint32_t>(i0) + lane, n_in - 1)];
    const uint32_t ei = min(q.entry, g.n - 1);
    const SpreadEntry E = g.entries[ei];
    const bool ok = in && q.entry < g.n && E.c_t && q.node < E.nn;
    uint32_t kq = 0, r0 = 0, deg = 0;
    if (ok) {
      kq = q.node == 0 ? E.c_t : g.k[E.n0 + q.node];
      r0 = min(g.row_ptr[E.nbase + q.node], g.n_edges);
      const uint32_t r1 = min(g.row_ptr[E.nbase + q.node + 1], g.n_edges);
      deg = kq && r1 > r0 ? r1 - r0 : 0u;
    }
    const uint32_t dn = deg <= g.wide ? deg : 0u;
    const uint32_t d_max = wave_max_u32(dn);
    for (uint32_t j = 0; j < d_max; ++j) {
      uint32_t vr = 0;
      bool push = false;
      if (j < dn) push = spread_edge(g, E, g.col[r0 + j], kq, L + 1, &vr);
      spread_append(g, qout, n_out, push, ei, vr, lane);
    }
    uint64_t todo = __ballot(deg > g.wide);
    while (todo) {
      const int src = __builtin_ctzll(todo);
      todo &= todo - 1;
      const uint32_t we = __shfl(ei, src, 64), wk = __shfl(kq, src, 64);
      const uint32_t w0 = __shfl(r0, src, 64), w1 = w0 + __shfl(deg, src, 64);
      const SpreadEntry W = g.entries[we];
      for (uint32_t j0 = w0; j0 < w1; j0 += kWave) {
        uint32_t vr = 0;
        bool push = false;
        if (j0 + lane < w1) push = spread_edge(g, W, g.col[j0 + lane], wk, L + 1, &vr);
        spread_append(g, qout, n_out, push, we, vr, lane);
      }
    }
  }
}

// One wave per strip: the strip's nodes with k > 0 and a hop, 64 at a time,
// column by column of those the 64 hold -- the nodes of the column and their k
// summed over the wave, one lane adding the pair to the wave's LDS row -- and
// the row's pairs that are not zero into the entry's rows.
__global__ __launch_bounds__(kAudBlock) void k_spread_sum(SpreadArgs g) {
  __shared__ uint32_t hr[kAudBlock / kWave][kHopsCols];
  __shared__ uint64_t hd[kAudBlock / kWave][kHopsCols];
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t w = threadIdx.x / kWave;
  const uint32_t s = __builtin_amdgcn_readfirstlane(blockIdx.x * (kAudBlock / kWave) + w);
  for (uint32_t c = lane; c < kHopsCols; c += kWave) {
    hr[w][c] = 0;
    hd[w][c] = 0;
  }
  __syncthreads();
  uint32_t ei = 0, n_vis = 0;
  bool valid = s < g.n_strips;
  AudStrip S{};
  SpreadEntry E{};
  if (valid) {
    S = g.strips[s];
    uint32_t lo = 0, hi = g.n;  // the last entry whose first strip is <= s: the one that holds it
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (g.entries[mid].strip0 <= s) lo = mid + 1;
      else hi = mid;
    }
    valid = lo != 0;
    ei = valid ? lo - 1 : 0;
    E = g.entries[ei];
    valid = valid && E.c_t && S.n && S.u0 + S.n <= E.nn;
  }
  if (valid) {
    for (uint32_t i0 = 0; i0 < S.n; i0 += kWave) {
      const uint32_t i = i0 + lane;
      const uint32_t at = E.n0 + S.u0 + min(i, S.n - 1);
      const uint32_t k = i < S.n ? g.k[at] : 0u;
      const uint32_t h = g.hop[at];
      const bool vis = k != 0 && h != kSpreadNone;
      const uint32_t c = min(h, kHopsCols - 1);
      uint64_t todo = __ballot(vis);
      n_vis += __popcll(todo);
      while (todo) {
        const int src = __builtin_ctzll(todo);
        const uint32_t cc = __shfl(c, src, 64);
        const bool mine = vis && c == cc;
        const uint64_t m = __ballot(mine);
        todo &= ~m;
        const uint64_t kc = dev::wave_sum_u64(mine ? k : 0u);
        if (lane == 0) {
          hr[w][cc] += __popcll(m);
          hd[w][cc] += kc;
        }
      }
    }
  }
  __syncthreads();
  if (!valid) return;
  unsigned long long* const reached = reinterpret_cast<unsigned long long*>(g.reached) + static_cast<size_t>(ei) * kHopsCols;
  unsigned long long* const deliv = reinterpret_cast<unsigned long long*>(g.deliv) + static_cast<size_t>(ei) * kHopsCols;
  for (uint32_t c = lane; c < kHopsCols; c += kWave)
    if (hr[w][c]) {
      atomicAdd(reached + c, static_cast<unsigned long long>(hr[w][c]));
      atomicAdd(deliv + c, static_cast<unsigned long long>(hd[w][c]));
    }
  if (lane == 0 && n_vis) atomicAdd(reinterpret_cast<unsigned long long*>(g.visited) + ei, static_cast<unsigned long long>(n_vis));
}

// a thread per peer: what it was sent beyond what it received
__global__ __launch_bounds__(kSpreadBlock) void k_spread_dup(SpreadArgs g) {
  const uint32_t p = blockIdx.x * kSpreadBlock + threadIdx.x;
  if (p < g.n_peers) g.dup[p] = g.copies[p] - g.recv[p];
}

// ---- the spread pass behind every window (ps_spread_track) ------------------------

// One thread, behind a tracked window's last level launch: the frontier the
// next launch would have read still holds items -- the window is counted as
// truncated --, and the three counts stand at zero for the next window.
__global__ __launch_bounds__(kWave) void k_spread_track_close(uint32_t* cnt, uint32_t next, unsigned long long* truncated) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  if (cnt[next % 3] != 0) atomicAdd(truncated, 1ull);
  cnt[0] = 0;
  cnt[1] = 0;
  cnt[2] = 0;
}

// ---- the audience's totals and lists on the device (ps_drain_topics_begin) ---
// What the host loop of ps_drain_topics does between its waits.

// the entry whose records hold record k: the last i < n with exc_off[i] <= k
// (k below exc_off[n]: that entry is not empty)
__device__ __forceinline__ uint32_t aud_entry_of(const uint64_t* __restrict__ exc_off, uint32_t n, uint64_t k) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (exc_off[mid] <= k) lo = mid + 1;
    else hi = mid;
  }
  return lo - 1;  // (exc_off[0] = 0 <= k)
}

constexpr uint32_t kAudTotalsPer = 8;  // strip counts a thread has in flight

// One block per entry (and one behind the last): the full nodes of its strips
// summed -- a strided read, a wave sum, one LDS word per wave --, its first
// record, and its key: it creates the topic's shared list if a node holds it.
__global__ __launch_bounds__(kAudBlock) void k_audience_totals(AudAssign g) {
  __shared__ uint64_t part[kAudBlock / kWave];
  const uint32_t i = blockIdx.x;
  if (i == g.n) {
    if (threadIdx.x == 0) {
      g.exc_off[i] = g.strip_off[g.n_strips];
      g.ekey[i] = 0;
    }
    return;
  }
  const AudEntry E = g.entries[i];
  const uint32_t s1 = g.entries[i + 1].strip0;
  uint64_t sum = 0;
  // (kAudTotalsPer loads in flight: a hot topic has 10^5 strips, and one load
  // a turn leaves the block waiting on memory latency 400 times over)
  for (uint32_t s0 = E.strip0 + threadIdx.x; s0 < s1; s0 += kAudBlock * kAudTotalsPer) {
    uint32_t v[kAudTotalsPer];
#pragma unroll
    for (uint32_t k = 0; k < kAudTotalsPer; ++k) {
      const uint32_t s = s0 + k * kAudBlock;
      v[k] = s < s1 ? g.strip_full[s] : 0u;
    }
#pragma unroll
    for (uint32_t k = 0; k < kAudTotalsPer; ++k) sum += v[k];
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) sum += shfl_u64(sum, static_cast<int>((threadIdx.x & (kWave - 1)) ^ m));
  if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x / kWave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t full = 0;
#pragma unroll
    for (uint32_t w = 0; w < kAudBlock / kWave; ++w) full += part[w];
    g.n_full[i] = full;
    g.exc_off[i] = g.strip_off[E.strip0];
    g.ekey[i] = full ? 1ull << 32 | E.segs : 0ull;
  }
}

// One thread per record slot up to exc_cap (and one behind): a record that
// holds a message creates a private list of its topic's segments
__global__ __launch_bounds__(kAudBlock) void k_audience_keys(AudAssign g) {
  const uint32_t k = blockIdx.x * kAudBlock + threadIdx.x;
  if (k > g.exc_cap) return;
  const uint64_t n_exc = g.strip_off[g.n_strips];
  uint64_t key = 0;
  if (k < g.exc_cap && k < n_exc && (g.rec_verdict[k] & kDrainRowAny))
    key = 1ull << 32 | g.entries[aud_entry_of(g.exc_off, g.n, k)].segs;
  g.rkey[k] = key;
}

// One thread per entry and per record slot: the list numbers and first
// segments from the two sums.  Entry i's lists start behind the shared lists of
// the entries before and the private lists of the records before its first;
// record k's list lies behind its entry's shared one and the private lists of
// the records before k.  Thread 0 leaves the counts in the control block.
__global__ __launch_bounds__(kAudBlock) void k_audience_lists(AudAssign g) {
  const uint32_t x = blockIdx.x * kAudBlock + threadIdx.x;
  const uint64_t n_exc = g.strip_off[g.n_strips];
  const uint32_t used = static_cast<uint32_t>(n_exc < g.exc_cap ? n_exc : g.exc_cap);
  if (x < g.n) {
    uint32_t mine = 0xFFFFFFFFu;  // (PS_NONE)
    if (g.ekey[x]) {
      const uint64_t e0 = g.exc_off[x];
      const uint64_t at = g.ekey_off[x] + g.rkey_off[e0 < used ? e0 : used];
      mine = static_cast<uint32_t>(at >> 32);
      if (mine < g.list_cap) g.lists[mine] = DrainQuery{g.entries[x].topic, kDrainMaskRow, static_cast<uint32_t>(at), 0};
    }
    g.topic_list[x] = mine;
  }
  if (x < g.exc_cap) {
    uint32_t mine = 0xFFFFFFFFu, peer = 0xFFFFFFFFu;
    if (x < used) {
      peer = g.rec_peer[x];
      if (g.rkey[x]) {
        const uint32_t i = aud_entry_of(g.exc_off, g.n, x);
        const uint64_t at = g.ekey_off[i + 1] + g.rkey_off[x];
        mine = static_cast<uint32_t>(at >> 32);
        if (mine < g.list_cap) g.lists[mine] = DrainQuery{g.entries[i].topic, g.rec_node[x], static_cast<uint32_t>(at), 0};
      }
    }
    g.exc_peer[x] = peer;
    g.exc_list[x] = mine;
  }
  if (x == 0) {
    const uint64_t all = g.ekey_off[g.n] + g.rkey_off[used];
    DrainCtl c{};
    c.n_lists = static_cast<uint32_t>(all >> 32);
    c.n_segs = static_cast<uint32_t>(all);
    c.over = (n_exc > g.exc_cap ? kDrainOverExc : 0u) |
             (c.n_lists > g.list_cap || c.n_segs > g.seg_bound ? kDrainOverLists : 0u);
    c.use_lists = c.over ? 0u : c.n_lists;
    c.use_segs = c.over ? 0u : c.n_segs;
    *g.ctl = c;
  }
}

// ---- the window's drain tables built on the device (ps_drain_begin) ----------

constexpr uint32_t kTabBlock = 256;

// the built topic (index into b.topic) whose range of `first` holds x
__device__ __forceinline__ uint32_t built_topic(const uint32_t* first, uint32_t n_built, uint32_t x) {
  uint32_t lo = 0, hi = n_built;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (first[mid] <= x) lo = mid + 1;
    else hi = mid;
  }
  return lo - 1;  // (first[0] = 0 <= x)
}

// One thread per window message: its id at its row bit, its mask bit set, its
// arrival key beside the id for the check below.
__global__ __launch_bounds__(kTabBlock) void k_drain_tables(DrainBuild b) {
  const uint32_t j = blockIdx.x * kTabBlock + threadIdx.x;
  if (j >= b.n_msgs) return;
  const DrainTopic T = b.topics[b.topic[built_topic(b.msg0, b.n_built, j)]];
  const uint32_t bit = b.bit[j], i = b.idx[j];
  if (bit >= T.n_pos || (bit >> 6) >= T.W) {  // a bit past the row
    *b.err = kDrainErrBit;
    return;
  }
  const uint64_t m = 1ull << (bit & 63);
  const uint64_t old = atomicOr(reinterpret_cast<unsigned long long*>(b.mask + T.aux0 + (bit >> 6)), m);
  if (old & m) {  // two messages share the bit
    *b.err = kDrainErrBit;
    return;
  }
  b.ids[T.tab0 + bit] = b.last_first + i;
  b.keys[T.tab0 + bit] = static_cast<uint64_t>(b.start[j]) << 32 | i;
}

// One thread per table position: a message bit's key must exceed the key of
// the nearest lower message bit of its topic (the emit lists a row's set bits
// in bit order, and that must be arrival order).
__global__ __launch_bounds__(kTabBlock) void k_drain_tables_check(DrainBuild b) {
  const uint64_t p = static_cast<uint64_t>(blockIdx.x) * kTabBlock + threadIdx.x;
  if (p >= b.n_pos) return;
  uint64_t w = p >> 6;
  const uint64_t here = b.mask[w];
  if (!(here >> (p & 63) & 1ull)) return;
  // the topic's first mask word: the last built topic whose table starts at or below p
  uint32_t lo = 0, hi = b.n_built;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (b.topics[b.topic[mid]].tab0 <= p) lo = mid + 1;
    else hi = mid;
  }
  const uint64_t w_first = b.topics[b.topic[lo - 1]].tab0 >> 6;
  uint64_t below = here & ((1ull << (p & 63)) - 1);
  while (!below && w > w_first) below = b.mask[--w];
  if (!below) return;  // the topic's lowest message bit
  const uint64_t q = w * 64 + (63 - __clzll(static_cast<long long>(below)));
  if (b.keys[p] <= b.keys[q]) *b.err = kDrainErrOrder;
}

// The view's header: off[q] of every query from the segment offsets, the
// total, and the table build's error word behind them.
__global__ __launch_bounds__(kTabBlock) void k_drain_offsets(const DrainQuery* __restrict__ queries, uint32_t n,
                                                             const uint64_t* __restrict__ seg_off, uint32_t n_segs,
                                                             const uint32_t* __restrict__ err,
                                                             uint64_t* __restrict__ hdr) {
  const uint32_t q = blockIdx.x * kTabBlock + threadIdx.x;
  if (q < n) hdr[q] = seg_off[queries[q].seg0];
  else if (q == n) hdr[n] = seg_off[n_segs];
  else if (q == n + 1) hdr[n + 1] = *err;
}

// ---- list assignment on the device (ps_drain_shared_begin) -------------------
// One thread per query, three passes around one scan: what the host loop of
// ps_drain_shared does between its two waits.

struct AssignRole {
  bool any, full, creates;
  uint32_t segs;  // segments of the list the query creates (0: creates none)
};

__device__ __forceinline__ bool assign_full(const DrainAssign& g, uint32_t q) {
  const uint32_t v = g.verdict[q];
  return (v & kDrainRowAny) && !(v & kDrainRowMissing) && g.share;
}

// (from k_drain_keys on: first[] is complete)
__device__ __forceinline__ AssignRole assign_role(const DrainAssign& g, uint32_t q, uint32_t t) {
  AssignRole r;
  r.any = g.verdict[q] & kDrainRowAny;
  r.full = assign_full(g, q);
  r.creates = r.any && (!r.full || g.first[t] == q);
  r.segs = r.creates ? (g.topics[t].n_pos + kDrainSegBits - 1) / kDrainSegBits : 0;
  return r;
}

// first[t] = the least full query of topic t: a 32-bit atomicMin, the minimum
// whatever the order.  One thread per *sorted* query (the classify pass's
// input: topic by topic, a topic's queries in ascending query order; the
// others are never full), so that the lowest full lane of a topic within a
// wave holds the wave's minimum for it and speaks for the lanes above:
// atomics on one word run one after the other, and a topic may have thousands
// of full queries.  (One atomic per full query: 0.81 ms for the assignment at
// 262,144 cfg3 pairs; skipping those above the word's current value, read
// past the L1: 0.51 ms, the whole grid being resident at once.)
__global__ __launch_bounds__(kTabBlock) void k_drain_first(DrainAssign g) {
  const uint32_t i = blockIdx.x * kTabBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & (kWave - 1);
  uint32_t q = 0, t = 0xFFFFFFFFu;
  bool full = false;
  if (i < g.n_sorted) {
    q = g.sorted[i].slot;
    t = g.queries[q].topic;
    full = assign_full(g, q);
  }
  const uint64_t below = __ballot(full) & ((1ull << lane) - 1);
  const uint32_t t_below = __shfl(t, below ? 63 - __clzll(static_cast<long long>(below)) : 0, 64);
  if (!full || (below && t_below == t)) return;  // (a topic's lanes are consecutive: the nearest full lane below decides)
  uint32_t* const w = g.first + t;
  if (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > q) atomicMin(w, q);
}

__global__ __launch_bounds__(kTabBlock) void k_drain_keys(DrainAssign g) {
  const uint32_t q = blockIdx.x * kTabBlock + threadIdx.x;
  if (q >= g.n) return;
  const AssignRole r = assign_role(g, q, g.queries[q].topic);
  g.key[q] = static_cast<uint64_t>(r.creates) << 32 | r.segs;
}

// key_off[q] = lists << 32 | segments created by the queries before q: a
// creating query's list number and first segment.  Nothing is stored past
// list_cap; the last query leaves the counts in the control block.
__global__ __launch_bounds__(kTabBlock) void k_drain_lists(DrainAssign g) {
  const uint32_t q = blockIdx.x * kTabBlock + threadIdx.x;
  if (q >= g.n) return;
  const DrainQuery Q = g.queries[q];
  const AssignRole r = assign_role(g, q, Q.topic);
  const uint64_t at = g.key_off[q];
  const uint32_t l = static_cast<uint32_t>(at >> 32), seg0 = static_cast<uint32_t>(at);
  uint32_t mine = 0xFFFFFFFFu;  // (PS_NONE)
  if (r.creates) {
    mine = l;
    if (l < g.list_cap) g.lists[l] = DrainQuery{Q.topic, r.full ? kDrainMaskRow : Q.node, seg0, 0};
  } else if (r.full) {
    mine = static_cast<uint32_t>(g.key_off[g.first[Q.topic]] >> 32);
  }
  g.list_of_query[q] = mine;
  if (q == g.n - 1) {
    DrainCtl c{};
    c.n_lists = l + (r.creates ? 1u : 0u);
    c.n_segs = seg0 + r.segs;
    const bool over = c.n_lists > g.list_cap || c.n_segs > g.seg_bound;  // (the second: never, by the bound's making)
    c.use_lists = over ? 0u : c.n_lists;
    c.use_segs = over ? 0u : c.n_segs;
    c.over = over ? kDrainOverLists : 0u;
    *g.ctl = c;
  }
}

// k_drain_count over the lists: the counts from the control block, zeros up to the bound
__global__ __launch_bounds__(kCountBlock) void k_drain_count_dev(DrainArgs a, const DrainCtl* __restrict__ ctl,
                                                                 uint32_t seg_bound, uint64_t* __restrict__ cnt) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t s = __builtin_amdgcn_readfirstlane(blockIdx.x * (kCountBlock / kWave) + threadIdx.x / kWave);
  if (s > seg_bound) return;
  a.n_queries = ctl->use_lists;
  uint32_t c = 0;
  if (s < ctl->use_segs) {
    DrainQuery Q;
    DrainTopic T;
    uint32_t k;
    if (locate(a, s, &Q, &T, &k)) c = __popcll(lane_word(a, T, Q.node, k * kDrainSegBits + lane * 64));
  }
  c = wave_sum_u32(c);
  if (lane == 0) cnt[s] = c;
}

// The view's header and list_off[0 .. list_cap]: a list's offset from its
// first segment's, the total from n_lists on.  The thread of the total also
// decides whether the ids fit (the emit behind reads ctl->over).
__global__ __launch_bounds__(kTabBlock) void k_drain_offsets_dev(const DrainQuery* __restrict__ lists, DrainCtl* ctl,
                                                                 uint32_t list_cap,
                                                                 const uint64_t* __restrict__ seg_off, uint64_t id_cap,
                                                                 const uint32_t* __restrict__ err,
                                                                 DrainSharedHdr* __restrict__ hdr,
                                                                 uint64_t* __restrict__ list_off) {
  const uint32_t l = blockIdx.x * kTabBlock + threadIdx.x;
  if (l > list_cap) return;
  const uint32_t n_lists = ctl->use_lists;
  const uint64_t total = seg_off[ctl->use_segs];
  list_off[l] = l < n_lists ? seg_off[lists[l].seg0] : total;
  if (l == 0) {
    const uint32_t over = ctl->over | (total > id_cap ? kDrainOverIds : 0u);
    ctl->over = over;
    hdr->total = total;
    hdr->n_lists = ctl->n_lists;
    hdr->over = over;
    hdr->err = *err;
    hdr->pad = 0;
  }
}

__global__ __launch_bounds__(kWave) void k_drain_emit_dev(DrainArgs a, const DrainCtl* __restrict__ ctl,
                                                          const uint64_t* __restrict__ off, uint32_t* __restrict__ out,
                                                          uint64_t out_cap) {
  __shared__ uint32_t stage[kDrainSegBits];
  if (ctl->over || blockIdx.x >= ctl->use_segs) return;  // (block-uniform)
  a.n_queries = ctl->use_lists;
  emit_segment<true>(a, blockIdx.x, off, 0, out, out_cap, stage);
}

// ---- the sink: a window's lists into the run's result (ps_sink_set) ----------

// Where k_drain_offsets_dev writes a view of its own, this writes the window's
// part of the run's: list_off from the run's list and id counts so far, row w
// of win_list with the window's list numbers rebased, and the next cursor.
// Every thread reads cur[w & 1], which this launch does not write; thread 0
// alone writes cur[(w + 1) & 1].  Nothing is stored past list_cap.
__global__ __launch_bounds__(kTabBlock) void k_sink_commit(SinkCommit c) {
  const uint32_t i = blockIdx.x * kTabBlock + threadIdx.x;
  const SinkCursor C = c.cur[c.w & 1];
  const DrainCtl ctl = *c.ctl;
  const uint64_t total = c.seg_off[ctl.use_segs];
  if (i <= ctl.use_lists && i <= c.win_list_cap) {
    const uint64_t at = static_cast<uint64_t>(C.lists) + i;
    if (at <= c.list_cap) c.list_off[at] = C.ids + (i < ctl.use_lists ? c.seg_off[c.lists[i].seg0] : total);
  }
  if (i < c.n) {
    const uint32_t v = c.win_lq[i];
    c.win_list[static_cast<uint64_t>(c.w) * c.n + i] = v == 0xFFFFFFFFu ? v : C.lists + v;  // (PS_NONE stays)
  }
  if (i == 0) {
    SinkCursor N{};
    N.ids = C.ids + total;
    N.lists = C.lists + ctl.n_lists;
    N.windows = C.windows + 1;
    N.over = C.over | ctl.over | (static_cast<uint64_t>(C.lists) + ctl.n_lists > c.list_cap ? kDrainOverLists : 0u) |
             (C.ids + total > c.id_cap ? kDrainOverIds : 0u);
    N.err = C.err | *c.err;
    c.cur[(c.w + 1) & 1] = N;
  }
}

// k_drain_emit_dev at the run's id count before this window: any base, so the
// wave's dword stores start at any multiple of four bytes
__global__ __launch_bounds__(kWave) void k_sink_emit(DrainArgs a, const DrainCtl* __restrict__ ctl,
                                                     const SinkCursor* __restrict__ cur, uint32_t w,
                                                     const uint64_t* __restrict__ off, uint32_t* __restrict__ out,
                                                     uint64_t id_cap) {
  __shared__ uint32_t stage[kDrainSegBits];
  if (cur[(w + 1) & 1].over || blockIdx.x >= ctl->use_segs) return;  // (block-uniform)
  a.n_queries = ctl->use_lists;
  const uint64_t base = cur[w & 1].ids;  // (no overflow: base + the window's ids <= id_cap)
  emit_segment<true>(a, blockIdx.x, off, 0, out + base, id_cap - base, stage);
}

// The audience sink's commit (ps_sink_set_topics): k_sink_commit's part for the
// window's lists, and the window's audience view into the run's -- row w of
// topic_list (rebased, PS_NONE kept) and n_full, exc_off[w * n + i] from the
// run's exact record count (the entry behind the row too: the next window
// writes the same value there), the records below the window's cap at that
// count, exc_list rebased.  Every thread reads cur[w & 1]; thread 0 alone
// writes cur[(w + 1) & 1].  Plain loads and stores; nothing past a cap.
__global__ __launch_bounds__(kTabBlock) void k_audience_sink_commit(AudSinkCommit c) {
  const uint32_t i = blockIdx.x * kTabBlock + threadIdx.x;
  const SinkCursor C = c.cur[c.w & 1];
  const DrainCtl ctl = *c.ctl;
  const uint64_t total = c.seg_off[ctl.use_segs];
  const uint64_t n_exc = c.win_exc_off[c.n];
  const uint64_t row = static_cast<uint64_t>(c.w) * c.n;
  if (i <= ctl.use_lists && i <= c.win_list_cap) {
    const uint64_t at = static_cast<uint64_t>(C.lists) + i;
    if (at <= c.list_cap) c.list_off[at] = C.ids + (i < ctl.use_lists ? c.seg_off[c.lists[i].seg0] : total);
  }
  if (i < c.n) {
    const uint32_t v = c.win_topic_list[i];
    c.topic_list[row + i] = v == 0xFFFFFFFFu ? v : C.lists + v;  // (PS_NONE stays)
    c.n_full[row + i] = c.win_n_full[i];
  }
  if (i <= c.n) c.exc_off[row + i] = C.exc + c.win_exc_off[i];
  if (i < c.win_exc_cap && i < n_exc) {
    const uint64_t at = C.exc + i;
    if (at < c.exc_cap) {
      const uint32_t v = c.win_exc_list[i];
      c.exc_peer[at] = c.win_exc_peer[i];
      c.exc_list[at] = v == 0xFFFFFFFFu ? v : C.lists + v;
    }
  }
  if (i == 0) {
    SinkCursor N{};
    N.ids = C.ids + total;
    N.lists = C.lists + ctl.n_lists;
    N.windows = C.windows + 1;
    N.exc = C.exc + n_exc;
    N.over = C.over | ctl.over | (static_cast<uint64_t>(C.lists) + ctl.n_lists > c.list_cap ? kDrainOverLists : 0u) |
             (C.ids + total > c.id_cap ? kDrainOverIds : 0u) | (N.exc > c.exc_cap ? kDrainOverExc : 0u);
    N.err = C.err | *c.err;
    c.cur[(c.w + 1) & 1] = N;
  }
}

}  // namespace

hipError_t launch_audience_sink_commit(const AudSinkCommit& c, hipStream_t s) {
  uint32_t threads = c.n + 1;
  if (c.win_list_cap + 1 > threads) threads = c.win_list_cap + 1;
  if (c.win_exc_cap > threads) threads = c.win_exc_cap;
  hipLaunchKernelGGL(k_audience_sink_commit, dim3((threads + kTabBlock - 1) / kTabBlock), dim3(kTabBlock), 0, s, c);
  return hipGetLastError();
}

hipError_t launch_sink_commit(const SinkCommit& c, hipStream_t s) {
  const uint32_t threads = c.win_list_cap + 1 > c.n ? c.win_list_cap + 1 : c.n;
  hipLaunchKernelGGL(k_sink_commit, dim3((threads + kTabBlock - 1) / kTabBlock), dim3(kTabBlock), 0, s, c);
  return hipGetLastError();
}

hipError_t launch_sink_emit(const DrainArgs& a, const DrainCtl* ctl, const SinkCursor* cur, uint32_t w,
                            uint32_t seg_bound, const uint64_t* off, uint32_t* out, uint64_t id_cap, hipStream_t s) {
  if (seg_bound == 0) return hipSuccess;
  hipLaunchKernelGGL(k_sink_emit, dim3(seg_bound), dim3(kWave), 0, s, a, ctl, cur, w, off, out, id_cap);
  return hipGetLastError();
}

hipError_t launch_drain_assign(const DrainAssign& g, hipStream_t s) {
  if (g.n == 0) return hipSuccess;
  const dim3 grid((g.n + kTabBlock - 1) / kTabBlock), block(kTabBlock);
  if (g.n_sorted) hipLaunchKernelGGL(k_drain_first, dim3((g.n_sorted + kTabBlock - 1) / kTabBlock), block, 0, s, g);
  hipLaunchKernelGGL(k_drain_keys, grid, block, 0, s, g);
  hipError_t rc = hipGetLastError();
  if (rc != hipSuccess) return rc;
  size_t bytes = g.scan_bytes;
  rc = hipcub::DeviceScan::ExclusiveSum(g.scan_temp, bytes, g.key, g.key_off, g.n, s);
  if (rc != hipSuccess) return rc;
  hipLaunchKernelGGL(k_drain_lists, grid, block, 0, s, g);
  return hipGetLastError();
}

hipError_t launch_drain_count_dev(const DrainArgs& a, const DrainCtl* ctl, uint32_t seg_bound, uint64_t* cnt,
                                  hipStream_t s) {
  const uint32_t per = kCountBlock / kWave;
  hipLaunchKernelGGL(k_drain_count_dev, dim3((seg_bound + 1 + per - 1) / per), dim3(kCountBlock), 0, s, a, ctl,
                     seg_bound, cnt);
  return hipGetLastError();
}

hipError_t launch_drain_offsets_dev(const DrainQuery* lists, DrainCtl* ctl, uint32_t list_cap, const uint64_t* seg_off,
                                    uint64_t id_cap, const uint32_t* err, DrainSharedHdr* hdr, uint64_t* list_off,
                                    hipStream_t s) {
  hipLaunchKernelGGL(k_drain_offsets_dev, dim3((list_cap + 1 + kTabBlock - 1) / kTabBlock), dim3(kTabBlock), 0, s, lists,
                     ctl, list_cap, seg_off, id_cap, err, hdr, list_off);
  return hipGetLastError();
}

hipError_t launch_drain_emit_dev(const DrainArgs& a, const DrainCtl* ctl, uint32_t seg_bound, const uint64_t* off,
                                 uint32_t* out, uint64_t id_cap, hipStream_t s) {
  if (seg_bound == 0) return hipSuccess;
  hipLaunchKernelGGL(k_drain_emit_dev, dim3(seg_bound), dim3(kWave), 0, s, a, ctl, off, out, id_cap);
  return hipGetLastError();
}

hipError_t launch_drain_tables(const DrainBuild& b, hipStream_t s) {
  if (b.n_msgs == 0) return hipSuccess;
  hipLaunchKernelGGL(k_drain_tables, dim3((b.n_msgs + kTabBlock - 1) / kTabBlock), dim3(kTabBlock), 0, s, b);
  hipError_t rc = hipGetLastError();
  if (rc != hipSuccess) return rc;
  hipLaunchKernelGGL(k_drain_tables_check, dim3(static_cast<uint32_t>((b.n_pos + kTabBlock - 1) / kTabBlock)),
                     dim3(kTabBlock), 0, s, b);
  return hipGetLastError();
}

hipError_t launch_drain_offsets(const DrainQuery* queries, uint32_t n, const uint64_t* seg_off, uint32_t n_segs,
                                const uint32_t* err, uint64_t* hdr, hipStream_t s) {
  hipLaunchKernelGGL(k_drain_offsets, dim3((n + 2 + kTabBlock - 1) / kTabBlock), dim3(kTabBlock), 0, s, queries, n,
                     seg_off, n_segs, err, hdr);
  return hipGetLastError();
}

hipError_t launch_drain_classify(const DrainArgs& a, const DrainClassBin* bins, uint32_t n_bins,
                                 const DrainClassQuery* queries, uint32_t n_waves, uint32_t* verdict, hipStream_t s) {
  if (n_waves == 0) return hipSuccess;
  const uint32_t per = kClassBlock / kWave;
  hipLaunchKernelGGL(k_drain_classify, dim3((n_waves + per - 1) / per), dim3(kClassBlock), 0, s, a, bins, n_bins, queries,
                     n_waves, verdict);
  return hipGetLastError();
}

hipError_t launch_audience_classify(const DrainArgs& a, const AudArgs& g, hipStream_t s) {
  const uint32_t per = kAudBlock / kWave;
  hipLaunchKernelGGL(k_audience_classify, dim3((g.n_strips + 1 + per - 1) / per), dim3(kAudBlock), 0, s, a, g);
  return hipGetLastError();
}

hipError_t launch_audience_emit(const AudArgs& g, const AudEmit& o, hipStream_t s) {
  if (g.n_strips == 0) return hipSuccess;
  const uint32_t per = kAudBlock / kWave;
  hipLaunchKernelGGL(k_audience_emit, dim3((g.n_strips + per - 1) / per), dim3(kAudBlock), 0, s, g, o);
  return hipGetLastError();
}

hipError_t launch_audience_load(const DrainArgs& a, const LoadArgs& g, hipStream_t s) {
  if (g.n_strips == 0) return hipSuccess;
  const uint32_t per = kAudBlock / kWave;
  hipLaunchKernelGGL(k_audience_load, dim3((g.n_strips + per - 1) / per), dim3(kAudBlock), 0, s, a, g);
  return hipGetLastError();
}

hipError_t launch_audience_hops(const DrainArgs& a, const HopsArgs& g, hipStream_t s) {
  if (g.n_strips == 0) return hipSuccess;
  const uint32_t per = kAudBlock / kWave;
  hipLaunchKernelGGL(k_audience_hops, dim3((g.n_strips + per - 1) / per), dim3(kAudBlock), 0, s, a, g);
  return hipGetLastError();
}

hipError_t launch_audience_hops_sum(const HopsArgs& g, hipStream_t s) {
  if (g.n_strips == 0 || g.n == 0 || g.max_cols == 0) return hipSuccess;
  hipLaunchKernelGGL(k_audience_hops_sum, dim3(g.n, g.max_cols), dim3(kHopsSumBlock), 0, s, g);
  return hipGetLastError();
}

hipError_t launch_audience_weights(const DrainArgs& a, const DownArgs& g, hipStream_t s) {
  if (g.n_strips == 0) return hipSuccess;
  const uint32_t per = kAudBlock / kWave;
  hipLaunchKernelGGL(k_audience_weights, dim3((g.n_strips + per - 1) / per), dim3(kAudBlock), 0, s, a, g);
  return hipGetLastError();
}

hipError_t launch_downstream_level(const DownArgs& g, uint32_t w0, uint32_t w1, hipStream_t s) {
  if (w1 <= w0) return hipSuccess;
  hipLaunchKernelGGL(k_downstream_level, dim3(w1 - w0), dim3(kDownBlock), 0, s, g, w0);
  return hipGetLastError();
}

hipError_t launch_downstream_top(const DownArgs& g, hipStream_t s) {
  if (g.n_strips == 0 || g.n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_downstream_top, dim3(g.n), dim3(kDownBlock), 0, s, g);
  return hipGetLastError();
}

hipError_t launch_audience_missed(const CutArgs& g, hipStream_t s) {
  if (g.d.n_strips == 0) return hipSuccess;
  const uint32_t per = kAudBlock / kWave;
  hipLaunchKernelGGL(k_audience_missed, dim3((g.d.n_strips + per - 1) / per), dim3(kAudBlock), 0, s, g);
  return hipGetLastError();
}

hipError_t launch_cut_level(const CutArgs& g, uint32_t w0, uint32_t w1, hipStream_t s) {
  if (w1 <= w0) return hipSuccess;
  hipLaunchKernelGGL(k_cut_level, dim3(w1 - w0), dim3(kDownBlock), 0, s, g, w0);
  return hipGetLastError();
}

hipError_t launch_cut_top(const CutArgs& g, hipStream_t s) {
  if (g.d.n_strips == 0 || g.d.n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_cut_top, dim3(g.d.n), dim3(kDownBlock), 0, s, g);
  return hipGetLastError();
}

hipError_t launch_blame_top(const BlameArgs& g, hipStream_t s) {
  if (g.d.n_strips == 0 || g.d.n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_blame_top, dim3(g.d.n), dim3(kDownBlock), 0, s, g);
  return hipGetLastError();
}

hipError_t launch_blame_level(const BlameArgs& g, uint32_t w0, uint32_t w1, hipStream_t s) {
  if (w1 <= w0) return hipSuccess;
  hipLaunchKernelGGL(k_blame_level, dim3(w1 - w0), dim3(kDownBlock), 0, s, g, w0);
  return hipGetLastError();
}

hipError_t launch_blame_count(const BlameArgs& g, hipStream_t s) {
  const uint32_t per = kAudBlock / kWave;
  hipLaunchKernelGGL(k_blame_count, dim3((g.d.n_strips + 1 + per - 1) / per), dim3(kAudBlock), 0, s, g);
  return hipGetLastError();
}

// (the grid covers the strips, a wave each, and the n + 1 record offsets, a thread each)
hipError_t launch_blame_emit(const BlameArgs& g, hipStream_t s) {
  const uint32_t per = kAudBlock / kWave;
  const uint32_t by_strip = (g.d.n_strips + per - 1) / per, by_entry = (g.d.n + 1 + kAudBlock - 1) / kAudBlock;
  const uint32_t blocks = by_strip > by_entry ? by_strip : by_entry;
  hipLaunchKernelGGL(k_blame_emit, dim3(blocks), dim3(kAudBlock), 0, s, g);
  return hipGetLastError();
}

// (a thread per request position, one block at least: the cursor moves on by a window whatever it holds)
hipError_t launch_blame_track_commit(const BlameArgs& g, const BlameTrack& t, hipStream_t s) {
  const uint32_t blocks = t.n_req ? (t.n_req + kAudBlock - 1) / kAudBlock : 1;
  hipLaunchKernelGGL(k_blame_track_commit, dim3(blocks), dim3(kAudBlock), 0, s, g, t);
  return hipGetLastError();
}

hipError_t launch_blame_track_emit(const BlameArgs& g, const BlameTrack& t, hipStream_t s) {
  if (g.d.n_strips == 0) return hipSuccess;
  const uint32_t per = kAudBlock / kWave;
  hipLaunchKernelGGL(k_blame_track_emit, dim3((g.d.n_strips + per - 1) / per), dim3(kAudBlock), 0, s, g, t);
  return hipGetLastError();
}

hipError_t launch_blame_gather(const BlameArgs& g, const BlameGather& q, hipStream_t s) {
  if (q.n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_blame_gather, dim3((q.n + kAudBlock - 1) / kAudBlock), dim3(kAudBlock), 0, s, g, q);
  return hipGetLastError();
}

// the sections of g.what as k_report_nodes' template: both subtree sections
// take the k word, the cut section the misses too
hipError_t launch_report_nodes(const DrainArgs& a, const ReportArgs& g, hipStream_t s) {
  if (g.n_strips == 0) return hipSuccess;
  if (g.what == 0 || (g.what & ~kReportAll)) return hipErrorInvalidValue;
  using Kernel = void (*)(DrainArgs, ReportArgs);
  static const Kernel table[2][2][3] = {
      {{nullptr, k_report_nodes<false, false, true, false>, k_report_nodes<false, false, true, true>},
       {k_report_nodes<false, true, false, false>, k_report_nodes<false, true, true, false>,
        k_report_nodes<false, true, true, true>}},
      {{k_report_nodes<true, false, false, false>, k_report_nodes<true, false, true, false>,
        k_report_nodes<true, false, true, true>},
       {k_report_nodes<true, true, false, false>, k_report_nodes<true, true, true, false>,
        k_report_nodes<true, true, true, true>}}};
  const uint32_t words = g.what & kReportCut ? 2u : g.what & kReportDown ? 1u : 0u;
  const Kernel k = table[g.what & kReportLoad ? 1 : 0][g.what & kReportHops ? 1 : 0][words];
  const uint32_t per = kAudBlock / kWave;
  hipLaunchKernelGGL(k, dim3((g.n_strips + per - 1) / per), dim3(kAudBlock), 0, s, a, g);
  return hipGetLastError();
}

hipError_t launch_report_level(const CutArgs& g, uint32_t w0, uint32_t w1, hipStream_t s) {
  if (w1 <= w0) return hipSuccess;
  hipLaunchKernelGGL(k_report_level, dim3(w1 - w0), dim3(kDownBlock), 0, s, g, w0);
  return hipGetLastError();
}

hipError_t launch_report_top(const CutArgs& g, hipStream_t s) {
  if (g.d.n_strips == 0 || g.d.n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_report_top, dim3(g.d.n), dim3(kDownBlock), 0, s, g);
  return hipGetLastError();
}

// the sections of g.what as k_dist_nodes' template; a wave per strip and one
// per entry behind them (the roots' share of `sent`) where load is selected
hipError_t launch_dist_nodes(const DrainArgs& a, const DistArgs& g, hipStream_t s) {
  if (g.what == 0 || (g.what & ~(kReportLoad | kReportHops | kReportDown))) return hipErrorInvalidValue;
  const uint32_t waves = g.n_strips + (g.what & kReportLoad ? g.n : 0u);
  if (waves == 0) return hipSuccess;
  using Kernel = void (*)(DrainArgs, DistArgs);
  static const Kernel table[2][2][2] = {
      {{nullptr, k_dist_nodes<false, false, true>}, {k_dist_nodes<false, true, false>, k_dist_nodes<false, true, true>}},
      {{k_dist_nodes<true, false, false>, k_dist_nodes<true, false, true>},
       {k_dist_nodes<true, true, false>, k_dist_nodes<true, true, true>}}};
  const Kernel k = table[g.what & kReportLoad ? 1 : 0][g.what & kReportHops ? 1 : 0][g.what & kReportDown ? 1 : 0];
  const uint32_t per = kAudBlock / kWave;
  hipLaunchKernelGGL(k, dim3((waves + per - 1) / per), dim3(kAudBlock), 0, s, a, g);
  return hipGetLastError();
}

hipError_t launch_dist_hops_sum(const DistArgs& g, uint32_t max_cols, hipStream_t s) {
  if (g.n_strips == 0 || g.n == 0 || max_cols == 0 || g.n_parts == 0) return hipSuccess;
  hipLaunchKernelGGL(k_dist_hops_sum, dim3(g.n, max_cols), dim3(kHopsSumBlock), 0, s, g);
  return hipGetLastError();
}

hipError_t launch_dist_sweep_level(const DistArgs& g, uint32_t level, uint32_t w0, uint32_t w1, hipStream_t s) {
  if (w1 <= w0) return hipSuccess;
  hipLaunchKernelGGL(k_dist_sweep_level, dim3(w1 - w0), dim3(kDownBlock), 0, s, g, level, w0);
  return hipGetLastError();
}

hipError_t launch_dist_apply(const DistArgs& g, uint32_t a0, uint32_t a1, hipStream_t s) {
  if (a1 <= a0) return hipSuccess;
  hipLaunchKernelGGL(k_dist_apply, dim3(a1 - a0), dim3(kDownBlock), 0, s, g, a0);
  return hipGetLastError();
}

hipError_t launch_dist_cut_nodes(const DrainArgs& a, const DistCutArgs& g, hipStream_t s) {
  if (g.d.n_strips == 0) return hipSuccess;
  const uint32_t per = kAudBlock / kWave;
  hipLaunchKernelGGL(k_dist_cut_nodes, dim3((g.d.n_strips + per - 1) / per), dim3(kAudBlock), 0, s, a, g);
  return hipGetLastError();
}

hipError_t launch_dist_cut_fill(const DistCutArgs& g, uint32_t n_fill, hipStream_t s) {
  if (n_fill == 0) return hipSuccess;
  hipLaunchKernelGGL(k_dist_cut_fill, dim3(n_fill), dim3(kDownBlock), 0, s, g);
  return hipGetLastError();
}

hipError_t launch_dist_cut_level(const DistCutArgs& g, uint32_t level, uint32_t w0, uint32_t w1, hipStream_t s) {
  if (w1 <= w0 || level == 0) return hipSuccess;
  hipLaunchKernelGGL(k_dist_cut_level, dim3(w1 - w0), dim3(kDownBlock), 0, s, g, level, w0);
  return hipGetLastError();
}

hipError_t launch_dist_blame_fill(const DistBlameArgs& g, uint32_t f0, uint32_t f1, hipStream_t s) {
  if (f1 <= f0) return hipSuccess;
  hipLaunchKernelGGL(k_dist_blame_fill, dim3(f1 - f0), dim3(kDownBlock), 0, s, g, f0);
  return hipGetLastError();
}

hipError_t launch_dist_blame_level(const DistBlameArgs& g, uint32_t level, uint32_t w0, uint32_t w1, hipStream_t s) {
  if (w1 <= w0 || level == 0) return hipSuccess;
  hipLaunchKernelGGL(k_dist_blame_level, dim3(w1 - w0), dim3(kDownBlock), 0, s, g, level, w0);
  return hipGetLastError();
}

hipError_t launch_dist_blame_count(const DistBlameArgs& g, hipStream_t s) {
  const uint32_t per = kAudBlock / kWave;
  hipLaunchKernelGGL(k_dist_blame_count, dim3((g.d.n_strips + 1 + per - 1) / per), dim3(kAudBlock), 0, s, g);
  return hipGetLastError();
}

// (the grid covers the strips, a wave each, and the n + 1 record offsets, a thread each)
hipError_t launch_dist_blame_emit(const DistBlameArgs& g, hipStream_t s) {
  const uint32_t per = kAudBlock / kWave;
  const uint32_t by_strip = (g.d.n_strips + per - 1) / per, by_entry = (g.d.n + 1 + kAudBlock - 1) / kAudBlock;
  const uint32_t blocks = by_strip > by_entry ? by_strip : by_entry;
  hipLaunchKernelGGL(k_dist_blame_emit, dim3(blocks), dim3(kAudBlock), 0, s, g);
  return hipGetLastError();
}

hipError_t launch_spread_nodes(const DrainArgs& a, const SpreadArgs& g, hipStream_t s) {
  if (g.n_strips == 0 || g.n == 0) return hipSuccess;
  const uint32_t per = kAudBlock / kWave;
  hipLaunchKernelGGL(k_spread_nodes, dim3((g.n_strips + per - 1) / per), dim3(kAudBlock), 0, s, a, g);
  return hipGetLastError();
}

hipError_t launch_spread_unreached(const SpreadArgs& g, hipStream_t s) {
  if (g.n_strips == 0 || g.n == 0) return hipSuccess;
  const uint32_t per = kAudBlock / kWave;
  hipLaunchKernelGGL(k_spread_unreached, dim3((g.n_strips + per - 1) / per), dim3(kAudBlock), 0, s, g);
  return hipGetLastError();
}

hipError_t launch_spread_level(const SpreadArgs& g, uint32_t level, uint32_t blocks, hipStream_t s) {
  if (g.n == 0 || g.q_cap == 0 || blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(k_spread_level, dim3(blocks), dim3(kSpreadBlock), 0, s, g, level);
  return hipGetLastError();
}

hipError_t launch_spread_sum(const SpreadArgs& g, hipStream_t s) {
  if (g.n_strips == 0 || g.n == 0) return hipSuccess;
  const uint32_t per = kAudBlock / kWave;
  hipLaunchKernelGGL(k_spread_sum, dim3((g.n_strips + per - 1) / per), dim3(kAudBlock), 0, s, g);
  return hipGetLastError();
}

hipError_t launch_spread_track_close(uint32_t* cnt, uint32_t n_levels, uint64_t* truncated, hipStream_t s) {
  hipLaunchKernelGGL(k_spread_track_close, dim3(1), dim3(kWave), 0, s, cnt, n_levels % 3,
                     reinterpret_cast<unsigned long long*>(truncated));
  return hipGetLastError();
}

hipError_t launch_spread_dup(const SpreadArgs& g, hipStream_t s) {
  if (g.n_peers == 0) return hipSuccess;
  hipLaunchKernelGGL(k_spread_dup, dim3((g.n_peers + kSpreadBlock - 1) / kSpreadBlock), dim3(kSpreadBlock), 0, s, g);
  return hipGetLastError();
}

hipError_t launch_audience_assign(const AudAssign& g, hipStream_t s) {
  const dim3 block(kAudBlock);
  hipLaunchKernelGGL(k_audience_totals, dim3(g.n + 1), block, 0, s, g);
  hipLaunchKernelGGL(k_audience_keys, dim3((g.exc_cap + 1 + kAudBlock - 1) / kAudBlock), block, 0, s, g);
  hipError_t rc = hipGetLastError();
  if (rc != hipSuccess) return rc;
  size_t bytes = g.scan_bytes;
  rc = hipcub::DeviceScan::ExclusiveSum(g.scan_temp, bytes, g.rkey, g.rkey_off, g.exc_cap + 1, s);
  if (rc != hipSuccess) return rc;
  bytes = g.scan_bytes;
  rc = hipcub::DeviceScan::ExclusiveSum(g.scan_temp, bytes, g.ekey, g.ekey_off, g.n + 1, s);
  if (rc != hipSuccess) return rc;
  const uint32_t threads = g.n > g.exc_cap ? g.n : g.exc_cap;
  hipLaunchKernelGGL(k_audience_lists, dim3((threads + kAudBlock - 1) / kAudBlock), block, 0, s, g);
  return hipGetLastError();
}

hipError_t launch_drain_count(const DrainArgs& a, uint32_t n_segs, uint64_t* cnt, hipStream_t s) {
  const uint32_t per = kCountBlock / kWave;
  hipLaunchKernelGGL(k_drain_count, dim3((n_segs + 1 + per - 1) / per), dim3(kCountBlock), 0, s, a, n_segs, cnt);
  return hipGetLastError();
}

hipError_t drain_scan(void* temp, size_t* temp_bytes, const uint64_t* cnt, uint64_t* off, uint32_t n, hipStream_t s) {
  return hipcub::DeviceScan::ExclusiveSum(temp, *temp_bytes, cnt, off, n, s);
}

hipError_t launch_drain_emit(const DrainArgs& a, uint32_t seg_lo, uint32_t seg_hi, const uint64_t* off, uint64_t off0,
                             uint32_t* out, uint64_t out_cap, bool staged, hipStream_t s) {
  if (seg_hi <= seg_lo) return hipSuccess;
  const dim3 grid(seg_hi - seg_lo);
  if (staged)
    hipLaunchKernelGGL(k_drain_emit<true>, grid, dim3(kWave), 0, s, a, seg_lo, off, off0, out, out_cap);
  else
    hipLaunchKernelGGL(k_drain_emit<false>, grid, dim3(kWave), 0, s, a, seg_lo, off, off0, out, out_cap);
  return hipGetLastError();
}

}  // namespace psamd

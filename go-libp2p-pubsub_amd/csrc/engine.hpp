// engine.hpp -- internal state of the engine (include/psengine.h) shared by
// its translation units:
//   graph.cpp  the node space: per-topic BFS numbering (host, or rebuilt on
//              the GPU by gbuild.hip), multi-GPU partition and ghost tables
//   plan.cpp   one window's layout, its launch plans (pull chunks, round
//              pairs, k_flood tasks, the ghost exchange) and its schedule
//              (WindowSchedule: seeds, launch grids, counter slots, the
//              prefix) -- pure host code, tested on the CPU through
//              include/psengine_plan.h
//   run.cpp    one window as a list of stages over a WindowRun (plan uploads,
//              streams and row sets, window start, level or compaction
//              rounds, finish), and ps_run* / ps_wait around it
//   drain_*.cpp  the batched drain of the last window (ps_drain*, the sink),
//              host side, one file per call family over drain_tables.cpp
//              (drain_impl.hpp)
//   api.cpp    the remaining C ABI (lifecycle, topics, membership, reads,
//              multi-GPU)
#pragma once
#include <hip/hip_runtime.h>

#include <array>
#include <chrono>
#include <cstdlib>
#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "dist.hpp"
#include "kernels.hpp"
#include "psengine.h"
#include "tree.hpp"

namespace psamd {

constexpr uint32_t kMaxRoundsCap = 4096;  // round buffers' minimum size (deeper windows grow them)
// counter rows of a level-aligned window at most (its rounds and its reach
// rows): a run slot's pinned block holds 2 x (PS_MAX_ROUNDS + 1) rows (the
// second half, the multi-rank apply rows, is free on one rank)
constexpr uint32_t kAlignedRowsMax = 2 * (PS_MAX_ROUNDS + 1);
constexpr uint32_t kMaxStartRound = 200;
constexpr uint32_t kDefaultWindow = 65536;
constexpr uint32_t kMaxWindow = 1u << 30;  // messages per topic per window at most (ps_config.msg_window)

inline uint32_t ceil_div(uint64_t a, uint64_t b) { return static_cast<uint32_t>((a + b - 1) / b); }

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  uint64_t gen = 0;  // allocations made (a shadow of the contents is valid for one)
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p) {
      (void)hipFree(p);
      psamd::note_device_free();  // (IPC exports of a freed range are stale)
    }
    p = nullptr;
    bytes = 0;
  }
  // Grow-only allocation; *fresh = a new allocation was made.
  hipError_t ensure(size_t n, bool* fresh = nullptr) {
    if (fresh) *fresh = false;
    if (n == 0) n = 16;
    if (n <= bytes) return hipSuccess;
    release();
    hipError_t e = hipMalloc(&p, n);
    if (e != hipSuccess) {
      p = nullptr;
      return e;
    }
    bytes = n;
    ++gen;
    if (fresh) *fresh = true;
    return hipSuccess;
  }
  void swap(DevBuf& o) {
    std::swap(p, o.p);
    std::swap(bytes, o.bytes);
    std::swap(gen, o.gen);
  }
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

enum class Kind { None, Join, Parent, Children };

struct TopicHost {
  bool exists = false;
  Kind kind = Kind::None;
  uint32_t root = 0, width = 2, max_width = 5;
  SubscriptionTree tree;
  std::vector<uint32_t> parent;  // Kind::Parent
  std::vector<uint32_t> rp, cl;  // Kind::Children
  // node space (set by build_graph / gpu_build_graph)
  uint32_t nbase = 0, n_nodes = 0, depth = 0;
  bool mesh = false;
  bool root_local = true;                // this rank owns the root
  uint32_t max_deg = 0;
  uint32_t top_levels = 1;  // GPU build: levels 1 .. top_levels - 1 fit the one-block top kernel
  std::vector<uint32_t> level_internal;  // BFS level -> owned nodes with children
  std::vector<uint32_t> level_off;       // BFS level -> first owned node (topic-relative)
  // multi-GPU: the owned nodes of level d are [level_off[d], level_off[d] +
  // level_local[d]) fed by a parent on this rank, then the ghost-fed ones
  // (parent on another rank), grouped by source rank (graph.cpp numbering)
  std::vector<uint32_t> level_local;
  // GPU rebuild: the upstream of every peer as last shipped to the device
  std::vector<uint32_t> par_mirror;
  bool par_dev_valid = false;  // the device parent array holds par_mirror
  bool par_full_dirty = true;  // Kind::Parent: re-diff the whole array
  // cross-rank edges by the parent's BFS level: (level, from rank, to rank, count)
  struct Cross {
    uint32_t level, from, to, count;
  };
  std::vector<Cross> cross;
  // Multi-GPU level mode: ghost parents.  gcnt[(d * world + a)
  // * world + b] = parents at level d - 1 owned by rank a with a child at
  // level d owned by rank b (a != b): each crosses once per round that writes
  // level d, as record k = its index among them (in a's node order).
  // This rank's parents to ship: send_node[i] (local node), send_dst[i]
  // (dest rank << 27 | k), grouped by the level of the children:
  // send_lvl[d] .. send_lvl[d + 1], node order within a level.
  std::vector<uint32_t> gcnt, send_node, send_dst, send_lvl;
  uint32_t ship0 = 0;  // this topic's first entry in the engine's ship array
};

struct RunMsg {
  uint32_t topic;
  uint32_t start;
  RunMsg() {}  // (left unset: ps_publish writes every element it appends)
  RunMsg(uint32_t t, uint32_t s) : topic(t), start(s) {}
};

// Messages of one topic in one window: a slice of the run's topic-sorted
// message index array (bit li of the topic block = message idx[li]).
struct WinSlice {
  const uint32_t* idx = nullptr;
  uint32_t n = 0;
};

// One start round of a topic's window and its word block [w0, w0 + wn) of
// every row: a tree node at level d receives the block in round start + d.
// A topic whose window messages share one start round has one group, the
// whole row.
struct StartGroup {
  uint32_t start, w0, wn;
};

// A level-aligned window (WindowLayout::aligned): the messages of one topic
// that start in one round, and their row bits [b0, b0 + n) (rows are packed
// node-major, bits sorted by start round).
struct AlignedGroup {
  uint32_t start, b0, n;
};
// The per-round split of a level-aligned window: reached and frontier
// counts per (topic, BFS level), from k_level_reach.  seg_lo[t]: topic t's
// first segment (levels 0 .. depth_t), kNone: inactive.
struct AlignedSplit {
  std::vector<uint32_t> seg_lo, seg_n;
  std::vector<std::vector<AlignedGroup>> groups;
  uint32_t n_segs = 0;
  uint32_t row0 = 0;  // the counter row of segment pair 0 (after the window's rounds)
  bool eager = false;
};

// Word offset of virtual word w of row u (relative to the topic's first
// node): node-major rows, or a kTopicGroups topic's group-major blocks.
uint64_t phys_word(const TopicDev& d, const std::vector<StartGroup>& G, uint64_t u, uint32_t w);

// One window's rows (plan_window_layout): the topic table, start groups,
// message bit positions, and how its rounds run.
struct WindowLayout {
  std::vector<TopicDev> tab;
  std::vector<std::vector<StartGroup>> groups;
  std::vector<std::vector<uint32_t>> pos;  // window slot -> row bit (start groups)
  std::vector<uint32_t> tstart;            // first start round per topic
  std::vector<uint32_t> wglob;             // row words of every active topic, on every rank
  std::vector<GroupDev> gtab;              // start groups of the group-major topics
  uint64_t wtot = 0;                       // row words of the window (this rank)
  uint32_t max_depth = 0, max_start = 0;
  uint32_t planned0 = 0;                   // rounds of the window: max depth + latest start + 1
  uint32_t round_cap = 0;
  bool multi = false;                      // some tree window has several start rounds
  // level-aligned start groups (one rank, ps_plan_opts.align_groups): every
  // topic's row is one node-major block with its messages' bits sorted by
  // start round (AlignedSplit::groups); the planners see one start (round
  // 0: planned0 = max depth + 1 launch rounds); true_rounds = planned0 +
  // the latest start round
  bool aligned = false;
  uint32_t true_rounds = 0;
  AlignedSplit split;
  bool any_mesh = false, need_direct = false;
  bool level = false;                      // level mode (else the compaction path)
};

// One window's schedule (plan_window_schedule): everything run.cpp needs to
// enqueue the window that the host can work out without the device.  The
// level plans themselves stay engine members (pull, pair, flood, ghost: cached
// across windows), as do the reduce descriptors, slot offsets and round kinds
// (desc_host, woff_host, round_kind: later code and the RunSlot read them).
struct WindowSchedule {
  std::vector<SeedDev> seeds;                  // root injections, grouped by round:
  std::vector<uint32_t> seed_off;              // round r's are [seed_off[r], seed_off[r + 1])
  std::vector<std::vector<uint8_t>> starts_of;  // topic -> start rounds present in the window
  bool deep = false;                           // deep_window(): per-round launches from round 1
  bool flood_ok = false;
  uint32_t flood_rounds = 0;                   // rounds 1..flood_rounds: k_flood
  bool changed = false, gch = false;           // level plans rebuilt (any; the ghost plan)
  std::vector<uint32_t> lgrid;                 // per-round launches: blocks (L and G parts together), 0 on a
                                               // multi-round launch's continuation rounds
  uint32_t n_slots = 0;                        // level mode: partial counter slots of the window
  uint32_t reach_rows = 0, reach_slot0 = 0;    // level-aligned: reach counter rows, their first pseudo-slot
  std::vector<std::vector<uint64_t>> cap;      // compaction on N ranks: cap[r][from * world + to] items
  uint64_t max_send = 0, max_recv = 0;         // ... and the largest round's region bytes
  uint64_t total = 0;                          // level mode: the window's row bytes
  bool alt_plan = false;                       // a deep window that may alternate row sets
  uint32_t pre_P = 0;                          // deep windows: the prefix is rounds 1..pre_P
  uint32_t mode = PS_MODE_COMPACT;
  std::chrono::steady_clock::time_point t_seeds;  // host timing: the seeds are done, the planners start
};

// Level mode, one launch kind per round; the round's chunks are
// [off[q], off[q+1]); on N ranks the chunks of nodes fed by a ghost parent
// come last, from gsplit[q] (they wait for the round's exchange).
struct PullPlan {
  std::vector<uint64_t> key;
  uint64_t version = 0;  // bumped by every change (run.cpp uploads on a new version)
  std::vector<PullChunk> chunks;
  std::vector<uint32_t> off, gsplit;
  std::vector<uint64_t> bytes;  // row bytes written per round
};
struct PairPlan {
  std::vector<uint64_t> key;
  uint64_t version = 0;
  std::vector<PullChunk> chunks;         // pair launches
  std::vector<ChainChunk> chain;         // chain launches
  std::vector<uint32_t> lo, hi, gsplit;  // round q: chunks (pair) or chain chunks of the launch starting at q
                                         // (chains: whole rows [lo, gsplit), column slices [gsplit, hi))
  std::vector<uint32_t> len;             // round q: rounds of the launch starting at q (0: none)
  std::vector<uint8_t> kind;             // per round: PS_K_*
  // chain launches run as reach + fill: round q's whole-row chunks [lo, gsplit) as
  // the segments [fill_lo[q], fill_hi[q]) -- none: the launch stays k_pull_chain's -- with fill_blocks[q]
  // reach blocks and the pieces [fill_p0[q], fill_p0[q] + fill_np[q]) of the plan's pieces
  std::vector<FillSeg> fill;
  std::vector<uint32_t> fill_lo, fill_hi, fill_blocks, fill_p0, fill_np;
};
struct FloodPlan {
  std::vector<uint64_t> key;
  uint64_t version = 0;
  std::vector<FloodTask> tasks;
  std::vector<FloodSeg> segs;
  std::vector<uint32_t> slot0, nslot;  // per round: partial counter slots
  uint32_t slots = 1;                  // slots of a window (slot 0: the timeout word)
  uint32_t granules = 0;
};
// Multi-GPU: the ghost exchange of a window.
struct GhostRound {
  std::vector<uint64_t> s_off, s_len, r_off, r_len;  // transport regions, bytes (send: in the round's half)
  uint32_t pack0 = 0, pack1 = 0;                     // the round's root segments (k_pack)
  uint64_t pack_units = 0;                           // their units (k_pack's stream)
  bool any = false;                                  // some rank ships rows this round (same on every rank)
  uint64_t rec_bytes = 0;                            // record bytes this rank receives (in place: roots' only)
};
struct GhostPlan {
  std::vector<uint64_t> key;
  std::vector<GhostRound> rounds;
  std::vector<GhostSeg> segs;     // per (round, topic, start group): record bases
  std::vector<std::vector<std::vector<uint32_t>>> seg_of;  // [round][topic][group] -> segs index (kNoneNode: none)
  std::vector<PackSeg> pack;      // roots' records (level-1 rounds)
  uint64_t send_half = 0;         // words per part of the send buffer (kSendBufs parts, by round)
  uint64_t recv_words = 0;
};

// The default plan options (ps_plan_opts_default; a new engine's `opts`): the
// one place the numbers stand, each with the measurement that chose it.
inline ps_plan_opts default_plan_opts() {
  ps_plan_opts o{};
  // k_flood: a single-rank level window's leading rounds in
  // one persistent launch; PSAMD_FLOOD=0 runs per-round launches instead
  o.flood = 1;
  o.flood_words = kFloodWords;  // row words per task (PSAMD_FLOOD_WORDS)
  // k_flood runs the leading rounds writing at most this many row bytes (with
  // chains after it: 4 MB; 16 MB was best before them, profiles/r03/ab_flood_top.txt)
  o.flood_top_bytes = 4ull << 20;
  o.flood_min_rounds = 4;  // k_flood only for at least this many leading rounds
  o.align_groups = 1;      // one-rank start-group windows run level-aligned
  o.flood_spin_ticks = 200000000u;  // dependency-wait bound: 2 s of s_memrealtime (100 MHz); PSAMD_FLOOD_SPIN_TICKS
  // rounds per launch at most (chain_max, 1..kChainLevels): 1 = one k_pull
  // per round, 2 = pairs (k_pull_pair), 3..6 chains.
  // Defaults by measurement (profiles/r03/ab_chain_v2.txt):
  // 4 for single-start windows (cfg3 burst 1.016 vs 1.033 ms at 6), 6 for
  // windows with start groups (paced cfg3 1.363 vs 1.443 ms at 4)
  o.chain_max = 4;
  o.chain_max_groups = 6;
  o.pad_words = 16;         // rows of at least this many words padded to even (PSAMD_PAD_WORDS)
  o.chain_tail = 1;         // a chain ending at the last round may be one round longer (PSAMD_CHAIN_TAIL)
  o.launch_bytes = 16000000;  // planner: a launch's ramp and tail as row bytes (PSAMD_LAUNCH_BYTES)
  o.chain_words = 4096;     // row words per chain wave, the planner's target (8192 until r05: cfg4 0.444 -> 0.404, cfg3 -0.5..1 %, profiles/r05/ab/)
  o.chain_waves = 12;       // chain launches: resident waves per CU at most
  o.chain_nt = 1;           // chain launches: level 0 and the inner levels stored non-temporally
  // cross-window overlap (PSAMD_OVERLAP=0: off) of windows
  // with at least these rounds and row bytes (PSAMD_OVERLAP_BYTES)
  o.overlap = 1;
  o.overlap_min_rounds = 12;
  o.overlap_min_bytes = 512ull << 20;
  // the exchange on its own stream beside the round's locally fed chunks
  // (-1 = auto): a transport that copies the records (RCCL; the loopback
  // with PS_DIST_F_COPY) yes; the zero-copy loopback no -- there it only
  // contends for the same GPU (4 loopback ranks, cfg4: 7.06 vs 6.32 ms/step,
  // profiles/r03/loopback)
  o.xchg_overlap = -1;
  // GPU rebuild of the node space: on by default for one
  // rank and tree topics (PSAMD_GPU_BUILD=0: host build)
  o.gpu_build = 1;
  return o;
}

}  // namespace psamd

struct ps_engine {
  ps_config cfg{};
  std::string err;
  hipStream_t stream = nullptr;
  hipStream_t xstream = nullptr;  // multi-GPU: the exchange, beside the round's local chunks
  hipEvent_t ev_run0 = nullptr, ev_run1 = nullptr;
  hipEvent_t ev_round = nullptr, ev_xchg = nullptr;  // multi-GPU: round boundary, exchange done
  // the plan options (ps_get_plan_opts / ps_set_plan_opts; the A/B
  // environment through api.cpp: read_switches)
  ps_plan_opts opts = psamd::default_plan_opts();
  bool xchg_overlap = true;  // opts.xchg_overlap resolved against the transport (api.cpp: refresh_xchg_overlap)
  // The A/B and debug switches that are no plan options, read from the
  // environment at creation (api.cpp: read_switches)
  struct Switches {
    bool host_timing = false;    // PSAMD_HOST_TIMING=1: host phase times to stderr
    bool flood_profile = false;  // PSAMD_FLOOD_PROFILE=1: per-wave phase times of k_flood to stderr (sync runs)
    // PSAMD_CHAIN_PROFILE=<file>: per-wave start / end / words of every
    // k_pull_chain launch of blocking windows, appended to <file> (debug)
    std::string chain_prof_path;
    bool twin = true;          // twin windows (PSAMD_TWIN=0: off)
    bool sig_windows = true;   // pipelined one-rank windows end with a pinned flag, not an event (A/B: PSAMD_SIG_WINDOWS=0)
    // a signalled window's reduce is held back (pend_reduce) to run in the
    // next window's first launch (A/B: PSAMD_FUSE_REDUCE=0)
    bool fuse_reduce = true;
    bool upload_reuse = true;  // the upload shadows below (A/B: PSAMD_UPLOAD_REUSE=0)
    uint32_t expand_opts = 0;       // ExpandArgs::opts (A/B only: PSAMD_NARROW=0 -> kExpandNoNarrow)
    uint32_t chain_words_lead = 0;  // A/B only (PSAMD_CHAIN_WORDS_LEAD): opts.chain_words for all but the last launch
    // chain launches as reach + fill (PSAMD_CHAIN_FILL=0: off): a launch whose whole
    // rows are at least chain_fill_bytes (PSAMD_CHAIN_FILL_BYTES; 0: every eligible launch) and on
    // average at least chain_fill_row_words wide (PSAMD_CHAIN_FILL_ROW_WORDS; 0: any width), at most
    // chain_fill_waves fill waves per CU (PSAMD_CHAIN_FILL_WAVES; 0: no cap), in pieces of about
    // chain_fill_piece words (PSAMD_CHAIN_FILL_PIECE)
    bool chain_fill = true;
    uint32_t chain_fill_piece = psamd::kFillPieceWords;
    uint64_t chain_fill_bytes = 512ull << 20;
    uint64_t chain_fill_row_words = psamd::kFillMinRowWords;
    uint32_t chain_fill_waves = psamd::kFillWaves;
  } env;
  std::vector<hipEvent_t> ev_k;  // pairs around expand launches
  uint32_t n_cus = 256, expand_grid = 2048;
  bool host_only = false;        // a planner probe (psengine_plan.h): no device
  psamd::WindowLayout probe;     // the probe's last planned window
  psamd::WindowSchedule probe_sched;  // ... and its schedule (PS_PLAN_SCHEDULE)
  // per-window uploads (topic table, seeds, descriptors) kept on the device:
  // the bytes last staged into each buffer, skipped when a window repeats them
  struct UploadShadow {
    uint64_t gen = 0;
    std::vector<uint8_t> data;
  };
  std::map<const psamd::DevBuf*, UploadShadow> upload_shadow;
  bool defer_into_signalled = false;  // the window being enqueued raises its flag in its reduce
  uint64_t sig_seq = 0;
  // a signalled window's reduce, held back to run in the next window's first
  // launch (k_window_turn) -- or alone, from ps_wait, if none comes first
  struct PendingReduce {
    bool valid = false;
    const void* owner = nullptr;  // the RunSlot whose flag it raises
    psamd::ReduceArgs args{};
  } pend_reduce;
  bool gpu_graph = false;     // the current node space was built on the GPU
  bool mirrors_valid = true;  // host copies of node_peer / flags / CSR are current
  std::vector<uint32_t> pairs_host, gstat_host, roots_host;
  // which build produced the node spaces since creation (PS_GRAPH_BUILD,
  // include/psengine_plan.h): plain host counters, bumped by gpu_build_graph
  // and upload_graph (the probe: its one host build)
  struct BuildReport {
    uint64_t gpu_builds = 0, host_builds = 0;
    uint64_t fb_stall = 0, fb_attempts = 0, fb_capacity = 0, fb_depth = 0;  // fall-backs to the host build
    uint64_t redo_grid = 0, redo_order = 0, redo_depth = 0;                // GPU attempts repeated
    uint32_t last_kind = 0;      // 0 none yet, 1 GPU, 2 host
    uint32_t last_attempts = 0;  // GPU attempts of the last build (a host build after a fall-back keeps them)
  } build_rep;
  bool live_dev_valid = false;  // d_live holds `live` (uploaded again only after ps_set_live)
  bool flags_built = false;     // the last GPU build wrote the node flags (no flags pass needed)
  uint32_t* pairs_pinned = nullptr;  // pinned staging of the parent deltas
  size_t pairs_pinned_cap = 0;       // (u32 words)
  std::vector<size_t> pair_off;
  psamd::DevBuf d_tpar, d_orph, d_local, d_first,
      d_gstat, d_cub, d_pairs, d_live, d_roots, d_cnt, d_fidx, d_childoff, d_lbstat, d_sigctr, d_kids, d_big, d_ndeg, d_nkat, d_query;
  std::chrono::steady_clock::time_point t_run0;
  // the lazy prune's reach queries, enqueued with the GPU rebuild that
  // precedes the run's last phase (its result comes back with the build's
  // readback, no round trip of its own); the prune uses a result whose peers
  // match its question, else asks the GPU itself
  struct EarlyQuery {
    uint32_t topic = 0;
    std::vector<uint32_t> peers;
    std::vector<uint8_t> out;
    bool launched = false, ready = false;
  };
  std::vector<EarlyQuery> early_q;
  // k_flood (opts.flood and the flood_* options)
  bool flood_broken = false;  // a dependency wait timed out once: per-level launches from then on
  uint32_t flood_grid = 0;    // resident blocks (0: k_flood unavailable)
  uint32_t pull_words = psamd::kPullWords;    // row words per k_pull chunk (512..4096 measured: 1024 best)
  uint32_t flood_epoch = 0;   // granule tag of the last launch (granules are never reset)
  psamd::FloodPlan flood;
  uint64_t flood_up = ~0ull;  // plan version of the tasks on the device
  psamd::DevBuf d_flood_tasks, d_flood_segs, d_flood_gran;
  psamd::DevBuf d_flood_prof;  // env.flood_profile
  uint32_t flood_prof_waves = 0;
  psamd::DevBuf d_chain_prof;  // env.chain_prof_path

  std::vector<psamd::TopicHost> topics;
  std::vector<uint8_t> live;
  bool graph_dirty = true, flags_dirty = true;
  uint64_t graph_epoch = 0, flags_epoch = 0;  // bumped by every upload

  // level mode, per-round counter slots and their reduce descriptors
  // (on the device: the run slot's woff)
  std::vector<uint32_t> woff_host, desc_host;
  // level-aligned windows: the (topic, level) pieces of k_level_reach, cached
  // per node space and active topic set
  psamd::DevBuf d_reach;
  std::vector<psamd::ReachPiece> reach_host;
  std::vector<uint64_t> reach_key;
  uint32_t n_reach = 0, reach_a = 0;  // pieces; those of levels <= the prefix P (first)
  // level mode, pull direction: per-round chunks of next-level nodes
  psamd::PullPlan pull;
  psamd::DevBuf d_pull;
  uint64_t pull_up = ~0ull;  // plan version of the chunks on the device
  // pair and chain launches (the opts.chain_* options)
  psamd::DevBuf d_chain;
  std::vector<uint64_t> chain_fail_key;  // a pair plan whose chain ranges overflowed the level tables: no chains
  psamd::DevBuf d_chain_ovf;
  psamd::DevBuf d_chain_meta, d_chain_cnt, d_chain_scan;  // the chunks' node entries (k_chain_meta)
  psamd::DevBuf d_fill_segs, d_fill_pieces;  // pair.fill and its pieces (uploaded / built with the chain chunks)
  uint64_t chain_fills = 0;                  // chain launches run as reach + fill (ps_chain_fill_launches)
  // rows of rounds writing at least this much store non-temporally (the MALL
  // cannot hold them for the next launch: reversing launch order and cached
  // stores measured 0-50 % slower, profiles/r03/ab_mall_reverse.txt)
  static constexpr uint64_t kNtBytes = 64ull << 20;
  psamd::PairPlan pair;
  psamd::DevBuf d_pp;
  uint64_t pair_up = ~0ull;
  std::vector<uint8_t> round_kind;  // per round of the current window: PS_K_* (empty: k_expand)

  // fused node space (host mirror)
  uint32_t n_nodes = 0, n_pad = 16;
  std::vector<uint32_t> node_peer, row_ptr, col;
  std::vector<uint32_t> node_parent;  // node-space parent on this rank (kNone: root / remote)
  std::vector<uint16_t> node_topic;
  std::vector<uint8_t> node_flags;

  psamd::DevBuf d_row_ptr, d_col, d_node_topic, d_node_flags, d_node_peer, d_node_parent;
  psamd::DevBuf d_ext0, d_ext1;  // compaction mode, one rank: arrival extents (ExpandArgs::ext_cur)
  // A row set: the seen rows, the two arrival rows and the nodes' generation
  // bytes.  `rows` always names the set the last window wrote, rows_other the
  // set a twin or alternating window writes next (they swap: §5.3d below).
  struct RowSet {
    psamd::DevBuf seen, arr0, arr1, gen;
    uint32_t gen_cur = 0;  // window generation stamped into gen (1..255)
    void swap(RowSet& o) {
      seen.swap(o.seen);
      arr0.swap(o.arr0);
      arr1.swap(o.arr1);
      gen.swap(o.gen);
      std::swap(gen_cur, o.gen_cur);
    }
  } rows, rows_other;
  psamd::DevBuf d_hop, d_flags, d_blk, d_frontier, d_nfront, d_wgcount, d_stats, d_digest;
  psamd::DevBuf d_remote_fed, d_send, d_recv, d_apply_stats;
  // multi-GPU level mode: ghost parents
  std::vector<uint32_t> ghost_ref;  // per node: remote parent's rank << 27 | record index, or kNone
  std::vector<psamd::ShipEntry> ship_host;  // every topic's send entries (TopicHost::ship0)
  psamd::GhostPlan ghost;
  psamd::DevBuf d_ghost_ref, d_ship, d_gsegs, d_pack;
  bool ghost_up = false;  // the ghost plan's segments and root segments are on the device
  uint32_t n_remote_fed = 0;
  std::vector<uint32_t> remote_fed;  // owned nodes whose parent is on another rank

  // multi-GPU: this engine owns a hash-partitioned share of every topic
  int32_t rank = 0, world = 1;
  bool inplace = false;  // PS_DIST_F_INPLACE: kSegInPlace segments, RankRows of every rank
  psamd::DevBuf d_rrows;
  std::vector<psamd::RankRows> rrows_host;
  bool rrows_dirty = false;
  uint32_t partition = PS_PART_PEER, split_depth = 0;
  std::unique_ptr<psamd::Transport> transport;

  // publishes not yet run
  std::vector<psamd::RunMsg> pending;
  bool pending_nonzero_start = false;  // some pending message starts after round 0
  bool pending_mixed = false;          // pending messages name more than one topic
  uint32_t pending_topic0 = 0;         // ... the topic of the first one
  uint32_t run_iota_n = 0;             // run_sorted / run_rank hold 0 .. n-1 (one-topic runs)
  bool run_zero_start = true;          // every message of the current run starts in round 0
  uint32_t next_msg = 0;

  // results of the last run
  uint32_t last_first = 0, last_n = 0;
  bool have_hops = false;
  std::vector<uint8_t> hops;  // [msg][peer]
  std::vector<psamd::RunMsg> last_msgs;  // messages of the last run, publish order
  std::vector<uint32_t> run_sorted;      // run message indices grouped by topic
  std::vector<uint32_t> run_topic_off;   // topic -> first position in run_sorted
  std::vector<uint32_t> run_rank;        // message -> position within its topic
  std::vector<uint32_t> last_lo, last_cnt;  // topic -> last window's rank range
  // topic -> the last window's row bit of each window message (empty: bit li
  // = the message's window slot; else the start-group layout, StartGroup)
  std::vector<std::vector<uint32_t>> last_pos;
  std::vector<std::vector<psamd::StartGroup>> last_groups;  // topic -> the last window's start groups
  std::vector<psamd::TopicDev> last_topics;
  bool have_window = false;
  // the last window's last round (WindowRun::r; a deferred window's RunSlot::r):
  // no hop ps_spread_track's pass can report lies beyond it
  uint32_t last_rounds = 0;
  std::map<uint32_t, std::vector<uint32_t>> peer_node;  // topic -> peer -> node (peer_node_map)
  std::vector<uint64_t> peer_node_epoch;                 // graph_epoch each map was built for
  uint64_t window_seq = 0;  // bumped whenever last_* change (a new last window)

  // The batched drain of the last window (host code:
  // drain_*.cpp, drain_impl.hpp).  The fields are grouped by what owns them;
  // copy_stream and ev_t serve every call.
  struct Drain {
    // one call's queries on the device, the ids per segment, their offsets
    // (the scan of the counts) and the scan's temporary storage
    struct Scratch {
      psamd::DevBuf d_queries, d_cnt, d_off, d_scan;
    };
    // the shared-list pass's device buffers (drain_shared.cpp: shared_pass;
    // DESIGN.md §5.5d): the lists and their counts, the input block (queries,
    // verdicts, sorted queries, bins), the numbering scan's keys and their
    // sums, the control block with the topics' first full queries behind it
    struct ListBufs {
      Scratch scratch;
      psamd::DevBuf d_in, d_key, d_aux;
    };

    // The window's tables (per topic: bit -> message id, message mask or
    // arrival order), one set per window: whichever call drains a window
    // first builds them (drain_tables.cpp) and every other call, the sink
    // included, reads them through p_*.  Every use is ordered on `stream`.
    struct Tables {
      uint64_t seq = ~0ull;  // window_seq the tables on the device were built for
      std::vector<psamd::DrainTopic> topics;
      // the host build (drain_tables: the synchronous calls)
      psamd::DevBuf d_topics, d_groups, d_ids, d_mask, d_order;
      // the device build (drain_tables_async: the begin calls and the sink;
      // DESIGN.md §5.5b): one uploaded block (topics, groups, the build's
      // message arrays, a gather topic's order), the id table (device-built
      // positions, then the gather topics' ids), the mask words with the
      // error word behind them, the check's keys
      psamd::DevBuf d_ablock, d_aids, d_amask, d_akeys;
      // the device build's error word (in d_amask), read by the kernels of the
      // begin calls and the sink; made on first use where only host builds ran
      uint32_t* d_err = nullptr;
      // the tables the device holds for `seq`, wherever they were built
      const psamd::DrainTopic* p_topics = nullptr;
      const psamd::DrainGroup* p_groups = nullptr;
      const uint32_t* p_ids = nullptr;
      const uint64_t* p_mask = nullptr;
      const uint32_t* p_order = nullptr;
    } tab;

    // The synchronous calls' buffers (ps_drain, ps_drain_shared,
    // ps_drain_topics: one call at a time, each waits for its own work).
    struct Sync {
      Scratch scratch;  // all three
      std::vector<psamd::DrainQuery> queries;  // ps_drain, ps_drain_shared: the resolved queries
      // ps_drain: the host copy of the segment offsets, the two output slabs
      // and, per slab, the events behind its emit and its copy
      std::vector<uint64_t> off;
      psamd::DevBuf d_slab[2];
      hipEvent_t ev_emit[2] = {nullptr, nullptr}, ev_copy[2] = {nullptr, nullptr};
      // ps_drain_shared: the classify pass's bins, sorted
      // queries and verdicts
      psamd::DevBuf d_cbins, d_cqueries, d_verdict;
      // ps_drain_shared, ps_drain_topics (the synchronous list tail): the
      // list queries' offsets header, with a zero error word behind it, and
      // their ids; ps_drain_shared's host copy of the header
      psamd::DevBuf d_hdr, d_lists;
      std::vector<uint64_t> hdr;
    } sync;

    // The sort's host scratch (drain_shared.cpp: drain_shared_sort), filled by
    // ps_drain_shared and, through shared_stage, by ps_drain_shared_begin and
    // the sink: every query's host verdict and the classified queries by topic
    struct Sort {
      std::vector<uint32_t> verdict;
      std::vector<psamd::DrainClassQuery> cqueries;
      // what the sort leaves beside them
      struct SharedSort {
        std::vector<psamd::DrainClassBin> bins;
        uint32_t n_class = 0, n_waves = 0;
        uint32_t n_rows = 0, n_gather = 0;  // queries with a row; those of kDrainGather topics
        uint64_t row_ids = 0, gather_ids = 0, bin_ids = 0;  // window messages: per such query; per bin
        uint32_t max_segs = 0;  // segments of the widest topic with a row queried
      };
    } sort;
    using SharedSort = Sort::SharedSort;

    // The switches read from the environment at ps_create (api.cpp: read_switches)
    struct Switches {
      uint64_t slab_ids = 64ull << 20;  // ps_drain: ids per slab (A/B: PSAMD_DRAIN_SLAB_IDS, at least one segment)
      bool staged = true;       // the synchronous calls: LDS-staged emit (A/B: PSAMD_DRAIN_EMIT=direct)
      bool timing = false;      // every call: PSAMD_DRAIN_TIMING=1, phases run apart, times to stderr
      bool mapped_out = false;  // ps_drain_begin: emit straight into the pinned view (A/B: PSAMD_DRAIN_ASYNC_OUT=mapped)
      // the shared calls, ps_drain_topics and the sink: full rows share their topic's list (A/B: PSAMD_DRAIN_SHARED=private)
      bool share = true;
      // ps_peer_load, ps_load_track: a full row is counted from its words like a partial one (A/B: PSAMD_LOAD_COUNT=rows)
      bool load_rows = false;
      // ps_topic_spread: a frontier node with more child entries than this is walked by its wave, lanes across
      // entries; up to it by its lane alone (A/B: PSAMD_SPREAD_WIDE, 0: every node by the wave)
      uint32_t spread_wide = 16;
      // ps_spread_track: level launches of a tracked window at most, to show that a truncated BFS is detected
      // and counted (A/B: PSAMD_SPREAD_TRACK_LEVELS; unset: the window's r + 1)
      uint32_t spread_track_levels = 0xFFFFFFFFu;
    } env;

    hipStream_t copy_stream = nullptr;        // results leave on it, beside whatever `stream` runs next
    hipEvent_t ev_t[2] = {nullptr, nullptr};  // PSAMD_DRAIN_TIMING: around one phase

    // ps_drain_begin / ps_drain_end.
    // Two drains may be outstanding, in slots that alternate.  A slot owns
    // its pinned input staging (queries and, when it builds them, the
    // window's table block), its count / offset / scan / result buffers and
    // its pinned view: (n + 2) u64 header words (off[0..n], the error word),
    // then from hdr_bytes the ids.
    struct Slot {
      bool enqueued = false;      // work is on the GPU (else the view was written by the host)
      bool emit_pending = false;  // ev_emit is recorded and ps_drain_end has not seen it complete
      const void* seen = nullptr;  // the row set its emit reads
      uint8_t* h_in = nullptr;
      size_t in_cap = 0;
      uint8_t* h_res = nullptr;
      uint8_t* h_res_dev = nullptr;  // h_res, device-mapped
      size_t res_cap = 0;
      ListBufs lb;  // (ps_drain_begin uses its scratch alone)
      psamd::DevBuf d_res;
      hipEvent_t ev_emit = nullptr, ev_done = nullptr;
      size_t n = 0, hdr_bytes = 0;
      uint64_t bound = 0;
      // ps_drain_shared_begin takes the same slots.  Its
      // view: a DrainSharedHdr, then list_off[list_cap + 1], list_of_query[n]
      // and ids[id_cap] at o_*
      enum Kind { kPlain, kShared, kTopics } kind = kPlain;  // whose end call completes it
      size_t list_cap = 0, id_cap = 0;
      size_t o_off = 0, o_lq = 0, o_ids = 0;
      // ps_drain_topics_begin too.  Its view: a
      // DrainSharedHdr, then topic_list[n], n_full[n], exc_off[n + 1],
      // exc_peer[exc_cap], exc_list[exc_cap], list_off[list_cap + 1] (o_off)
      // and ids[id_cap] (o_ids); behind what the device writes, n_nodes[n]
      // from the host.  The strips' verdicts, counts and records are the
      // slot's own: two drains may be outstanding beside a synchronous call.
      size_t exc_cap = 0;
      size_t o_tl = 0, o_nf = 0, o_eo = 0, o_ep = 0, o_el = 0, o_nn = 0;
      psamd::DevBuf d_verdict, d_exc, d_full, d_rec;
    } slot[2];
    uint32_t slot_head = 0, slot_count = 0;

    // ps_drain_topics: the strips, verdict bytes and strip
    // counts on the device, the exception records behind them, and the
    // answer the call lends (host memory; the ids pinned) until the next call
    struct Audience {
      psamd::DevBuf d_strips, d_verdict, d_exc, d_full, d_rec;
      std::vector<psamd::AudStrip> strips;
      std::vector<uint32_t> strip_full, topic_list, exc_peer, exc_list, exc_node;
      std::vector<uint8_t> exc_verdict;
      std::vector<uint64_t> strip_off, n_nodes, n_full, exc_off, list_off;
      uint8_t* h_ids = nullptr;
      size_t ids_cap = 0;
    } aud;

    // ps_sink_set / ps_sink_take: standing queries drained
    // behind every window of a run into one result per run.  Two results may
    // be untaken, in slots that alternate; a slot owns its result on the
    // device (win_list rows; the two cursors with list_off behind them; ids),
    // its pinned view and the pinned staging of its run's windows.  The
    // per-window passes share one set of device buffers: they all run on
    // `stream`, one window after the other.
    // What the audience pass's stage step leaves beside the entries and the
    // strips (drain_topics.cpp: aud_stage): the shape its buffers and grids
    // are sized by, and the engine's own caps for the window
    struct AudShape {
      uint32_t ns = 0;                          // strips
      uint64_t n_verdicts = 0, row_bytes = 0;   // nodes with a row to classify; the row bytes read
      uint32_t max_segs = 0;                    // segments of the widest named topic with a row
      uint64_t own_exc = 0, own_lists = 0, own_ids = 0;
    };

    struct Sink {
      bool on = false;
      // one sink of one kind: standing (topic, peer) queries (ps_sink_set), or
      // standing topics drained as ps_drain_topics does (ps_sink_set_topics,
      // `peer` is empty); the take call of the kind completes it
      enum Kind { kQueries, kTopics } kind = kQueries;
      std::vector<uint32_t> topic, peer;
      size_t list_cap = 0, id_cap = 0;  // the caller's (both zero: the engine's, summed over the windows)
      size_t exc_cap = 0;               // kTopics: the caller's (there each cap that is zero is the engine's)
      struct Chunk {
        uint8_t* h = nullptr;
        size_t cap = 0;
      };
      struct Res {
        psamd::DevBuf d_wl, d_off, d_ids;  // d_off: SinkCursor[2] in its first 256 bytes
        std::vector<Chunk> arena;          // pinned staging: every window of the run takes its own region
        size_t arena_used = 0;             // ... of the last chunk
        uint8_t* h_res = nullptr;
        size_t res_cap = 0;
        hipEvent_t ev_done = nullptr;
        bool enqueued = false;  // (else the host wrote the view: a run without a window)
        uint32_t windows = 0;
        size_t list_cap = 0, id_cap = 0;     // as far as the last window
        size_t o_wl = 0, o_off = 0, o_ids = 0;  // the view: a SinkCursor, then these
        uint64_t run = 0;                    // the run's number (drain_fence)
        // kTopics: d_wl holds the topic_list rows; the n_full and exc_off rows
        // and the exception records beside it, grown with their contents kept;
        // n_nodes rows from the host, written into the view (o_nn) behind what
        // the copies bring.  The view: a SinkCursor, topic_list (o_wl), n_full,
        // exc_off, exc_peer, exc_list, list_off (o_off), ids (o_ids), n_nodes.
        psamd::DevBuf d_nf, d_eo, d_ep, d_el;
        std::vector<uint64_t> n_nodes;
        size_t exc_cap = 0;
        size_t o_nf = 0, o_eo = 0, o_ep = 0, o_el = 0, o_nn = 0;
      } res[2];
      uint32_t head = 0, count = 0;  // untaken results, oldest first
      Res* open = nullptr;           // the run being enqueued
      uint64_t runs = 0, runs_done = 0;  // runs opened; the last whose result was seen complete
      // the last sink emit per row set: a window about to write the set waits for it
      struct Fence {
        const void* seen = nullptr;
        hipEvent_t ev = nullptr;
        uint64_t run = 0;  // 0: nothing pending
      } fence[2];
      hipEvent_t last_ev = nullptr;  // the fence event behind the open run's last window
      double host_ms = 0;            // PSAMD_DRAIN_TIMING: the open run's host time in the sink
      // per-window passes: the window's list_of_query beside their buffers
      ListBufs lb;
      psamd::DevBuf d_lq;
      // the sorted queries of the last window, kept while the node space and
      // the topics' window shapes stay
      std::vector<uint64_t> sort_key;
      std::vector<uint8_t> sort_tail;
      SharedSort sort_r;
      // kTopics: the entry table and the strips on the device, kept while
      // what they are cut from stays (strip_key: graph_epoch and each standing
      // topic's table flags, n_pos, node range); the window's verdicts, strip
      // counts, records and window-local view (one set: all on `stream`)
      psamd::DevBuf d_strips, d_verdict, d_exc, d_full, d_rec, d_view;
      std::vector<uint64_t> strip_key;
      size_t strip_bytes = 0;  // PSAMD_DRAIN_TIMING: the bytes the open run's windows uploaded for them
    } sink;

    // What the standing passes behind a run's windows keep alike
    // (drain_standing.cpp).
    // Pinned staging, one arena per run in turn (run k: arena[k & 1]): every
    // window of the run takes a region of its own, and the arena is reused
    // once the last pass of the run two before is complete (ev)
    struct PassArena {
      Sink::Res mem;  // (its arena alone: drain_tables.cpp sink_stage)
      hipEvent_t ev = nullptr;
      bool pending = false;
    };
    // the last pass per row set: a window about to write the set on another
    // stream waits for it (run.cpp: drain_fence)
    struct PassFence {
      const void* seen = nullptr;
      hipEvent_t ev = nullptr;
      bool pending = false;
    };
    // One tracker (ps_*_track / ps_*_take): the standing topics, the counts
    // since the last take or track call, and what orders its passes against
    // the runs around them.  Every family owns one; none shares an arena or an
    // event with another, since each pass may still be pending when the next
    // run opens.
    struct Standing {
      const char* name;  // in messages: load, hops, downstream, cut, report, blame, spread
      bool on = false;
      std::vector<uint32_t> topic;
      // windows; (mesh topic, window) pairs left out of the tree answers
      uint64_t windows = 0, skipped = 0;
      // the pass's input block stays on the device while what it is cut from
      // stays: graph_epoch, each standing topic's table shape and node range,
      // and what the family adds (standing_key_topic)
      std::vector<uint64_t> strip_key;
      PassArena arena[2];
      uint64_t runs = 0;
      PassArena* open = nullptr;  // the run being enqueued
      PassFence fence[2];
      hipEvent_t ev_take = nullptr;
    };
    // A blocking call's answer (ps_peer_load and its like): the sums on the
    // device, the staged input block, the pinned copy handed out -- the
    // family's take hands its totals out through the same pinned copy
    struct Answer {
      psamd::DevBuf d_out;
      std::vector<uint8_t> stage;  // (the upload is waited for in the call)
      uint8_t* h_out = nullptr;
      size_t out_cap = 0;
    };

    // ps_peer_load / ps_load_track / ps_load_take (host code:
    // drain_load.cpp): per-peer recv / sent sums from the audience pass's
    // verdicts, k_audience_load behind k_audience_classify.  The blocking
    // call and the standing pass each own their entries and strips, verdict
    // bytes and strip counts; nothing here is the sinks'.
    struct Load {
      // one pass's device buffers: entries | strips in one block, the verdict
      // bytes, the two strip counts classify leaves beside them
      struct Pass {
        psamd::DevBuf d_in, d_verdict, d_exc, d_full;
      };
      // what the grids and buffers of a pass are sized by
      struct Shape {
        uint32_t ns = 0;
        uint64_t n_verdicts = 0;
      };
      Pass sync, track;  // ps_peer_load's, the standing pass's
      Answer ans;        // recv | sent in peer space
      Standing st{"load"};
      psamd::DevBuf d_acc;  // the totals, recv | sent in peer space
      Shape kept;           // the block on the device (st.strip_key)
    } load;

    // ps_topic_hops / ps_hops_track / ps_hops_take (host
    // code: drain_hops.cpp): per tree topic, nodes / reached / deliv by BFS
    // level from the audience pass's verdicts, k_audience_hops and
    // k_audience_hops_sum behind k_audience_classify.  Shaped as Load: the
    // blocking call and the standing pass each own their buffers, and nothing
    // here is the sinks' or the load pass's.
    struct Hops {
      // one pass's device buffers: entries | levels | strips in one block, the
      // verdict bytes and strip counts of classify, the (strip, level) partials
      struct Pass {
        psamd::DevBuf d_in, d_verdict, d_exc, d_full, d_part_r, d_part_d;
      };
      // what hops_stage leaves beside the block: where its parts lie and what
      // the grids and buffers are sized by
      struct Shape {
        size_t n = 0;                 // tree topics: the entries
        size_t o_lvl = 0, o_strips = 0, bytes = 0;
        uint32_t ns = 0, max_cols = 0;
        uint64_t n_verdicts = 0, n_parts = 0, row_bytes = 0;
      };
      Pass sync, track;  // ps_topic_hops's, the standing pass's
      Answer ans;        // nodes | reached | deliv, [n][PS_MAX_ROUNDS] each by request position
      Standing st{"hops"};
      psamd::DevBuf d_acc;  // the totals, laid out as the answer
      Shape kept;           // the block on the device (st.strip_key)
    } hops;

    // ps_peer_downstream / ps_downstream_track / ps_downstream_take (DESIGN.md
    // §5.5k; host code: drain_downstream.cpp): per peer, the nodes and the
    // window messages strictly below its nodes in the named tree topics, from
    // the audience pass's verdicts: k_audience_weights behind
    // k_audience_classify, then one k_downstream_level launch per BFS level,
    // bottom-up, and k_downstream_top.  Shaped as Hops: the blocking call and
    // the standing pass each own their buffers, and nothing here is the
    // sinks', the load pass's or the hop pass's.
    struct Downstream {
      // one pass's device buffers: entries | levels | work | strips in one
      // block, the verdict bytes and strip counts of classify, and the
      // scratch k | w_n | w_k (16 bytes a node, grow-only)
      struct Pass {
        psamd::DevBuf d_in, d_verdict, d_exc, d_full, d_scratch;
      };
      // what down_entries leaves beside the block: where its parts lie, what
      // the grids and buffers are sized by, and the work items of each level
      // launch: launch j's are [launch[j], launch[j + 1])
      struct Shape {
        size_t n = 0;  // tree topics: the entries
        size_t o_lvl = 0, o_work = 0, o_strips = 0, bytes = 0;
        uint32_t ns = 0;
        uint64_t n_verdicts = 0, n_nodes = 0, row_bytes = 0;
        std::vector<uint32_t> launch;
      };
      explicit Downstream(const char* name) : st{name} {}
      Pass sync, track;  // ps_peer_downstream's, the standing pass's
      Answer ans;        // below | carried in peer space
      Standing st;
      psamd::DevBuf d_acc;  // the totals, laid out as the answer
      Shape kept;           // the block on the device (st.strip_key)
    } down{"downstream"};

    // ps_peer_cut / ps_cut_track / ps_cut_take (host code:
    // drain_cut.cpp): per peer, what its nodes missed, and for its cut points
    // -- nodes that lack messages under a full parent -- their number, the
    // nodes behind them and the deliveries lost at and behind them:
    // k_audience_missed behind k_audience_weights, then k_cut_level per BFS
    // level and k_cut_top over the downstream pass's plan.  The alias stays:
    // the state has the downstream pass's shape, member for member, with four
    // arrays where that holds two (missed | cuts | orphaned | lost in the
    // answer and the totals); it shares no buffer with it.
    using Cut = Downstream;
    Cut cut{"cut"};

    // ps_peer_report / ps_report_track / ps_report_take (host
    // code: drain_report.cpp): the four answers above from one pass --
    // k_report_nodes behind one k_audience_classify, k_audience_hops_sum, and
    // one bottom-up sweep (k_report_level / k_report_top where both subtree
    // sections are selected, else that section's own level kernels).  Shaped
    // as the others: the blocking call and the standing pass each own their
    // buffers, and nothing here is another family's.
    struct Report {
      // one pass's device buffers: the input block (report entries | hop
      // entries | downstream entries | levels | work | strips), the verdict
      // bytes and strip counts of classify, the hop partials, the scratch
      // k | w_n | w_k
      struct Pass {
        psamd::DevBuf d_in, d_verdict, d_exc, d_full, d_part_r, d_part_d, d_scratch;
      };
      // where the block's parts lie and what the grids and buffers are sized by
      struct Shape {
        size_t n = 0, n_tree = 0;  // entries: all of them, the tree topics in front
        size_t o_hops = 0, o_down = 0, o_lvl = 0, o_work = 0, o_strips = 0, bytes = 0;
        uint32_t ns = 0, max_cols = 0;
        uint64_t n_verdicts = 0, n_parts = 0, n_nodes = 0, row_bytes = 0;
        std::vector<uint32_t> launch;
      };
      // where the eleven arrays lie in an output block of 64-bit words, in
      // ps_report's order: recv sent nodes reached deliv below carried missed
      // cuts orphaned lost; off[11]: the block's words
      struct Out {
        size_t off[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      };
      Pass sync, track;  // ps_peer_report's, the standing pass's
      Answer ans;        // the cleared output block
      Standing st{"report"};
      uint32_t what = 0;    // the standing sections
      psamd::DevBuf d_acc;  // the totals: the output block's layout over the standing topics
      Shape kept;           // the block on the device (st.strip_key)
    } report;

    // ps_dist_report (host code: drain_dist.cpp): a rank's
    // share of the load, hop and downstream sections -- k_dist_nodes behind
    // one k_audience_classify, k_dist_hops_sum, then k_dist_sweep_level per level with the
    // transport's exchange and k_dist_apply where a level's edges cross ranks.
    // Blocking only; buffers of its own.
    struct Dist {
      // the input block (entries | levels | send bases | work | apply | strips),
      // classify's verdicts and counts, the hop partials, the per-node words
      // k | acc_n | acc_k, the sweep's send and receive records, the cleared
      // output block
      psamd::DevBuf d_in, d_verdict, d_exc, d_full, d_part_r, d_part_d, d_scratch, d_send, d_recv, d_out;
      // ps_dist_cut (§5.5o) works in the same buffers -- both calls block -- and
      // in the words of its downward exchange: the parents' k sent and received
      psamd::DevBuf d_dsend, d_drecv;
      std::vector<uint8_t> stage;  // (the upload is waited for in the call)
      uint8_t* h_out = nullptr;
      size_t out_cap = 0;
      // ps_dist_blame (§5.5r) too, with 8-byte pairs in d_dsend / d_drecv: the
      // sweep's words cut_peer | cut_hop, a word per owned node each; the
      // strips' record counts, their exclusive sum and its temporary; the
      // entries' record offsets; the record arrays the call was asked for
      psamd::DevBuf d_cut, d_cnt, d_off, d_scan, d_rec_off, d_rec;
      // pinned: rec_off and the record arrays lent until the next ps_dist_blame
      uint8_t *h_off = nullptr, *h_rec = nullptr;
      size_t off_cap = 0, rec_cap = 0;
    } dist;

    // ps_topic_spread (host code: drain_spread.cpp): hops and
    // duplicate copies of meshes and trees -- k_spread_nodes behind one
    // k_audience_classify, one k_spread_level launch per BFS level over the
    // child lists, k_spread_sum and k_spread_dup.  Blocking only; buffers of
    // its own.
    struct Spread {
      // one pass's device buffers: the input block (entries | strips),
      // classify's verdicts and counts, the per-node words k | hop, the three
      // frontier counts with the two queues behind them
      struct Pass {
        psamd::DevBuf d_in, d_verdict, d_exc, d_full, d_scratch, d_queue;
      };
      Pass pass;
      psamd::DevBuf d_out;  // the cleared output block
      std::vector<uint8_t> stage, seed;  // (the uploads are waited for in the call)
      // the pinned copy of the output block; behind it the frontier count the
      // host reads between batches of level launches
      uint8_t* h_out = nullptr;
      size_t out_cap = 0;
    } spread;

    // ps_topic_blame / ps_blame (host code: drain_blame.cpp):
    // each missed subscriber with its cut point -- k_blame_top and one
    // k_blame_level launch per BFS level, top-down, behind the downstream
    // pass's front (k_audience_classify, k_audience_weights) over its plan;
    // then k_blame_count, the scan and k_blame_emit into records, or
    // k_blame_gather for explicit queries.  Blocking only; buffers of its own.
    struct Blame {
      // the front's buffers and the staged input block, as down_front and
      // down_sync_stage take them
      Downstream::Pass front;
      std::vector<uint8_t> stage;  // (the upload is waited for in the call)
      // the sweep's words cut_node | cut_level, a word per node each; the
      // strips' record counts, their exclusive sum and its temporary; the
      // entries' record offsets; the record arrays the call was asked for
      psamd::DevBuf d_cut, d_cnt, d_off, d_scan, d_rec_off, d_rec;
      // ps_blame: queries | topic table | levels in one block, the four outputs
      psamd::DevBuf d_q, d_out;
      std::vector<uint8_t> qstage;  // (the upload is waited for in the call)
      // pinned: rec_off, the record arrays lent until the next ps_topic_blame,
      // and ps_blame's outputs
      uint8_t *h_off = nullptr, *h_rec = nullptr, *h_out = nullptr;
      size_t off_cap = 0, rec_cap = 0, out_cap = 0;
    } blame;

    // ps_blame_track / ps_blame_take (host code:
    // drain_blame_track.cpp): the blame pass behind every window of a run, its
    // records appended at a cursor on the device -- k_blame_track_commit and
    // k_blame_track_emit behind the blocking call's front, sweep, count and
    // scan.  Nothing here is the blocking call's or another tracker's.
    struct BlameTrack {
      // the tracker, the pass's buffers and the block kept on the device, as
      // the other subtree trackers keep theirs (down_window_stage)
      Standing st{"blame"};
      Downstream::Pass track;
      Downstream::Shape kept;
      size_t rec_cap = 0;  // the caller's (zero: the engine's, summed as the windows come)
      uint64_t cap = 0;    // the cap in effect as far as the last window
      // the sweep's words, the strips' record counts, their exclusive sum and
      // its temporary; request position -> the entry behind it; the two
      // cursors (BlameCursor[2]); the run's rec_off and the five record
      // arrays, grown with their contents kept
      psamd::DevBuf d_cut, d_cnt, d_off, d_scan, d_map, d_cur, d_rec_off, d_rec[5];
      // pinned: the cursor read at a take, rec_off and the record arrays lent
      // until the next ps_blame_take or ps_blame_track
      uint8_t *h_cur = nullptr, *h_off = nullptr, *h_rec = nullptr;
      size_t cur_cap = 0, off_cap = 0, view_cap = 0;
      hipEvent_t ev_t[2] = {nullptr, nullptr};  // PSAMD_DRAIN_TIMING: around a window's phases
    } blame_trk;

    // ps_spread_track / ps_spread_take (host code:
    // drain_spread_track.cpp): the spread pass behind every window of a run,
    // meshes and trees alike -- the blocking call's kernels with the window's
    // last round + 1 level launches enqueued whole, k_spread_track_close behind
    // them, adding into totals.  Nothing here is the blocking call's or another
    // tracker's.
    struct SpreadTrack {
      Standing st{"spread"};
      Spread::Pass track;
      // what the kept block (st.strip_key) was cut into
      struct Shape {
        uint32_t ns = 0;
        uint64_t n_verdicts = 0;
      } kept;
      // the totals: the truncated windows' count, then the blocking call's
      // output block over the standing topics (dup written by the take)
      psamd::DevBuf d_acc;
      Answer ans;  // the pinned copy a take hands out from
      uint64_t level_launches = 0;  // since the last take or track call (PSAMD_DRAIN_TIMING)
      hipEvent_t ev_t[2] = {nullptr, nullptr};  // PSAMD_DRAIN_TIMING: around a window's phases
    } spread_trk;

    // the seven trackers, in the order run.cpp's hooks run them behind the sink
    std::array<Standing*, 7> standing() {
      return {&load.st, &hops.st, &down.st, &cut.st, &report.st, &blame_trk.st, &spread_trk.st};
    }
  } drain;

  // The slot tables of ps_dist_report's cross-rank sweep (graph.cpp
  // build_dist_slots), built on the first report after a node-space build
  struct DistSlots {
    uint64_t epoch = ~0ull;       // graph_epoch the tables stand for
    std::vector<uint32_t> gslot;  // per node: a remote parent's owner << 27 | its record index there; kNone: none
    std::vector<uint32_t> plist;  // per ghost record this rank receives as the parents' owner: the parent's node
    // per topic, by (children's level L, children's rank b): the first word
    // of plist, TopicHost::gcnt[(L * world + rank) * world + b] of them
    std::vector<std::vector<uint32_t>> pl_off;
    psamd::DevBuf d_gslot, d_plist;
  } dist_slots;

  // per-window uploads (topic table, seeds, reduce descriptors) go through
  // pinned staging: a copy from pageable memory blocks the host until the
  // stream has drained, so the next batch's launches would only be issued
  // once the previous batch had finished (a ~35 us bubble per pipelined
  // step).  Two slots alternate; a slot is rewritten only after the copies
  // of its previous use have completed: slot i belongs to asynchronous run
  // slot i (synchronous runs use slot 0 with nothing in flight).
  struct Staging {
    uint8_t* h = nullptr;
    uint8_t* d = nullptr;  // the slot's device-mapped address
    size_t cap = 0;
  };
  // A run slot.  Asynchronous runs (ps_run_async / ps_wait): the last window
  // of a run may leave its stats on the stream (pinned readback) so that the
  // host plans the next run while this one's kernels execute; two runs may
  // be in flight, in slots that alternate.  A slot owns what a window of its
  // run must not share with a window of the other: the pinned counters and
  // flag, the upload staging, the per-window tables on the device and the
  // gate event (§5.3 below).  Synchronous runs use slot 0's staging and
  // tables with the engine's own ev_run0 / ev_run1.
  struct RunSlot {
    Staging stg;
    psamd::DevBuf topics, woff, groups, partials, seeds;  // the per-window tables (upload_shadow keys: stable addresses)
    psamd::DevBuf fill_pop;  // per topic: set bits of its root row in this window (k_fill_popc)
    hipEvent_t ev_gate = nullptr;
    ps_stats st{};
    bool deferred = false;
    uint32_t r = 0, launches = 0;
    uint32_t mode = PS_MODE_COMPACT, flood_rounds = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;  // around the window's kernels
    uint64_t* hs = nullptr;      // pinned: (PS_MAX_ROUNDS + 1) x kNumCtr counters
    uint64_t* hs_dev = nullptr;  // hs, device-mapped (k_reduce_rounds writes it)
    uint64_t* ha = nullptr;      // pinned: apply counters of a multi-GPU window
    // signalled windows (no end event): sig[0] = the window's sequence number
    // once done, sig[1] / sig[2] = its start / end s_memrealtime stamps
    uint64_t* sig = nullptr;
    uint64_t* sig_dev = nullptr;
    uint64_t seq = 0;
    bool signalled = false;
    uint32_t planned0 = 0;
    uint32_t true_rounds = 0;   // level-aligned windows: rounds by start round (else planned0)
    psamd::AlignedSplit split;  // level-aligned windows: the per-round split
    int32_t world = 1;
    std::vector<uint8_t> kinds;  // round_kind of the window
    hipStream_t stream = nullptr;  // the stream the window's kernels ran on
  };
  RunSlot slot[2];
  uint32_t infl_head = 0, infl_count = 0;  // the runs in flight: slot[infl_head] the oldest
  bool defer_phase = false;  // the current phase may defer its last window's stats
  bool defer_last = false;   // ... and this window is that last window
  RunSlot* defer_into = nullptr;  // the slot of the asynchronous run being enqueued
  // the slot whose staging and tables the window being enqueued uses
  RunSlot& run_slot() { return defer_into ? *defer_into : slot[0]; }

  // Cross-window overlap.  A deep single-rank window (at
  // least overlap_min_rounds rounds, one start round) plans no k_flood; its
  // leading launches -- a few % of its bytes, rounds 1..P, latency bound --
  // form the prefix.  Its gate is the launch that starts at round P + 1 (the
  // last one reading a level <= P).  A pipelined window whose predecessor
  // (other slot) is in flight with the same plan runs its window init and
  // prefix on pstream once that predecessor's gate is done, beside the
  // predecessor's remaining launches: they touch only levels > P + 1, and the
  // per-window tables (topics, seeds, reduce descriptors, partial slots) are
  // per slot.  opts.overlap = 0 (PSAMD_OVERLAP=0): off.
  hipStream_t pstream = nullptr;
  hipStream_t rstream = nullptr;  // a pipelined window's counter reduce, beside the next window
  // the lazy prune's reach queries: they read the node space of the window
  // just enqueued (its build is complete), not its rows, so they run beside
  // the window's kernels instead of behind them
  hipStream_t qstream = nullptr;
  hipEvent_t ev_pre = nullptr, ev_end = nullptr;
  bool gate_valid = false;
  RunSlot* gate_slot = slot;       // the slot whose ev_gate the last gate was recorded on
  std::vector<uint64_t> gate_key;  // plan versions, node-space epochs and P of the gate's window
  uint64_t overlapped = 0;         // windows whose prefix ran beside their predecessor (stats)
  RunSlot* last_slot = slot;       // the slot of the last enqueued window's tables

  // Twin windows.  A pipelined one-rank level window whose
  // plan is already on the device runs ENTIRELY beside its predecessor: on
  // the other of two streams (stream / tstream), into the other of two row
  // sets (seen + arrivals + generation bytes, swapped so that `rows`
  // always names the last window's), with its own slot's tables and signal
  // counter.  Nothing the two share is written by either (node space, plan
  // tables, reach pieces are read-only; uploads make a window a non-twin).
  // Work on `stream` that changes shared state first waits for tstream's
  // last window (twin_join); a twin window on tstream first waits for work
  // `stream` did since tstream last followed it (e_seq).  env.twin = false
  // (PSAMD_TWIN=0): off.
  hipStream_t tstream = nullptr;
  hipEvent_t ev_tend = nullptr, ev_e2t = nullptr;
  bool t_pending = false;            // tstream ran a window `stream` has not waited for
  uint64_t e_seq = 1, t_seq = 0;     // shared-state work on `stream` / the last that tstream followed
  hipStream_t last_win_stream = nullptr;

  int fail(int code, const std::string& m) {
    err = m;
    return code;
  }
  int hip_fail(hipError_t e, const char* what) {
    err = std::string(what) + ": " + hipGetErrorString(e);
    return PS_E_DEVICE;
  }
};

#define HIP_TRY(expr, what)                              \
  do {                                                   \
    hipError_t _e = (expr);                              \
    if (_e != hipSuccess) return e->hip_fail(_e, what); \
  } while (0)

namespace psamd {

// graph.cpp
bool topic_ok(const ps_engine* e, uint32_t topic);
void peer_children(const ps_engine* e, const TopicHost& T, std::vector<uint32_t>& rp, std::vector<uint32_t>& cl);
void partition_topic(const std::vector<uint32_t>& order, const std::vector<uint32_t>& bfs_parent,
                     const std::vector<uint32_t>& level, int32_t world, uint32_t part, uint32_t split_depth,
                     std::vector<int32_t>& owner);
int build_graph(ps_engine* e);  // host node space (any rank count); no device calls
int build_dist_slots(ps_engine* e, ps_engine::DistSlots* S);  // ps_dist_report's slot tables (host only)
void build_flags(ps_engine* e);
int ensure_mirrors(ps_engine* e);
int upload_graph(ps_engine* e);
// run.cpp: the engine stream waits for tstream's last twin window (a no-op
// when none is pending); every change of shared device state goes after it
int twin_join(ps_engine* e);
// run.cpp: stream s, about to start a window into the current row set (rows.seen
// & co.), waits for every pending ps_drain_begin emit that reads that set (a
// no-op when none is pending, or for `stream`, which the drains run on)
int drain_fence(ps_engine* e, hipStream_t s);
// drain_tables.cpp: frees the drain's stream, events and pinned memory (ps_destroy)
void drain_destroy(ps_engine* e);
// drain_sink.cpp, the sink (ps_sink_set; all no-ops while none is set).  A run
// asks sink_precheck before it touches the pending messages (both results
// untaken, or an answer that may pass 2^30 ids), opens a result, calls
// sink_window behind every window it remembered and closes the result behind
// the last one; sink_abort gives the open result's slot up (a run that failed).
int sink_precheck(ps_engine* e);
int sink_open(ps_engine* e);
int sink_window(ps_engine* e);
int sink_close(ps_engine* e);
void sink_abort(ps_engine* e);
// The standing passes' window hooks (ps_*_track; each a no-op while nothing
// is tracked or no run is open), each in its family's file.  run.cpp calls them
// behind every window it remembered, behind sink_window and in this order.
int load_window(ps_engine* e);
int hops_window(ps_engine* e);
int downstream_window(ps_engine* e);
int cut_window(ps_engine* e);
int report_window(ps_engine* e);
int blame_window(ps_engine* e);
int spread_window(ps_engine* e);
// drain_standing.cpp: around a run, over Drain::standing(), where sink_open and
// sink_abort are called: the run's pinned staging of a tracker (a no-op while
// nothing is tracked); a failed run gives it up
int standing_open(ps_engine* e, ps_engine::Drain::Standing& S);
void standing_abort(ps_engine* e, ps_engine::Drain::Standing& S);

// The last window's messages of topic t, in window-slot order (slot li = the
// topic's rank last_lo + li): their run indices, a slice of run_sorted
inline WinSlice window_slice(const ps_engine* e, uint32_t t) {
  WinSlice w;
  w.idx = e->run_sorted.data() + e->run_topic_off[t] + e->last_lo[t];
  w.n = e->last_cnt[t];
  return w;
}
// ... and their row bits by window slot (last_pos), looked up once per topic:
// null where bit li is slot li itself
inline const uint32_t* window_bits(const ps_engine* e, uint32_t t) {
  return t < e->last_pos.size() && !e->last_pos[t].empty() ? e->last_pos[t].data() : nullptr;
}
inline uint32_t window_bit(const uint32_t* bits, uint32_t li) { return bits ? bits[li] : li; }
// topic -> peer -> node of the current node space (kNone: the root on the rank
// that owns it, a peer not subscribed or another rank's), built once per node
// space; d = the topic's entry of last_topics.  (Inline: the drains look it
// up once per query.)
inline const std::vector<uint32_t>& peer_node_map(ps_engine* e, uint32_t topic, const TopicDev& d) {
  auto& pm = e->peer_node[topic];
  if (e->peer_node_epoch.size() != e->topics.size()) e->peer_node_epoch.assign(e->topics.size(), ~0ull);
  if (e->peer_node_epoch[topic] != e->graph_epoch) {
    pm.assign(e->cfg.n_peers, kNone);
    const uint32_t u0 = (d.flags & kTopicRootLocal) ? 1 : 0;
    for (uint32_t k = u0; k < d.n_nodes; ++k) pm[e->node_peer[d.nbase + k]] = k;
    e->peer_node_epoch[topic] = e->graph_epoch;
  }
  return pm;
}

// plan.cpp (host only: no device calls)
int plan_window_layout(ps_engine* e, const std::vector<RunMsg>& msgs, const std::vector<WinSlice>& win,
                       WindowLayout& L);
bool plan_pull_chunks(ps_engine* e, const WindowLayout& L);  // true: the plan changed
bool plan_pair_chunks(ps_engine* e, const WindowLayout& L, uint32_t first);
bool plan_flood_tasks(ps_engine* e, const WindowLayout& L, uint32_t rounds);
int plan_ghost(ps_engine* e, const WindowLayout& L, bool* changed);
void annotate_chunks(ps_engine* e, const WindowLayout& L);
uint32_t plan_flood_rounds(const ps_engine* e, const WindowLayout& L);
// A deep single-start window: chains from round 1, no k_flood.
bool deep_window(const ps_engine* e, const WindowLayout& L);
// The window's schedule: seeds, start rounds, the level planners above in
// their order (or the compaction capacities), then plan_schedule_pairs.  The
// planner probe and run.cpp both plan a window through it.  Fills
// e->round_kind, desc_host and woff_host; writes every topic's round-0 seed
// range into L.tab.  No HIP call -- but on N ranks with in-place rows the
// ghost plan hands this rank's row-set address (rows.seen.p) to the others, so
// run.cpp allocates the window's row set before it plans the schedule.
int plan_window_schedule(ps_engine* e, const std::vector<RunMsg>& msgs, const std::vector<WinSlice>& win,
                         WindowLayout& L, WindowSchedule& S);
// Its pair part: the pair / chain plan and all that hangs on it (round kinds,
// reduce descriptors, slots, launch grids, row bytes, the prefix).  run.cpp
// calls it a second time when the uploaded chains overflow the level tables
// (pair.key cleared: the plan is rebuilt without chains).
void plan_schedule_pairs(ps_engine* e, const WindowLayout& L, WindowSchedule& S);
// Compaction mode: round r's k_expand grid, from the frontier bound of the
// start rounds present.
uint32_t round_grid(const ps_engine* e, const WindowLayout& L, const WindowSchedule& S, uint32_t r);

// run.cpp
int run_body(ps_engine* e, ps_stats* st, bool may_defer);
bool accumulate_window(ps_stats* st, const uint64_t* hs, const uint64_t* ha, uint32_t r, uint32_t planned0,
                       uint32_t mode, uint32_t flood_rounds, uint32_t launches, int32_t world,
                       const std::vector<uint8_t>& kinds, bool by_round = true);
// A level-aligned window's per-round deliveries and frontier entries from
// its reach rows (hs rows split.row0 ..): false when they disagree with the
// kernels' per-level counters (rows 1 .. r)
bool split_aligned_window(ps_stats* st, const uint64_t* hs, uint32_t r, uint32_t true_rounds,
                          const AlignedSplit& sp, std::string* why = nullptr);

}  // namespace psamd

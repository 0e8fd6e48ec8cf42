// kernels.hpp -- device data layout shared by the HIP kernels and the host
// runtime.  See DESIGN.md §4 (HBM layout) and §5 (kernels).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace psamd {

// node_flags bits (one byte per tree node)
enum : uint8_t {
  kNodeLive = 1,      // subscribed and live: receives and forwards
  kNodeInternal = 2,  // has at least one child: enters the next frontier
  kNodeSplit = 4,     // some child is owned by another rank (direct path)
};

// col[] entry of a child owned by another rank: rank and its local node id
constexpr uint32_t kRemoteBit = 0x80000000u;
constexpr uint32_t kRemoteRankShift = 27;
constexpr uint32_t kRemoteIdMask = (1u << kRemoteRankShift) - 1u;
constexpr int kMaxRanks = 16;

// One delivery addressed to a node of another rank: node id at the owner,
// word of its row, the arriving bits.  Regions: 16-B header (u32 count) +
// capacity items.
struct XItem {
  uint32_t node;
  uint32_t word;
  uint64_t mask;
};
constexpr uint32_t kRegionHeader = 16;

// TopicDev.flags
enum : uint32_t {
  // A node may have several parents (general child lists): the seen
  // test-and-set and the arrival OR are 64-bit atomics, rows are cleared
  // eagerly per window and consumed-and-cleared per round.
  kTopicMesh = 1,
  kTopicRootLocal = 2,  // this rank owns the topic root (node nbase)
  // Tree topic whose messages of this window all start in one round: every
  // node receives exactly once, so a node's arrival row equals its freshly
  // written seen row.  Arrival rows are then neither stored nor read: a
  // (non-root) parent's row is read from `seen`.
  kTopicSingleStart = 4,
  // Tree topic whose window messages start in several rounds, laid out for
  // level mode (one rank): start group g (GroupDev [group_lo, + group_n))
  // owns the words [w0, w0 + wn) of every row -- "virtual" word w of node u
  // -- stored group-major: block g of node u at wbase + n_nodes * w0 +
  // (u - nbase) * wn, so a round's rows are contiguous per group.
  kTopicGroups = 8,
  // A level-aligned window's topic with several start rounds (one rank): one
  // node-major row, message bits sorted by start round; GroupDev [group_lo,
  // + group_n) hold each start group's bits [b0, b0 + n) of the row and the
  // virtual words [w0, w0 + wn) the group-major layout would give it, so the
  // digest reads both layouts alike.  Kernels other than the digest see a
  // single-start topic.
  kTopicPacked = 16,
};
struct GroupDev {
  uint32_t w0, wn;
  uint32_t b0, n;  // kTopicPacked: the group's bits of the packed row
};
constexpr uint32_t kEntrySplit = 0x100;  // per-entry flag bit next to TopicDev.flags

// One topic of the fused node space.  Node u of topic t (nbase <= u <
// nbase + n_nodes) owns the 64-message words [wbase + (u-nbase)*W, +W) of the
// seen bitset and of the two arrival buffers.  Tree topics are numbered in
// BFS order, so the children of a node are consecutive node ids.
// Hop record (parity mode): the delivery round of every (node, message) as
// u16, so paths deeper than 254 hops stay exact up to the host's saturation.
constexpr uint16_t kHopRecNone = 0xFFFF;
__host__ __device__ inline uint16_t hop_round(uint32_t round) {
  return static_cast<uint16_t>(round < 0xFFFEu ? round : 0xFFFEu);
}

struct TopicDev {
  uint64_t wbase;    // first word of the topic's mask block
  uint32_t w_msgs;   // message words in use (W may carry one pad word)
  uint32_t group_lo;  // kTopicGroups: the topic's start groups in the GroupDev table
  uint32_t nbase;    // first node of the topic (its root)
  uint32_t n_nodes;  // nodes in the topic
  uint32_t W;        // 64-message words per node in this window (0 = idle)
  uint32_t flags;    // kTopic*
  uint32_t seed_lo, seed_n;  // the topic's round-0 seeds (k_window_init applies them when asked)
  uint32_t group_n;     // kTopicGroups: number of start groups
  uint32_t root_words;  // words at wbase k_window_init zeroes for the root (W; group-major: block 0)
};

// One root injection: words of a topic root that start flooding in a round.
struct SeedDev {
  uint64_t woff;    // word offset (root row + word)
  uint64_t mask;    // messages entering at this round
  uint32_t node;    // root node index
  uint32_t assign;  // 1: the word is set to mask (group-major root blocks, not zeroed by
                    // k_window_init), 0: or-ed in
};

// Per-wave counters written by the expand kernel, reduced per round; they
// also feed the algorithmic byte model.
enum : int {
  kCtrDeliveries = 0,
  kCtrDuplicates,
  kCtrEntries,
  kCtrEntryWords,
  kCtrChildren,
  kCtrMeshChildren,
  kCtrSeenReads,
  kCtrSeenWrites,
  kCtrArrivalWrites,
  kCtrClearWords,
  kNumCtr
};

struct ExpandArgs {
  const uint32_t* frontier;
  const uint32_t* n_front;
  const uint32_t* row_ptr;
  const uint32_t* col;
  const uint16_t* node_topic;
  const uint8_t* node_flags;
  const TopicDev* topics;
  uint64_t* a_cur;   // arrivals of the current frontier
  uint64_t* a_next;  // arrivals for the next frontier
  uint64_t* seen;    // per-node delivered bitset (the dedup record)
  // arrival extents (one rank; nullptr: whole rows): per node the word range
  // [lo, hi) of its arrival row written this round (lo | hi << 16), kept for
  // multi-start tree topics of 64..kStageWords words; the row outside it is
  // stale and never read
  uint32_t* ext_cur;
  uint32_t* ext_next;
  uint8_t* gen;      // per-node window generation of its seen row (tree topics)
  uint8_t* next_flag;
  uint8_t* blk_flag;  // one byte per kFlagsPerBlock nodes: some flag set
  uint64_t* partials;  // [n_waves][kNumCtr]
  uint16_t* hop_rec;   // [word*64 + bit] = round (kHopRecNone: none), record mode only
  uint32_t gen_cur;
  uint8_t* send;                  // send regions of this round (multi-GPU compaction mode)
  uint64_t send_off[kMaxRanks];   // byte offset of the region for each rank
  uint32_t opts;                  // kExpand* switches (A/B)
};
constexpr uint32_t kExpandNoNarrow = 1;  // narrow entries one at a time (the entry loop), not flattened

// Level mode, pull direction: one wave copies the parents' rows into the
// rows of a contiguous run of next-level nodes [node_begin, node_end) of one
// topic (at most kPullMaxKids nodes, about kPullWords words).
struct PullChunk {
  uint32_t node_begin, node_end;  // nodes written in round r (level d)
  uint32_t topic;
  uint32_t p_lo, p_hi;  // parents of [node_begin, node_end) (consecutive ids), kNone: unknown
  uint32_t W;           // row words (a start group's block width for kTopicGroups)
  uint32_t row0_lo, row0_hi;  // word offset of the row of the topic's first node (nbase)
  // multi-GPU: PullArgs::ship entries [e_lo, e_hi) -- ghost records of the
  // next round for nodes of this chunk, written by the wave that writes them
  uint32_t e_lo, e_hi;
  // k_pull_pair: the children of [node_begin, node_end) (consecutive ids,
  // filled in on the device), written in round q + 1 by the same wave; c_lo =
  // kNoneNode: a run written in round q + 1 itself (level 1 under a root)
  uint32_t c_lo, c_hi;
  // multi-GPU: GhostSeg of this round (a ghost-fed node reads its parent's
  // record there) and of the next round (the records [e_lo, e_hi) ship
  // into); kNoneNode: none
  uint32_t gin, gout;
  uint32_t group;  // host: the start group (index in the topic's groups) whose block the chunk writes
  uint32_t lvl0;   // first node of the chunk's level: the once-per-parent count looks back no further
                   // (ghost record indices start again at every level)
};
constexpr uint32_t kPullMaxKids = 512;
constexpr uint32_t kNoneNode = 0xFFFFFFFFu;
constexpr uint32_t kPullWords = 1024;

// Multi-GPU level mode.  Before round q each rank ships the
// rows of its parents of the level written in round q - 1 that have children
// on other ranks -- once per destination rank -- as records of W words (the
// start group's block): record k of the (round, topic, group)'s a -> b block
// is a's k-th such parent in a's node order.  No header: a reached parent's
// block holds every message of its start group (a tree, one start round per
// block), so its first word is non-zero; an unreached parent's record starts
// with a zero word and its children stay unreached.
struct ShipEntry {
  uint32_t node;  // the parent (local node id)
  uint32_t dst;   // destination rank << 27 | record index k
};
struct GhostSeg {              // one (round, topic, start group)
  uint64_t rbase[kMaxRanks];   // recv buffer: first word of the records from rank a
                               // (kSegInPlace: the block's first row in rank a's seen rows)
  uint64_t sbase[kMaxRanks];   // send buffer: first word of the records to rank b (the round's half)
  uint32_t rw;                 // record words (the block width)
  uint32_t topic;
  uint32_t flags;              // kSegInPlace
  uint32_t gbase[kMaxRanks];   // kSegInPlace: the topic's first node at rank a (its generation bytes)
};
// PS_DIST_F_INPLACE: a ghost-fed node of this segment reads its parent's row
// where the owner wrote it (RankRows of the owner, the parent's topic-relative
// id there in ghost_ref), reached iff the owner stamped its generation byte
// this window -- no record is written or shipped
constexpr uint32_t kSegInPlace = 1u;
struct RankRows {
  const uint64_t* seen;
  const uint8_t* gen;
};
// k_pack: a topic root's records (round s_g + 1 of each start group g), from
// its seeded row; one segment per (round, topic, group).
struct PackSeg {
  uint32_t e0, e1;  // the root's ship entries
  uint32_t gseg;    // GhostSeg of the round
  uint32_t W;
  uint64_t row;     // word offset of the root's row (block)
  uint64_t unit0;   // the segment's first unit in the launch's flattened stream (pack_units)
};
__host__ __device__ inline uint32_t pack_units(uint32_t W) { return (W & 1u) ? W : W >> 1; }
struct PullArgs {
  const uint32_t* node_parent;  // node-space parent (kNone for roots and remote parents)
  // k_pull_chain: every chain chunk's node entries (16 bits: parent index
  // relative to the level above, live bit), levels in order, from
  // ChainChunk::first[kChainLevels] (k_chain_meta, once per plan)
  const uint32_t* chain_meta;
  const uint8_t* node_flags;
  const TopicDev* topics;
  const uint64_t* a_cur;  // arrivals of round-1 (topic roots' seeded rows)
  uint64_t* seen;
  uint8_t* gen;
  uint16_t* hop_rec;
  uint64_t* partials;  // [n_blocks][kNumCtr]
  // multi-GPU: a node whose parent lives on another rank (ghost_ref[node] =
  // rank << 27 | k, kNoneNode otherwise) reads record k of that rank in this
  // round's receive buffer (GhostSeg gin)
  const uint32_t* ghost_ref;  // null: one rank
  const GhostSeg* gsegs;
  const uint64_t* recv;
  // multi-GPU: the next round's records of the nodes written now
  // (PullChunk e_lo/e_hi, GhostSeg gout), stored into the send buffer
  const ShipEntry* ship;
  uint64_t* send;
  // per source rank a: the base its records are addressed from (record k of
  // (round, topic, group) block at rsrc[a] + GhostSeg::rbase[a] + k * rw):
  // the receive buffer for every rank, or -- the zero-copy loopback -- rank
  // a's own send region, offset so that the same rbase applies
  const uint64_t* rsrc[kMaxRanks];
  const RankRows* rrows;  // PS_DIST_F_INPLACE: every rank's row set (kSegInPlace segments)
  uint32_t gen_cur;
  uint32_t slot_mod;   // block b adds its counters into partial slot b % slot_mod (zeroed per window)
  // k_pull_pair: round q + 1's partial slots; all_current: every generation
  // byte was stamped up front (PS_F_NO_LAZY_SEEN), so every parent counts as
  // reached, as the generation test of a separate launch would find
  uint64_t* partials2;
  uint32_t all_current;
  // k_pull_chain: the CSR offsets (a run's children are consecutive ids) and
  // the partial slots of each round of the launch
  const uint32_t* row_ptr;
  uint64_t* partials_r[6];  // (kChainLevels)
  // debug (PSAMD_CHAIN_PROFILE): per chunk kChainProf words -- s_memrealtime
  // at the chunk's start and end, row words written, HW_ID and XCC_ID; null: off
  uint64_t* prof;
};
constexpr uint32_t kChainProf = 4;
// k_pull_pair: per wave, a run of at most kPairPar nodes
// whose rows (at most kPairWords words in all) stay in LDS for its children,
// streamed kPairKids children at a time
constexpr uint32_t kPairWords = 768;  // (1024: 17 resident waves/CU, cfg3 +3 % slower; 512: 1 parent of 330 words)
constexpr uint32_t kPairPar = 128;
constexpr uint32_t kPairKids = 256;
// k_pull_chain: up to kChainLevels rounds in one launch.  A
// wave owns a run of level-d nodes and a column slice [w0, w0 + S) of their
// rows (S = W: whole rows, the usual case; slices only for rows wider than
// the stage).  It writes the run (round q, the parents' rows from HBM) and
// keeps those rows in its LDS stage; then, level by level, every descendant
// of the run (round q + k: the level-(d + k) nodes of the subtree, one
// contiguous id range per level).  In a single-start window a reached node's
// row is its parent's row as round q + k - 1 wrote it, and that row is a
// stage row: a node's entry in the level table is the stage slot of the row
// its parent holds (kChainNone: unreached), so no level below the run reads
// a row from HBM.  Level ranges are at most kChainCap nodes (the host sizes
// the runs; k_chain_ranges fills and checks the ranges on the device).
constexpr uint32_t kChainLevels = 6;
static_assert(sizeof(PullArgs::partials_r) / sizeof(uint64_t*) == kChainLevels, "a slot row per chain level");
constexpr uint32_t kChainKids = 256;   // nodes resolved per sub-run of a level
constexpr uint32_t kChainPar = 128;    // nodes of a run at most (stage slots < kChainZero)
constexpr uint32_t kChainWords = 768;  // LDS stage words per wave: the run's rows (slices)
constexpr uint32_t kChainCap = 1024;   // nodes of one level of a chunk at most (the LDS level tables)
constexpr uint8_t kChainNone = 0xFF;   // level table: unreached
constexpr uint8_t kChainZero = 0xFE;   // level table: reached with a zero row (PS_F_NO_LAZY_SEEN only)
struct ChainChunk {
  uint32_t node_begin, node_end;  // the run (level d)
  uint32_t topic;
  uint32_t p_lo, p_hi;            // parents of the run (consecutive ids), kNone: unknown
  uint32_t W;                     // row stride, words
  uint32_t row0_lo, row0_hi;      // row of the topic's first node (its start group's block)
  uint32_t w0, S;                 // the column slice of every row (rows reach 2^24 words)
  uint8_t levels;                 // levels written: d .. d + levels - 1 (rounds r0 + k of the launch)
  uint8_t r0;                     // the run's round within the launch (a start group entering late: > 0)
  uint16_t group;                 // host: the start group
  // first node of levels d .. d + levels: a run [x0, x1) of level d + k has
  // the children [row_ptr[x0] - row_ptr[first[k]] + first[k + 1], ...x1...)
  uint32_t first[kChainLevels + 1];
  // level k >= 1 of the chunk: the descendants [lo[k], hi[k]) (k_chain_ranges)
  uint32_t lo[kChainLevels], hi[kChainLevels];
  // the topic's first node, and its root node if this rank owns it (the
  // root's row is the seeded arrival row), else kNoneNode: node-space
  // properties, so the kernel needs no topic-table read before its loads
  uint32_t nbase, root;
};
static_assert(sizeof(ChainChunk) == 128, "two chunk descriptors per 256-B line");
// ChainChunk::lo / hi from the device CSR; *overflow is set non-zero when a
// level range exceeds cap (the plan is then not used)
hipError_t launch_chain_ranges(ChainChunk* chunks, uint32_t n, const uint32_t* row_ptr, uint32_t cap,
                               uint32_t* overflow, hipStream_t s);
// The chunks' node entries (PullArgs::chain_meta) after their ranges: per
// chunk its node count (counts[i]), an exclusive scan into
// ChainChunk::first[kChainLevels] (the device copy's; first[] past the
// chain's levels is unused there), the entries from node_parent and the live
// flags.  *entries: the buffer's size in entries, read back by the caller
// with the ranges' overflow word (`tail`: counts[n] after the scan).
hipError_t launch_chain_meta(ChainChunk* chunks, uint32_t n, const uint32_t* node_parent, const uint8_t* node_flags,
                             uint32_t* counts, void* scan_temp, size_t scan_bytes, uint32_t* meta, bool fill,
                             hipStream_t s);
size_t chain_meta_scan_bytes(uint32_t n);
// slices: chunks of rows wider than the stage (column slices; their own launch)
// inner_nt: level 0 and the inner levels store non-temporally (false: plain, A/B)
// waves_per_cu: resident chain waves per CU at most (an LDS pad; 0: no cap)
hipError_t launch_pull_chain(const PullArgs& a, const ChainChunk* chunks, uint32_t n_chunks, uint32_t round,
                             bool record, bool nt, bool slices, bool inner_nt, uint32_t waves_per_cu,
                             hipStream_t s);
// ChainChunk::p_lo / p_hi from the device node_parent (GPU-built graphs)
hipError_t launch_chain_parents(ChainChunk* chunks, uint32_t n, const uint32_t* node_parent, hipStream_t s);
// A chain launch as reach + fill (fill.hip): in a
// single-start window every reached node's row is its topic root's seeded
// row, an unreached one's is zeros, and levels d .. d + levels - 1 of a topic
// are one contiguous id range (BFS numbering), so their rows are one
// contiguous word range of `seen`.  k_fill_reach decides reach for every node
// of the launch's levels, stamps generations and adds the chain launch's
// counters; k_fill_rows then writes each topic's range front to back in
// line-aligned pieces, one wave each, from the root row in LDS.
struct FillSeg {  // one topic's whole rows of one chain launch
  uint64_t row0;  // word offset of the row of the topic's first node (the root: its seeded row in a_cur)
  uint32_t topic, W;
  uint32_t nbase, levels;
  uint32_t first[kChainLevels + 1];  // first node of levels d .. d + levels (node ids)
  uint32_t piece0;                   // the segment's first piece in its launch
  uint32_t blk0;                     // ... and its first k_fill_reach block (kFillReachBlock nodes each)
  uint32_t pw;                       // words per piece: a multiple of kFillLine, at most kFillPieceNodes rows
};
static_assert(sizeof(FillSeg) == 64, "four segments per 256-B line");
struct FillPiece {      // one wave's contiguous words [w0, w0 + nw) of `seen`
  uint64_t w0, row0;    // row0: the topic root's row
  uint32_t nw, W;
  uint32_t node0, off0;  // the node holding word w0, and w0's word within its row
};
static_assert(sizeof(FillPiece) == 32, "one scalar load per wave");
constexpr uint32_t kFillLine = 16;            // words of a 128-B line: pieces start and end on lines
constexpr uint32_t kFillPieceWords = 2048;    // 16 KB per wave (tools/probe/chain_write_probe.hip)
constexpr uint32_t kFillPieceNodes = 2048;    // nodes with a word in one piece at most (+ 2: k_fill_rows' LDS bytes)
constexpr uint32_t kFillWaves = 16;           // resident fill waves per CU at most (profiles/chain_fill/sweep.txt)
constexpr uint32_t kFillReachBlock = 256;
// A launch is filled only if its rows average at least this many words.  The reach pass costs per
// node (cfg3's bulk launch: 24 us for 1.5 M nodes, 16 ns each), the fill gains per byte written
// (6.0 against 4.9 TB/s: 0.3 ps per row word), which breaks even at 53 words; 128 leaves a margin
// (cfg4's 16-word rows lose: 0.56 against 0.39 ms/step, profiles/chain_fill/ab.json).
constexpr uint32_t kFillMinRowWords = 128;
__host__ __device__ inline uint64_t fill_seg_begin(const FillSeg& s) {
  return s.row0 + static_cast<uint64_t>(s.first[0] - s.nbase) * s.W;
}
__host__ __device__ inline uint64_t fill_seg_end(const FillSeg& s) {
  return s.row0 + static_cast<uint64_t>(s.first[s.levels] - s.nbase) * s.W;
}
// words per piece of rows of W words, for pieces of about `words`
__host__ __device__ inline uint32_t fill_piece_words(uint32_t W, uint32_t words) {
  const uint64_t cap = (static_cast<uint64_t>(kFillPieceNodes) * W) & ~static_cast<uint64_t>(kFillLine - 1);
  const uint32_t w = (words < kFillLine ? kFillLine : words) & ~(kFillLine - 1);
  return cap < w ? static_cast<uint32_t>(cap < kFillLine ? kFillLine : cap) : w;
}
__host__ __device__ inline uint32_t fill_seg_pieces(const FillSeg& s) {
  const uint64_t wb = fill_seg_begin(s), we = fill_seg_end(s);
  if (we <= wb) return 0;
  const uint64_t a = wb & ~static_cast<uint64_t>(kFillLine - 1);
  return static_cast<uint32_t>((we - a + s.pw - 1) / s.pw);
}
// Piece j of a segment: cut at multiples of the piece size from the line
// holding the segment's first word, so only a segment's first and last
// pieces have an edge off a line.
__host__ __device__ inline FillPiece fill_piece(const FillSeg& s, uint32_t j) {
  const uint64_t wb = fill_seg_begin(s), we = fill_seg_end(s);
  const uint64_t a = wb & ~static_cast<uint64_t>(kFillLine - 1);
  const uint64_t b = a + static_cast<uint64_t>(j) * s.pw, e = b + s.pw;
  FillPiece p;
  p.w0 = b < wb ? wb : b;
  p.row0 = s.row0;
  p.nw = static_cast<uint32_t>((e > we ? we : e) - p.w0);
  p.W = s.W;
  const uint64_t rel = p.w0 - s.row0;
  p.node0 = s.nbase + static_cast<uint32_t>(rel / s.W);
  p.off0 = static_cast<uint32_t>(rel % s.W);
  return p;
}
struct FillReachArgs {
  const FillSeg* segs;
  uint32_t n_segs;
  const uint32_t* node_parent;
  const uint8_t* node_flags;
  uint8_t* gen;
  uint32_t gen_cur;
  const uint32_t* pop;  // per topic: the popcount of its root row (k_fill_popc, once per window)
  uint64_t* partials_r[kChainLevels];
  uint32_t slot_mod;
};
// pieces[] of the launch's segments from segs[] (once per plan, on the device)
hipError_t launch_fill_pieces(const FillSeg* segs, uint32_t n_segs, FillPiece* pieces, uint32_t n_pieces,
                              hipStream_t s);
// pop[topic] of every segment's topic, from its root row in a_cur
hipError_t launch_fill_popc(const FillSeg* segs, uint32_t n_segs, const uint64_t* a_cur, uint32_t* pop, hipStream_t s);
hipError_t launch_fill_reach(const FillReachArgs& a, uint32_t n_blocks, hipStream_t s);
hipError_t launch_fill_rows(const FillPiece* pieces, uint32_t n_pieces, const uint64_t* a_cur, uint64_t* seen,
                            const uint8_t* gen, uint32_t gen_cur, uint32_t waves_per_cu, hipStream_t s);

constexpr uint32_t kPullSlots = 256;  // partial slots per round of a pull launch
// k_pull_pair: every wave adds its counters with atomics (no block
// reduction) into slot wave % kPairSlots.  (4096 slots: no faster than 256,
// and k_reduce_rounds folds each round's slots in one block -- 26 us per
// step -- and k_window_init zeroes them.)
constexpr uint32_t kPairSlots = kPullSlots;

// k_flood (flood.hip): every round of a single-start tree
// window in one persistent launch.  A task = the nodes [nb, ne) of one BFS
// level of one topic (at most kFloodMaxNodes = one per lane, about
// kFloodWords row words), written in round `round`; tasks are listed level by
// level.  A task publishes which of its nodes were reached as granules: one
// 8-B word {epoch << 32 | reach bits} per `gsz` consecutive nodes of its level
// (data and flag in one store); its children's tasks poll those granules.
struct FloodTask {
  uint32_t nb, ne;          // nodes written (consecutive ids of one level)
  uint32_t topic, round;
  uint32_t slot0, nslot;    // the round's partial counter slots
  uint32_t g_own, gsz;      // granules written: g_own, g_own + 1, ... (gsz nodes each)
  uint32_t p_lo, p_hi;      // parents of the run (consecutive ids)              [k_flood_deps]
  uint32_t pg_lo, pg_hi;    // parent granules to poll; kNoneNode: parent = root [k_flood_deps]
  uint32_t pnode0, pgsz;    // parent level: first node and nodes per granule    [k_flood_deps]
  uint32_t pseg;            // host: the parent level's segment (kNoneNode: root)
  uint32_t seg;             // the task's own segment (row stride and base)
};
// One level of one topic (of one start group): tasks task0 .. task0 +
// n_tasks - 1 of `per` nodes each from node0, granules gbase .. of gsz nodes
// each; rows of W words, node u's at row0 + (u - nbase) * W.
struct FloodSeg {
  uint32_t task0, node0, per, n_tasks;
  uint32_t gbase, gsz, nodes, W;
  uint64_t row0;  // word offset of the topic's first node's row (its start group's block region)
};
struct FloodArgs {
  const FloodTask* tasks;
  const FloodSeg* segs;
  const uint32_t* node_parent;
  const uint8_t* node_flags;
  const TopicDev* topics;
  uint64_t* seen;
  uint8_t* gen;
  uint16_t* hop_rec;
  uint64_t* granules;   // per granule: epoch << 32 | reach bits, once its task's rows are stored
  uint64_t* partials;   // counter slots (FloodTask::slot0 ...), zeroed per window
  uint32_t* err;        // set when a dependency wait times out
  uint32_t n_tasks;
  uint32_t epoch;       // this launch's granule tag (never 0)
  uint32_t gen_cur;
  uint32_t spin_ticks;  // wait bound, s_memrealtime ticks (100 MHz)
  uint64_t* prof;       // debug (PSAMD_FLOOD_PROFILE): per wave kFloodProf s_memrealtime stamps / sums
  uint32_t prof_split;  // debug: pf[7] sums the waits of tasks of later rounds
};
// per-wave profile words: first task start, last task end, then summed ticks
// waiting, resolving, streaming, publishing; tasks run; waiting in rounds > prof_split
constexpr uint32_t kFloodProf = 8;
constexpr uint32_t kFloodMaxNodes = 64;       // one node per lane
constexpr uint32_t kFloodGranule = 32;        // reach bits per granule at most
constexpr uint32_t kFloodWords = 2048;        // row words per task (16 KB)
constexpr uint32_t kFloodBlocksPerCu = 4;     // resident 256-thread blocks per CU the grid uses

struct ApplyArgs {
  const uint8_t* recv;
  uint64_t recv_off[kMaxRanks];  // region from each rank
  uint64_t cap_pre[kMaxRanks + 1];  // prefix of region capacities (items)
  uint32_t world;
  const uint16_t* node_topic;
  const uint8_t* node_flags;
  const TopicDev* topics;
  uint64_t* seen;
  uint64_t* a_next;
  uint8_t* next_flag;
  uint8_t* blk_flag;
  uint16_t* hop_rec;
  uint64_t* stats;  // [kNumCtr] of this round (deliveries, duplicates)
  uint8_t* gen;     // level mode: stamp a node reached (null: compaction mode)
  uint32_t gen_cur;
};

constexpr int kBlock = 256;
constexpr int kFlagsPerThread = 16;
constexpr int kFlagsPerBlock = kBlock * kFlagsPerThread;  // 4096 nodes
constexpr int kFlagBlockShift = 12;

// host-side launchers (kernels.hip)
// Per-window parameters (topic table, seeds, reduce descriptors) copied by
// one small kernel straight from the pinned staging slot (device-mapped host
// memory): one launch instead of a blit per array and its barrier packets.
constexpr uint32_t kStageMax = 4;
struct StageCopy {
  const uint32_t* src[kStageMax];
  uint32_t* dst[kStageMax];
  uint32_t words[kStageMax];
  uint32_t n;
};
hipError_t launch_stage_copy(const StageCopy& c, hipStream_t s);

// Loopback exchange (one GPU): up to kMaxCopyRegions device regions of
// whole 16-B units copied by one launch.
constexpr uint32_t kMaxCopyRegions = 16;
struct CopyRegions {
  const uint4* src[kMaxCopyRegions];
  uint4* dst[kMaxCopyRegions];
  uint64_t units[kMaxCopyRegions];
  uint32_t n;
};
hipError_t launch_copy_regions(const CopyRegions& c, hipStream_t s);
// Process-shared exchange (dist.cpp IpcTransport): stream-ordered device
// flags in IPC-mapped memory.  launch_flag_set stores `value` into `flag`
// (system-scope release, after every launch before it on the stream);
// launch_flag_wait holds the stream until every non-null flag[q] >= value[q]
// (system-scope acquire polls) or `timeout_ticks` of the 100 MHz clock pass,
// then ORs 1 into *err (pinned host memory) and lets the stream go on.
struct FlagWait {
  const uint64_t* flag[kMaxRanks];
  uint64_t value[kMaxRanks];
};
hipError_t launch_flag_set(uint64_t* flag, uint64_t value, hipStream_t s);
hipError_t launch_flag_wait(const FlagWait& w, uint32_t* err, uint64_t timeout_ticks, hipStream_t s);
// Window start: zero and stamp the roots' rows (every row of a mesh topic);
// optionally in the same launch (WindowStart): the staged per-window copies
// (topics_src / seeds_src then point at the staged sources), the round-0
// seeds of tree roots (each topic's block, after its zeroing), and zeroing
// of the pull partial slots.
struct WindowStart {
  StageCopy copy{};
  const SeedDev* seeds = nullptr;  // apply round-0 seeds (tree topics only)
  uint64_t* zero = nullptr;        // words to clear
  uint64_t zero_words = 0;
  uint64_t* t0 = nullptr;          // (signalled windows) the start stamp, s_memrealtime into pinned memory
};
// A signalled window's end, after its reduce on the same stream: the end
// stamp into sig[2], then seq into sig[0] (pinned; system-scope release) --
// ps_wait polls it instead of waiting on an event, whose record costs the
// queue ~10 us between windows (profiles/r04/cfg2)
hipError_t launch_window_done(uint64_t* sig, uint64_t seq, hipStream_t s);
// ... or raised by the reduce's last block (no launch of its own): ctr a
// zeroed device word (left zero again)
struct WindowSignal {
  uint64_t* flag = nullptr;
  uint32_t* ctr = nullptr;
  uint64_t seq = 0;
};
hipError_t launch_window_init(const TopicDev* topics, uint32_t n_topics, uint64_t* seen,
                              uint64_t* a0, uint64_t* a1, uint8_t* gen, uint32_t gen_cur,
                              bool any_mesh, const WindowStart& ws, hipStream_t s);
// A signalled window's reduce held back until the next window starts: the
// two run as one launch (the reduce's blocks first, then the init's), one
// kernel boundary less per pipelined window.  The two touch
// disjoint memory: the reduce reads its own slot's partials and descriptors,
// the init writes the other slot's.
// A level-aligned window's per-(topic, level) reach counts:
// the nodes [lo, hi) of segment seg (one BFS level of one topic; a level is
// cut into pieces of at most kReachPiece nodes).  out[2 * seg] += reached
// nodes, out[2 * seg + 1] += frontier nodes (reached and internal).  Reached:
// the generation byte is this window's (eager seen: the row's first word is
// non-zero -- its first message's bit); a topic root always.
struct ReachPiece {
  uint32_t seg, lo, hi, topic;
};
constexpr uint32_t kReachPiece = 16384;
hipError_t launch_level_reach(const ReachPiece* pieces, uint32_t n, const uint8_t* gen, uint32_t gen_cur,
                              const uint8_t* node_flags, const TopicDev* topics, const uint64_t* seen, bool eager,
                              uint64_t* out, hipStream_t s);

struct ReduceArgs {
  const uint64_t* partials = nullptr;
  const uint32_t* desc = nullptr;
  uint32_t n_rounds = 0;  // > 0
  uint64_t* round_stats = nullptr;
  uint64_t* host_stats = nullptr;
  WindowSignal sig{};
};
hipError_t launch_window_turn(const ReduceArgs& rd, const TopicDev* topics, uint32_t n_topics, uint64_t* seen,
                              uint64_t* a0, uint64_t* a1, uint8_t* gen, uint32_t gen_cur, bool any_mesh,
                              const WindowStart& ws, hipStream_t s);
// stamp: mark the nodes' generation current (compaction mode)
hipError_t launch_init_nodes(const uint32_t* nodes, uint32_t n, const uint16_t* node_topic,
                             const TopicDev* topics, uint64_t* seen, uint64_t* a0, uint64_t* a1,
                             uint8_t* gen, uint32_t gen_cur, bool stamp, hipStream_t s);
hipError_t launch_apply(const ApplyArgs& a, uint32_t round, bool record, hipStream_t s);
// next_flag / blk_flag may be null (level mode: the root is in the schedule)
hipError_t launch_seed(const SeedDev* seeds, uint32_t lo, uint32_t hi, uint64_t* arrivals,
                       uint64_t* seen, uint8_t* next_flag, uint8_t* blk_flag, hipStream_t s);
hipError_t launch_expand(const ExpandArgs& a, uint32_t round, bool record, uint32_t grid, hipStream_t s);
// Level mode, pull direction: one wave per chunk, grid = ceil(n_chunks / 4)
// blocks; nt: the row stores are non-temporal (rounds nobody re-reads soon);
// cap: an nt round runs at most 5 blocks per CU (one rank; N ranks keep full
// residency)
hipError_t launch_pull(const PullArgs& a, const PullChunk* chunks, uint32_t n_chunks,
                       uint32_t grid, uint32_t round, bool record, bool nt, bool cap, hipStream_t s);

// Level mode, rounds q and q + 1 in one launch (one rank): a wave writes its
// run's rows (round q, always non-temporal: the run's children are written
// from LDS, nothing re-reads them), then the children's rows (round q + 1;
// nt2: non-temporal too)
// One-wave workgroups, one chunk each (grid = n_chunks); a chunk's rows fit
// the kPairWords LDS stage
hipError_t launch_pull_pair(const PullArgs& a, const PullChunk* chunks, uint32_t n_chunks, uint32_t grid,
                            uint32_t round, bool record, bool nt2, hipStream_t s);
// Fills PullChunk::c_lo / c_hi of pair chunks from the device CSR (children
// of a BFS-numbered run are consecutive ids)
hipError_t launch_pair_kids(PullChunk* chunks, uint32_t n, const uint32_t* row_ptr, const uint32_t* col,
                            hipStream_t s);

// multi-GPU level mode: the roots' records of the round into the send buffer
hipError_t launch_pack(const ShipEntry* ship, const PackSeg* segs, uint32_t n_segs, uint64_t total_units,
                       const GhostSeg* gsegs, const uint64_t* seen, uint64_t* send, hipStream_t s);
// Fills PullChunk::p_lo / p_hi from the device node_parent (GPU-built graphs).
hipError_t launch_chunk_parents(PullChunk* chunks, uint32_t n, const uint32_t* node_parent, hipStream_t s);
// k_flood (flood.hip): grid = resident blocks (<= flood_blocks_per_cu x CUs)
hipError_t launch_flood(const FloodArgs& a, uint32_t grid, bool record, hipStream_t s);
// FloodTask::p_lo / p_hi / pg_lo / pg_hi / pnode0 / pgsz from node_parent and the segments
hipError_t launch_flood_deps(FloodTask* tasks, uint32_t n, const FloodSeg* segs, const uint32_t* node_parent,
                             hipStream_t s);
hipError_t flood_blocks_per_cu(int* out);
// Level mode: round q's counters = sum of the partial slots desc[3q],
// desc[3q] + desc[3q+2], ... < desc[3q+1], for q = 1..n_rounds.
// host_stats (nullable): device-mapped pinned rows that receive the same
// counters, so an asynchronous run needs no readback copy
hipError_t launch_reduce_rounds(const uint64_t* partials, const uint32_t* desc, uint32_t n_rounds,
                                uint64_t* round_stats, uint64_t* host_stats, const WindowSignal& sig, hipStream_t s);
// second instance: entries the staged kernel leaves (mesh, split, wide rows,
// fan-out > 64); writes the same counters to partials + n_waves*kNumCtr
hipError_t launch_expand_direct(const ExpandArgs& a, uint32_t round, bool record, uint32_t grid,
                                hipStream_t s);
constexpr uint32_t kStageMaxWords = 704;  // widest row of the staged path
hipError_t launch_flag_count(const uint8_t* flags, const uint8_t* blk_flag, uint32_t n_pad,
                             uint32_t* wg_count, const uint64_t* partials, uint32_t n_waves,
                             uint64_t* round_stats, hipStream_t s);
hipError_t launch_flag_compact(uint8_t* flags, uint8_t* blk_flag, uint32_t n_pad,
                               const uint32_t* wg_count, uint32_t* frontier, uint32_t* n_front,
                               hipStream_t s);
hipError_t launch_digest(const uint64_t* seen, const uint8_t* gen, uint32_t gen_cur,
                         const uint32_t* node_peer, const uint16_t* node_topic,
                         const TopicDev* topics, const GroupDev* groups, uint32_t n_nodes, uint64_t* out,
                         hipStream_t s);

// ---- batched drain (drain.hip) -------------------------------
// A query's row is cut into segments of kDrainSegBits positions: lane l of
// the segment's wave owns the 64 positions of "lane word" 64 k + l.  For a
// topic whose row bits ascend in arrival order a position is a virtual row
// bit and the lane word is the row word under the topic's message mask; for
// the others (kDrainGather: a mesh window with several start rounds) a
// position is an arrival rank and the lane word is gathered bit by bit
// through the topic's order table.  ids[tab0 + position] is the message id.
constexpr uint32_t kDrainSegWords = 64;
constexpr uint32_t kDrainSegBits = 64 * kDrainSegWords;
constexpr uint32_t kDrainGather = 0x10000;  // DrainTopic.flags, next to kTopic*
struct DrainTopic {
  uint64_t wbase;   // first word of the topic's rows
  uint64_t tab0;    // first entry of the topic's id table
  uint64_t aux0;    // first mask word; kDrainGather: first entry of the order table
  uint32_t nbase, n_nodes, W, flags;
  uint32_t group_lo, group_n;  // kTopicGroups: the start groups (DrainGroup)
  uint32_t n_pos;   // positions in use (a multiple of 64 unless kDrainGather)
  uint32_t pad;
};
struct DrainGroup {
  uint32_t w0, wn;
};
struct DrainQuery {
  uint32_t topic;
  uint32_t node;  // topic-relative; kDrainMaskRow: the topic's message mask itself (ps_drain_shared)
  uint32_t seg0;  // the query's first segment (a query with an empty answer has none)
  uint32_t pad;
};
constexpr uint32_t kDrainMaskRow = 0xFFFFFFFFu;  // DrainQuery.node (mask-layout topics only)
struct DrainArgs {
  const uint64_t* seen;
  const uint8_t* gen;
  uint32_t gen_cur;
  const DrainTopic* topics;
  const DrainGroup* groups;
  const uint64_t* mask;
  const uint32_t* order;
  const uint32_t* ids;
  const DrainQuery* queries;
  uint32_t n_queries;
};
// cnt[s] = delivered positions of segment s, for s < n_segs; cnt[n_segs] = 0
hipError_t launch_drain_count(const DrainArgs& a, uint32_t n_segs, uint64_t* cnt, hipStream_t s);
// off[i] = cnt[0] + .. + cnt[i - 1] for i < n (temp == nullptr: sizes *temp_bytes)
hipError_t drain_scan(void* temp, size_t* temp_bytes, const uint64_t* cnt, uint64_t* off, uint32_t n, hipStream_t s);
// the ids of segments [seg_lo, seg_hi) to out[off[s] - off0 ..), below out_cap;
// staged: through LDS with coalesced stores, else each lane stores its own
hipError_t launch_drain_emit(const DrainArgs& a, uint32_t seg_lo, uint32_t seg_hi, const uint64_t* off, uint64_t off0,
                             uint32_t* out, uint64_t out_cap, bool staged, hipStream_t s);

// The mask-layout tables of a window built on the device (ps_drain_begin):
// window message j of the n_built topics that take this build (topic[k]'s
// messages are j in [msg0[k], msg0[k + 1]); their tables lie back to back
// from position 0, so a topic's first mask word is tab0 / 64) has run index
// idx[j], row bit bit[j] and start round start[j].  ids and mask are cleared
// (kNone / 0) on the stream before the build; err is cleared with them.
constexpr uint32_t kDrainErrOrder = 1;  // a topic's arrival keys do not ascend with the row bit
constexpr uint32_t kDrainErrBit = 2;    // a bit past the row, or two messages on one bit
struct DrainBuild {
  const DrainTopic* topics;
  const uint32_t* topic;  // [n_built]
  const uint32_t* msg0;   // [n_built + 1]
  const uint32_t* idx;
  const uint32_t* bit;
  const uint32_t* start;
  uint32_t n_built, n_msgs, last_first;
  uint64_t n_pos;  // table positions of the built topics together
  uint32_t* ids;
  uint64_t* mask;
  uint64_t* keys;  // start round << 32 | run index, by position (the check's scratch)
  uint32_t* err;
};
// k_drain_tables, then k_drain_tables_check
hipError_t launch_drain_tables(const DrainBuild& b, hipStream_t s);
// hdr[q] = seg_off[queries[q].seg0] for q < n, hdr[n] = seg_off[n_segs], hdr[n + 1] = *err
hipError_t launch_drain_offsets(const DrainQuery* queries, uint32_t n, const uint64_t* seg_off, uint32_t n_segs,
                                const uint32_t* err, uint64_t* hdr, hipStream_t s);

// ---- the shared drain's classify pass (ps_drain_shared) ----
// The queries of mask-layout topics, sorted by topic: bin b holds the n_q
// queries from q0 of one topic, whose row is `words` mask words wide.  Rows of
// up to 64 words take 1 << lanes_log2 lanes each (the power of two at or above
// `words`), 64 >> lanes_log2 queries to a step of 64 lanes; wider rows take
// `waves` whole steps each.  A wave runs kDrainClassPer consecutive steps of
// one bin (the bin's step count rounds up to that); its first wave is wave0.
constexpr uint32_t kDrainClassPer = 4;  // (8: 58 VGPRs, 7 waves per SIMD, 12 % slower on cfg3)
struct DrainClassBin {
  uint32_t topic, q0, n_q, wave0;
  uint32_t words, lanes_log2, waves, pad;
};
struct DrainClassQuery {
  uint32_t node;  // topic-relative
  uint32_t slot;  // the caller's query index: where the verdict goes
};
// verdict[slot] (cleared before the launch) of every query: which of the
// topic's message bits its row holds
constexpr uint32_t kDrainRowMissing = 1;  // a message bit the row does not hold: not full
constexpr uint32_t kDrainRowAny = 2;      // a message bit the row holds: not empty
hipError_t launch_drain_classify(const DrainArgs& a, const DrainClassBin* bins, uint32_t n_bins,
                                 const DrainClassQuery* queries, uint32_t n_waves, uint32_t* verdict, hipStream_t s);

// ---- the shared drain in two halves (ps_drain_shared_begin) --
// What ps_drain_shared does on the host between its two waits, on the device:
// the lists numbered by first use and their segments laid out from the
// verdicts, then count / scan / offsets / emit over those lists with the
// counts read from a control block -- the host knows only the caps.
constexpr uint32_t kDrainOverLists = 1;  // DrainCtl.over: more lists than list_cap
constexpr uint32_t kDrainOverIds = 2;    // ... more ids than id_cap
constexpr uint32_t kDrainOverExc = 4;    // ... more exception records than exc_cap (ps_drain_topics_begin)
struct DrainCtl {
  uint32_t n_lists, n_segs;  // exact, whatever the caps
  uint32_t use_lists, use_segs;  // what the passes behind run over: the above, or 0 past list_cap
  uint32_t over;             // kDrainOver*
  uint32_t pad[3];
};
// The view's first 256 bytes (the parts behind are 256-byte aligned)
struct DrainSharedHdr {
  uint64_t total;
  uint32_t n_lists;
  uint32_t over;  // kDrainOver*
  uint32_t err;   // the table build's error word (kDrainErr*)
  uint32_t pad;
};
struct DrainAssign {
  const DrainTopic* topics;
  const DrainQuery* queries;  // [n] topic and node of every query (seg0 unused)
  const uint32_t* verdict;    // [n] kDrainRow* after the classify pass
  const DrainClassQuery* sorted;  // [n_sorted] the classify pass's queries: by topic, ascending slot within one
  uint32_t n_sorted;
  uint32_t n;
  uint32_t share;             // 0: a full row takes a private list (the PSAMD_DRAIN_SHARED seam)
  uint32_t* first;            // [topics] least full query of the topic; preset to all ones
  uint64_t* key;              // [n] creates << 32 | segments created; key_off: its exclusive scan
  uint64_t* key_off;
  void* scan_temp;
  size_t scan_bytes;
  DrainQuery* lists;          // [list_cap]
  uint32_t list_cap;
  uint32_t seg_bound;         // segments list_cap lists hold at most: what the passes behind are sized for
  uint32_t* list_of_query;    // [n], in the view
  DrainCtl* ctl;
};
// k_drain_first, k_drain_keys, the scan, k_drain_lists
hipError_t launch_drain_assign(const DrainAssign& g, hipStream_t s);
// As launch_drain_count / _offsets / _emit with a.queries = the lists and the
// counts from ctl: cnt[s] for every s <= seg_bound (zero from ctl->use_segs
// on); the header, list_off[0 .. list_cap] (the total from n_lists on) and
// kDrainOverIds; the ids, below id_cap, of at most seg_bound segments and
// none once ctl->over is set.
hipError_t launch_drain_count_dev(const DrainArgs& a, const DrainCtl* ctl, uint32_t seg_bound, uint64_t* cnt,
                                  hipStream_t s);
hipError_t launch_drain_offsets_dev(const DrainQuery* lists, DrainCtl* ctl, uint32_t list_cap, const uint64_t* seg_off,
                                    uint64_t id_cap, const uint32_t* err, DrainSharedHdr* hdr, uint64_t* list_off,
                                    hipStream_t s);
hipError_t launch_drain_emit_dev(const DrainArgs& a, const DrainCtl* ctl, uint32_t seg_bound, const uint64_t* off,
                                 uint32_t* out, uint64_t id_cap, hipStream_t s);

// ---- a topic's audience (ps_drain_topics) -------------------
// The non-root nodes of the requested topics that have window messages, cut
// into strips: runs of consecutive nodes of one topic, kAudStripBytes of rows
// at most (a row counted at the lanes it takes: the power of two at or above
// its mask words up to 64 words, the words themselves above) and at least one
// node.  Strips lie in request order, a topic's in node order; verdict byte
// v0 + i belongs to node u0 + i.  Nothing here comes from a subscriber list:
// the host builds the strips from the topics' node ranges alone.
constexpr uint32_t kAudStripBytes = 16384;
struct AudStrip {
  uint32_t topic;
  uint32_t u0, n;   // topic-relative first node, nodes
  uint32_t nbase;   // the topic's first node (node_peer, gen)
  uint64_t v0;      // the strip's first verdict byte
};
struct AudArgs {
  const AudStrip* strips;
  uint32_t n_strips;
  uint32_t share;     // 0: a full row is an exception too (the PSAMD_DRAIN_SHARED seam)
  uint8_t* verdict;   // one kDrainRow* byte per node; kDrainRowAny alone: the row is full
  uint64_t* n_exc;    // [n_strips + 1] per strip: the nodes that are not full; 0 behind the last
  uint32_t* n_full;   // [n_strips] ... and the full ones
};
// k_audience_classify: one wave streams one strip's rows under the topic's
// message mask (a tree node of another generation is "none", its row not
// read; every node of a kDrainGather topic is any | missing, as
// ps_drain_shared treats its rows) and leaves the verdict bytes and the
// strip's two counts.
hipError_t launch_audience_classify(const DrainArgs& a, const AudArgs& g, hipStream_t s);
// k_audience_emit: one wave per strip reads the verdict bytes alone and
// writes the nodes that are not full, in node order, from record off[strip]
// on (the exclusive sum of n_exc), below cap: the node's peer, its
// topic-relative number and its verdict.
struct AudEmit {
  const uint32_t* node_peer;
  const uint64_t* off;
  uint32_t* peer;
  uint32_t* node;
  uint8_t* verdict;
  uint64_t cap;
};
hipError_t launch_audience_emit(const AudArgs& g, const AudEmit& o, hipStream_t s);
// the exception records ps_drain_topics brings with its first copy; the most
// ps_drain_topics_begin's own exc_cap holds
constexpr uint64_t kAudPrefix = 1ull << 16;

// ---- a topic's audience in two halves (ps_drain_topics_begin) --
// What ps_drain_topics does on the host between its waits, on the device: the
// per-topic totals from the strips' counts, then the lists numbered in request
// order -- entry i's shared list if a node holds it, then a private one per
// "any" record of [exc_off[i], exc_off[i + 1]) -- and their segments laid out,
// around two exclusive sums of creates << 32 | segments keys (as k_drain_keys):
// one over the entries, one over the first exc_cap records.  The lists then go
// through k_drain_count_dev / _offsets_dev / _emit_dev.
struct AudEntry {
  uint32_t topic;
  uint32_t strip0;  // the entry's first strip (entry n: n_strips)
  uint32_t segs;    // segments of one of the topic's lists
  uint32_t pad;
};
struct AudAssign {
  const AudEntry* entries;     // [n + 1]
  uint32_t n, n_strips;
  const uint32_t* strip_full;  // [n_strips] AudArgs::n_full
  const uint64_t* strip_off;   // [n_strips + 1] the exclusive sum of AudArgs::n_exc
  const uint32_t* rec_peer;    // the records k_audience_emit wrote
  const uint32_t* rec_node;
  const uint8_t* rec_verdict;
  uint32_t exc_cap, list_cap;
  uint32_t seg_bound;          // segments list_cap lists hold at most
  uint64_t* ekey;              // [n + 1] an entry's key (a shared list); ekey_off: its exclusive sum
  uint64_t* ekey_off;
  uint64_t* rkey;              // [exc_cap + 1] a record's key (a private list), zero from the record count on
  uint64_t* rkey_off;
  void* scan_temp;
  size_t scan_bytes;
  uint32_t* topic_list;        // the view: [n]
  uint64_t* n_full;            // [n]
  uint64_t* exc_off;           // [n + 1]
  uint32_t* exc_peer;          // [exc_cap]
  uint32_t* exc_list;          // [exc_cap]
  DrainQuery* lists;           // [list_cap]
  DrainCtl* ctl;
};
// k_audience_totals, k_audience_keys, the two scans, k_audience_lists: n_full
// and exc_off exact whatever the caps; exc_peer / exc_list for the records
// below exc_cap (PS_NONE behind the count); nothing stored past a cap; the
// control block with kDrainOverExc / kDrainOverLists.
hipError_t launch_audience_assign(const AudAssign& g, hipStream_t s);

// ---- the sink: every window of a run into one result (ps_sink_set) --
// The run cursor: what the windows so far have added to the result.  Two of
// them alternate: window w reads cur[w & 1] as its base -- the window header,
// which nothing writes while the window's commit and emit run -- and its
// commit leaves cur[(w + 1) & 1] for the next window.  The one the last window
// left is the result's header.
struct SinkCursor {
  uint64_t ids;      // ids so far: exact while the lists fit
  uint32_t lists;    // lists so far: exact, whatever the caps
  uint32_t windows;  // windows so far
  uint32_t over;     // kDrainOver*, sticky: no id is emitted from the first overflow on
  uint32_t err;      // the windows' table error words (kDrainErr*)
  uint64_t exc;      // the audience sink's exception records so far: exact, whatever the caps (else 0)
};
static_assert(sizeof(SinkCursor) == 32, "two cursors alternate in the result's first 64 bytes");
struct SinkCommit {
  const DrainQuery* lists;      // the window's lists (k_drain_lists)
  const DrainCtl* ctl;          // ... and their counts
  const uint64_t* seg_off;      // the window's scanned segment counts
  const uint32_t* win_lq;       // [n] the window's own list numbers (PS_NONE: none)
  const uint32_t* err;          // the window's table error word
  SinkCursor* cur;              // [2]
  uint64_t* list_off;           // [list_cap + 1] the run's
  uint32_t* win_list;           // [windows x n] the run's
  uint32_t w, n;                // the window's number in the run; queries
  uint32_t win_list_cap;        // lists this window's passes were sized for
  uint32_t list_cap;            // the run's caps as far as this window
  uint64_t id_cap;
};
// k_sink_commit: list_off[base + l], row w of win_list, the next cursor.
hipError_t launch_sink_commit(const SinkCommit& c, hipStream_t s);
// k_sink_emit: k_drain_emit_dev with the output base read from cur[w & 1] and
// the verdict on the caps from cur[(w + 1) & 1]
hipError_t launch_sink_emit(const DrainArgs& a, const DrainCtl* ctl, const SinkCursor* cur, uint32_t w,
                            uint32_t seg_bound, const uint64_t* off, uint32_t* out, uint64_t id_cap, hipStream_t s);

// ---- the audience sink: ps_drain_topics behind every window (ps_sink_set_topics) --
// The window's audience view as launch_audience_assign left it (window-local
// list numbers, exc_off from 0), its lists and control block, the scanned
// segment counts -- and the run's result they go into at the run cursor.
struct AudSinkCommit {
  const DrainQuery* lists;      // the window's lists (k_audience_lists)
  const DrainCtl* ctl;          // ... and their counts
  const uint64_t* seg_off;      // the window's scanned segment counts
  const uint32_t* win_topic_list;  // [n] the window's view
  const uint64_t* win_n_full;      // [n]
  const uint64_t* win_exc_off;     // [n + 1]
  const uint32_t* win_exc_peer;    // [win_exc_cap]
  const uint32_t* win_exc_list;    // [win_exc_cap]
  const uint32_t* err;          // the window's table error word
  SinkCursor* cur;              // [2]
  uint64_t* list_off;           // [list_cap + 1] the run's
  uint32_t* topic_list;         // [windows x n] the run's
  uint64_t* n_full;             // [windows x n]
  uint64_t* exc_off;            // [windows x n + 1]
  uint32_t* exc_peer;           // [exc_cap]
  uint32_t* exc_list;           // [exc_cap]
  uint32_t w, n;                // the window's number in the run; topics
  uint32_t win_list_cap, win_exc_cap;  // what this window's passes were sized for
  uint32_t list_cap, exc_cap;   // the run's caps as far as this window
  uint64_t id_cap;
};
// k_audience_sink_commit: list_off[base + l], rows w of topic_list / n_full /
// exc_off, the window's records at the run's record count, the next cursor.
// Nothing is stored past a cap.  k_sink_emit follows it as it follows k_sink_commit.
hipError_t launch_audience_sink_commit(const AudSinkCommit& c, hipStream_t s);

// ---- per-peer load (ps_peer_load, ps_load_track) --------------
// The audience pass's verdicts turned into per-peer sums, in peer space: a
// non-root node whose row holds k of its topic's c_t window messages adds k to
// recv[its peer] and k * its CSR children to sent[its peer]; the root, no
// recipient, adds c_t * its children to sent.  The entry table of the strips
// (AudEntry's shape: request order, entry n closes the table) carries what the
// strips do not: the topic's window messages and its root's node.
constexpr uint32_t kLoadNoRoot = 0xFFFFFFFFu;
struct LoadEntry {
  uint32_t topic;
  uint32_t strip0;  // the entry's first strip (entry n: n_strips)
  uint32_t c_t;     // the topic's messages in the window
  uint32_t root;    // the root's node (node space), kLoadNoRoot: none on this rank
};
struct LoadArgs {
  const AudStrip* strips;
  uint32_t n_strips;
  const LoadEntry* entries;  // [n + 1]
  uint32_t n;
  const uint8_t* verdict;    // AudArgs::verdict after k_audience_classify
  const uint32_t* node_peer;
  const uint32_t* row_ptr;
  uint32_t count_rows;       // 1: a full row is counted from its words too (the PSAMD_LOAD_COUNT seam)
  uint64_t* recv;            // [n_peers] added into
  uint64_t* sent;            // [n_peers]
};
// k_audience_load: one wave per strip behind k_audience_classify.  A full row
// counts c_t, an empty or stale one nothing; any other row, and every row of a
// kDrainGather topic, is counted by the wave, one row at a time.
hipError_t launch_audience_load(const DrainArgs& a, const LoadArgs& g, hipStream_t s);

// ---- deliveries by hop per topic (ps_topic_hops, ps_hops_track) --
// The audience pass's verdicts turned into three histograms per tree topic, by
// BFS level: a non-root node of level d whose row holds k of its topic's c_t
// window messages adds 1 to nodes, (k > 0) to reached and k to deliv, in
// column min(d, kHopsCols - 1) of the topic's row.  The strips are the
// audience pass's, cut with no regard to levels; the entry table (request
// order among the tree topics, entry n closes it) carries the topic's level
// table -- levels[lvl0 + d], d in [0, depth + 1]: the first node of level d,
// topic-relative, n_nodes behind the last -- and its strip length, so that a
// level's strips follow from its node range.  Strip s of an entry leaves one
// partial per level d it meets, in slot part0 + (s - strip0) + (d - 1): strips
// and levels both ascend along a topic's nodes, so no two pairs share a slot.
constexpr uint32_t kHopsCols = 256;  // PS_MAX_ROUNDS
struct HopsEntry {
  uint32_t topic;
  uint32_t strip0;  // the entry's first strip (entry n: n_strips)
  uint32_t c_t;     // the topic's messages in the window
  uint32_t row;     // the topic's row of the outputs: its position in the request
  uint32_t lvl0;    // the topic's level table in HopsArgs::levels
  uint32_t depth;   // its deepest level
  uint32_t per;     // nodes of every strip of the entry but the last
  uint32_t part0;   // the entry's first partial slot (it owns strips + depth of them)
};
struct HopsArgs {
  const AudStrip* strips;
  uint32_t n_strips;
  const HopsEntry* entries;  // [n + 1]
  uint32_t n;
  const uint32_t* levels;
  const uint8_t* verdict;    // AudArgs::verdict after k_audience_classify
  const uint64_t* n_exc;     // AudArgs::n_exc: 0 = every node of the strip is full
  uint32_t count_rows;       // 1: a full row is counted from its words too (the PSAMD_LOAD_COUNT seam)
  uint32_t max_cols;         // columns 1 .. max_cols are summed: the deepest entry's, kHopsCols - 1 at most
  uint32_t* part_reached;    // per (strip, level) slot
  uint64_t* part_deliv;
  uint64_t* nodes;           // [rows][kHopsCols] each, added into
  uint64_t* reached;
  uint64_t* deliv;
};
// k_audience_hops: one wave per strip behind k_audience_classify, a node per
// lane, level by level; a strip without exceptions takes its partials from the
// level bounds alone.  k_audience_hops_sum: one block per (entry, column) adds
// the column's run of partials -- the last column every level from
// kHopsCols - 1 on -- and the level's size into the three outputs: one writer
// per word, plain loads and stores.
hipError_t launch_audience_hops(const DrainArgs& a, const HopsArgs& g, hipStream_t s);
hipError_t launch_audience_hops_sum(const HopsArgs& g, hipStream_t s);

// ---- audience behind each peer (ps_peer_downstream, ps_downstream_track) --
// The audience pass's verdicts turned into two sums per peer, over the subtrees
// of its nodes: a node u of a tree topic (the root too) adds the nodes strictly
// below it to below[its peer] and the window messages their rows hold to
// carried[its peer].  Three kernels over three scratch arrays, an entry's
// n_nodes words of each from n0 (the root's first): k[u] the messages u's row
// holds (the root's 0), w_n[u] = 1 + the nodes below u, w_k[u] = k[u] + the k
// below u.  The entry table (request order among the tree topics, entry n
// closes it) carries the level table as HopsEntry does; a node's children are
// its CSR range one level down (BFS numbering: level d + 1 lists the children
// of level d's nodes in node order).  k_audience_weights writes k over the
// audience pass's strips.  k_downstream_level, launched once per level from
// the level above an entry's deepest upwards, sums a level's nodes from their
// children's words -- the launch before wrote them; the deepest level's nodes
// are leaves, (1, k), and are read as that -- over a work list of (entry,
// level, node range) items, a block each.  The levels [0, top) of an entry,
// from the root down to the first level wider than a block, are walked upwards
// by one block in k_downstream_top.
constexpr uint32_t kDownBlock = 256;  // nodes of a work item at most: a thread each
struct DownEntry {
  uint32_t topic;
  uint32_t strip0;  // the entry's first strip (entry n: n_strips)
  uint32_t c_t;     // the topic's messages in the window
  uint32_t nbase;   // the topic's first node (its root) in node space
  uint32_t lvl0;    // the topic's level table in DownArgs::levels
  uint32_t depth;   // its deepest level
  uint32_t n0;      // the entry's first word of k / w_n / w_k
  uint32_t top;     // levels [0, top) are k_downstream_top's, min(top, depth) at most
};
struct DownWork {
  uint32_t entry, level;
  uint32_t lo, hi;  // topic-relative nodes of that level, at most kDownBlock
};
struct DownArgs {
  const AudStrip* strips;
  uint32_t n_strips;
  const DownEntry* entries;  // [n + 1]
  uint32_t n;
  const uint32_t* levels;
  const DownWork* work;      // launch by launch
  const uint8_t* verdict;    // AudArgs::verdict after k_audience_classify
  const uint64_t* n_exc;     // AudArgs::n_exc: 0 = every node of the strip is full
  uint32_t count_rows;       // 1: a full row is counted from its words too (the PSAMD_LOAD_COUNT seam)
  const uint32_t* node_peer;
  const uint32_t* row_ptr;
  uint32_t* k;
  uint32_t* w_n;
  uint64_t* w_k;
  uint64_t* below;           // [n_peers] added into
  uint64_t* carried;         // [n_peers]
};
// k_audience_weights: one wave per strip behind k_audience_classify, a node per lane
hipError_t launch_audience_weights(const DrainArgs& a, const DownArgs& g, hipStream_t s);
// k_downstream_level over work items [w0, w1): one launch of the bottom-up pass
hipError_t launch_downstream_level(const DownArgs& g, uint32_t w0, uint32_t w1, hipStream_t s);
// k_downstream_top: one block per entry, behind the last level launch
hipError_t launch_downstream_top(const DownArgs& g, hipStream_t s);

// ---- losses blamed on their cut points (ps_peer_cut, ps_cut_track) --
// The same strips, entries, level tables, work list and scratch as the pass
// above (DownArgs, whose below / carried stay unused), turned into four sums
// per peer.  With miss(v) = c_t - k(v), the root counting as full: a node v
// adds miss(v) to missed[its peer]; a non-root node u that lacks messages
// under a full parent is a cut point and adds 1 to cuts, w_n[u] - 1 to
// orphaned and c_t * w_n[u] - w_k[u] to lost, each at its peer.
// k_audience_missed runs over the strips behind k_audience_weights.
// k_cut_level / k_cut_top are k_downstream_level / k_downstream_top without
// the peer sums of their own: they build w_n and w_k bottom-up and find the
// cut points from the parent's side -- a full node walks its children's words
// anyway --, so that no parent array is needed, no launch covers the deepest
// level, and node_peer is read for cut points only.  Level 0 counts as full
// whatever k[root] holds (k_audience_weights stores 0 there).
struct CutArgs {
  DownArgs d;
  uint64_t* missed;    // [n_peers] each, added into
  uint64_t* cuts;
  uint64_t* orphaned;
  uint64_t* lost;
};
// k_audience_missed: one wave per strip behind k_audience_weights, a node per lane
hipError_t launch_audience_missed(const CutArgs& g, hipStream_t s);
// k_cut_level over work items [w0, w1): one launch of the bottom-up pass
hipError_t launch_cut_level(const CutArgs& g, uint32_t w0, uint32_t w1, hipStream_t s);
// k_cut_top: one block per entry, behind the last level launch
hipError_t launch_cut_top(const CutArgs& g, hipStream_t s);

// ---- each missed subscriber and its cut point (ps_topic_blame, ps_blame) --
// The pass above asks what hangs behind a cut point; this one asks, for every
// node that lacks messages, which cut point it hangs behind.  The same strips,
// entries, level tables and work list (DownArgs; w_n, w_k, below and carried
// stay unused) and k from k_audience_weights, walked the other way: with
// cut(u) = u where u's parent is full (level 0 counts as full) and
// cut(parent(u)) else, for every non-root node u with k(u) < c_t, two scratch
// words of the pass's own per node, an entry's from n0 as k's:
//   cut_node[u]   cut(u), topic-relative; kBlameNone where k(u) == c_t
//   cut_level[u]  the BFS level of cut(u); kBlameNone where k(u) == c_t
//   k_blame_top     one block per entry walks the levels [0, top) downwards, a
//                   barrier between two levels: a node of level d visits its
//                   CSR child range in level d + 1 (cut_nodes' range
//                   arithmetic and clamping; a lane a node, a node with more
//                   than a wave's worth of children spread over the wave) and
//                   writes each child's two words -- (child, d + 1) where the
//                   node is full, else the node's own two.
//   k_blame_level   the same visit over work items [w0, w1); the launches run
//                   in the reverse of the bottom-up order, behind k_blame_top,
//                   so a level's own words were written by the launch before
//                   (level `top`'s by k_blame_top).  Every word has one
//                   writer: no atomics, plain stores; stream order is the
//                   only order between the launches.
//   k_blame_count   one wave per strip: its nodes with k < c_t into n_rec
//                   (n_rec[n_strips] = 0); drain_scan turns them into off.
//   k_blame_emit    one wave per strip: those nodes in node order from record
//                   off[strip] on, below cap -- the node's peer, the peer of
//                   cut(u), the node's level (its topic's level table, binary
//                   search), cut_level and c_t - k; an array that is null is
//                   not written.  rec_off[i] = off[entries[i].strip0] for i in
//                   [0, n]: the records of entry i, rec_off[n] the total.
//   k_blame_gather  one thread per DrainQuery {topic, node} (node: topic-
//                   relative, the root 0, kBlameNone: the peer holds no node of
//                   the topic) through a table per topic id: the topic's entry
//                   (kBlameNone: idle in the window -- the sweep's scratch is
//                   not read) and its level table among `levels`.
constexpr uint32_t kBlameNone = 0xFFFFFFFFu;  // PS_NONE
struct BlameTopic {
  uint32_t entry;  // the topic's entry among DownArgs::entries; kBlameNone: none, or idle in the window
  uint32_t lvl0;   // its level table in BlameGather::levels: depth + 2 words
  uint32_t depth;
  uint32_t pad;
};
struct BlameArgs {
  DownArgs d;
  uint32_t* cut_node;
  uint32_t* cut_level;
  uint64_t* n_rec;       // [n_strips + 1]
  const uint64_t* off;   // [n_strips + 1] the exclusive sum of n_rec
  uint64_t* rec_off;     // [n + 1]
  uint32_t* rec_peer;    // [cap] each; null: not asked for
  uint32_t* rec_cut_peer;
  uint32_t* rec_hop;
  uint32_t* rec_cut_hop;
  uint32_t* rec_missed;
  uint64_t cap;
};
struct BlameGather {
  const DrainQuery* queries;  // [n]
  uint32_t n;
  const BlameTopic* topics;   // by topic id
  const uint32_t* levels;
  uint32_t* cut_peer;         // [n] each, written in full
  uint32_t* hop;
  uint32_t* cut_hop;
  uint32_t* missed;
};
// k_blame_top, then k_blame_level over work items [w0, w1)
hipError_t launch_blame_top(const BlameArgs& g, hipStream_t s);
hipError_t launch_blame_level(const BlameArgs& g, uint32_t w0, uint32_t w1, hipStream_t s);
hipError_t launch_blame_count(const BlameArgs& g, hipStream_t s);
hipError_t launch_blame_emit(const BlameArgs& g, hipStream_t s);
hipError_t launch_blame_gather(const BlameArgs& g, const BlameGather& q, hipStream_t s);

// ---- blame records behind every window (ps_blame_track, ps_blame_take) --
// The pass above behind every window of a run, its records appended where a
// cursor on the device stands: the front, the sweep, k_blame_count and the scan
// as they are, then
//   k_blame_track_commit  a thread per request position i of window w (the
//                   host counts the windows): rec_off[w * n_req + 1 + i] =
//                   base + off[entries[ent[i]].strip0], with base the records
//                   of the windows before, cur[w & 1].total, and ent[i] the
//                   tree topics among the positions [0, i] -- the entry behind
//                   position i, so that an idle position and one skipped as a
//                   mesh repeat their predecessor.  n_strips == 0: a window
//                   without a row to read, every offset the base; entries and
//                   off are not read.  The grid's first thread writes
//                   rec_off[0] = 0 in window 0 and the cursor of the window
//                   behind, cur[(w + 1) & 1]: total + the window's records;
//                   over once total passes `cap`; stored = min(total, cap)
//                   until a window has overflowed, then as it stands.  The two
//                   cursors alternate so that every word has one writer and
//                   no thread reads a word this launch writes.
//   k_blame_track_emit    k_blame_emit's strips (ballot, lane prefix, node
//                   order, the level by binary search) from record base +
//                   off[strip] on, below `cap`; nothing where cur[w & 1].over
//                   is set: a window before overflowed.  All five arrays.
struct BlameCursor {
  uint64_t total;   // records of the windows so far, stored or not
  uint64_t stored;  // of them kept: the arrays hold exactly the first `stored`
  uint64_t over;    // 1: a window passed the cap in effect; nothing is stored behind it
  uint64_t pad;
};
struct BlameTrack {
  BlameCursor* cur;     // [2]
  const uint32_t* ent;  // [n_req]
  uint64_t* rec_off;    // [(w + 1) * n_req + 1]
  uint64_t w;
  uint64_t cap;         // the cap in effect: the record arrays hold that many
  uint32_t n_req;
};
// (BlameArgs: d, cut_node, cut_level, n_rec, off and the five arrays; rec_off and cap stay unused)
hipError_t launch_blame_track_commit(const BlameArgs& g, const BlameTrack& t, hipStream_t s);
hipError_t launch_blame_track_emit(const BlameArgs& g, const BlameTrack& t, hipStream_t s);

// ---- the four answers from one pass (ps_peer_report, ps_report_track) --
// What the four families above compute, each behind a classify of its own,
// behind one: k_report_nodes works a node's k out once and feeds every section
// selected in `what` (PS_REPORT_*) from it -- recv / sent as k_audience_load,
// the (strip, level) partials as k_audience_hops into HopsArgs' slots (the
// unchanged k_audience_hops_sum sums them), the k word as k_audience_weights,
// missed as k_audience_missed.  Its entry table covers every strip: the tree
// entries first, in the order of HopsArgs::entries and DownArgs::entries (one
// index serves all three tables), then the entries that feed the load section
// alone (meshes; every topic where nothing else is selected).
// k_report_level / k_report_top are the one bottom-up sweep where both subtree
// sections are selected: cut_nodes' walk with down_nodes' two adds.  With one
// of them selected the pass launches that section's own level kernels.
constexpr uint32_t kReportLoad = 1u, kReportHops = 2u, kReportDown = 4u, kReportCut = 8u, kReportAll = 15u;
struct ReportEntry {
  uint32_t topic;
  uint32_t strip0;  // the entry's first strip (entry n: n_strips)
  uint32_t c_t;     // the topic's messages in the window
  uint32_t root;    // the root's node (node space), kLoadNoRoot: none on this rank
  uint32_t tree;    // 1: a tree topic, the fields below stand; 0: the entry feeds the load section alone
  uint32_t lvl0;    // HopsEntry::lvl0
  uint32_t depth;   // HopsEntry::depth
  uint32_t part0;   // HopsEntry::part0
  uint32_t n0;      // DownEntry::n0
  uint32_t pad[3];
};
struct ReportArgs {
  const AudStrip* strips;
  uint32_t n_strips;
  const ReportEntry* entries;  // [n + 1]
  uint32_t n;
  uint32_t what;             // PS_REPORT_* bits: the template the launch picks
  const uint32_t* levels;
  const uint8_t* verdict;    // AudArgs::verdict after k_audience_classify
  const uint64_t* n_exc;     // AudArgs::n_exc: 0 = every node of the strip is full
  uint32_t count_rows;       // 1: a full row is counted from its words too (the PSAMD_LOAD_COUNT seam)
  const uint32_t* node_peer;
  const uint32_t* row_ptr;
  uint64_t* recv;            // [n_peers] each, added into (load)
  uint64_t* sent;
  uint32_t* part_reached;    // HopsArgs' slots (hops)
  uint64_t* part_deliv;
  uint32_t* k;               // DownArgs::k (downstream, cut)
  uint64_t* missed;          // [n_peers], added into (cut)
};
// k_report_nodes: one wave per strip behind k_audience_classify, a node per lane
hipError_t launch_report_nodes(const DrainArgs& a, const ReportArgs& g, hipStream_t s);
// k_report_level over work items [w0, w1), k_report_top: the bottom-up pass
// with all six sums of CutArgs (d.below and d.carried too)
hipError_t launch_report_level(const CutArgs& g, uint32_t w0, uint32_t w1, hipStream_t s);
hipError_t launch_report_top(const CutArgs& g, hipStream_t s);

// ---- a rank's share of the report (ps_dist_report) ------------
// Load, hops and downstream for the nodes one rank owns, on whatever node
// numbering the window ran on: one rank's BFS order, or a sharded rank's --
// level by level, a level's locally fed nodes ahead of its ghost-fed ones, a
// level possibly empty, node 0 the root only on the root's owner.  The entry
// table follows the request (entry i is topic[i], row i of the hop arrays;
// entry n closes it); a tree entry carries the rank's own level table as
// HopsEntry does and its first word n0 of the three per-node arrays k, acc_n
// and acc_k, which the host clears ahead of the pass.
//   k_dist_nodes        one wave per strip behind k_audience_classify, a node
//                       per lane: k once, into recv / sent, into a partial
//                       pair per (strip, level) in HopsArgs' slots and into
//                       the k word.  Nothing is written for a root by position:
//                       a root's words stay as cleared.
//   k_dist_hops_sum     k_audience_hops_sum over a level table whose levels
//                       may be empty: one block per (entry, column).
//   k_dist_sweep_level  one launch per absolute level L, the deepest first,
//                       level 0 last: node u adds its accumulator (acc_n,
//                       acc_k) -- what lies strictly below it -- to below /
//                       carried of its peer and pushes (1 + acc_n, k + acc_k)
//                       to its parent: into the parent's accumulator where this
//                       rank owns it (node_parent), else into the record
//                       send[base[sb0 + L * world + a] + j] of the parent's
//                       owner a and record index j (gslot[u] = a << 27 | j);
//                       a root pushes nothing.
//   k_dist_apply        behind a level's exchange: a received record into the
//                       accumulator of the parent it names (plist).
// Stream order and the transport's own ordering are the only order between
// the launches; every add is a relaxed device-scope 64-bit atomic, a zero add
// skipped.  Every table-derived index is clamped into its entry's words.
struct DistEntry {
  uint32_t topic;
  uint32_t strip0;  // the entry's first strip (entry n: n_strips)
  uint32_t c_t;     // the topic's messages in the window
  uint32_t root;    // the root's node (node space), kLoadNoRoot: none on this rank
  uint32_t tree;    // 1: a tree topic, the fields below stand; 0: the entry feeds the load section alone
  uint32_t lvl0;    // the topic's level table in DistArgs::levels: depth + 2 words
  uint32_t depth;   // its deepest level
  uint32_t nbase;   // the topic's first node in node space
  uint32_t nn;      // its nodes on this rank
  uint32_t n0;      // the entry's first word of k / acc_n / acc_k
  uint32_t sb0;     // the entry's first word of DistArgs::send_base: (depth + 1) * world words
  uint32_t per;     // nodes of every strip of the entry but the last (HopsEntry::per)
  uint32_t part0;   // the entry's first partial slot: it owns strips + depth of them (HopsEntry::part0)
  uint32_t pad;
};
static_assert(sizeof(DistEntry) == 56, "DistEntry is uploaded as laid out here");
struct DistRec {
  uint64_t n, k;  // nodes and window messages of the subtrees pushed so far
};
struct DistWork {
  uint32_t entry;
  uint32_t lo, hi;  // topic-relative nodes of the launch's level, at most kDownBlock
};
struct DistApply {
  uint32_t entry;
  uint32_t rec0;   // the item's first received record
  uint32_t pl0;    // ... and its first word of DistArgs::plist
  uint32_t n;      // records, at most kDownBlock
};
struct DistArgs {
  const AudStrip* strips;
  uint32_t n_strips;
  const DistEntry* entries;  // [n + 1]
  uint32_t n;
  uint32_t what;             // PS_REPORT_* bits within PS_REPORT_DIST
  uint32_t world;
  const uint32_t* levels;
  const uint8_t* verdict;    // AudArgs::verdict after k_audience_classify
  const uint64_t* n_exc;     // AudArgs::n_exc: 0 = every node of the strip is full
  uint32_t count_rows;       // 1: a full row is counted from its words too (the PSAMD_LOAD_COUNT seam)
  const uint32_t* node_peer;
  const uint32_t* node_parent;
  const uint32_t* row_ptr;
  uint64_t* recv;            // [n_peers] each, added into (load)
  uint64_t* sent;
  uint32_t* part_reached;    // per (strip, level) slot (hops)
  uint64_t* part_deliv;
  uint32_t n_parts;
  uint64_t* nodes;           // [n][kHopsCols] each, added into (hops)
  uint64_t* reached;
  uint64_t* deliv;
  uint32_t* k;               // per-node words (downstream)
  uint64_t* acc_n;
  uint64_t* acc_k;
  uint64_t* below;           // [n_peers] each, added into (downstream)
  uint64_t* carried;
  const DistWork* work;      // launch by launch
  const uint32_t* gslot;     // per node of the node space: owner << 27 | record index of a remote parent, kNone
  const uint32_t* send_base; // per (entry, level, owner): the first record of the entry's run in that region
  DistRec* send;             // the sweep's send records
  uint32_t n_send;
  const DistApply* apply;    // exchange by exchange
  const uint32_t* plist;     // per ghost record this rank receives: the parent's node
  const DistRec* rcv;        // the sweep's received records
  uint32_t n_recv, n_plist;
};
hipError_t launch_dist_nodes(const DrainArgs& a, const DistArgs& g, hipStream_t s);
// k_dist_hops_sum over columns 1 .. max_cols (the deepest entry's, kHopsCols - 1 at most)
hipError_t launch_dist_hops_sum(const DistArgs& g, uint32_t max_cols, hipStream_t s);
// k_dist_sweep_level over work items [w0, w1): the nodes of level `level`
hipError_t launch_dist_sweep_level(const DistArgs& g, uint32_t level, uint32_t w0, uint32_t w1, hipStream_t s);
// k_dist_apply over apply items [a0, a1): one exchange's records
hipError_t launch_dist_apply(const DistArgs& g, uint32_t a0, uint32_t a1, hipStream_t s);

// ---- a rank's share of the cut (ps_dist_cut) ------------------
// ps_peer_cut's four sums for the nodes one rank owns, decided from the
// child's side: u is a cut point iff k(u) < c_t and its parent's k == c_t (a
// root counts as c_t).  DistArgs' tables, words and sweep (d) carry it; a
// remote parent's k arrives ahead of the sweep in one downward exchange whose
// regions mirror the sweep's with the two ranks swapped: a word per (remote
// parent, child rank) pair, the pair's record index (gslot / plist) its place.
//   k_dist_cut_nodes  k_dist_nodes<false, false, true> plus c_t - k into
//                     missed of the node's peer.
//   k_dist_cut_fill   one block per fill item, a thread per plist record this
//                     rank holds as the parents' owner: the parent's k (c_t for
//                     the entry's root) into down_send[rec0 + j].
//   k_dist_cut_level  k_dist_sweep_level's launch: node u of level L >= 1
//                     with (acc_n, acc_k), its k and its parent's -- the k word
//                     of a local parent, else down_recv[down_base[sb0 + L *
//                     world + a] + j] -- adds 1, acc_n and c_t * (1 + acc_n) -
//                     (k + acc_k) into cuts, orphaned and lost of its peer
//                     where it is a cut point, then pushes as the sweep does.
//                     below and carried are not written.
// k_dist_apply is the sweep's.  Order, atomics and clamping as above.
struct DistCutArgs {
  DistArgs d;                 // recv .. carried unused
  uint64_t* missed;           // [n_peers] each, added into
  uint64_t* cuts;
  uint64_t* orphaned;
  uint64_t* lost;
  const DistApply* fill;      // fill items: rec0 the first word of down_send, pl0 of plist, n words
  uint32_t* down_send;        // the parents' k, region by region
  const uint32_t* down_recv;  // ... as received
  const uint32_t* down_base;  // per (entry, level, owner) as send_base: the first word of the run in down_recv
  uint32_t n_down_send, n_down_recv;
};
hipError_t launch_dist_cut_nodes(const DrainArgs& a, const DistCutArgs& g, hipStream_t s);
// k_dist_cut_fill over fill items [0, n_fill)
hipError_t launch_dist_cut_fill(const DistCutArgs& g, uint32_t n_fill, hipStream_t s);
// k_dist_cut_level over work items [w0, w1): the nodes of level `level` (>= 1)
hipError_t launch_dist_cut_level(const DistCutArgs& g, uint32_t level, uint32_t w0, uint32_t w1, hipStream_t s);

// ---- a rank's share of the blame (ps_dist_blame) ---------------
// ps_topic_blame's records for the non-root nodes one rank owns, where cut(u)
// and every node on the way up to it may live on any rank.  DistArgs' tables
// and k word (d; k_dist_nodes<false, false, true> leaves k) carry it; two words
// of the pass's own per owned node, an entry's from n0 as k's:
//   cut_peer[u]  the peer of cut(u) -- a peer id, since a remote cut point has
//                no node on this rank; kBlameNone where k(u) >= c_t
//   cut_hop[u]   the BFS level of cut(u); kBlameNone where k(u) >= c_t
// The sweep runs top-down and is decided at the child, from its parent's pair
// alone: none (the parent is full, or the entry's root) makes u its own cut
// point, anything else is inherited.  A remote parent's pair arrives in a
// downward exchange per level -- a pair exists only once the level above has
// run -- whose regions mirror the sweep's upward ones with the two ranks
// swapped: 8 bytes per (remote parent, child rank) pair, the pair's record
// index (gslot / plist) its place.
//   k_dist_blame_fill   one block per fill item of level L, a thread per plist
//                       record this rank holds as the parents' owner: the
//                       parent's pair, (none, none) where it is full or the
//                       entry's root, into down_send[rec0 + j].
//   k_dist_blame_level  one block per work item of level L >= 1, a thread per
//                       node: none where k(u) >= c_t; else the parent's pair
//                       -- the two words of a local parent, or down_recv[
//                       down_base[sb0 + L * world + a] + j] -- or (peer(u), L)
//                       where that pair is none.  One writer per word: plain
//                       stores, no atomics.
//   k_dist_blame_count  k_blame_count over the rank's strips and DistEntry.
//   k_dist_blame_emit   k_blame_emit: the records in node order (ballot and
//                       lane prefix); rec_hop from the rank's own level table,
//                       whose levels may be empty.
// Stream order and the transport's own ordering are the only order between the
// launches.  Every table-derived index is clamped into its entry's words or its
// region.
struct DistBlameArgs {
  DistArgs d;                 // recv .. carried, acc_n, acc_k, send, rcv unused
  uint32_t* cut_peer;         // per-node words, beside d.k
  uint32_t* cut_hop;
  const DistApply* fill;      // fill items, level by level: rec0 the first pair of down_send, pl0 of plist, n pairs
  uint2* down_send;           // the parents' pairs, level by level, region by region
  const uint2* down_recv;     // ... as received
  const uint32_t* down_base;  // per (entry, level, owner) as send_base: the first pair of the run in down_recv
  uint32_t n_down_send, n_down_recv;
  uint64_t* n_rec;            // [n_strips + 1]
  const uint64_t* off;        // [n_strips + 1] the exclusive sum of n_rec
  uint64_t* rec_off;          // [n + 1]
  uint32_t* rec_peer;         // [cap] each; null: not asked for
  uint32_t* rec_cut_peer;
  uint32_t* rec_hop;
  uint32_t* rec_cut_hop;
  uint32_t* rec_missed;
  uint64_t cap;
};
// k_dist_blame_fill over fill items [f0, f1): one level's
hipError_t launch_dist_blame_fill(const DistBlameArgs& g, uint32_t f0, uint32_t f1, hipStream_t s);
// k_dist_blame_level over work items [w0, w1): the nodes of level `level` (>= 1)
hipError_t launch_dist_blame_level(const DistBlameArgs& g, uint32_t level, uint32_t w0, uint32_t w1, hipStream_t s);
hipError_t launch_dist_blame_count(const DistBlameArgs& g, hipStream_t s);
hipError_t launch_dist_blame_emit(const DistBlameArgs& g, hipStream_t s);

// ---- hops and duplicate copies, meshes too (ps_topic_spread) ----
// A frontier BFS over the CSR child lists, from the rows the window left: the
// forwarders F of a topic are its root and every non-root node whose row holds
// k > 0 of its c_t window messages; a forwarder's hop is its BFS distance from
// the root within F, and a visited forwarder q sends k'(q) (c_t for the root)
// along every child entry whose target is in F.  The entry table follows the
// request (entry i is topic[i], row i of the per-topic outputs; entry n closes
// it); an entry owns nn words of the two per-node arrays from n0, the root's
// first: k, and the hop word (kSpreadNone: not visited).
//   k_spread_nodes  one wave per strip behind k_audience_classify, a node per
//                   lane: k into its word and into recv of the node's peer;
//                   per entry the nodes with k > 0 and, for a tree, those
//                   with k == 0.
//   k_spread_unreached  a mesh's nodes with k == 0, each peer once: where a
//                   parent lists a peer twice the node space keeps a node for
//                   either entry, and every child entry names the later one.
//                   One wave per strip, a node per lane (an entry's first
//                   strip: its root too) walks its child entries; a named
//                   node with k == 0 is counted by the entry that turns its
//                   hop word from kSpreadNone into kSpreadNamed -- a word the
//                   BFS never reads, so the launch may run beside the levels.
//   k_spread_level  launch L: the frontier queue [L & 1], cnt[L % 3] items
//                   (the host seeds queue 0 with the roots), a lane per item;
//                   an item's child entries one by one where it has at most
//                   `wide` of them, else by the whole wave, lanes across
//                   entries.  A target in F adds the item's k' to copies of
//                   its peer; a non-root target whose hop word one
//                   compare-and-swap turns from kSpreadNone into L + 1 is
//                   appended to queue [(L + 1) & 1], once whatever names it.
//                   The launch clears cnt[(L + 2) % 3], which no launch before
//                   L + 1 adds to.  The grid is the host's; its waves stride
//                   over the items.
//   k_spread_sum    one wave per strip: the hop words of the nodes with k > 0
//                   into a (reached, deliv) pair per column in LDS, the pairs
//                   that are not zero added to the entry's rows; the visited
//                   nodes per entry.
//   k_spread_dup    a thread per peer: dup = copies - recv (modulo 2^64).
// Stream order is the only order between the launches; every add is a relaxed
// device-scope atomic on integers, so the sums do not depend on the order;
// every index that comes from a table is checked against its array.
constexpr uint32_t kSpreadNone = 0xFFFFFFFFu;
constexpr uint32_t kSpreadNamed = 0xFFFFFFFEu;  // the hop word of a node without messages that a child entry names
struct SpreadEntry {
  uint32_t topic;
  uint32_t strip0;  // the entry's first strip (entry n: n_strips)
  uint32_t c_t;     // the topic's messages in the window (0: the entry takes no part)
  uint32_t nbase;   // the topic's first node (its root) in node space
  uint32_t nn;      // its nodes, the root included
  uint32_t n0;      // the entry's first word of k / hop
  uint32_t mesh;    // 1: a mesh in the window's node space (k_spread_unreached counts its unreached nodes)
  uint32_t pad;
};
struct SpreadItem {
  uint32_t entry, node;  // a frontier node, topic-relative
};
struct SpreadArgs {
  const AudStrip* strips;
  uint32_t n_strips;
  const SpreadEntry* entries;  // [n + 1]
  uint32_t n;
  const uint8_t* verdict;    // AudArgs::verdict after k_audience_classify
  const uint64_t* n_exc;     // AudArgs::n_exc: 0 = every node of the strip is full
  uint32_t count_rows;       // 1: a full row is counted from its words too (the PSAMD_LOAD_COUNT seam)
  uint32_t wide;             // child entries from which an item is walked by the wave
  const uint32_t* node_peer;
  const uint32_t* row_ptr;
  const uint32_t* col;
  uint32_t n_edges, n_peers;
  uint32_t* k;               // per-node words
  uint32_t* hop;
  SpreadItem* queue;         // [2][q_cap]
  uint32_t q_cap;
  uint32_t* cnt;             // [3] items of the queues, by launch % 3
  uint64_t* reached;         // [n][kHopsCols] each, added into
  uint64_t* deliv;
  uint64_t* unreached;       // [n] each, added into
  uint64_t* holders;         // nodes with k > 0
  uint64_t* visited;
  uint64_t* recv;            // [n_peers] each; recv and copies added into, dup written
  uint64_t* copies;
  uint64_t* dup;
};
hipError_t launch_spread_nodes(const DrainArgs& a, const SpreadArgs& g, hipStream_t s);
hipError_t launch_spread_unreached(const SpreadArgs& g, hipStream_t s);
// k_spread_level for level `level` on `blocks` blocks
hipError_t launch_spread_level(const SpreadArgs& g, uint32_t level, uint32_t blocks, hipStream_t s);
hipError_t launch_spread_sum(const SpreadArgs& g, hipStream_t s);
hipError_t launch_spread_dup(const SpreadArgs& g, hipStream_t s);
// ps_spread_track: a tracked window enqueues its level
// launches 0 .. n_levels - 1 whole, with no read of the frontier count between them.
//   k_spread_track_close  behind the last of them, one thread: the count of the
//                   frontier launch n_levels would have read, cnt[n_levels % 3];
//                   not zero: the BFS was cut short, 1 added to *truncated.
//                   The three counts are left zero.  One writer per word,
//                   ordered by the stream alone.
hipError_t launch_spread_track_close(uint32_t* cnt, uint32_t n_levels, uint64_t* truncated, hipStream_t s);

}  // namespace psamd

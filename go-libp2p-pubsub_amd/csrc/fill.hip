// fill.hip -- a bulk chain launch of a single-start window as reach + fill
// (DESIGN.md §5.1d).  Every reached node's row is its topic root's seeded row
// and an unreached node's row is zeros, so the rows of the launch's levels
// need no copy down the subtrees: k_fill_reach decides reach from metadata
// alone (one lane per node), stamps generations and adds the counters the
// chain launch would have added; k_fill_rows writes each topic's contiguous
// range of rows front to back, one line-aligned piece per wave, from the
// root row held in LDS.  Reference: subtree.forwardMessage
// (subtree.go:319-354).
#include <cstddef>

#include "devutil.hpp"
#include "kernels.hpp"

namespace psamd {

namespace {

using namespace dev;

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// The launch's pieces from its segments: piece i belongs to the last segment
// whose first piece is <= i (segments hold at least one node).
__global__ __launch_bounds__(kBlock) void k_fill_pieces(const FillSeg* __restrict__ segs, uint32_t n_segs,
                                                        FillPiece* __restrict__ pieces, uint32_t n_pieces) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_pieces) return;
  uint32_t lo = 0, hi = n_segs;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (segs[mid].piece0 <= i)
      lo = mid;
    else
      hi = mid;
  }
  pieces[i] = fill_piece(segs[lo], i - segs[lo].piece0);
}

// pop[topic]: the set bits of the topic root's seeded row (one wave per segment).
__global__ __launch_bounds__(64) void k_fill_popc(const FillSeg* __restrict__ segs, uint32_t n_segs,
                                                  const uint64_t* __restrict__ a_cur, uint32_t* __restrict__ pop) {
  const uint32_t si = blockIdx.x;
  if (si >= n_segs) return;
  const uint64_t* row = a_cur + segs[si].row0;
  const uint32_t W = segs[si].W;
  uint32_t n = 0;
  for (uint32_t i = threadIdx.x; i < W; i += 64) n += static_cast<uint32_t>(__popcll(row[i]));
  n = __reduce_add_sync(~0ull, n);
  if (threadIdx.x == 0) pop[segs[si].topic] = n;
}

__device__ __forceinline__ uint64_t* fill_slots(const FillReachArgs& a, uint32_t i) {
  switch (i) {
    case 0: return a.partials_r[0];
    case 1: return a.partials_r[1];
    case 2: return a.partials_r[2];
    case 3: return a.partials_r[3];
    case 4: return a.partials_r[4];
    default: return a.partials_r[5];
  }
}

// Reach of every node of the launch's levels, one lane per node: u of level
// d + k is reached iff it and its k ancestors inside the launch are live and
// its ancestor of level d - 1 was reached this window (generation current:
// the chain launch's rule for its runs' parents).  Stamps the generation of a
// reached node and counts, per level, what the chain launch counts: nodes,
// nodes reached, their row words and deliveries, and reached parents (a
// parent counts at its first child).  The parent words read are the root
// row's, once per segment.
__global__ __launch_bounds__(kFillReachBlock) void k_fill_reach(FillReachArgs a) {
  const uint32_t b = blockIdx.x;
  uint32_t lo = 0, hi = a.n_segs;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a.segs[mid].blk0 <= b)
      lo = mid;
    else
      hi = mid;
  }
  const FillSeg* const S = a.segs + lo;
  const uint32_t levels = S->levels, W = S->W, cur = a.gen_cur & 0xFF;
  const uint32_t u0 = S->first[0], end = S->first[levels];
  const uint32_t u = u0 + (b - S->blk0) * kFillReachBlock + threadIdx.x;
  const bool in = u < end;
  const uint32_t uc = in ? u : u0;
  uint32_t k = 0;
  for (uint32_t j = 1; j < kChainLevels; ++j) k += (j < levels && uc >= S->first[j]) ? 1u : 0u;
  const uint32_t par = a.node_parent[uc];
  const uint32_t par_prev = a.node_parent[uc - 1];  // (level d >= 1: uc - 1 is a node of the topic)
  const bool live = a.node_flags[uc] & kNodeLive;
  uint32_t p = par;
  bool live_above = true;
  for (uint32_t j = 0; j < k; ++j) {
    live_above = live_above && (a.node_flags[p] & kNodeLive);
    p = a.node_parent[p];
  }
  const bool up = in && live_above && a.gen[p] == cur;
  const bool ok = up && live;
  const bool first = up && par != par_prev;
  if (ok) a.gen[uc] = static_cast<uint8_t>(cur);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t slot = (static_cast<uint64_t>(b) * (kFillReachBlock / 64) + wave) % a.slot_mod;
  const uint64_t pop = a.pop[S->topic];
  for (uint32_t j = 0; j < levels; ++j) {
    const uint64_t nodes = __ballot(in && k == j);
    if (nodes == 0) continue;
    const uint64_t reached = __popcll(__ballot(ok && k == j));
    const uint64_t parents = __popcll(__ballot(first && k == j));
    const uint64_t pwords = (j == 0 && b == S->blk0 && wave == 0) ? W : 0u;
    const uint64_t v7[7] = {reached * pop, reached * W, static_cast<uint64_t>(__popcll(nodes)), reached, parents,
                            pwords, 0ull};
    uint64_t* const partials = fill_slots(a, j);
    if (partials && lane < kNumCtr) {
      const uint64_t v = pull_ctr_pick(v7, lane);
      if (v) atomicAdd(reinterpret_cast<unsigned long long*>(partials + slot * kNumCtr + lane),
                       static_cast<unsigned long long>(v));
    }
  }
}

template <bool kNT>
__device__ __forceinline__ void fill_store16(uint64_t* p, const u32x4& v) {
  if constexpr (kNT)
    __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p));
  else
    *reinterpret_cast<u32x4*>(p) = v;
}

// One piece per wave: the root row and the generation bytes of the piece's
// nodes into LDS in one batch (one round trip after the descriptor), then the
// piece's words in order -- word r of the row for a reached node, zero for an
// unreached one (stale under its old generation byte, never read) -- as 16-B
// units, 8 stores of 1 KB in flight; a piece's odd first or last word goes as
// one 8-B store (only a segment's first and last pieces can have one).
template <bool kNT>
__global__ __launch_bounds__(64) void k_fill_rows(const FillPiece* __restrict__ pieces, uint32_t n_pieces,
                                                  const uint64_t* __restrict__ a_cur, uint64_t* __restrict__ seen,
                                                  const uint8_t* __restrict__ gen, uint32_t gen_cur) {
  constexpr uint32_t kU = 8;
  constexpr uint32_t kGenWords = (kFillPieceNodes + 2 + 3) / 4 + 2;  // a piece's nodes, from a dword boundary
  __shared__ __attribute__((aligned(16))) uint64_t row[kChainWords];
  __shared__ uint32_t genl[kGenWords];
  if (blockIdx.x >= n_pieces) return;
  const FillPiece* const pc = pieces + blockIdx.x;
  const uint32_t lane = threadIdx.x;
  const uint32_t cur = gen_cur & 0xFF;
  const uint64_t w0 = pc->w0;
  const uint32_t nw = pc->nw, W = pc->W, node0 = pc->node0, off0 = pc->off0;
  const uint64_t* const src = a_cur + pc->row0;
  const uint32_t nn = (off0 + nw + W - 1) / W;  // nodes with a word in the piece
  const uint32_t g0 = node0 & ~3u;
  const uint32_t nd = (((node0 + nn + 3u) & ~3u) - g0) >> 2;
  const uint32_t* const gen32 = reinterpret_cast<const uint32_t*>(gen + g0);
  for (uint32_t i = lane; i < nd; i += 64) genl[i] = gen32[i];
  for (uint32_t i = lane; i < W; i += 64) row[i] = src[i];
  __syncthreads();
  const uint8_t* const genb = reinterpret_cast<const uint8_t*>(genl) + (node0 - g0);
  const float rw = 1.0f / static_cast<float>(W);
  // word i of the piece -> (node kk of the piece, word r of its row); off0 + i < 2^24
  auto split = [&](uint32_t i, int32_t& kk, int32_t& r) {
    const uint32_t li = off0 + i;
    kk = static_cast<int32_t>(static_cast<float>(li) * rw);
    r = static_cast<int32_t>(li) - kk * static_cast<int32_t>(W);
    const int32_t lo = r < 0, hi = r >= static_cast<int32_t>(W);
    kk += hi - lo;
    r += (lo - hi) * static_cast<int32_t>(W);
  };
  auto word = [&](uint32_t i) {
    int32_t kk, r;
    split(i, kk, r);
    return genb[kk] == cur ? row[r] : 0ull;
  };
  uint64_t* const out = seen + w0;
  const uint32_t h = static_cast<uint32_t>(w0 & 1u);  // an odd first word: units start at word 1
  const uint32_t nu = (nw - h) >> 1;
  if (h && lane == 0) out[0] = word(0);
  if (((nw - h) & 1u) && lane == 1) out[nw - 1] = word(nw - 1);
  // even rows from an even word: a unit never straddles two rows
  const bool even = !(W & 1u) && !((off0 + h) & 1u);
  for (uint32_t c0 = 0; c0 < nu; c0 += kU * 64) {
    u32x4 x[kU];
#pragma unroll
    for (uint32_t q = 0; q < kU; ++q) {
      const uint32_t c = min(c0 + q * 64 + lane, nu - 1);  // (lanes past the end repeat the last unit)
      int32_t kk, r;
      split(h + 2 * c, kk, r);
      if (even) {
        x[q] = genb[kk] == cur ? *reinterpret_cast<const u32x4*>(row + r) : u32x4{0, 0, 0, 0};
      } else {
        const uint64_t a0 = genb[kk] == cur ? row[r] : 0ull;
        const bool wrap = static_cast<uint32_t>(r) + 1 == W;
        const uint64_t a1 = genb[kk + (wrap ? 1 : 0)] == cur ? row[wrap ? 0 : r + 1] : 0ull;
        x[q] = u32x4{static_cast<uint32_t>(a0), static_cast<uint32_t>(a0 >> 32), static_cast<uint32_t>(a1),
                     static_cast<uint32_t>(a1 >> 32)};
      }
    }
#pragma unroll
    for (uint32_t q = 0; q < kU; ++q) {
      const uint32_t c = c0 + q * 64 + lane;
      if (c < nu) fill_store16<kNT>(out + h + 2 * c, x[q]);
    }
  }
}

}  // namespace

hipError_t launch_fill_pieces(const FillSeg* segs, uint32_t n_segs, FillPiece* pieces, uint32_t n_pieces,
                              hipStream_t s) {
  if (n_segs == 0 || n_pieces == 0) return hipSuccess;
  hipLaunchKernelGGL(k_fill_pieces, dim3((n_pieces + kBlock - 1) / kBlock), dim3(kBlock), 0, s, segs, n_segs, pieces,
                     n_pieces);
  return hipGetLastError();
}

hipError_t launch_fill_popc(const FillSeg* segs, uint32_t n_segs, const uint64_t* a_cur, uint32_t* pop, hipStream_t s) {
  if (n_segs == 0) return hipSuccess;
  hipLaunchKernelGGL(k_fill_popc, dim3(n_segs), dim3(64), 0, s, segs, n_segs, a_cur, pop);
  return hipGetLastError();
}

hipError_t launch_fill_reach(const FillReachArgs& a, uint32_t n_blocks, hipStream_t s) {
  if (a.n_segs == 0 || n_blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(k_fill_reach, dim3(n_blocks), dim3(kFillReachBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_fill_rows(const FillPiece* pieces, uint32_t n_pieces, const uint64_t* a_cur, uint64_t* seen,
                            const uint8_t* gen, uint32_t gen_cur, uint32_t waves_per_cu, hipStream_t s) {
  if (n_pieces == 0) return hipSuccess;
  // at most waves_per_cu resident waves per CU through an LDS pad (160 KB of
  // LDS per CU, 512-B granules), as the chain launch's other caps; 0: no cap
  static const size_t fixed = [] {
    hipFuncAttributes fa{};
    return hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(k_fill_rows<false>)) == hipSuccess
               ? fa.sharedSizeBytes
               : size_t{0};
  }();
  size_t pad = 0;
  if (waves_per_cu) {
    const size_t per = (160u * 1024u) / waves_per_cu - 512u;
    pad = per > fixed ? per - fixed : 0;
  }
  hipLaunchKernelGGL(k_fill_rows<false>, dim3(n_pieces), dim3(64), pad, s, pieces, n_pieces, a_cur, seen, gen, gen_cur);
  return hipGetLastError();
}

}  // namespace psamd

// chain_write_probe.hip -- is k_pull_chain's write pattern itself slower
// than a plain write stream on MI355X?  (profiles/r04: the bulk chain launch
// writes 3.6 GB of rows at 4.5 TB/s, the one-shot 8-KB probe reaches ~6.)
// Each one-wave workgroup writes L segments, segment k of S_k bytes at
// region_k + w * S_k (the chain's level streams: a run's rows, its children's,
// ...), 16 B per lane, 1 KB per store instruction, the data from LDS as the
// chain's stage stream reads it.  Variants: the segments' sizes and count,
// non-temporal or plain stores, LDS per wave (residency), and one contiguous
// segment per wave (the one-shot probe) for reference.
//   hipcc -O3 --offload-arch=gfx950 chain_write_probe.hip -o cwp && ./cwp
// ./cwp <MiB> 1: the table of k_fill_shape only (a chain launch as reach +
// fill): pieces of 8-128 KB, default and nt stores, 8, 12 and
// 16 one-wave workgroups per CU, and hipMemsetAsync (profiles/chain_fill/probe.txt).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x)                                                                          \
  do {                                                                                 \
    hipError_t e_ = (x);                                                               \
    if (e_ != hipSuccess) {                                                            \
      std::fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_));   \
      std::exit(1);                                                                    \
    }                                                                                  \
  } while (0)

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

struct Seg {
  unsigned long long base[6];  // region of segment k (bytes)
  unsigned size[6];            // bytes per wave (multiple of 1 KB)
  int n;
};

template <bool kNT>
__global__ __launch_bounds__(64) void k_segs(char* __restrict__ out, Seg sg) {
  extern __shared__ u32x4 lds[];  // >= 64 x 16 B used; the rest pads residency
  const unsigned lane = threadIdx.x;
  lds[lane] = u32x4{lane, blockIdx.x, 1u, 2u};
  __syncthreads();
  const unsigned long long w = blockIdx.x;
  for (int k = 0; k < sg.n; ++k) {
    u32x4* o = reinterpret_cast<u32x4*>(out + sg.base[k] + w * sg.size[k]);
    const unsigned units = sg.size[k] / 16;
    for (unsigned i0 = 0; i0 < units; i0 += 8 * 64) {
      u32x4 x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) x[u] = lds[(lane + u) & 63];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const unsigned i = i0 + u * 64 + lane;
        if (i < units) {
          if constexpr (kNT)
            __builtin_nontemporal_store(x[u], o + i);
          else
            o[i] = x[u];
        }
      }
    }
  }
}

// The fill's shape (a bulk chain launch as reach + fill): the
// launch's rows are one contiguous range of nodes, every reached node's row is
// the topic's root row, an unreached one's is zeros.  Each one-wave workgroup
// writes one contiguous piece of the range: it copies the row (row_units
// 16-B units; 165 = cfg3's 330-word hot topic) into LDS, reads the generation
// bytes of the piece's nodes in one batch (one per lane: a piece holds at most
// 64 rows), and streams unit i as the row's unit i mod row_units or zero, 8
// stores in flight.
template <bool kNT>
__global__ __launch_bounds__(64) void k_fill_shape(u32x4* __restrict__ out, const u32x4* __restrict__ row,
                                                   const unsigned char* __restrict__ gen, unsigned cur,
                                                   unsigned row_units, unsigned piece_units,
                                                   unsigned long long total_units) {
  extern __shared__ u32x4 lds[];  // >= row_units x 16 B used; the rest pads residency
  const unsigned lane = threadIdx.x;
  const unsigned long long u0 = static_cast<unsigned long long>(blockIdx.x) * piece_units;
  if (u0 >= total_units) return;
  const unsigned long long left = total_units - u0;
  const unsigned units = left < piece_units ? static_cast<unsigned>(left) : piece_units;
  const unsigned long long node0 = u0 / row_units;
  const unsigned long long node1 = (u0 + units - 1) / row_units;  // node1 - node0 < 64
  const unsigned char g = node0 + lane <= node1 ? gen[node0 + lane] : 0;
  for (unsigned i = lane; i < row_units; i += 64) lds[i] = row[i];
  __syncthreads();
  const unsigned long long reach = __ballot(g == cur);
  unsigned n = static_cast<unsigned>((u0 + lane) / row_units - node0);
  unsigned off = static_cast<unsigned>((u0 + lane) % row_units);
  u32x4* o = out + u0;
  for (unsigned i0 = 0; i0 < units; i0 += 8 * 64) {
    u32x4 x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      x[u] = (reach >> n) & 1 ? lds[off] : u32x4{0, 0, 0, 0};
      off += 64;
      while (off >= row_units) off -= row_units, ++n;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const unsigned i = i0 + u * 64 + lane;
      if (i < units) {
        if constexpr (kNT)
          __builtin_nontemporal_store(x[u], o + i);
        else
          o[i] = x[u];
      }
    }
  }
}

int main(int argc, char** argv) {
  const size_t total = (argc > 1 ? std::atoll(argv[1]) : 3600) * (1ull << 20);  // bytes per launch
  char* buf = nullptr;
  CK(hipMalloc(&buf, total + (64ull << 20)));
  hipEvent_t a, b;
  CK(hipEventCreate(&a));
  CK(hipEventCreate(&b));
  auto run_fill = [&](unsigned piece_kb, bool nt, unsigned per_cu) {
    const unsigned row_units = 165, cur = 7;
    const unsigned long long total_units = total / 16;
    const unsigned piece_units = piece_kb * 64;
    const size_t nodes = static_cast<size_t>(total_units / row_units) + 2;
    static unsigned char* gen = nullptr;
    static u32x4* row = nullptr;
    if (!gen) {  // every 97th node unreached, the rest stamped with the window's generation
      std::vector<unsigned char> h(nodes);
      for (size_t i = 0; i < nodes; ++i) h[i] = i % 97 ? cur : cur - 1;
      CK(hipMalloc(&gen, nodes));
      CK(hipMemcpy(gen, h.data(), nodes, hipMemcpyHostToDevice));
      std::vector<u32x4> r(row_units);
      for (unsigned i = 0; i < row_units; ++i) r[i] = u32x4{i, ~i, i * 3u, 5u};
      CK(hipMalloc(&row, row_units * sizeof(u32x4)));
      CK(hipMemcpy(row, r.data(), row_units * sizeof(u32x4), hipMemcpyHostToDevice));
    }
    const size_t lds = (160u * 1024u) / per_cu - 512u;  // per_cu one-wave workgroups fit per CU
    const unsigned waves = static_cast<unsigned>((total_units + piece_units - 1) / piece_units);
    float best = 1e30f, worst = 0;
    for (int rep = 0; rep < 6; ++rep) {
      CK(hipEventRecord(a));
      if (nt)
        hipLaunchKernelGGL(k_fill_shape<true>, dim3(waves), dim3(64), lds, 0, reinterpret_cast<u32x4*>(buf), row, gen,
                           cur, row_units, piece_units, total_units);
      else
        hipLaunchKernelGGL(k_fill_shape<false>, dim3(waves), dim3(64), lds, 0, reinterpret_cast<u32x4*>(buf), row, gen,
                           cur, row_units, piece_units, total_units);
      CK(hipEventRecord(b));
      CK(hipEventSynchronize(b));
      float ms = 0;
      CK(hipEventElapsedTime(&ms, a, b));
      if (rep && ms < best) best = ms;
      if (rep && ms > worst) worst = ms;
    }
    std::printf("fill piece=%3u KB nt=%d per-CU=%2u waves=%7u: %7.1f us (worst %7.1f)  %.2f TB/s\n", piece_kb, nt ? 1 : 0,
                per_cu, waves, best * 1e3, worst * 1e3, static_cast<double>(total) / (best * 1e-3) / 1e12);
    std::fflush(stdout);
  };
  if (argc > 2 && std::atoi(argv[2]) == 1) {  // the fill's table only
    for (unsigned per_cu : {8u, 12u, 16u})
      for (bool nt : {false, true})
        for (unsigned kb : {8u, 16u, 32u, 64u, 128u}) run_fill(kb, nt, per_cu);
    float best = 1e30f;
    for (int rep = 0; rep < 6; ++rep) {
      CK(hipEventRecord(a));
      CK(hipMemsetAsync(buf, 3, total, 0));
      CK(hipEventRecord(b));
      CK(hipEventSynchronize(b));
      float ms = 0;
      CK(hipEventElapsedTime(&ms, a, b));
      if (rep && ms < best) best = ms;
    }
    std::printf("hipMemsetAsync: %7.1f us  %.2f TB/s\n", best * 1e3, static_cast<double>(total) / (best * 1e-3) / 1e12);
    return 0;
  }
  auto run = [&](const char* name, std::vector<unsigned> sizes, bool nt, size_t lds) {
    Seg sg{};
    sg.n = static_cast<int>(sizes.size());
    unsigned per = 0;
    for (unsigned s : sizes) per += s;
    const unsigned waves = static_cast<unsigned>(total / per);
    unsigned long long off = 0;
    for (int k = 0; k < sg.n; ++k) {
      sg.base[k] = off;
      sg.size[k] = sizes[k];
      off += static_cast<unsigned long long>(sizes[k]) * waves;
      off = (off + 4095) & ~4095ull;
    }
    float best = 1e30f;
    for (int rep = 0; rep < 6; ++rep) {
      CK(hipEventRecord(a));
      if (nt)
        hipLaunchKernelGGL(k_segs<true>, dim3(waves), dim3(64), lds, 0, buf, sg);
      else
        hipLaunchKernelGGL(k_segs<false>, dim3(waves), dim3(64), lds, 0, buf, sg);
      CK(hipEventRecord(b));
      CK(hipEventSynchronize(b));
      float ms = 0;
      CK(hipEventElapsedTime(&ms, a, b));
      if (rep && ms < best) best = ms;
    }
    const double bytes = static_cast<double>(per) * waves;
    std::printf("%-34s nt=%d lds=%6zu waves=%7u per-wave=%6u B: %7.1f us  %.2f TB/s\n", name, nt ? 1 : 0, lds, waves,
                per, best * 1e3, bytes / (best * 1e-3) / 1e12);
    std::fflush(stdout);
  };
  for (bool nt : {true, false})
    for (size_t lds : {1024ul, 9472ul, 20480ul}) {
      run("chain 2.6K,5.3K,10.6K,21K,2K", {2688, 5376, 10752, 21504, 2048}, nt, lds);
      run("one segment 42K", {42368}, nt, lds);
      run("one segment 8K", {8192}, nt, lds);
      run("chain small 1K,2K,4K,8K,1K", {1024, 2048, 4096, 8192, 1024}, nt, lds);
    }
  return 0;
}

// Calibrated per-junction error bounds (estimation.PressureEstimator.calibrate_bounds / coverage_report): split-conformal
// calibration needs, per node, ONE order statistic per level of |estimate - truth| over the snapshots of a held-out store.
//   gatres_node_error_quantiles  the exact r-th smallest |e| per column of an [S][N] error matrix that is never formed, for up to
//                                GATRES_NODE_QUANTILE_MAX_LEVELS levels in one launch;
//   gatres_node_bound_coverage   per node, how many of its counted entries lie inside each bound.
// e is the e of gatres_node_error_moments (k_estimate.hip): fp32(est - D(truth)), no contraction; with `available` only the
// hidden entries are counted, as in gatres_node_error_moments_available.
//
// The select is an MSB-first radix select on the 32-bit pattern of fabsf(e) (as unsigned integers that is the IEEE order, with
// NaN above +inf and one zero), eight bits per pass, four passes.  Every pass re-reads est and truth and re-forms e: the two
// matrices of a calibration store (a few MB) stay in L2 / Infinity Cache, a scratch copy of |e| would cost a write and a read of
// the same size and a buffer the caller has to own.  Parallelism is over nodes only (one launch, no global atomics, no scratch),
// and a pass is bound by the latency of its trips over the rows, not by bytes: so a workgroup takes few nodes -- BQ_G = 8, 49
// workgroups at 388 nodes -- and many rows at a time.
//
// LDS plan: hist[level][node][bin] of uint32 with a node stride of BQ_BINS + 1 = 257 dwords, so the bank of (node, bin) is
// (node + bin) mod 32: the lanes of a 32-lane group that hold different nodes and the SAME bin (the common case: the errors of
// neighbouring junctions share their exponent) hit different banks, and a wave that walks the bins of one node reads
// consecutive dwords.  The waves add with LDS atomic adds; the counts are integers, so the result does not depend on their
// order.  Pass 0 has no prefix yet and fills one histogram whatever Q is; from then on every live level has its own, and an
// entry is added to those whose prefix its upper bits equal.  Q * 8 224 B, 64.3 KB at Q = 8.
#include "gatres_common.h"

namespace {

constexpr int BQ_G = 8;                        // nodes of a workgroup
constexpr int BQ_WAVES = 16;
constexpr int BQ_T = BQ_WAVES * GATRES_WAVE;
constexpr int BQ_SLOTS = BQ_T / BQ_G;          // rows a workgroup takes side by side
constexpr int BQ_WPN = BQ_WAVES / BQ_G;        // waves that walk one node: they split its levels
constexpr int BQ_U = 4;                        // rows in flight per thread and trip
constexpr int BQ_BITS = 8, BQ_BINS = 1 << BQ_BITS, BQ_PASSES = 32 / BQ_BITS;
constexpr int BQ_STRIDE = BQ_BINS + 1;         // dwords between the histograms of two nodes
constexpr int BQ_MAXQ = GATRES_NODE_QUANTILE_MAX_LEVELS;
static_assert(BQ_WAVES % BQ_G == 0 && GATRES_WAVE % BQ_G == 0 && BQ_BINS == 4 * GATRES_WAVE, "the walk: four bins per lane");

struct BqLevels { double q[BQ_MAXQ]; };

constexpr size_t bq_lds_bytes(int Q) {
  return 4 * ((size_t)Q * BQ_G * BQ_STRIDE + (size_t)2 * BQ_G * BQ_MAXQ + 2 * BQ_G);
}

// The counted entry's key: the pattern of fabsf(e)
__device__ __forceinline__ uint32_t bq_key(float p, float t, float scale, float offset) {
  return __float_as_uint(fabsf(__fsub_rn(p, gatres_descale(t, scale, offset))));
}

// Inclusive sum over the lanes 0 .. lane of a wave
__device__ __forceinline__ uint32_t bq_scan(uint32_t c, int lane) {
#pragma unroll
  for (int off = 1; off < GATRES_WAVE; off <<= 1) {
    const uint32_t t = __shfl_up(c, off, GATRES_WAVE);
    if (lane >= off) c += t;
  }
  return c;
}

// The whole wave walks the BQ_BINS bins of one histogram h: the bin that holds the r-th smallest entry (1-based, r <= the
// histogram's total) and r less the entries in the bins below it.  r and the results are uniform over the wave.
__device__ __forceinline__ uint32_t bq_walk(const uint32_t* h, int lane, uint32_t& r) {
  uint32_t base = 0;
  for (int j = 0; j < BQ_BINS / GATRES_WAVE; ++j) {
    const uint32_t c = h[j * GATRES_WAVE + lane];
    const uint32_t incl = bq_scan(c, lane);
    const uint32_t tot = __shfl(incl, GATRES_WAVE - 1, GATRES_WAVE);
    if (r <= base + tot) {
      const int L = __ffsll((unsigned long long)__ballot(base + incl >= r)) - 1;
      r -= base + __shfl(incl - c, L, GATRES_WAVE);
      return (uint32_t)(j * GATRES_WAVE + L);
    }
    base += tot;
  }
  return BQ_BINS - 1;                          // (not reached: r <= total)
}

// Workgroup b takes the nodes [8 b, 8 b + 8).  Element side: lane l of wave w is node 8 b + l % 8 in row slot 8 w + l / 8 of
// BQ_SLOTS = 128, so eight lanes read 32 consecutive bytes of a row and a thread takes the rows slot, slot + 128, ..., BQ_U of
// them in flight.  Walk side: the waves w and w + 8 are node 8 b + w % 8 and take its even and its odd levels.  Per pass: zero
// the histograms, add every counted entry whose upper bits equal a live prefix of its node, walk.
// The first pass gives n_v and with it the ranks; a level with r > n_v is dead from then on (rank 0: +inf).
template <bool AVAIL>
__global__ __launch_bounds__(BQ_T) void node_error_quantiles_kernel(const float* __restrict__ est, const float* __restrict__ truth,
                                                                    long long S, int N, float scale, float offset,
                                                                    const int* __restrict__ observed, int K,
                                                                    const uint8_t* __restrict__ available, BqLevels lv, int Q,
                                                                    float* __restrict__ bounds, double* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) unsigned char bq_smem[];
  uint32_t* hist = reinterpret_cast<uint32_t*>(bq_smem);                 // [Q][BQ_G][BQ_STRIDE]
  uint32_t* st_pref = hist + (size_t)Q * BQ_G * BQ_STRIDE;               // [BQ_G][BQ_MAXQ]: the prefix of (node, level) so far
  uint32_t* st_rank = st_pref + BQ_G * BQ_MAXQ;                          // [BQ_G][BQ_MAXQ]: its rank among the entries under the prefix
  uint32_t* st_n = st_rank + BQ_G * BQ_MAXQ;                             // [BQ_G]: n_v
  int* seen = reinterpret_cast<int*>(st_n + BQ_G);                       // [BQ_G]: k + 1 of the sensor at the node
  const int tid = threadIdx.x, lane = tid % GATRES_WAVE, wave = tid / GATRES_WAVE;
  const int v_lo = blockIdx.x * BQ_G, node = lane % BQ_G, v = v_lo + node;
  const long long slot = wave * (GATRES_WAVE / BQ_G) + lane / BQ_G;
  const int w_node = wave % BQ_G, w_part = wave / BQ_G;
  int sensor = -1;
  if (AVAIL) {
    if (tid < BQ_G) seen[tid] = 0;
    __syncthreads();
    for (int k = tid; k < K; k += BQ_T) {
      const int o = observed[k];
      if (o >= v_lo && o < v_lo + BQ_G) seen[o - v_lo] = k + 1;
    }
    __syncthreads();
    sensor = seen[node] - 1;
  }
#pragma unroll 1
  for (int pass = 0; pass < BQ_PASSES; ++pass) {
    const int nh = pass == 0 ? 1 : Q;
    for (int i = tid; i < nh * BQ_G * BQ_STRIDE; i += BQ_T) hist[i] = 0;
    __syncthreads();                             // (the histograms are zero, the walk's state is that of the last pass)
    uint32_t pf[BQ_MAXQ];
    unsigned live = 1;                           // the levels of the node that are still sought (pass 0: one histogram for all)
    if (pass) {
      live = 0;
#pragma unroll
      for (int q = 0; q < BQ_MAXQ; ++q) {
        pf[q] = st_pref[node * BQ_MAXQ + q];
        if (q < Q && st_rank[node * BQ_MAXQ + q]) live |= 1u << q;
      }
    }
    const int sh = 32 - BQ_BITS * (pass + 1);                // the pass's digit: bits [sh, sh + 8)
    if (v < N && live) {
      uint32_t* hn = hist + node * BQ_STRIDE;
      for (long long s0 = slot; s0 < S; s0 += (long long)BQ_U * BQ_SLOTS) {
        float p[BQ_U], t[BQ_U];
        uint8_t av[BQ_U] = {};
#pragma unroll
        for (int u = 0; u < BQ_U; ++u) {
          const long long s = s0 + (long long)u * BQ_SLOTS;
          p[u] = s < S ? est[s * N + v] : 0.f;
          t[u] = s < S ? truth[s * N + v] : 0.f;
        }
        if (AVAIL && sensor >= 0) {               // (a row past the end reads the last row's byte, which the loop below skips)
#pragma unroll
          for (int u = 0; u < BQ_U; ++u) {
            const long long s = s0 + (long long)u * BQ_SLOTS;
            av[u] = available[(s < S ? s : S - 1) * K + sensor];
          }
        }
#pragma unroll
        for (int u = 0; u < BQ_U; ++u) {
          if (s0 + (long long)u * BQ_SLOTS >= S) continue;
          if (AVAIL && av[u]) continue;
          const uint32_t key = bq_key(p[u], t[u], scale, offset);
          const uint32_t d = (key >> sh) & (BQ_BINS - 1);
          if (pass == 0) {
            atomicAdd(hn + d, 1u);
          } else {
            const uint32_t hi = key >> (sh + BQ_BITS);
#pragma unroll
            for (int q = 0; q < BQ_MAXQ; ++q)
              if (((live >> q) & 1u) && hi == pf[q]) atomicAdd(hn + (size_t)q * BQ_G * BQ_STRIDE + d, 1u);
          }
        }
      }
    }
    __syncthreads();
    // ---- the walk.  Its state lives in LDS; every value is uniform over the wave, and every lane stores it (the same bits to
    // one address), so a lane reads back what it has written itself; the other wave of the node sees it after a barrier.
    uint32_t* pref = st_pref + w_node * BQ_MAXQ;
    uint32_t* rank = st_rank + w_node * BQ_MAXQ;
    if (pass == 0) {
      const uint32_t* h = hist + w_node * BQ_STRIDE;
      uint32_t c = 0;
#pragma unroll
      for (int j = 0; j < BQ_BINS / GATRES_WAVE; ++j) c += h[j * GATRES_WAVE + lane];
      const uint32_t n = __shfl(bq_scan(c, lane), GATRES_WAVE - 1, GATRES_WAVE);
      for (int q = w_part; q < Q; q += BQ_WPN) {
        const double r = ceil((double)((unsigned long long)n + 1ULL) * lv.q[q]);
        rank[q] = r <= (double)n ? (uint32_t)r : 0u;          // (r >= 1: the level is positive)
        pref[q] = 0;
      }
      if (w_part == 0) st_n[w_node] = n;
    }
    for (int q = w_part; q < Q; q += BQ_WPN) {
      uint32_t r = rank[q];
      if (!r) continue;
      const uint32_t d = bq_walk(hist + ((size_t)(pass ? q : 0) * BQ_G + w_node) * BQ_STRIDE, lane, r);
      rank[q] = r;
      pref[q] = (pref[q] << BQ_BITS) | d;
    }
    __syncthreads();                             // (every wave has walked: the histograms may be zeroed)
  }
  if (tid < Q * BQ_G) {
    const int q = tid / BQ_G, nd = tid % BQ_G;
    const bool live = st_rank[nd * BQ_MAXQ + q] != 0;
    if (v_lo + nd < N) bounds[(size_t)q * N + v_lo + nd] = __uint_as_float(live ? st_pref[nd * BQ_MAXQ + q] : 0x7f800000u);
  }
  if (tid < BQ_G && v_lo + tid < N) counts[v_lo + tid] = (double)st_n[tid];
}

// ---- coverage ------------------------------------------------------------------------------------------------------------------
constexpr int BC_WAVES = 8;
constexpr int BC_T = BC_WAVES * GATRES_WAVE;
constexpr int BC_U = 8;
constexpr int BC_F = 1 + BQ_MAXQ;              // the counted entries and the hits per level

// The traversal of node_error_moments_kernel (k_estimate.hip): workgroup b takes the nodes [64 b, 64 b + 64), lane l of every
// wave node 64 b + l, wave w the rows w, w + 8, ... with BC_U of them in flight.  The counters are integers: the waves' partials
// are added through LDS and written as doubles.
template <bool AVAIL>
__global__ __launch_bounds__(BC_T) void node_bound_coverage_kernel(const float* __restrict__ est, const float* __restrict__ truth,
                                                                   long long S, int N, float scale, float offset,
                                                                   const int* __restrict__ observed, int K,
                                                                   const uint8_t* __restrict__ available,
                                                                   const float* __restrict__ bounds, int Q,
                                                                   double* __restrict__ table) {
  __shared__ uint32_t part[BC_WAVES][BC_F][GATRES_WAVE];
  __shared__ int seen[GATRES_WAVE];
  const int lane = threadIdx.x % GATRES_WAVE, wave = threadIdx.x / GATRES_WAVE;
  const int v_lo = blockIdx.x * GATRES_WAVE, v = v_lo + lane;
  int sensor = -1;
  if (AVAIL) {
    if (threadIdx.x < GATRES_WAVE) seen[threadIdx.x] = 0;
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += BC_T) {
      const int o = observed[k];
      if (o >= v_lo && o < v_lo + GATRES_WAVE) seen[o - v_lo] = k + 1;
    }
    __syncthreads();
    sensor = seen[lane] - 1;
  }
  uint32_t a[BC_F] = {};
  float b[BQ_MAXQ];
#pragma unroll
  for (int q = 0; q < BQ_MAXQ; ++q) b[q] = (q < Q && v < N) ? bounds[(size_t)q * N + v] : __uint_as_float(0x7fc00000u);
  if (v < N) {
    for (long long s0 = wave; s0 < S; s0 += (long long)BC_U * BC_WAVES) {
      float p[BC_U], t[BC_U];
      uint8_t av[BC_U] = {};
#pragma unroll
      for (int u = 0; u < BC_U; ++u) {
        const long long s = s0 + (long long)u * BC_WAVES;
        p[u] = s < S ? est[s * N + v] : 0.f;
        t[u] = s < S ? truth[s * N + v] : 0.f;
      }
      if (AVAIL && sensor >= 0) {
#pragma unroll
        for (int u = 0; u < BC_U; ++u) {
          const long long s = s0 + (long long)u * BC_WAVES;
          av[u] = available[(s < S ? s : S - 1) * K + sensor];
        }
      }
#pragma unroll
      for (int u = 0; u < BC_U; ++u) {
        if (s0 + (long long)u * BC_WAVES >= S) continue;
        if (AVAIL && av[u]) continue;
        const float ae = __uint_as_float(bq_key(p[u], t[u], scale, offset));
        a[0] += 1u;
#pragma unroll
        for (int q = 0; q < BQ_MAXQ; ++q) a[1 + q] += ae <= b[q] ? 1u : 0u;      // (false for a NaN on either side)
      }
    }
  }
#pragma unroll
  for (int f = 0; f < BC_F; ++f) part[wave][f][lane] = a[f];
  __syncthreads();
  if (wave == 0 && v < N) {
    double* rec = table + (size_t)v * BC_F;
#pragma unroll
    for (int f = 0; f < BC_F; ++f) {
      unsigned long long s = 0;
      for (int w = 0; w < BC_WAVES; ++w) s += part[w][f][lane];
      rec[f] = (double)s;
    }
  }
}

// What both entry points refuse about their inputs
static bool bq_inputs_ok(const float* est, const float* truth, int64_t S, int32_t N, const int32_t* observed, int32_t K,
                         const uint8_t* available, int32_t Q) {
  if (!est || !truth || S < 1 || N < 1 || Q < 1 || Q > BQ_MAXQ) return false;
  if (S > INT32_MAX || S > INT64_MAX / 4 / N) return false;       // (the histograms count in 32 bits)
  if (available && (!observed || K < 1 || K > N)) return false;
  return true;
}

// Does the output [out, out + bytes) overlap an input the launch reads?
static bool bq_output_overlaps(const void* out, uint64_t bytes, const float* est, const float* truth, int64_t S, int32_t N,
                               const int32_t* observed, int32_t K, const uint8_t* available) {
  const uint64_t mat = 4 * (uint64_t)S * (uint64_t)N;
  if (bytes_overlap(out, bytes, est, mat) || bytes_overlap(out, bytes, truth, mat)) return true;
  if (observed && K >= 1 && K <= N && bytes_overlap(out, bytes, observed, 4 * (uint64_t)K)) return true;
  if (available && bytes_overlap(out, bytes, available, (uint64_t)S * (uint64_t)K)) return true;
  return false;
}

}  // namespace

extern "C" int gatres_node_error_quantiles(const float* est, const float* truth, int64_t num_snapshots, int32_t nodes_per_graph,
                                           double scale, double offset, const int32_t* observed, int32_t num_observed,
                                           const uint8_t* available, const double* levels, int32_t num_levels, float* bounds,
                                           double* counts, void* stream) {
  if (!levels || !bounds || !counts) return GATRES_E_BADARG;
  if (!bq_inputs_ok(est, truth, num_snapshots, nodes_per_graph, observed, num_observed, available, num_levels)) return GATRES_E_BADARG;
  BqLevels lv = {};
  for (int q = 0; q < num_levels; ++q) {
    if (!(levels[q] > 0.0 && levels[q] < 1.0)) return GATRES_E_BADARG;          // (a NaN fails both comparisons)
    lv.q[q] = levels[q];
  }
  const uint64_t b_bytes = 4 * (uint64_t)num_levels * (uint64_t)nodes_per_graph, c_bytes = 8 * (uint64_t)nodes_per_graph;
  if (bytes_overlap(bounds, b_bytes, counts, c_bytes) ||
      bq_output_overlaps(bounds, b_bytes, est, truth, num_snapshots, nodes_per_graph, observed, num_observed, available) ||
      bq_output_overlaps(counts, c_bytes, est, truth, num_snapshots, nodes_per_graph, observed, num_observed, available))
    return GATRES_E_BADARG;
  const size_t lds = bq_lds_bytes(num_levels);
  if (lds > 64 * 1024) {                         // (the histograms of eight levels pass the 64 KB a kernel gets unasked; per device)
    const void* fn = available ? reinterpret_cast<const void*>(&node_error_quantiles_kernel<true>)
                               : reinterpret_cast<const void*>(&node_error_quantiles_kernel<false>);
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return (int)e;
    }
  }
  const dim3 grid((nodes_per_graph + BQ_G - 1) / BQ_G);
  if (available)
    hipLaunchKernelGGL(node_error_quantiles_kernel<true>, grid, dim3(BQ_T), lds, gatres_stream(stream), est, truth,
                       (long long)num_snapshots, (int)nodes_per_graph, (float)scale, (float)offset, observed, (int)num_observed,
                       available, lv, (int)num_levels, bounds, counts);
  else
    hipLaunchKernelGGL(node_error_quantiles_kernel<false>, grid, dim3(BQ_T), lds, gatres_stream(stream), est, truth,
                       (long long)num_snapshots, (int)nodes_per_graph, (float)scale, (float)offset, (const int*)nullptr, 0,
                       (const uint8_t*)nullptr, lv, (int)num_levels, bounds, counts);
  return gatres_launch_status();
}

extern "C" int gatres_node_bound_coverage(const float* est, const float* truth, int64_t num_snapshots, int32_t nodes_per_graph,
                                          double scale, double offset, const int32_t* observed, int32_t num_observed,
                                          const uint8_t* available, const float* bounds, int32_t num_levels, double* table,
                                          void* stream) {
  if (!bounds || !table) return GATRES_E_BADARG;
  if (!bq_inputs_ok(est, truth, num_snapshots, nodes_per_graph, observed, num_observed, available, num_levels)) return GATRES_E_BADARG;
  static_assert(BC_F == 1 + GATRES_NODE_QUANTILE_MAX_LEVELS, "record layout");
  const uint64_t t_bytes = 8 * (uint64_t)BC_F * (uint64_t)nodes_per_graph;
  if (bytes_overlap(table, t_bytes, bounds, 4 * (uint64_t)num_levels * (uint64_t)nodes_per_graph) ||
      bq_output_overlaps(table, t_bytes, est, truth, num_snapshots, nodes_per_graph, observed, num_observed, available))
    return GATRES_E_BADARG;
  const dim3 grid((nodes_per_graph + GATRES_WAVE - 1) / GATRES_WAVE);
  if (available)
    hipLaunchKernelGGL(node_bound_coverage_kernel<true>, grid, dim3(BC_T), 0, gatres_stream(stream), est, truth,
                       (long long)num_snapshots, (int)nodes_per_graph, (float)scale, (float)offset, observed, (int)num_observed,
                       available, bounds, (int)num_levels, table);
  else
    hipLaunchKernelGGL(node_bound_coverage_kernel<false>, grid, dim3(BC_T), 0, gatres_stream(stream), est, truth,
                       (long long)num_snapshots, (int)nodes_per_graph, (float)scale, (float)offset, (const int*)nullptr, 0,
                       (const uint8_t*)nullptr, bounds, (int)num_levels, table);
  return gatres_launch_status();
}

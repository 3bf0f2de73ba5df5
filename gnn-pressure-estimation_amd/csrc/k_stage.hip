// The staging launches: every launch of the mask sampler's own grid (k_mask.h: MASK_WGS workgroups of 1024 per graph), whose
// workgroups first put the batch into x (and y) and then sample the step's mask -- the copy's stores drain while the keys are
// ranked -- and the gather that collates without a mask.
//   gatres_mask_generate                    the sampler alone                                        } mask_generate_kernel
//   gatres_stage_batch_mask                 a flat copy of a device-resident batch, then the sampler }
//   gatres_stage_rows_mask                  collation of rows of ONE snapshot matrix [S][N], then the sampler
//   gatres_stage_rows_mask_required         ... then the sampler that always masks the required (sensor) nodes
//   gatres_stage_rows_mask_sensors          ... then, per graph, the mask of a FIXED sensor layout or the sampler's
//   gatres_stage_rows_mask_sensors_noisy    ... with measurement noise on the readings the layout keeps, drawn in the launch
//   gatres_stage_multi_rows_mask_required   collation from SEVERAL snapshot matrices (one per water network), required sampler
//   gatres_gather_multi_rows                that collation alone, for num_batches x num_graphs graphs in one launch
// A collated graph's row is contiguous in the source and in the destination: copy_row walks it 16 bytes per lane where the two
// starts allow it, and the row index, the pointer table and the index tables are read once per graph, by uniform (scalar) loads.
#include "gatres_common.h"
#include "k_mask.h"

namespace {

// dst[0 .. n) = src[0 .. n) (and dst2 likewise when given) by the threads `t` of `T` (of one or several workgroups): a scalar
// head up to dst's first 16-byte boundary, the body as float4 where src (and dst2) share dst's phase inside 16 bytes (float by
// float otherwise), a scalar tail.  n may be smaller than the head.
__device__ __forceinline__ void copy_row(const float* __restrict__ src, float* __restrict__ dst, float* __restrict__ dst2,
                                         int n, int t, int T) {
  const uintptr_t ps = reinterpret_cast<uintptr_t>(src), pd = reinterpret_cast<uintptr_t>(dst);
  const bool vec = ((ps ^ pd) & 15u) == 0 && (!dst2 || ((reinterpret_cast<uintptr_t>(dst2) ^ pd) & 15u) == 0);
  if (!vec) {
    for (int i = t; i < n; i += T) {
      const float s = src[i];
      dst[i] = s;
      if (dst2) dst2[i] = s;
    }
    return;
  }
  int head = (int)(((16u - (unsigned)(pd & 15u)) & 15u) >> 2);      // floats in front of the first 16-byte boundary
  if (head > n) head = n;
  const int nvec = (n - head) / 4, tail0 = head + 4 * nvec;
  for (int v = t; v < nvec; v += T) {
    const float4 r = ld4(src + head + 4 * v);
    st4(dst + head + 4 * v, r);
    if (dst2) st4(dst2 + head + 4 * v, r);
  }
  // (head and tail: at most 3 + 3 floats, taken by the first threads)
  if (t < head) {
    const float s = src[t];
    dst[t] = s;
    if (dst2) dst2[t] = s;
  }
  if (t < n - tail0) {
    const float s = src[tail0 + t];
    dst[tail0 + t] = s;
    if (dst2) dst2[tail0 + t] = s;
  }
}

// A graph's collation on the sampler's grid: the MASK_WGS * 1024 threads of the graph's workgroups (this one being `wq`) copy
// its row of n floats to x_dst + off, and to y_dst + off when y_dst is given and is another buffer.
__device__ __forceinline__ void collate_graph(const float* __restrict__ src, float* x_dst, float* y_dst, long long off, int n,
                                              int wq) {
  copy_row(src, x_dst + off, y_dst && y_dst != x_dst ? y_dst + off : nullptr, n, wq * 1024 + (int)threadIdx.x, MASK_WGS * 1024);
}

// ... from ONE snapshot matrix: graph g is row rows[g] of data[.][N] and goes to [g * N, (g + 1) * N).
__device__ __forceinline__ void collate_matrix_graph(const float* __restrict__ data, const long long* __restrict__ rows, int N,
                                                     float* x_dst, float* y_dst, int g, int wq) {
  collate_graph(data + rows[g] * (long long)N, x_dst, y_dst, (long long)g * N, N, wq);
}

// The sampler's own launch; gatres_stage_batch_mask's copy of the batch rides on it (two sources, no rows: a plain grid-stride
// loop).
__global__ __launch_bounds__(1024) void mask_generate_kernel(const int* __restrict__ node_ptr, double rate,
                                                             uint64_t seed, const uint64_t* __restrict__ step_counter,
                                                             uint8_t* __restrict__ mask,
                                                             const float* __restrict__ x_src, const float* __restrict__ y_src,
                                                             float* __restrict__ x_dst, float* __restrict__ y_dst,
                                                             long long num_nodes) {
  if (x_src && x_src != x_dst) {
    for (long long v = (long long)blockIdx.x * 1024 + threadIdx.x; v < num_nodes; v += (long long)gridDim.x * 1024) {
      x_dst[v] = x_src[v];
      if (y_src && y_dst) y_dst[v] = y_src[v];
    }
  }
  mask_sample_graph<1024, MASK_WGS>(node_ptr, rate, seed, step_counter ? step_counter[0] : 0, mask, blockIdx.x / MASK_WGS,
                          blockIdx.x % MASK_WGS);
}

// Collation from one snapshot matrix, then the sampler (REQ: the one that always masks required[]).
template <bool REQ>
__global__ __launch_bounds__(1024) void stage_rows_mask_kernel(const float* __restrict__ data, const long long* __restrict__ rows,
                                                               int N, float* x_dst, float* y_dst,
                                                               const int* __restrict__ node_ptr, double rate, uint64_t seed,
                                                               const uint64_t* __restrict__ step_counter,
                                                               const int* __restrict__ required, int num_required,
                                                               uint8_t* __restrict__ mask) {
  const int g = blockIdx.x / MASK_WGS, wq = blockIdx.x % MASK_WGS;
  collate_matrix_graph(data, rows, N, x_dst, y_dst, g, wq);
  mask_sample_graph<1024, MASK_WGS, REQ>(node_ptr, rate, seed, step_counter ? step_counter[0] : 0, mask, g, wq, required,
                                         num_required);
}

// ---------------------------------------------------------------------------------------- a fixed sensor layout's mask
// Per graph either the LAYOUT mask (everything hidden but the sensors, each sensor dropped with probability sensor_dropout) or
// the sampler's RANDOM mask, chosen per graph and step with probability layout_share; include/gatres.h states the draws.  The
// layout mask is built in LDS one tile of 4096 nodes at a time -- the inverse of observed[] over the tile as bytes, so a
// workgroup's table is sized by the tile, not by the graph -- and leaves as one 32-bit store per thread.  No atomics: every
// byte has one writer.
constexpr int SENS_T = 1024;                   // threads of a workgroup (the sampler's)
constexpr int SENS_TILE = 4 * SENS_T;          // mask bytes of one LDS pass: one 32-bit word per thread

// Workgroup (g, wq).  The mode of graph g is one hash of (seed, step, g): the same in the graph's MASK_WGS workgroups and in
// every thread, known before the first barrier -- a random-mode workgroup runs mask_sample_graph exactly as mask_generate_kernel
// does and never meets the layout path's barriers.
// Layout mode: the workgroup owns the nodes [vlo, vhi) of its graph, the sampler's slices.  In the batch's flat mask array that
// is [lo, hi); tiles start at lo rounded down to a multiple of four, so that thread t of a tile holds the four bytes of one
// aligned 32-bit word (words_ok: the mask's address is a multiple of four; else byte stores).  A word that straddles lo or hi
// is stored byte by byte, only the bytes inside: the neighbouring slice's workgroup, or another graph's, writes the others.
// NOISE (gatres_stage_rows_mask_sensors_noisy; the instantiation without it reads neither argument and is today's kernel): a
// sensor that KEEPS its reading in a layout-mode graph is staged as data + sigma[k] * z in x_dst, z = obs_noise(...) keyed by
// (noise_seed, member = step, source row, k).  Interleaved over the graph's workgroups (collate_graph), the element at a sensor
// node may be copied by another workgroup than the one that owns the node's mask slice, and a later store of the noisy value
// would race with it.  So here the mode is drawn before any store; a random-mode graph is collated as ever, and in a layout-mode
// graph every workgroup copies its OWN slice of the row, meets the first tile's barrier and then, in the k-loop that opens
// s_open[], stores the noisy value (read from data, not from x_dst) over its own clean copy: every element of x_dst has one
// final writer, ordered by the workgroup's barrier.  Only lanes that hold a kept sensor with sigma[k] != 0 draw; sigma[k] == 0
// leaves the clean copy, bit for bit.  y_dst (when it is another buffer) gets the clean row.
template <bool NOISE>
__global__ __launch_bounds__(SENS_T) void stage_rows_mask_sensors_kernel(
    const float* __restrict__ data, const long long* __restrict__ rows, int N, float* x_dst, float* y_dst,
    const int* __restrict__ node_ptr, const int* __restrict__ observed, int K, uint32_t t_drop, uint32_t t_share, double rate,
    uint64_t seed, const uint64_t* __restrict__ step_counter, uint8_t* __restrict__ mask, int words_ok,
    const float* __restrict__ sigma, uint64_t noise_seed) {
  __shared__ uint32_t s_word[SENS_T];
  const int g = blockIdx.x / MASK_WGS, wq = blockIdx.x % MASK_WGS;
  const int tid = threadIdx.x;
  if constexpr (!NOISE) collate_matrix_graph(data, rows, N, x_dst, y_dst, g, wq);
  const uint64_t step = step_counter ? step_counter[0] : 0;
  const uint64_t base = seed + 0x9E3779B97F4A7C15ULL * (step + 1);
  const bool layout = (uint32_t)(mix64(base + 0x94D049BB133111EBULL * (uint64_t)(g + 1)) >> 40) < t_share;
  if (!layout) {
    if constexpr (NOISE) collate_matrix_graph(data, rows, N, x_dst, y_dst, g, wq);
    mask_sample_graph<SENS_T, MASK_WGS>(node_ptr, rate, seed, step, mask, g, wq);
    return;
  }
  const int n0 = node_ptr[g], n = node_ptr[g + 1] - n0;
  const int per = (n + MASK_WGS - 1) / MASK_WGS, vlo = min(n, wq * per), vhi = min(n, vlo + per);
  const long long lo = (long long)n0 + vlo, hi = (long long)n0 + vhi;
  // NOISE: the slice [clo, chi) of the row this workgroup copies -- the mask slice [vlo, vhi) of a graph of N nodes; cut from N,
  // so that the copy stays inside the row whatever node_ptr says -- and the noise's stream of this step
  const long long row = NOISE ? rows[g] : 0, xoff = (long long)g * N;
  const int cper = (N + MASK_WGS - 1) / MASK_WGS, clo = min(N, wq * cper), chi = min(N, clo + cper);
  uint64_t noise_stream = 0;
  if constexpr (NOISE) {
    copy_row(data + row * (long long)N + clo, x_dst + xoff + clo, y_dst && y_dst != x_dst ? y_dst + xoff + clo : nullptr, chi - clo,
             tid, SENS_T);
    noise_stream = obs_noise_stream(noise_seed, step);
  }
  uint8_t* s_open = reinterpret_cast<uint8_t*>(s_word);          // [SENS_TILE]: 1 = hidden, 0 = a sensor that kept its reading
  for (long long t0 = lo & ~3LL; t0 < hi; t0 += SENS_TILE) {      // (uniform in the workgroup: every thread meets the barriers)
    s_word[tid] = 0x01010101u;
    __syncthreads();                                              // (NOISE: the slice's clean copy is behind this barrier)
    for (int k = tid; k < K; k += SENS_T) {
      const int v = observed[k];
      const long long f = (long long)n0 + v;
      if (v >= vlo && v < vhi && f >= t0 && f < t0 + SENS_TILE &&
          (uint32_t)(mix64(base + 0xBF58476D1CE4E5B9ULL * (uint64_t)(n0 + v + 1)) >> 40) >= t_drop) {
        s_open[f - t0] = 0;
        if constexpr (NOISE) {
          const float sg = sigma[k];
          if (v >= clo && v < chi && sg != 0.f)                    // (a sensor met in one tile pass only: one store)
            x_dst[xoff + v] = __fadd_rn(data[row * (long long)N + v], __fmul_rn(sg, obs_noise(noise_stream, row, K, k)));
        }
      }
    }
    __syncthreads();
    const long long f = t0 + 4 * tid;
    if (f < hi && f + 4 > lo) {
      const uint32_t w = s_word[tid];
      if (words_ok && f >= lo && f + 4 <= hi) {
        *reinterpret_cast<uint32_t*>(mask + f) = w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (f + e >= lo && f + e < hi) mask[f + e] = (uint8_t)((w >> (8 * e)) & 0xffu);
      }
    }
    __syncthreads();                                              // (the next tile refills the table)
  }
}

// -------------------------------------------------------------------------- several snapshot matrices (multi_snapshot_store.py)
// A batch holds graphs of different topologies side by side, so every graph names its own source -- a network (an entry of a
// device table of matrix pointers) and a row inside it -- and node_ptr gives both where the graph goes and how wide it is.

// The source row of graph g (nullptr: a table entry out of range -- the host builds the tables and checks them; the kernel
// only never follows a bad one).
__device__ __forceinline__ const float* multi_source(const float* const* __restrict__ src_table, int num_networks,
                                                     const int* __restrict__ net_of_graph, const long long* __restrict__ rows,
                                                     long long g_row, int g, int n, int& net_out) {
  const int net = net_of_graph[g];
  net_out = net;
  if (net < 0 || net >= num_networks) return nullptr;
  const float* base = src_table[net];
  return base ? base + rows[g_row] * (long long)n : nullptr;
}

// gatres_stage_rows_mask_required with per-graph sources; the mask comes from the same sampler, keyed the same way, so a
// one-network call writes the same x and the same mask bytes.
__global__ __launch_bounds__(1024) void stage_multi_rows_mask_kernel(const float* const* __restrict__ src_table, int num_networks,
                                                                     const int* __restrict__ net_of_graph,
                                                                     const long long* __restrict__ rows,
                                                                     const int* __restrict__ node_ptr, float* x_dst, float* y_dst,
                                                                     double rate, uint64_t seed,
                                                                     const uint64_t* __restrict__ step_counter,
                                                                     const int* __restrict__ req_ptr, const int* __restrict__ req_idx,
                                                                     uint8_t* __restrict__ mask) {
  const int g = blockIdx.x / MASK_WGS, wq = blockIdx.x % MASK_WGS;
  const int n0 = node_ptr[g], n = node_ptr[g + 1] - n0;
  int net;
  const float* src = multi_source(src_table, num_networks, net_of_graph, rows, g, g, n, net);
  if (src && n > 0) collate_graph(src, x_dst, y_dst, n0, n, wq);
  const int* required = nullptr;
  int num_required = 0;
  if (req_ptr && src) {
    const int r0 = req_ptr[net];
    num_required = req_ptr[net + 1] - r0;
    required = req_idx + r0;
    if (num_required < 0) num_required = 0;
  }
  mask_sample_graph<1024, MASK_WGS, true>(node_ptr, rate, seed, step_counter ? step_counter[0] : 0, mask, g, wq, required,
                                          num_required);
}

constexpr int GATHER_T = 256;

// One workgroup per (batch, graph): dst[batch * batch_stride + node_ptr[g] ..) = the graph's row.
__global__ __launch_bounds__(GATHER_T) void gather_multi_rows_kernel(const float* const* __restrict__ src_table, int num_networks,
                                                                     const int* __restrict__ net_of_graph,
                                                                     const long long* __restrict__ rows,
                                                                     const int* __restrict__ node_ptr, int num_graphs,
                                                                     float* __restrict__ dst, long long batch_stride) {
  const int g = blockIdx.x % num_graphs;
  const long long batch = blockIdx.x / num_graphs;
  const int n0 = node_ptr[g], n = node_ptr[g + 1] - n0;
  int net;
  const float* src = multi_source(src_table, num_networks, net_of_graph, rows, (long long)blockIdx.x, g, n, net);
  if (src && n > 0) copy_row(src, dst + batch * batch_stride + n0, nullptr, n, (int)threadIdx.x, GATHER_T);
}

// What every launch of the sampler's grid refuses; with from_rows also what every collation from one snapshot matrix refuses.
bool stage_args_ok(const int32_t* node_ptr, const uint8_t* mask, int32_t num_graphs, double mask_rate, bool from_rows = false,
                   const float* data = nullptr, const int64_t* rows = nullptr, const float* x_dst = nullptr,
                   int32_t nodes_per_graph = 0) {
  if (!node_ptr || !mask || num_graphs <= 0 || !(mask_rate >= 0.0 && mask_rate <= 1.0)) return false;
  return !from_rows || (data && rows && x_dst && nodes_per_graph > 0 && data != x_dst);
}

static_assert(sizeof(long long) == sizeof(int64_t), "row indices");

}  // namespace

extern "C" int gatres_mask_generate(const int32_t* node_ptr, int32_t num_graphs, double mask_rate, uint64_t seed,
                                    const uint64_t* step_counter, uint8_t* mask, void* stream) {
  if (!stage_args_ok(node_ptr, mask, num_graphs, mask_rate)) return GATRES_E_BADARG;
  hipLaunchKernelGGL(mask_generate_kernel, dim3(num_graphs * MASK_WGS), dim3(1024), 0, gatres_stream(stream), node_ptr, mask_rate,
                     seed, step_counter, mask, nullptr, nullptr, nullptr, nullptr, 0LL);
  return gatres_launch_status();
}

extern "C" int gatres_stage_batch_mask(const float* x_src, const float* y_src, float* x_dst, float* y_dst, int64_t num_nodes,
                                       const int32_t* node_ptr, int32_t num_graphs, double mask_rate, uint64_t seed,
                                       const uint64_t* step_counter, uint8_t* mask, void* stream) {
  if (!stage_args_ok(node_ptr, mask, num_graphs, mask_rate)) return GATRES_E_BADARG;
  if (!x_src || !x_dst || num_nodes <= 0 || ((y_src == nullptr) != (y_dst == nullptr))) return GATRES_E_BADARG;
  hipLaunchKernelGGL(mask_generate_kernel, dim3(num_graphs * MASK_WGS), dim3(1024), 0, gatres_stream(stream), node_ptr, mask_rate,
                     seed, step_counter, mask, x_src, y_src, x_dst, y_dst, (long long)num_nodes);
  return gatres_launch_status();
}

extern "C" int gatres_stage_rows_mask(const float* data, const int64_t* rows, int32_t nodes_per_graph, float* x_dst,
                                      float* y_dst, const int32_t* node_ptr, int32_t num_graphs, double mask_rate,
                                      uint64_t seed, const uint64_t* step_counter, uint8_t* mask, void* stream) {
  if (!stage_args_ok(node_ptr, mask, num_graphs, mask_rate, true, data, rows, x_dst, nodes_per_graph)) return GATRES_E_BADARG;
  hipLaunchKernelGGL(stage_rows_mask_kernel<false>, dim3(num_graphs * MASK_WGS), dim3(1024), 0, gatres_stream(stream), data,
                     reinterpret_cast<const long long*>(rows), (int)nodes_per_graph, x_dst, y_dst, node_ptr, mask_rate, seed,
                     step_counter, nullptr, 0, mask);
  return gatres_launch_status();
}

extern "C" int gatres_stage_rows_mask_required(const float* data, const int64_t* rows, int32_t nodes_per_graph, float* x_dst,
                                               float* y_dst, const int32_t* node_ptr, int32_t num_graphs, double mask_rate,
                                               uint64_t seed, const uint64_t* step_counter, const int32_t* required,
                                               int32_t num_required, uint8_t* mask, void* stream) {
  if (!stage_args_ok(node_ptr, mask, num_graphs, mask_rate, true, data, rows, x_dst, nodes_per_graph)) return GATRES_E_BADARG;
  if (num_required < 0 || (num_required > 0 && !required)) return GATRES_E_BADARG;
  // utils/auxil.py:151-153: the sampled part int(n*rate) - r must be positive
  if (num_required > 0 && (int)((double)nodes_per_graph * mask_rate) - num_required <= 0) return GATRES_E_BADARG;
  hipLaunchKernelGGL(stage_rows_mask_kernel<true>, dim3(num_graphs * MASK_WGS), dim3(1024), 0, gatres_stream(stream), data,
                     reinterpret_cast<const long long*>(rows), (int)nodes_per_graph, x_dst, y_dst, node_ptr, mask_rate, seed,
                     step_counter, required, (int)num_required, mask);
  return gatres_launch_status();
}

// gatres_stage_rows_mask_sensors and its noisy sibling: one set of checks, one launch, the noise a compile-time fact.
template <bool NOISE>
static int stage_rows_mask_sensors(const float* data, const int64_t* rows, int32_t nodes_per_graph, float* x_dst, float* y_dst,
                                   const int32_t* node_ptr, int32_t num_graphs, const int32_t* observed, int32_t num_observed,
                                   double sensor_dropout, double layout_share, double mask_rate, uint64_t seed,
                                   const uint64_t* step_counter, uint8_t* mask, const float* sigma, uint64_t noise_seed,
                                   void* stream) {
  if (!stage_args_ok(node_ptr, mask, num_graphs, mask_rate, true, data, rows, x_dst, nodes_per_graph)) return GATRES_E_BADARG;
  if (!observed || num_observed < 1 || num_observed > nodes_per_graph) return GATRES_E_BADARG;
  if (!(sensor_dropout >= 0.0 && sensor_dropout < 1.0) || !(layout_share >= 0.0 && layout_share <= 1.0)) return GATRES_E_BADARG;
  if (NOISE) {
    if (!sigma) return GATRES_E_BADARG;
    const uint64_t total = (uint64_t)nodes_per_graph * (uint64_t)num_graphs, sb = 4 * (uint64_t)num_observed;
    if (bytes_overlap(sigma, sb, x_dst, 4 * total) || bytes_overlap(sigma, sb, y_dst, 4 * total) ||
        bytes_overlap(sigma, sb, mask, total)) return GATRES_E_BADARG;
  }
  const uint32_t t_drop = (uint32_t)(sensor_dropout * 16777216.0), t_share = (uint32_t)(layout_share * 16777216.0);
  const int words_ok = (reinterpret_cast<uintptr_t>(mask) & 3u) == 0;
  hipLaunchKernelGGL(stage_rows_mask_sensors_kernel<NOISE>, dim3((unsigned)num_graphs * MASK_WGS), dim3(SENS_T), 0,
                     gatres_stream(stream), data, reinterpret_cast<const long long*>(rows), (int)nodes_per_graph, x_dst, y_dst,
                     node_ptr, observed, (int)num_observed, t_drop, t_share, mask_rate, seed, step_counter, mask, words_ok, sigma,
                     noise_seed);
  return gatres_launch_status();
}

extern "C" int gatres_stage_rows_mask_sensors(const float* data, const int64_t* rows, int32_t nodes_per_graph, float* x_dst,
                                              float* y_dst, const int32_t* node_ptr, int32_t num_graphs, const int32_t* observed,
                                              int32_t num_observed, double sensor_dropout, double layout_share, double mask_rate,
                                              uint64_t seed, const uint64_t* step_counter, uint8_t* mask, void* stream) {
  return stage_rows_mask_sensors<false>(data, rows, nodes_per_graph, x_dst, y_dst, node_ptr, num_graphs, observed, num_observed,
                                        sensor_dropout, layout_share, mask_rate, seed, step_counter, mask, nullptr, 0, stream);
}

extern "C" int gatres_stage_rows_mask_sensors_noisy(const float* data, const int64_t* rows, int32_t nodes_per_graph, float* x_dst,
                                                    float* y_dst, const int32_t* node_ptr, int32_t num_graphs,
                                                    const int32_t* observed, int32_t num_observed, double sensor_dropout,
                                                    double layout_share, double mask_rate, uint64_t seed,
                                                    const uint64_t* step_counter, uint8_t* mask, const float* sigma,
                                                    uint64_t noise_seed, void* stream) {
  return stage_rows_mask_sensors<true>(data, rows, nodes_per_graph, x_dst, y_dst, node_ptr, num_graphs, observed, num_observed,
                                       sensor_dropout, layout_share, mask_rate, seed, step_counter, mask, sigma, noise_seed, stream);
}

extern "C" int gatres_stage_multi_rows_mask_required(const float* const* src_table, int32_t num_networks,
                                                     const int32_t* net_of_graph, const int64_t* rows, const int32_t* node_ptr,
                                                     int32_t num_graphs, float* x_dst, float* y_dst, double mask_rate,
                                                     uint64_t seed, const uint64_t* step_counter, const int32_t* req_ptr,
                                                     const int32_t* req_idx, uint8_t* mask, void* stream) {
  if (!stage_args_ok(node_ptr, mask, num_graphs, mask_rate)) return GATRES_E_BADARG;
  if (!src_table || !net_of_graph || !rows || !x_dst || num_networks <= 0) return GATRES_E_BADARG;
  if ((!req_ptr) != (!req_idx)) return GATRES_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(x_dst) | reinterpret_cast<uintptr_t>(y_dst)) & 3u) return GATRES_E_BADARG;
  hipLaunchKernelGGL(stage_multi_rows_mask_kernel, dim3((unsigned)num_graphs * MASK_WGS), dim3(1024), 0, gatres_stream(stream),
                     src_table, (int)num_networks, net_of_graph, reinterpret_cast<const long long*>(rows), node_ptr, x_dst, y_dst,
                     mask_rate, seed, step_counter, req_ptr, req_idx, mask);
  return gatres_launch_status();
}

// (no mask, no rate: the gather's checks are all its own)
extern "C" int gatres_gather_multi_rows(const float* const* src_table, int32_t num_networks, const int32_t* net_of_graph,
                                        const int64_t* rows, const int32_t* node_ptr, int32_t num_graphs, int32_t num_batches,
                                        float* dst, int64_t batch_stride, void* stream) {
  if (!src_table || !net_of_graph || !rows || !node_ptr || !dst) return GATRES_E_BADARG;
  if (num_networks <= 0 || num_graphs <= 0 || num_batches <= 0 || batch_stride <= 0) return GATRES_E_BADARG;
  if (reinterpret_cast<uintptr_t>(dst) & 3u) return GATRES_E_BADARG;
  if ((long long)num_graphs * (long long)num_batches > 0x7fffffffLL) return GATRES_E_BADARG;
  hipLaunchKernelGGL(gather_multi_rows_kernel, dim3((unsigned)((long long)num_graphs * num_batches)), dim3(GATHER_T), 0,
                     gatres_stream(stream), src_table, (int)num_networks, net_of_graph, reinterpret_cast<const long long*>(rows),
                     node_ptr, (int)num_graphs, dst, (long long)batch_stride);
  return gatres_launch_status();
}

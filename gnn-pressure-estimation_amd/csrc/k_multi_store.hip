// Collation from SEVERAL snapshot matrices (multi_snapshot_store.py: one [S_k][N_k] matrix per water network): a batch holds
// graphs of different topologies side by side, so every graph names its own source -- a network (an entry of a device table
// of matrix pointers) and a row inside it -- and node_ptr gives both where the graph goes and how wide it is.
//   gatres_stage_multi_rows_mask_required: gatres_stage_rows_mask_required with per-graph sources; the mask comes from the
//     same sampler (k_mask.h), keyed the same way, so a one-network call writes the same x and the same mask bytes.
//   gatres_gather_multi_rows: the gather alone for num_batches x num_graphs graphs in one launch (an epoch's full batches,
//     laid out batch by batch in one buffer).
// A graph's row is contiguous in the source and in the destination: lanes walk it node by node, 16 bytes per lane where the
// two starts allow it.  The pointer table and the index tables are read once per graph, by uniform (scalar) loads.
#include "gatres_common.h"
#include "k_mask.h"

namespace {

// dst[0 .. n) = src[0 .. n) by the threads `t` of `T` (of one or several workgroups): a scalar head up to dst's first 16-byte
// boundary, the body as float4 if src is aligned there too (float by float otherwise), a scalar tail.
__device__ __forceinline__ void copy_row(const float* __restrict__ src, float* __restrict__ dst, float* __restrict__ dst2,
                                         int n, int t, int T) {
  int head = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) / 4u);
  if (head > n) head = n;
  const bool vec = (reinterpret_cast<uintptr_t>(src + head) & 15u) == 0 &&
                   (!dst2 || (reinterpret_cast<uintptr_t>(dst2 + head) & 15u) == 0);
  if (!vec) {
    for (int i = t; i < n; i += T) {
      const float s = src[i];
      dst[i] = s;
      if (dst2) dst2[i] = s;
    }
    return;
  }
  const int nvec = (n - head) / 4, tail0 = head + 4 * nvec;
  const float4* __restrict__ s4 = reinterpret_cast<const float4*>(src + head);
  float4* __restrict__ d4 = reinterpret_cast<float4*>(dst + head);
  float4* __restrict__ e4 = dst2 ? reinterpret_cast<float4*>(dst2 + head) : nullptr;
  for (int v = t; v < nvec; v += T) {
    const float4 r = s4[v];
    d4[v] = r;
    if (e4) e4[v] = r;
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

// MASK_WGS workgroups per graph, as the sampler's other launches: together they copy the graph's row, then each ranks its
// slice of the graph's keys.  The copy's stores drain while the keys are ranked.
__global__ __launch_bounds__(1024) void stage_multi_rows_mask_kernel(const float* const* __restrict__ src_table, int num_networks,
                                                                     const int* __restrict__ net_of_graph,
                                                                     const long long* __restrict__ rows,
                                                                     const int* __restrict__ node_ptr, float* __restrict__ x_dst,
                                                                     float* __restrict__ y_dst, double rate, uint64_t seed,
                                                                     const uint64_t* __restrict__ step_counter,
                                                                     const int* __restrict__ req_ptr, const int* __restrict__ req_idx,
                                                                     uint8_t* __restrict__ mask) {
  const int g = blockIdx.x / MASK_WGS, wq = blockIdx.x % MASK_WGS;
  const int n0 = node_ptr[g], n = node_ptr[g + 1] - n0;
  int net;
  const float* src = multi_source(src_table, num_networks, net_of_graph, rows, g, g, n, net);
  if (src && n > 0) copy_row(src, x_dst + n0, y_dst ? y_dst + n0 : nullptr, n, wq * 1024 + (int)threadIdx.x, MASK_WGS * 1024);
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

}  // namespace

extern "C" int gatres_stage_multi_rows_mask_required(const float* const* src_table, int32_t num_networks,
                                                     const int32_t* net_of_graph, const int64_t* rows, const int32_t* node_ptr,
                                                     int32_t num_graphs, float* x_dst, float* y_dst, double mask_rate,
                                                     uint64_t seed, const uint64_t* step_counter, const int32_t* req_ptr,
                                                     const int32_t* req_idx, uint8_t* mask, void* stream) {
  if (!src_table || !net_of_graph || !rows || !node_ptr || !x_dst || !mask) return GATRES_E_BADARG;
  if (num_networks <= 0 || num_graphs <= 0 || !(mask_rate >= 0.0 && mask_rate <= 1.0)) return GATRES_E_BADARG;
  if ((!req_ptr) != (!req_idx)) return GATRES_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(x_dst) | reinterpret_cast<uintptr_t>(y_dst)) & 3u) return GATRES_E_BADARG;
  if (x_dst == y_dst) y_dst = nullptr;                    // (one buffer serves both: written once)
  hipLaunchKernelGGL(stage_multi_rows_mask_kernel, dim3((unsigned)num_graphs * MASK_WGS), dim3(1024), 0, gatres_stream(stream),
                     src_table, (int)num_networks, net_of_graph, reinterpret_cast<const long long*>(rows), node_ptr, x_dst, y_dst,
                     mask_rate, seed, step_counter, req_ptr, req_idx, mask);
  return gatres_launch_status();
}

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

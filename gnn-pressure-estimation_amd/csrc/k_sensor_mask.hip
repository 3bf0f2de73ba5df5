// Staging launch of fine-tuning to a FIXED sensor layout (GATResTrainer.set_sensor_layout): gatres_stage_rows_mask's collation
// with the layout's mask written in the same launch.
//   gatres_stage_rows_mask_sensors   per graph either the LAYOUT mask (everything hidden but the sensors, each sensor dropped
//                                    with probability sensor_dropout) or the sampler's RANDOM mask (k_mask.h, unchanged), chosen
//                                    per graph and step with probability layout_share; include/gatres.h states the draws.
// The grid is the sampler's: MASK_WGS workgroups of 1024 per graph.  Together they copy the graph's row (16-byte accesses where
// source and destination share their phase inside 16 bytes: always when the graph size is a multiple of four), then each writes
// the mask of its slice of the graph's nodes.  The layout mask is built in LDS one tile of 4096 nodes at a time -- the inverse of
// observed[] over the tile as bytes, so a workgroup's table is sized by the tile, not by the graph -- and leaves as one 32-bit
// store per thread.  No atomics: every byte has one writer.
#include "k_mask.h"

namespace {

constexpr int SENS_T = 1024;                   // threads of a workgroup (the sampler's)
constexpr int SENS_TILE = 4 * SENS_T;          // mask bytes of one LDS pass: one 32-bit word per thread

// dst[0..n) = src[0..n) (and dst2 likewise when given) by the T threads that share the row, this one being thread t.
__device__ __forceinline__ void sens_copy_row(const float* __restrict__ src, float* __restrict__ dst, float* __restrict__ dst2,
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

// Workgroup (g, wq).  The mode of graph g is one hash of (seed, step, g): the same in the graph's MASK_WGS workgroups and in
// every thread, known before the first barrier -- a random-mode workgroup runs mask_sample_graph exactly as mask_generate_kernel
// does and never meets the layout path's barriers.
// Layout mode: the workgroup owns the nodes [vlo, vhi) of its graph, the sampler's slices.  In the batch's flat mask array that
// is [lo, hi); tiles start at lo rounded down to a multiple of four, so that thread t of a tile holds the four bytes of one
// aligned 32-bit word (words_ok: the mask's address is a multiple of four; else byte stores).  A word that straddles lo or hi
// is stored byte by byte, only the bytes inside: the neighbouring slice's workgroup, or another graph's, writes the others.
__global__ __launch_bounds__(SENS_T) void stage_rows_mask_sensors_kernel(
    const float* __restrict__ data, const long long* __restrict__ rows, int N, float* __restrict__ x_dst, float* __restrict__ y_dst,
    const int* __restrict__ node_ptr, const int* __restrict__ observed, int K, uint32_t t_drop, uint32_t t_share, double rate,
    uint64_t seed, const uint64_t* __restrict__ step_counter, uint8_t* __restrict__ mask, int words_ok) {
  __shared__ uint32_t s_word[SENS_T];
  const int g = blockIdx.x / MASK_WGS, wq = blockIdx.x % MASK_WGS;
  const int tid = threadIdx.x;
  sens_copy_row(data + rows[g] * (long long)N, x_dst + (long long)g * N, y_dst ? y_dst + (long long)g * N : nullptr, N,
                wq * SENS_T + tid, MASK_WGS * SENS_T);
  const uint64_t step = step_counter ? step_counter[0] : 0;
  const uint64_t base = seed + 0x9E3779B97F4A7C15ULL * (step + 1);
  const bool layout = (uint32_t)(mix64(base + 0x94D049BB133111EBULL * (uint64_t)(g + 1)) >> 40) < t_share;
  if (!layout) {
    mask_sample_graph<SENS_T, MASK_WGS>(node_ptr, rate, seed, step, mask, g, wq);
    return;
  }
  const int n0 = node_ptr[g], n = node_ptr[g + 1] - n0;
  const int per = (n + MASK_WGS - 1) / MASK_WGS, vlo = min(n, wq * per), vhi = min(n, vlo + per);
  const long long lo = (long long)n0 + vlo, hi = (long long)n0 + vhi;
  uint8_t* s_open = reinterpret_cast<uint8_t*>(s_word);          // [SENS_TILE]: 1 = hidden, 0 = a sensor that kept its reading
  for (long long t0 = lo & ~3LL; t0 < hi; t0 += SENS_TILE) {      // (uniform in the workgroup: every thread meets the barriers)
    s_word[tid] = 0x01010101u;
    __syncthreads();
    for (int k = tid; k < K; k += SENS_T) {
      const int v = observed[k];
      const long long f = (long long)n0 + v;
      if (v >= vlo && v < vhi && f >= t0 && f < t0 + SENS_TILE &&
          (uint32_t)(mix64(base + 0xBF58476D1CE4E5B9ULL * (uint64_t)(n0 + v + 1)) >> 40) >= t_drop)
        s_open[f - t0] = 0;
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

}  // namespace

extern "C" int gatres_stage_rows_mask_sensors(const float* data, const int64_t* rows, int32_t nodes_per_graph, float* x_dst,
                                              float* y_dst, const int32_t* node_ptr, int32_t num_graphs, const int32_t* observed,
                                              int32_t num_observed, double sensor_dropout, double layout_share, double mask_rate,
                                              uint64_t seed, const uint64_t* step_counter, uint8_t* mask, void* stream) {
  if (!data || !rows || !x_dst || !node_ptr || !observed || !mask || data == x_dst) return GATRES_E_BADARG;
  if (num_graphs <= 0 || nodes_per_graph <= 0 || num_observed < 1 || num_observed > nodes_per_graph) return GATRES_E_BADARG;
  if (!(sensor_dropout >= 0.0 && sensor_dropout < 1.0) || !(layout_share >= 0.0 && layout_share <= 1.0) ||
      !(mask_rate >= 0.0 && mask_rate <= 1.0))
    return GATRES_E_BADARG;
  static_assert(sizeof(long long) == sizeof(int64_t), "row indices");
  if (x_dst == y_dst) y_dst = nullptr;                    // (one buffer serves both: written once)
  const uint32_t t_drop = (uint32_t)(sensor_dropout * 16777216.0), t_share = (uint32_t)(layout_share * 16777216.0);
  const int words_ok = (reinterpret_cast<uintptr_t>(mask) & 3u) == 0;
  hipLaunchKernelGGL(stage_rows_mask_sensors_kernel, dim3((unsigned)num_graphs * MASK_WGS), dim3(SENS_T), 0, gatres_stream(stream),
                     data, reinterpret_cast<const long long*>(rows), (int)nodes_per_graph, x_dst, y_dst, node_ptr, observed,
                     (int)num_observed, t_drop, t_share, mask_rate, seed, step_counter, mask, words_ok);
  return gatres_launch_status();
}

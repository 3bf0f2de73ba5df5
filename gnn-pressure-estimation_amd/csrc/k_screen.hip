// Device side of the screening of sensor readings (estimation.PressureEstimator.loo_residuals / screen / estimate_screened): a
// reading that is present and wrong.  The leave-one-out pass runs (snapshot, left-out sensor) pairs through the layouts staging
// and the forward; then
//   gatres_loo_residuals  reads, per pair, the model's prediction at the hidden sensor's node and writes it and the residual
//                         reading - prediction, in physical units;
//   gatres_screen_reject  one rejection round: per snapshot the available sensor whose residual exceeds its bound by the largest
//                         factor is taken out of the availability matrix.
// Both are small element passes without atomics; every value is a function of the inputs alone, whatever the launch geometry.
#include "gatres_common.h"

namespace {

constexpr unsigned int QUIET_NAN = 0x7fc00000u;

// ---- leave-one-out residuals -------------------------------------------------------------------------------------------------------
constexpr int LR_T = 256;

// Graph g of the batch per thread and trip; the grid is capped and strides over the graphs.  A reading that is not there is not
// loaded where `available` says so.  A sensor index outside [0, N) reads nothing: both outputs are NaN.
template <bool FULL_ROWS>
__global__ __launch_bounds__(LR_T) void loo_residuals_kernel(const float* __restrict__ out, const uint8_t* __restrict__ mask,
                                                             const float* __restrict__ src, int N, long long graphs,
                                                             long long first_pair, const int* __restrict__ observed, int K,
                                                             float scale, float offset, const uint8_t* __restrict__ available,
                                                             int nan_is_missing, float* __restrict__ pred,
                                                             float* __restrict__ resid) {
  const float qnan = __uint_as_float(QUIET_NAN);
  for (long long g = (long long)blockIdx.x * LR_T + threadIdx.x; g < graphs; g += (long long)gridDim.x * LR_T) {
    const long long p = first_pair + g;
    const long long s = p / K;
    const int k = (int)(p - s * K);
    const int v = observed[k];
    float pr = qnan, res = qnan;
    if (v >= 0 && v < N) {
      pr = gatres_descale(out[g * N + v], scale, offset);
      const bool there = !available || available[p] != 0;
      if (there && mask[g * N + v] != 0) {
        const float r = FULL_ROWS ? gatres_descale(src[s * N + v], scale, offset) : src[p];
        if (!(nan_is_missing && r != r)) res = __fsub_rn(r, pr);
      }
    }
    pred[p] = pr;
    resid[p] = res;
  }
}

// ---- one rejection round -----------------------------------------------------------------------------------------------------------
constexpr int SR_T = 256;
constexpr int SR_LANES = 64;                   // one wave per snapshot
constexpr int SR_WAVES = 4;
static_assert(SR_WAVES * SR_LANES == SR_T, "whole waves");

// The order of the candidates as one unsigned 64-bit key, larger is better: the score's bits mapped so that unsigned order is
// the IEEE order (-0 below +0, a NaN score below everything), then the smaller k.  0 is "no candidate": a candidate's low word
// is at least 1.
__device__ __forceinline__ unsigned long long screen_key(float score, int k) {
  const unsigned int u = __float_as_uint(score);
  unsigned int o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  if (score != score) o = 0u;
  return ((unsigned long long)o << 32) | (unsigned long long)(0xffffffffu - (unsigned int)k);
}

__global__ __launch_bounds__(SR_T) void screen_reject_kernel(const float* __restrict__ resid, const float* __restrict__ bound,
                                                             const float* __restrict__ inv_bound, uint8_t* available,
                                                             long long S, int K, int min_sensors, int round, int max_rounds,
                                                             int* __restrict__ rejected, uint8_t* __restrict__ flagged) {
  const int lane = threadIdx.x & (SR_LANES - 1), wave = threadIdx.x / SR_LANES;
  for (long long s = (long long)blockIdx.x * SR_WAVES + wave; s < S; s += (long long)gridDim.x * SR_WAVES) {
    const long long row = s * K;
    unsigned long long best = 0ull;
    int present = 0;
    for (int k = lane; k < K; k += SR_LANES) {
      const bool a = available[row + k] != 0;
      const float r = resid[row + k], ar = fabsf(r);
      const bool cand = a && r == r && ar > bound[k];            // (a NaN bound compares false, +inf is never exceeded)
      present += a ? 1 : 0;
      if (flagged) flagged[row + k] = cand ? 1 : 0;
      if (cand) {
        const unsigned long long key = screen_key(__fmul_rn(ar, inv_bound[k]), k);
        best = key > best ? key : best;
      }
    }
#pragma unroll
    for (int d = SR_LANES / 2; d > 0; d >>= 1) {
      const unsigned long long other = __shfl_xor(best, d, SR_LANES);
      best = other > best ? other : best;
      present += __shfl_xor(present, d, SR_LANES);
    }
    if (lane == 0) {
      int k_star = -1;
      if (best != 0ull && present - 1 >= min_sensors) {
        k_star = (int)(0xffffffffu - (unsigned int)(best & 0xffffffffull));
        available[row + k_star] = 0;
      }
      rejected[s * max_rounds + round] = k_star;
    }
  }
}

}  // namespace

extern "C" int gatres_loo_residuals(const float* out, const uint8_t* mask, const float* src, int32_t layout, int64_t src_rows,
                                    int64_t first_pair, int32_t nodes_per_graph, int32_t num_graphs, const int32_t* observed,
                                    int32_t num_observed, double scale, double offset, const uint8_t* available,
                                    int32_t nan_is_missing, float* pred, float* resid, void* stream) {
  if (!out || !mask || !src || !observed || !pred || !resid || nodes_per_graph <= 0 || num_graphs <= 0) return GATRES_E_BADARG;
  if (layout != GATRES_OBSERVED_FULL_ROWS && layout != GATRES_OBSERVED_READINGS) return GATRES_E_BADARG;
  if (num_observed <= 0 || num_observed > nodes_per_graph) return GATRES_E_BADARG;
  if ((int64_t)nodes_per_graph * num_graphs > INT32_MAX) return GATRES_E_BADARG;
  if (src_rows <= 0 || src_rows > INT64_MAX / 4 / nodes_per_graph) return GATRES_E_BADARG;      // (and so src_rows * K fits)
  const int64_t pairs = src_rows * num_observed;
  if (first_pair < 0 || first_pair > pairs - num_graphs) return GATRES_E_BADARG;
  // (the batch's entries of pred and resid against each other and against everything the launch reads)
  const uint64_t total = (uint64_t)nodes_per_graph * (uint64_t)num_graphs, w_bytes = 4 * (uint64_t)num_graphs;
  const uint64_t src_bytes = 4 * (uint64_t)src_rows *
                             (uint64_t)(layout == GATRES_OBSERVED_FULL_ROWS ? nodes_per_graph : num_observed);
  const float* w[2] = {pred + first_pair, resid + first_pair};
  if (bytes_overlap(w[0], w_bytes, w[1], w_bytes)) return GATRES_E_BADARG;
  for (const float* t : w) {
    if (bytes_overlap(t, w_bytes, out, 4 * total) || bytes_overlap(t, w_bytes, mask, total) ||
        bytes_overlap(t, w_bytes, src, src_bytes) || bytes_overlap(t, w_bytes, observed, 4 * (uint64_t)num_observed) ||
        bytes_overlap(t, w_bytes, available, (uint64_t)pairs))
      return GATRES_E_BADARG;
  }
  long long wgs = ((long long)num_graphs + LR_T - 1) / LR_T;
  if (wgs > 256) wgs = 256;
  const dim3 grid((unsigned)wgs), block(LR_T);
  if (layout == GATRES_OBSERVED_FULL_ROWS)
    hipLaunchKernelGGL(loo_residuals_kernel<true>, grid, block, 0, gatres_stream(stream), out, mask, src, (int)nodes_per_graph,
                       (long long)num_graphs, (long long)first_pair, observed, (int)num_observed, (float)scale, (float)offset,
                       available, (int)(nan_is_missing != 0), pred, resid);
  else
    hipLaunchKernelGGL(loo_residuals_kernel<false>, grid, block, 0, gatres_stream(stream), out, mask, src, (int)nodes_per_graph,
                       (long long)num_graphs, (long long)first_pair, observed, (int)num_observed, (float)scale, (float)offset,
                       available, (int)(nan_is_missing != 0), pred, resid);
  return gatres_launch_status();
}

extern "C" int gatres_screen_reject(const float* resid, const float* bound, const float* inv_bound, uint8_t* available,
                                    int64_t num_snapshots, int32_t num_observed, int32_t min_sensors, int32_t round,
                                    int32_t max_rounds, int32_t* rejected, uint8_t* flagged, void* stream) {
  if (!resid || !bound || !inv_bound || !available || !rejected) return GATRES_E_BADARG;
  if (num_snapshots <= 0 || num_observed <= 0 || min_sensors < 1 || max_rounds < 1 || round < 0 || round >= max_rounds)
    return GATRES_E_BADARG;
  if (num_snapshots > INT64_MAX / 4 / num_observed || num_snapshots > INT64_MAX / 4 / max_rounds) return GATRES_E_BADARG;
  const uint64_t cells = (uint64_t)num_snapshots * (uint64_t)num_observed, k_bytes = 4 * (uint64_t)num_observed;
  const uint64_t rej_bytes = 4 * (uint64_t)num_snapshots * (uint64_t)max_rounds;
  // (what the launch writes -- available, rejected, flagged -- against what it reads and against each other)
  const void* wr[3] = {available, rejected, flagged};
  const uint64_t wn[3] = {cells, rej_bytes, cells};
  for (int i = 0; i < 3; ++i) {
    if (bytes_overlap(wr[i], wn[i], resid, 4 * cells) || bytes_overlap(wr[i], wn[i], bound, k_bytes) ||
        bytes_overlap(wr[i], wn[i], inv_bound, k_bytes))
      return GATRES_E_BADARG;
    for (int j = i + 1; j < 3; ++j)
      if (bytes_overlap(wr[i], wn[i], wr[j], wn[j])) return GATRES_E_BADARG;
  }
  long long wgs = ((long long)num_snapshots + SR_WAVES - 1) / SR_WAVES;
  if (wgs > 1024) wgs = 1024;
  hipLaunchKernelGGL(screen_reject_kernel, dim3((unsigned)wgs), dim3(SR_T), 0, gatres_stream(stream), resid, bound, inv_bound,
                     available, (long long)num_snapshots, (int)num_observed, (int)min_sensors, (int)round, (int)max_rounds,
                     rejected, flagged);
  return gatres_launch_status();
}

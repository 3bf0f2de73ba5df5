// Device side of the sensitivity pass (estimation.PressureEstimator.sensitivity / sensitivity_map / linear_spread): the Jacobian
// J[j, k] = d estimate_j / d reading_k in reverse mode.  One graph of a batch carries one target junction: its seed g_out = e_j is
// written by gatres_stage_observed_targets (k_estimate.hip), the model's backward leaves g_x = d out_j / d x, and
//   gatres_sensitivity_gather  picks the sensors' entries of g_x into one row of J per graph, in physical units per physical unit;
//   gatres_sensitivity_fold    folds the rows of a chunk of snapshots into one fp64 record per (target, sensor);
//   gatres_sensitivity_spread  the first-order spread sqrt(sum_k (J[r][k] * sigma[k])^2) of every row.
// All three are small element passes; the fold and the spread sum in fp64 in a fixed order, without atomics: the same bits on
// every run and however a pass was cut into launches.
#include "gatres_common.h"

namespace {

// ---- gather --------------------------------------------------------------------------------------------------------------------
constexpr int SG_T = 256;

// Element i = g * K + k of the batch per thread and trip; the grid is capped and strides over the elements.  A masked sensor
// (missing, or hidden by the caller) reads as 0 whatever its g_x entry holds: the fused kernels write g_x at every node.  A NaN
// in *fault (the last float of the throw-away parameter gradient: a split launch whose partner never arrived) makes every entry
// of the batch a NaN.
__global__ __launch_bounds__(SG_T) void sensitivity_gather_kernel(const float* __restrict__ g_x, const uint8_t* __restrict__ mask,
                                                                  const float* __restrict__ fault, int N, long long total,
                                                                  const int* __restrict__ observed, int K, float unit,
                                                                  float* __restrict__ J, long long J_stride, long long first_row) {
  const bool failed = fault && (__float_as_uint(*fault) & 0x7fffffffu) > 0x7f800000u;      // (a NaN, by the bits)
  for (long long i = (long long)blockIdx.x * SG_T + threadIdx.x; i < total; i += (long long)gridDim.x * SG_T) {
    const long long g = i / K;
    const int k = (int)(i - g * K);
    const int v = observed[k];
    float r = 0.f;
    if (v >= 0 && v < N && !mask[g * N + v]) r = __fmul_rn(g_x[g * N + v], unit);
    if (failed) r = __int_as_float(0x7fc00000);
    J[(first_row + g) * J_stride + k] = r;
  }
}

// ---- fold ----------------------------------------------------------------------------------------------------------------------
constexpr int SF_T = 64;
constexpr int SF_U = 8;                        // a lane's rows in flight per trip

// Lane o = t * K + k owns the record of (target t, sensor k): it folds J[(s * T + t) * J_stride + k], s = 0 .. S - 1, strictly in
// that order, starting from the table's record when `accumulate`.  The lanes of a wave read consecutive floats of a row (and of
// the next target's row where a row ends).
__global__ __launch_bounds__(SF_T) void sensitivity_fold_kernel(const float* __restrict__ J, long long S, int T, int K,
                                                                long long J_stride, double* __restrict__ table, int accumulate) {
  const long long o = (long long)blockIdx.x * SF_T + threadIdx.x;
  if (o >= (long long)T * K) return;
  const long long t = o / K;
  const int k = (int)(o - t * K);
  double* rec = table + o * GATRES_SENSITIVITY_RECORD;
  double a[GATRES_SENSITIVITY_RECORD] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (accumulate) {
#pragma unroll
    for (int f = 0; f < GATRES_SENSITIVITY_RECORD; ++f) a[f] = rec[f];
  }
  for (long long s0 = 0; s0 < S; s0 += SF_U) {
    float r[SF_U];
#pragma unroll
    for (int u = 0; u < SF_U; ++u) {
      const long long s = s0 + u < S ? s0 + u : S - 1;      // (a row past the end reads the last one, which the loop below skips)
      r[u] = J[(s * T + t) * J_stride + k];
    }
#pragma unroll
    for (int u = 0; u < SF_U; ++u) {                        // (in snapshot order: the same association as a plain loop)
      if (s0 + u >= S) continue;
      const double j = (double)r[u], aj = fabs(j);
      if (r[u] != 0.f) a[0] += 1.0;
      a[1] += j;
      a[2] += aj;
      a[3] += j * j;
      a[4] = fmax(a[4], aj);
    }
  }
#pragma unroll
  for (int f = 0; f < GATRES_SENSITIVITY_RECORD; ++f) rec[f] = a[f];
}

// ---- spread --------------------------------------------------------------------------------------------------------------------
constexpr int SS_T = 256;

// One row per thread: the terms in sensor order, every operation in fp64 and rounded once (no contraction: the library is
// compiled with -ffp-contract=off).  The product of two fp32 values is exact in fp64.
__global__ __launch_bounds__(SS_T) void sensitivity_spread_kernel(const float* __restrict__ J, long long rows, int K,
                                                                  long long J_stride, const float* __restrict__ sigma,
                                                                  float* __restrict__ out) {
  const long long r = (long long)blockIdx.x * SS_T + threadIdx.x;
  if (r >= rows) return;
  const float* row = J + r * J_stride;
  double sum = 0.0;
  for (int k = 0; k < K; ++k) {
    const double p = (double)row[k] * (double)sigma[k];
    sum += p * p;
  }
  out[r] = (float)sqrt(sum);
}

}  // namespace

extern "C" int gatres_sensitivity_gather(const float* g_x, const uint8_t* mask, const float* fault, int32_t nodes_per_graph,
                                         int32_t num_graphs, const int32_t* observed, int32_t num_observed, double unit, float* J,
                                         int64_t J_rows, int64_t J_stride, int64_t first_row, void* stream) {
  if (!g_x || !mask || !observed || !J || nodes_per_graph <= 0 || num_graphs <= 0) return GATRES_E_BADARG;
  if (num_observed <= 0 || num_observed > nodes_per_graph) return GATRES_E_BADARG;
  if ((int64_t)nodes_per_graph * num_graphs > INT32_MAX) return GATRES_E_BADARG;
  if (J_stride < num_observed || J_rows <= 0 || J_rows > INT64_MAX / 4 / J_stride) return GATRES_E_BADARG;
  if (first_row < 0 || first_row > J_rows - num_graphs) return GATRES_E_BADARG;
  // (the rows [first_row, first_row + num_graphs) of J, strides included, against everything the launch reads)
  const uint64_t total = (uint64_t)nodes_per_graph * (uint64_t)num_graphs;
  const float* j0 = J + first_row * J_stride;
  const uint64_t j_bytes = 4 * (uint64_t)num_graphs * (uint64_t)J_stride;
  if (bytes_overlap(j0, j_bytes, g_x, 4 * total) || bytes_overlap(j0, j_bytes, mask, total) ||
      bytes_overlap(j0, j_bytes, observed, 4 * (uint64_t)num_observed) || (fault && bytes_overlap(j0, j_bytes, fault, 4)))
    return GATRES_E_BADARG;
  const long long elements = (long long)num_graphs * num_observed;
  long long wgs = (elements + SG_T - 1) / SG_T;
  if (wgs > 256) wgs = 256;
  hipLaunchKernelGGL(sensitivity_gather_kernel, dim3((unsigned)wgs), dim3(SG_T), 0, gatres_stream(stream), g_x, mask, fault,
                     (int)nodes_per_graph, elements, observed, (int)num_observed, (float)unit, J, (long long)J_stride,
                     (long long)first_row);
  return gatres_launch_status();
}

extern "C" int gatres_sensitivity_fold(const float* J, int64_t num_snapshots, int32_t num_targets, int32_t num_observed,
                                       int64_t J_stride, double* table, int32_t accumulate, void* stream) {
  if (!J || !table || num_snapshots <= 0 || num_targets < 1 || num_observed < 1 || J_stride < num_observed) return GATRES_E_BADARG;
  if (num_snapshots > INT64_MAX / 4 / num_targets / J_stride) return GATRES_E_BADARG;
  static_assert(GATRES_SENSITIVITY_RECORD == 5, "record layout");
  const uint64_t records = (uint64_t)num_targets * (uint64_t)num_observed;
  if (bytes_overlap(J, 4 * (uint64_t)num_snapshots * (uint64_t)num_targets * (uint64_t)J_stride, table,
                    8 * GATRES_SENSITIVITY_RECORD * records)) return GATRES_E_BADARG;
  hipLaunchKernelGGL(sensitivity_fold_kernel, dim3((unsigned)((records + SF_T - 1) / SF_T)), dim3(SF_T), 0, gatres_stream(stream),
                     J, (long long)num_snapshots, (int)num_targets, (int)num_observed, (long long)J_stride, table,
                     (int)(accumulate != 0));
  return gatres_launch_status();
}

extern "C" int gatres_sensitivity_spread(const float* J, int64_t rows, int32_t num_observed, int64_t J_stride, const float* sigma,
                                         float* out, void* stream) {
  if (!J || !sigma || !out || rows <= 0 || num_observed < 1 || J_stride < num_observed) return GATRES_E_BADARG;
  if (rows > INT64_MAX / 4 / J_stride || (rows + SS_T - 1) / SS_T > INT32_MAX) return GATRES_E_BADARG;
  const uint64_t j_bytes = 4 * (uint64_t)rows * (uint64_t)J_stride, s_bytes = 4 * (uint64_t)num_observed, o_bytes = 4 * (uint64_t)rows;
  if (bytes_overlap(J, j_bytes, out, o_bytes) || bytes_overlap(sigma, s_bytes, out, o_bytes) ||
      bytes_overlap(J, j_bytes, sigma, s_bytes)) return GATRES_E_BADARG;
  hipLaunchKernelGGL(sensitivity_spread_kernel, dim3((unsigned)((rows + SS_T - 1) / SS_T)), dim3(SS_T), 0, gatres_stream(stream),
                     J, (long long)rows, (int)num_observed, (long long)J_stride, sigma, out);
  return gatres_launch_status();
}

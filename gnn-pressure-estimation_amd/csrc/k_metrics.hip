// Device side of the evaluation epoch (evaluation.py:240-351 of the reference, our evaluation.evaluate_store): the
// masked-metric moments of one batch (gatres_masked_metrics) -- one fixed-layout fp64 record per batch from which
// evaluation.metrics_from_moments forms the loss and the seven metrics of get_metric_fn_collection
// (utils/auxil.py:101-140,185-203) on the host.  (The epoch's staging launch, gatres_stage_rows_mask_required: k_stage.hip.)
//
// The moments kernel is ONE workgroup: each thread accumulates its strided elements in index order, the waves reduce by a
// fixed butterfly, thread 0 adds the 16 wave partials in wave order.  No atomics, no floating-point reordering between runs:
// the same bits on every run.  The descaled values are rounded exactly as torch rounds `scaled * std + mean` (a multiply and
// an add, each rounded to fp32, no contraction), so the per-element predicates -- |t| > 0.01 and |t - p| <= t * 0.1 -- and
// therefore the two counts are those of the host functions.  The sums themselves are fp64; the centred sums are taken in a
// second pass around the first pass's means (descaled pressures sit around 50 m: raw second moments would cancel).
#include "gatres_common.h"

namespace {

constexpr int MET_T = 1024;
constexpr int MET_WAVES = MET_T / GATRES_WAVE;
constexpr int MET_U = 8;               // strides per trip of the element loops

__device__ __forceinline__ double met_wave_sum(double v) {
#pragma unroll
  for (int off = GATRES_WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// Sum of v over the workgroup, the same association on every run; the result is valid in thread 0 only.
template <int F>
__device__ __forceinline__ void met_block_sum(double (&v)[F], double (*lds)[F]) {
  const int lane = threadIdx.x % GATRES_WAVE, wave = threadIdx.x / GATRES_WAVE;
#pragma unroll
  for (int f = 0; f < F; ++f) v[f] = met_wave_sum(v[f]);
  if (lane == 0)
#pragma unroll
    for (int f = 0; f < F; ++f) lds[wave][f] = v[f];
  __syncthreads();
  if (threadIdx.x == 0)
#pragma unroll
    for (int f = 0; f < F; ++f) {
      double s = 0.0;
      for (int w = 0; w < MET_WAVES; ++w) s += lds[w][f];
      v[f] = s;
    }
  __syncthreads();
}

__global__ __launch_bounds__(MET_T) void masked_metrics_kernel(const float* __restrict__ out, const float* __restrict__ y,
                                                               const uint8_t* __restrict__ mask, int N, float scale,
                                                               float offset, double* __restrict__ table, int slot,
                                                               int capacity, unsigned long long* __restrict__ cursor) {
  __shared__ double s_p1[MET_WAVES][9];
  __shared__ double s_p2[MET_WAVES][3];
  __shared__ double s_mean[2];
  const int tid = threadIdx.x;
  // pass 1: counts and plain sums
  double a[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // M, loss, |d|, d^2, p, t, n_keep, rel, n_acc
  for (long long i0 = tid; i0 < N; i0 += MET_U * MET_T) {
    // (MET_U strides' loads in flight at once -- the launch is one workgroup, so it is load latency that it waits on; the
    //  elements are then taken in stride order: the same association as a plain loop)
    uint8_t mk[MET_U];
    float ov[MET_U], yv[MET_U];
#pragma unroll
    for (int u = 0; u < MET_U; ++u) {
      const long long i = i0 + u * MET_T;
      mk[u] = i < N ? mask[i] : 0;
      ov[u] = i < N ? out[i] : 0.f;
      yv[u] = i < N ? y[i] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < MET_U; ++u) {
      if (!mk[u]) continue;
      const float so = ov[u], st = yv[u];
      const double ds = (double)so - (double)st;
      const float p = gatres_descale(so, scale, offset), t = gatres_descale(st, scale, offset);
      const double d = (double)p - (double)t;
      a[0] += 1.0;
      a[1] += ds * ds;
      a[2] += fabs(d);
      a[3] += d * d;
      a[4] += (double)p;
      a[5] += (double)t;
      if (fabsf(t) > 0.01f) {                                        // calculate_rel_error: keep = |t| > 0.01
        a[6] += 1.0;
        a[7] += fabs(fabs((double)t - (double)p) / (double)t);
      }
      if (fabsf(__fsub_rn(t, p)) <= __fmul_rn(t, 0.1f)) a[8] += 1.0;  // calculate_accuracy(threshold=0.1)
    }
  }
  met_block_sum<9>(a, s_p1);
  if (tid == 0) {
    s_mean[0] = a[4] / a[0];
    s_mean[1] = a[5] / a[0];
  }
  __syncthreads();
  // pass 2: sums centred on the means
  const double pm = s_mean[0], tm = s_mean[1];
  double c[3] = {0.0, 0.0, 0.0};                                   // (p-pm)^2, (t-tm)^2, (p-pm)(t-tm)
  for (long long i0 = tid; i0 < N; i0 += MET_U * MET_T) {
    uint8_t mk[MET_U];
    float ov[MET_U], yv[MET_U];
#pragma unroll
    for (int u = 0; u < MET_U; ++u) {
      const long long i = i0 + u * MET_T;
      mk[u] = i < N ? mask[i] : 0;
      ov[u] = i < N ? out[i] : 0.f;
      yv[u] = i < N ? y[i] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < MET_U; ++u) {
      if (!mk[u]) continue;
      const double dp = (double)gatres_descale(ov[u], scale, offset) - pm, dt = (double)gatres_descale(yv[u], scale, offset) - tm;
      c[0] += dp * dp;
      c[1] += dt * dt;
      c[2] += dp * dt;
    }
  }
  met_block_sum<3>(c, s_p2);
  if (tid == 0) {
    int b = slot;
    if (cursor) {
      b += (int)cursor[0];
      cursor[0] += 1ULL;               // (one workgroup: nothing else in this launch reads the cursor)
    }
    if (b >= 0 && b < capacity) {
      double* r = table + (size_t)b * GATRES_METRICS_RECORD;
      r[0] = a[0]; r[1] = a[1]; r[2] = a[2]; r[3] = a[3]; r[4] = a[4]; r[5] = a[5];
      r[6] = c[0]; r[7] = c[1]; r[8] = c[2];
      r[9] = a[6]; r[10] = a[7]; r[11] = a[8];
      for (int f = 12; f < GATRES_METRICS_RECORD; ++f) r[f] = 0.0;
    }
  }
}

}  // namespace

extern "C" int gatres_masked_metrics(const float* out, const float* y, const uint8_t* mask, int32_t num_nodes, double scale,
                                     double offset, double* table, int32_t slot, int32_t capacity, uint64_t* cursor,
                                     void* stream) {
  if (!out || !y || !mask || !table || num_nodes <= 0 || capacity <= 0) return GATRES_E_BADARG;
  if (!cursor && (slot < 0 || slot >= capacity)) return GATRES_E_BADARG;
  hipLaunchKernelGGL(masked_metrics_kernel, dim3(1), dim3(MET_T), 0, gatres_stream(stream), out, y, mask, (int)num_nodes,
                     (float)scale, (float)offset, table, (int)slot, (int)capacity,
                     reinterpret_cast<unsigned long long*>(cursor));
  return gatres_launch_status();
}

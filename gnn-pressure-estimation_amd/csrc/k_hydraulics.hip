// Hydraulically consistent training snapshots (hydraulics.py: HydraulicNetwork.simulate / generate_store).  gatres.h states the
// model, the law at low flow and the solver; this file restates them on the device:
//   gatres_hydraulic_draw    random demands and roughness coefficients, a pure function of (seed, global scenario, cell);
//   gatres_hydraulic_solve   one workgroup per scenario: the whole Newton loop (global-gradient form) with the band matrix, the
//                            vectors and the pipe state in LDS, in fp64;
//   gatres_hydraulic_valid   the scenario filter: converged, not failed, every junction pressure inside a range.
// Every sum runs in a fixed order and nothing is shared between scenarios: a scenario's bits depend neither on the number of
// scenarios, nor on its position, nor on the launch.  No atomics.
#include "gatres_common.h"

#include <float.h>
#include <math.h>

namespace {

constexpr int HY_T = 256;                                  // threads of a solve workgroup
constexpr int HY_GRID_CAP = 1024;                          // workgroups of a solve launch; the scenarios beyond are taken by a loop
constexpr size_t HY_LDS_BUDGET = 160 * 1024;               // what one workgroup may take of a CU's LDS: all of it
constexpr double HY_LINEAR_G = 1e-7;                       // the law at low flow (gatres.h)
static_assert(HY_GRID_CAP == GATRES_HYD_GRID_CAP && HY_LDS_BUDGET == GATRES_HYD_LDS_BUDGET, "gatres.h states both");
static_assert(GATRES_HYD_STATUS == 4, "status record");

__device__ __forceinline__ bool hy_finite(double v) { return fabs(v) <= DBL_MAX; }        // (false for a NaN)

// pipe_headloss of gatres.h / hydraulics.py
__device__ __forceinline__ void pipe_headloss(double q, double r, double* h, double* g) {
  const double ra = r * pow(fabs(q), 0.852);
  double gg = 1.852 * ra, hh = ra * q;
  if (gg < HY_LINEAR_G) {
    gg = HY_LINEAR_G;
    hh = HY_LINEAR_G * q;
  }
  *h = hh;
  *g = gg;
}

// ---- the draws ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hydraulic_draw_kernel(const double* __restrict__ d_lo, const double* __restrict__ d_hi,
                                                             const double* __restrict__ c_lo, const double* __restrict__ c_hi,
                                                             long long S, int N, int P, uint64_t seed, long long first,
                                                             double* __restrict__ demand, double* __restrict__ roughness) {
  const long long cells = (long long)N + P, total = S * cells;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += gridDim.x * 256ll) {
    const long long s = i / cells;
    const int cell = (int)(i - s * cells);
    const uint64_t stream = mix64(seed + 0x9E3779B97F4A7C15ULL * ((uint64_t)(first + s) + 1));
    const uint64_t h = mix64(stream + 0xBF58476D1CE4E5B9ULL * ((uint64_t)cell + 1));
    const double u = (double)(h >> 11) * 0x1p-53;          // (a 53-bit integer: exact)
    if (cell < N) {
      const double lo = d_lo[cell], span = d_hi[cell] - lo;
      demand[s * N + cell] = lo + span * u;
    } else {
      const int p = cell - N;
      const double lo = c_lo[p], span = c_hi[p] - lo;
      roughness[s * P + p] = lo + span * u;
    }
  }
}

// ---- the solver --------------------------------------------------------------------------------------------------------------------
struct HydArgs {
  const int *pipe_a, *pipe_b;
  const double *coef, *q_start;
  const uint8_t* fixed;
  const double* elevation;
  const int *order, *position;
  const double *demand, *roughness, *fixed_head;
  long long fh_stride, S;
  int N, P, W, max_iter;
  double accuracy;
  float* pressure;
  double *head, *flow;
  int* status;
  double* final_dq;
};

// LDS of a workgroup, as gatres.h states it
static inline uint64_t hy_lds_bytes(uint64_t N, uint64_t P, uint64_t W) {
  return 8 * (N * (W + 1) + 2 * N + 4 * P) + 4 * (2 * P + N) + 64;
}

__global__ __launch_bounds__(HY_T) void hydraulic_solve_kernel(const HydArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hy_smem[];
  const int N = A.N, P = A.P, W = A.W, BW = W + 1, tid = threadIdx.x;
  double* band = reinterpret_cast<double*>(hy_smem);       // [N][BW]: band[r * BW + k] = A[r][r - k], rows in solver order
  double* y = band + (size_t)N * BW;                       // [N] the right-hand side, then the substitutions' vector
  double* H = y + N;                                       // [N] heads by solver row
  double* q = H + N;                                       // [P] flows
  double* rr = q + P;                                      // [P] resistance r_p of the scenario
  double* pinv = rr + P;                                   // [P] 1 / g_p; after the flow update |dq_p|
  double* yv = pinv + P;                                   // [P] h_p / g_p; after the flow update |q_p|
  double* red = yv + P;                                    // [4] the two sums of the stop rule
  int* sa = reinterpret_cast<int*>(red + 4);               // [P] solver rows of a pipe's ends
  int* sb = sa + P;                                        // [P]
  int* fx = sb + P;                                        // [N] fixed flag by solver row
  int* flag = fx + N;                                      // [4]: [0] static arrays refused, [1] scenario failed

  // the static arrays, checked: nothing below indexes with a value that was not checked here
  if (tid == 0) flag[0] = 0;
  __syncthreads();
  for (int n = tid; n < N; n += HY_T) {
    const int r = A.position[n];
    bool ok = r >= 0 && r < N;
    if (ok) ok = A.order[r] == n;                          // (holds for every n: position is a permutation, order its inverse)
    if (ok) fx[r] = A.fixed[n] ? 1 : 0;
    else flag[0] = 1;
  }
  __syncthreads();
  const bool perm_ok = flag[0] == 0;
  for (int p = tid; p < P; p += HY_T) {
    const int a = A.pipe_a[p], b = A.pipe_b[p];
    bool ok = perm_ok && a >= 0 && a < N && b >= 0 && b < N && a != b;
    int ra = 0, rb = 0;
    if (ok) {
      ra = A.position[a];
      rb = A.position[b];
      const int gap = ra > rb ? ra - rb : rb - ra;
      if (fx[ra] == 0 && fx[rb] == 0 && gap > W) ok = false;
    }
    if (!ok) {
      ra = rb = 0;
      flag[0] = 1;
    }
    sa[p] = ra;
    sb[p] = rb;
  }
  __syncthreads();
  const bool static_bad = flag[0] != 0;
  const double nan = __longlong_as_double(0x7FF8000000000000ll);

  for (long long s = blockIdx.x; s < A.S; s += gridDim.x) {
    const double* dem = A.demand + s * N;
    const double* rough = A.roughness + s * P;
    const double* fh = A.fixed_head + s * A.fh_stride;
    if (tid == 0) flag[1] = static_bad ? 1 : 0;
    __syncthreads();
    if (!static_bad) {
      for (int p = tid; p < P; p += HY_T) {
        const double c = rough[p], r = A.coef[p] / pow(c, 1.852), q0 = A.q_start[p];
        if (!(c > 0.0) || !hy_finite(c) || !(r > 0.0) || !hy_finite(r) || !hy_finite(q0)) flag[1] = 1;
        rr[p] = r;
        q[p] = q0;
      }
      for (int n = tid; n < N; n += HY_T) {
        const int r = A.position[n];
        const bool fixed = fx[r] != 0;
        const double v = fixed ? fh[n] : dem[n];
        if (!hy_finite(v)) flag[1] = 1;
        H[r] = fixed ? v : 0.0;
      }
    }
    __syncthreads();
    bool failed = flag[1] != 0, converged = false;         // (read from LDS after a barrier: the same in every thread)
    int iters = 0;
    double rel = 0.0;
    if (!failed)
      for (int it = 1; it <= A.max_iter; ++it) {
        iters = it;
        // the law at the present flows
        for (int p = tid; p < P; p += HY_T) {
          double h, g;
          pipe_headloss(q[p], rr[p], &h, &g);
          pinv[p] = 1.0 / g;
          yv[p] = h / g;
        }
        __syncthreads();
        // assembly: one thread per row, over the pipes in pipe order
        for (int n = tid; n < N; n += HY_T) {
          const int r = A.position[n];
          double* row = band + (size_t)r * BW;
          for (int k = 0; k < BW; ++k) row[k] = 0.0;
          if (fx[r]) {
            row[0] = 1.0;
            y[r] = H[r];
          } else {
            double diag = 0.0, f = -dem[n];
            for (int p = 0; p < P; ++p) {
              const int a = sa[p], b = sb[p];
              if (a != r && b != r) continue;
              const int o = a == r ? b : a;
              const double pi = pinv[p], t = q[p] - yv[p];
              diag += pi;
              f = b == r ? f + t : f - t;
              if (fx[o]) f += pi * H[o];
              else if (o < r) row[r - o] -= pi;            // (r - o <= W: checked above)
            }
            row[0] = diag;
            y[r] = f;
          }
        }
        __syncthreads();
        // banded LDL^T, column by column, the columns left unscaled (v_ij = L_ij d_j), with the forward substitution
        bool bad = false;
        for (int j = 0; j < N; ++j) {
          const double d = band[(size_t)j * BW];
          if (!(d > 0.0) || !hy_finite(d)) {               // (the same value in every thread)
            bad = true;
            break;
          }
          const int m = W < N - 1 - j ? W : N - 1 - j;
          const double zj = y[j] / d;
          for (int e = tid; e < m * m; e += HY_T) {
            const int r = e / m + 1, c = e - (r - 1) * m + 1;
            if (c <= r) {
              const double vr = band[(size_t)(j + r) * BW + r], vc = band[(size_t)(j + c) * BW + c];
              band[(size_t)(j + r) * BW + (r - c)] -= vr * (vc / d);
            }
          }
          for (int t = tid; t < m; t += HY_T) y[j + 1 + t] -= band[(size_t)(j + 1 + t) * BW + (t + 1)] * zj;
          __syncthreads();
        }
        if (bad) {
          failed = true;
          break;
        }
        // backward substitution, column by column
        for (int k = N - 1; k >= 0; --k) {
          const double xk = y[k] / band[(size_t)k * BW];
          const int m = W < k ? W : k;
          for (int t = tid + 1; t <= m; t += HY_T) y[k - t] -= band[(size_t)k * BW + t] * xk;
          if (tid == 0) H[k] = xk;
          __syncthreads();
        }
        // the flows
        for (int p = tid; p < P; p += HY_T) {
          const double dq = yv[p] - (H[sa[p]] - H[sb[p]]) * pinv[p], qn = q[p] - dq;
          q[p] = qn;
          pinv[p] = fabs(dq);
          yv[p] = fabs(qn);
        }
        __syncthreads();
        if (tid == 0 || tid == 64) {                       // one thread per sum, in pipe order
          const double* v = tid == 0 ? pinv : yv;
          double sum = 0.0;
          for (int p = 0; p < P; ++p) sum += v[p];
          red[tid == 0 ? 0 : 1] = sum;
        }
        __syncthreads();
        const double dqs = red[0], qs = red[1];
        if (!hy_finite(dqs) || !hy_finite(qs)) {
          failed = true;
          break;
        }
        rel = qs > 0.0 ? dqs / qs : (dqs > 0.0 ? __longlong_as_double(0x7FF0000000000000ll) : 0.0);
        converged = dqs <= A.accuracy * qs;
        if (converged) break;
      }
    // outputs, in the caller's order
    for (int n = tid; n < N; n += HY_T) {
      const double hv = failed ? nan : H[A.position[n]];   // (position was checked unless static_bad, which is failed)
      A.pressure[s * N + n] = (float)(hv - A.elevation[n]);
      if (A.head) A.head[s * N + n] = hv;
    }
    if (A.flow)
      for (int p = tid; p < P; p += HY_T) A.flow[s * P + p] = failed ? nan : q[p];
    if (tid == 0) {
      int* st = A.status + s * GATRES_HYD_STATUS;
      st[0] = iters;
      st[1] = converged && !failed ? 1 : 0;
      st[2] = failed ? 1 : 0;
      st[3] = 0;
      A.final_dq[s] = failed ? nan : rel;
    }
    __syncthreads();                                       // (the next scenario writes the shared arrays again)
  }
}

// ---- the filter --------------------------------------------------------------------------------------------------------------------
constexpr int HV_LANES = 64;

__global__ __launch_bounds__(HV_LANES) void hydraulic_valid_kernel(const float* __restrict__ pressure, const int* __restrict__ status,
                                                                   const uint8_t* __restrict__ fixed, long long S, int N,
                                                                   double p_lo, double p_hi, uint8_t* __restrict__ valid) {
  for (long long s = blockIdx.x; s < S; s += gridDim.x) {
    const int* st = status + s * GATRES_HYD_STATUS;
    int ok = st[1] != 0 && st[2] == 0 ? 1 : 0;
    for (int n = threadIdx.x; n < N; n += HV_LANES) {
      const double v = (double)pressure[s * N + n];
      if (fixed[n] == 0 && !(v >= p_lo && v <= p_hi)) ok = 0;
    }
#pragma unroll
    for (int d = HV_LANES / 2; d > 0; d >>= 1) ok &= __shfl_xor(ok, d, HV_LANES);
    if (threadIdx.x == 0) valid[s] = (uint8_t)ok;
  }
}

static inline bool bytes_overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a && b && a0 < b0 + nb && b0 < a0 + na;
}

// Does one of the written ranges overlap a read range or another written range?
static bool any_overlap(const void* const* wr, const uint64_t* wn, int nw, const void* const* rd, const uint64_t* rn, int nr) {
  for (int i = 0; i < nw; ++i) {
    for (int j = 0; j < nr; ++j)
      if (bytes_overlap(wr[i], wn[i], rd[j], rn[j])) return true;
    for (int j = i + 1; j < nw; ++j)
      if (bytes_overlap(wr[i], wn[i], wr[j], wn[j])) return true;
  }
  return false;
}

static inline bool hy_counts_ok(int64_t S, int32_t N, int32_t P) {
  return S >= 1 && N >= 1 && P >= 1 && S <= INT64_MAX / 64 / ((int64_t)N + (int64_t)P);    // (every byte count below fits)
}

}  // namespace

extern "C" int gatres_hydraulic_draw(const double* d_lo, const double* d_hi, const double* c_lo, const double* c_hi,
                                     int64_t num_scenarios, int32_t num_nodes, int32_t num_pipes, uint64_t seed,
                                     int64_t first_scenario, double* demand, double* roughness, void* stream) {
  if (!d_lo || !d_hi || !c_lo || !c_hi || !demand || !roughness) return GATRES_E_BADARG;
  if (!hy_counts_ok(num_scenarios, num_nodes, num_pipes)) return GATRES_E_BADARG;
  if (first_scenario < 0 || first_scenario > (1ll << 62) - num_scenarios) return GATRES_E_BADARG;
  const uint64_t S = (uint64_t)num_scenarios, N = (uint64_t)num_nodes, P = (uint64_t)num_pipes;
  const void* wr[2] = {demand, roughness};
  const uint64_t wn[2] = {8 * S * N, 8 * S * P};
  const void* rd[4] = {d_lo, d_hi, c_lo, c_hi};
  const uint64_t rn[4] = {8 * N, 8 * N, 8 * P, 8 * P};
  if (any_overlap(wr, wn, 2, rd, rn, 4)) return GATRES_E_BADARG;
  const uint64_t total = S * (N + P);
  uint64_t wgs = (total + 255) / 256;
  if (wgs > 4096) wgs = 4096;
  hipLaunchKernelGGL(hydraulic_draw_kernel, dim3((unsigned)wgs), dim3(256), 0, gatres_stream(stream), d_lo, d_hi, c_lo, c_hi,
                     (long long)num_scenarios, (int)num_nodes, (int)num_pipes, seed, (long long)first_scenario, demand, roughness);
  return gatres_launch_status();
}

extern "C" int gatres_hydraulic_solve(const int32_t* pipe_a, const int32_t* pipe_b, const double* coef, const double* q_start,
                                      const uint8_t* fixed, const double* elevation, const int32_t* order, const int32_t* position,
                                      int32_t half_bandwidth, const double* demand, const double* roughness,
                                      const double* fixed_head, int64_t fixed_head_stride, int64_t num_scenarios, int32_t num_nodes,
                                      int32_t num_pipes, double accuracy, int32_t max_iter, float* pressure, double* head,
                                      double* flow, int32_t* status, double* final_dq, void* stream) {
  if (!pipe_a || !pipe_b || !coef || !q_start || !fixed || !elevation || !order || !position) return GATRES_E_BADARG;
  if (!demand || !roughness || !fixed_head || !pressure || !status || !final_dq) return GATRES_E_BADARG;
  if (!hy_counts_ok(num_scenarios, num_nodes, num_pipes) || num_nodes < 2) return GATRES_E_BADARG;
  if (half_bandwidth < 1 || half_bandwidth > num_nodes - 1) return GATRES_E_BADARG;
  if (max_iter < 1 || !(accuracy > 0.0) || !(accuracy <= DBL_MAX)) return GATRES_E_BADARG;
  if (fixed_head_stride != 0 && fixed_head_stride != (int64_t)num_nodes) return GATRES_E_BADARG;
  const uint64_t S = (uint64_t)num_scenarios, N = (uint64_t)num_nodes, P = (uint64_t)num_pipes;
  const uint64_t lds = hy_lds_bytes(N, P, (uint64_t)half_bandwidth);
  if (lds > HY_LDS_BUDGET) return GATRES_E_BADARG;
  const void* wr[5] = {pressure, head, flow, status, final_dq};
  const uint64_t wn[5] = {4 * S * N, 8 * S * N, 8 * S * P, 4 * GATRES_HYD_STATUS * S, 8 * S};
  const void* rd[11] = {pipe_a, pipe_b, coef, q_start, fixed, elevation, order, position, demand, roughness, fixed_head};
  const uint64_t rn[11] = {4 * P, 4 * P, 8 * P, 8 * P, N, 8 * N, 4 * N, 4 * N, 8 * S * N, 8 * S * P,
                           fixed_head_stride ? 8 * S * N : 8 * N};
  if (any_overlap(wr, wn, 5, rd, rn, 11)) return GATRES_E_BADARG;
  if (lds > 64 * 1024) {                                   // (past the 64 KB a kernel gets unasked; per device)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&hydraulic_solve_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return (int)e;
    }
  }
  HydArgs a;
  a.pipe_a = pipe_a; a.pipe_b = pipe_b; a.coef = coef; a.q_start = q_start; a.fixed = fixed; a.elevation = elevation;
  a.order = order; a.position = position; a.demand = demand; a.roughness = roughness; a.fixed_head = fixed_head;
  a.fh_stride = (long long)fixed_head_stride; a.S = (long long)num_scenarios;
  a.N = (int)num_nodes; a.P = (int)num_pipes; a.W = (int)half_bandwidth; a.max_iter = (int)max_iter; a.accuracy = accuracy;
  a.pressure = pressure; a.head = head; a.flow = flow; a.status = status; a.final_dq = final_dq;
  const long long wgs = num_scenarios < HY_GRID_CAP ? (long long)num_scenarios : HY_GRID_CAP;
  hipLaunchKernelGGL(hydraulic_solve_kernel, dim3((unsigned)wgs), dim3(HY_T), (size_t)lds, gatres_stream(stream), a);
  return gatres_launch_status();
}

extern "C" int gatres_hydraulic_valid(const float* pressure, const int32_t* status, const uint8_t* fixed, int64_t num_scenarios,
                                      int32_t num_nodes, double p_lo, double p_hi, uint8_t* valid, void* stream) {
  if (!pressure || !status || !fixed || !valid) return GATRES_E_BADARG;
  if (!hy_counts_ok(num_scenarios, num_nodes, 1)) return GATRES_E_BADARG;
  if (!(p_lo <= p_hi)) return GATRES_E_BADARG;             // (a NaN fails the comparison)
  const uint64_t S = (uint64_t)num_scenarios, N = (uint64_t)num_nodes;
  const void* wr[1] = {valid};
  const uint64_t wn[1] = {S};
  const void* rd[3] = {pressure, status, fixed};
  const uint64_t rn[3] = {4 * S * N, 4 * GATRES_HYD_STATUS * S, N};
  if (any_overlap(wr, wn, 1, rd, rn, 3)) return GATRES_E_BADARG;
  const long long wgs = num_scenarios < 4096 ? (long long)num_scenarios : 4096;
  hipLaunchKernelGGL(hydraulic_valid_kernel, dim3((unsigned)wgs), dim3(HV_LANES), 0, gatres_stream(stream), pressure,
                     (const int*)status, fixed, (long long)num_scenarios, (int)num_nodes, p_lo, p_hi, valid);
  return gatres_launch_status();
}

// Hydraulically consistent training snapshots (hydraulics.py: HydraulicNetwork.simulate / generate_store).  gatres.h states the
// model, the law at low flow and the solver; this file restates them on the device:
//   gatres_hydraulic_draw    random demands and roughness coefficients, a pure function of (seed, global scenario, cell);
//   gatres_hydraulic_solve   one workgroup per scenario: the whole Newton loop (global-gradient form) with the band matrix, the
//                            vectors and the pipe state in LDS, in fp64;
//   gatres_hydraulic_valid   the scenario filter: converged, not failed, every junction pressure inside a range;
//   gatres_hydraulic_series  one workgroup per SERIES: T steps of one scenario with demand patterns and tanks, the band in LDS for
//                            the whole series, each step's Newton started from the step before (or cold), the tank levels moved
//                            by explicit Euler after every step;
//   gatres_hydraulic_series_valid   the series filter: every step converged, none failed or (unless allowed) clamped, in range.
// The Newton loop and the check of the static arrays are stated once, in k_hydraulics_dev.h, for both solver kernels.
// Every sum runs in a fixed order and nothing is shared between scenarios: a scenario's bits depend neither on the number of
// scenarios, nor on its position, nor on the launch.  No atomics.
#include "k_hydraulics_dev.h"

namespace {

constexpr int HY_GRID_CAP = 1024;                          // workgroups of a solve launch; the scenarios beyond are taken by a loop
constexpr size_t HY_LDS_BUDGET = 160 * 1024;               // what one workgroup may take of a CU's LDS: all of it
static_assert(HY_GRID_CAP == GATRES_HYD_GRID_CAP && HY_LDS_BUDGET == GATRES_HYD_LDS_BUDGET, "gatres.h states both");
static_assert(GATRES_HYD_STATUS == 4, "status record");

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
  double* band = reinterpret_cast<double*>(hy_smem);       // [N][BW]: the arrays of the Newton loop are described at HyLds
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
  const HyLds L = {band, y, H, q, rr, pinv, yv, red, sa, sb, fx};

  // the static arrays, checked: nothing below indexes with a value that was not checked here
  const bool static_bad = hy_check_static(L, A.position, A.order, A.fixed, A.pipe_a, A.pipe_b, N, P, W, flag, tid);
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
    if (!failed) {
      const HyNewton nw = hy_newton(L, A.position, dem, N, P, W, A.max_iter, A.accuracy, tid);     // k_hydraulics_dev.h
      iters = nw.iters;
      converged = nw.converged;
      failed = nw.failed;
      rel = nw.rel;
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

// ---- the series: T steps of one scenario, with demand patterns and tanks (gatres.h: THE SERIES) --------------------------------------
struct HydSeriesArgs {
  const int *pipe_a, *pipe_b;
  const double *coef, *q_start;
  const uint8_t* fixed;
  const double* elevation;
  const int *order, *position;
  const int* tank_node;
  const double *tank_area, *tank_min, *tank_max;
  const int* pattern;
  const double* mult;
  const double *demand, *roughness, *fixed_head, *level0;
  long long mult_stride, fh_stride, S;
  int T, N, P, W, K, M, max_iter, warm;
  double dt, accuracy;
  float* pressure;
  double *head, *flow, *level;
  int* status;
  double* final_dq;
};

// LDS of a series workgroup, as gatres.h states it
static inline uint64_t hy_series_lds_bytes(uint64_t N, uint64_t P, uint64_t W, uint64_t K) {
  return hy_lds_bytes(N, P, W) + 8 * N + 40 * K;
}

__global__ __launch_bounds__(HY_T) void hydraulic_series_kernel(const HydSeriesArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hy_smem[];
  const int N = A.N, P = A.P, W = A.W, K = A.K, M = A.M, T = A.T, BW = W + 1, tid = threadIdx.x;
  double* band = reinterpret_cast<double*>(hy_smem);       // the arrays of the Newton loop are described at HyLds
  double* y = band + (size_t)N * BW;
  double* H = y + N;
  double* q = H + N;
  double* rr = q + P;
  double* pinv = rr + P;
  double* yv = pinv + P;
  double* red = yv + P;                                    // [4]
  double* dem = red + 4;                                   // [N] the step's demand by node: demand * multiplier, rounded once
  double* lev = dem + N;                                   // [K] the tank levels of the present step
  double* area = lev + K;                                  // [K] the tank constants
  double* lmin = area + K;                                 // [K]
  double* lmax = lmin + K;                                 // [K]
  int* sa = reinterpret_cast<int*>(lmax + K);              // [P]
  int* sb = sa + P;                                        // [P]
  int* fx = sb + P;                                        // [N]
  int* tnode = fx + N;                                     // [K] a tank's node
  int* trow = tnode + K;                                   // [K] and its solver row
  int* flag = trow + K;                                    // [4]: [0] static arrays refused, [1] step failed, [2] a level clamped
  const HyLds L = {band, y, H, q, rr, pinv, yv, red, sa, sb, fx};

  bool perm_ok = false;
  bool static_bad = hy_check_static(L, A.position, A.order, A.fixed, A.pipe_a, A.pipe_b, N, P, W, flag, tid, &perm_ok);
  // the tanks and the patterns, checked the same way (flag[0] keeps the verdict)
  for (int k = tid; k < K; k += HY_T) {
    const int node = A.tank_node[k];
    const double ar = A.tank_area[k], lo = A.tank_min[k], hi = A.tank_max[k];
    bool ok = perm_ok && node >= 0 && node < N;
    if (ok) ok = A.fixed[node] != 0;
    for (int j = 0; ok && j < k; ++j) ok = A.tank_node[j] != node;
    if (!(ar > 0.0) || !hy_finite(ar) || !(lo <= hi)) ok = false;       // (a NaN limit fails the comparison)
    tnode[k] = ok ? node : 0;
    trow[k] = ok ? A.position[node] : 0;
    area[k] = ar;
    lmin[k] = lo;
    lmax[k] = hi;
    if (!ok) flag[0] = 1;
  }
  for (int n = tid; n < N; n += HY_T) {
    const int m = A.pattern[n];
    if (m < 0 || m >= M) flag[0] = 1;
  }
  __syncthreads();
  static_bad = flag[0] != 0;
  const double nan = __longlong_as_double(0x7FF8000000000000ll);

  for (long long s = blockIdx.x; s < A.S; s += gridDim.x) {
    const double* base = A.demand + s * N;
    const double* rough = A.roughness + s * P;
    const double* fh = A.fixed_head + s * A.fh_stride;
    const double* mult = A.mult + s * A.mult_stride;
    if (tid == 0) flag[1] = static_bad ? 1 : 0;
    __syncthreads();
    if (!static_bad) {
      for (int p = tid; p < P; p += HY_T) {
        const double c = rough[p], r = A.coef[p] / pow(c, 1.852), q0 = A.q_start[p];
        if (!(c > 0.0) || !hy_finite(c) || !(r > 0.0) || !hy_finite(r) || !hy_finite(q0)) flag[1] = 1;
        rr[p] = r;
        q[p] = q0;
      }
      for (int n = tid; n < N; n += HY_T) {                // the reservoirs keep their heads; a tank's row is set at every step
        const int r = A.position[n];
        const bool fixed = fx[r] != 0;
        const double v = fixed ? fh[n] : 0.0;
        if (!hy_finite(v)) flag[1] = 1;
        H[r] = v;
      }
      for (int k = tid; k < K; k += HY_T) lev[k] = A.level0[s * K + k];
    }
    for (int k = tid; k < K; k += HY_T) A.level[(s * (T + 1)) * K + k] = A.level0[s * K + k];       // row 0: as given
    __syncthreads();
    bool dead = flag[1] != 0;                              // (the same in every thread; once set, every later step is failed)

    for (int t = 0; t < T; ++t) {
      const long long st_i = s * T + t;
      int iters = 0;
      bool converged = false;
      double rel = 0.0;
      if (!dead) {
        // the step's inputs: one rounded product per junction, the tank heads, the start of the flows
        for (int m = tid; m < M; m += HY_T) {
          const double v = mult[(long long)m * T + t];
          if (!(v >= 0.0) || !hy_finite(v)) flag[1] = 1;
        }
        for (int n = tid; n < N; n += HY_T) {
          double v = 0.0;
          if (fx[A.position[n]] == 0) {
            v = base[n] * mult[(long long)A.pattern[n] * T + t];
            if (!hy_finite(v)) flag[1] = 1;
          }
          dem[n] = v;
        }
        for (int k = tid; k < K; k += HY_T) {
          const double v = A.elevation[tnode[k]] + lev[k];
          if (!hy_finite(v)) flag[1] = 1;
          H[trow[k]] = v;
        }
        if (t > 0 && !A.warm)
          for (int p = tid; p < P; p += HY_T) q[p] = A.q_start[p];
        __syncthreads();
        dead = flag[1] != 0;
        if (!dead) {
          const HyNewton nw = hy_newton(L, A.position, dem, N, P, W, A.max_iter, A.accuracy, tid);   // k_hydraulics_dev.h
          iters = nw.iters;
          converged = nw.converged;
          dead = nw.failed;
          rel = nw.rel;
        }
      }
      // outputs, in the caller's order
      for (int n = tid; n < N; n += HY_T) {
        const double hv = dead ? nan : H[A.position[n]];   // (position was checked unless static_bad, which is dead)
        A.pressure[st_i * N + n] = (float)(hv - A.elevation[n]);
        if (A.head) A.head[st_i * N + n] = hv;
      }
      if (A.flow)
        for (int p = tid; p < P; p += HY_T) A.flow[st_i * P + p] = dead ? nan : q[p];
      // the levels: explicit Euler, one thread per tank, the tank's pipes added up in pipe order
      if (tid == 0) flag[2] = 0;
      __syncthreads();
      for (int k = tid; k < K; k += HY_T) {
        double nl = nan;
        if (!dead) {
          const int r = trow[k];
          double inflow = 0.0;
          for (int p = 0; p < P; ++p) {
            if (sb[p] == r) inflow += q[p];
            if (sa[p] == r) inflow -= q[p];
          }
          const double vol = inflow * A.dt;
          nl = lev[k] + vol / area[k];
          if (nl < lmin[k]) {
            nl = lmin[k];
            flag[2] = 1;
          } else if (nl > lmax[k]) {
            nl = lmax[k];
            flag[2] = 1;
          }
          lev[k] = nl;
        }
        A.level[(s * (T + 1) + t + 1) * K + k] = nl;
      }
      __syncthreads();
      if (tid == 0) {
        int* st = A.status + st_i * GATRES_HYD_STATUS;
        st[0] = iters;
        st[1] = converged && !dead ? 1 : 0;
        st[2] = dead ? 1 : 0;
        st[3] = !dead && flag[2] != 0 ? 1 : 0;
        A.final_dq[st_i] = dead ? nan : rel;
      }
    }
    __syncthreads();                                       // (the next series writes the shared arrays again)
  }
}

// ---- the filter --------------------------------------------------------------------------------------------------------------------
constexpr int HV_LANES = 64;

__global__ __launch_bounds__(HV_LANES) void hydraulic_series_valid_kernel(const float* __restrict__ pressure,
                                                                          const int* __restrict__ status,
                                                                          const uint8_t* __restrict__ fixed, long long S, int T, int N,
                                                                          double p_lo, double p_hi, int allow_limited,
                                                                          uint8_t* __restrict__ valid) {
  for (long long s = blockIdx.x; s < S; s += gridDim.x) {
    int ok = 1;
    for (int t = threadIdx.x; t < T; t += HV_LANES) {
      const int* st = status + (s * T + t) * GATRES_HYD_STATUS;
      if (st[1] == 0 || st[2] != 0 || (!allow_limited && st[3] != 0)) ok = 0;
    }
    for (int t = 0; t < T; ++t) {
      const float* row = pressure + (s * T + t) * N;
      for (int n = threadIdx.x; n < N; n += HV_LANES) {
        const double v = (double)row[n];
        if (fixed[n] == 0 && !(v >= p_lo && v <= p_hi)) ok = 0;
      }
    }
#pragma unroll
    for (int d = HV_LANES / 2; d > 0; d >>= 1) ok &= __shfl_xor(ok, d, HV_LANES);
    if (threadIdx.x == 0) valid[s] = (uint8_t)ok;
  }
}

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

extern "C" int gatres_hydraulic_series(const int32_t* pipe_a, const int32_t* pipe_b, const double* coef, const double* q_start,
                                       const uint8_t* fixed, const double* elevation, const int32_t* order, const int32_t* position,
                                       int32_t half_bandwidth, const int32_t* tank_node, const double* tank_area,
                                       const double* tank_min_level, const double* tank_max_level, int32_t num_tanks,
                                       const int32_t* pattern_of_node, const double* mult, int64_t mult_stride, int32_t num_patterns,
                                       const double* demand, const double* roughness, const double* fixed_head,
                                       int64_t fixed_head_stride, const double* initial_level, int64_t num_series, int32_t num_steps,
                                       int32_t num_nodes, int32_t num_pipes, double dt, int32_t warm_start, double accuracy,
                                       int32_t max_iter, float* pressure, double* head, double* flow, double* level, int32_t* status,
                                       double* final_dq, void* stream) {
  if (!pipe_a || !pipe_b || !coef || !q_start || !fixed || !elevation || !order || !position) return GATRES_E_BADARG;
  if (!pattern_of_node || !mult || !demand || !roughness || !fixed_head || !pressure || !status || !final_dq) return GATRES_E_BADARG;
  if (num_tanks < 0 || num_steps < 1 || num_patterns < 1) return GATRES_E_BADARG;
  if (num_tanks > 0 && (!tank_node || !tank_area || !tank_min_level || !tank_max_level || !initial_level || !level))
    return GATRES_E_BADARG;
  if (!hy_counts_ok(num_series, num_nodes, num_pipes) || num_nodes < 2) return GATRES_E_BADARG;
  // every byte count below fits: S * (T + 1) * (N + P + K) * 64 and S * M * T * 64
  const int64_t per_step = (int64_t)num_nodes + (int64_t)num_pipes + (int64_t)num_tanks + GATRES_HYD_STATUS;
  if (num_series > INT64_MAX / 64 / per_step / ((int64_t)num_steps + 1)) return GATRES_E_BADARG;
  if ((int64_t)num_patterns > INT64_MAX / 64 / num_series / (int64_t)num_steps) return GATRES_E_BADARG;
  if (half_bandwidth < 1 || half_bandwidth > num_nodes - 1) return GATRES_E_BADARG;
  if (max_iter < 1 || !(accuracy > 0.0) || !(accuracy <= DBL_MAX)) return GATRES_E_BADARG;
  if (!(dt > 0.0) || !(dt <= DBL_MAX)) return GATRES_E_BADARG;
  if (fixed_head_stride != 0 && fixed_head_stride != (int64_t)num_nodes) return GATRES_E_BADARG;
  if (mult_stride != 0 && mult_stride != (int64_t)num_patterns * (int64_t)num_steps) return GATRES_E_BADARG;
  const uint64_t S = (uint64_t)num_series, T = (uint64_t)num_steps, N = (uint64_t)num_nodes, P = (uint64_t)num_pipes,
                 K = (uint64_t)num_tanks, M = (uint64_t)num_patterns;
  const uint64_t lds = hy_series_lds_bytes(N, P, (uint64_t)half_bandwidth, K);
  if (lds > HY_LDS_BUDGET) return GATRES_E_BADARG;
  const void* wr[6] = {pressure, head, flow, K ? level : nullptr, status, final_dq};
  const uint64_t wn[6] = {4 * S * T * N, 8 * S * T * N, 8 * S * T * P, 8 * S * (T + 1) * K, 4 * GATRES_HYD_STATUS * S * T, 8 * S * T};
  const void* rd[18] = {pipe_a, pipe_b, coef, q_start, fixed, elevation, order, position, K ? tank_node : nullptr,
                        K ? tank_area : nullptr, K ? tank_min_level : nullptr, K ? tank_max_level : nullptr, pattern_of_node, mult,
                        demand, roughness, fixed_head, K ? initial_level : nullptr};
  const uint64_t rn[18] = {4 * P, 4 * P, 8 * P, 8 * P, N, 8 * N, 4 * N, 4 * N, 4 * K, 8 * K, 8 * K, 8 * K, 4 * N,
                           mult_stride ? 8 * S * M * T : 8 * M * T, 8 * S * N, 8 * S * P, fixed_head_stride ? 8 * S * N : 8 * N,
                           8 * S * K};
  if (any_overlap(wr, wn, 6, rd, rn, 18)) return GATRES_E_BADARG;
  if (lds > 64 * 1024) {                                   // (past the 64 KB a kernel gets unasked; per device)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&hydraulic_series_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return (int)e;
    }
  }
  HydSeriesArgs a;
  a.pipe_a = pipe_a; a.pipe_b = pipe_b; a.coef = coef; a.q_start = q_start; a.fixed = fixed; a.elevation = elevation;
  a.order = order; a.position = position; a.tank_node = tank_node; a.tank_area = tank_area; a.tank_min = tank_min_level;
  a.tank_max = tank_max_level; a.pattern = pattern_of_node; a.mult = mult; a.demand = demand; a.roughness = roughness;
  a.fixed_head = fixed_head; a.level0 = initial_level; a.mult_stride = (long long)mult_stride;
  a.fh_stride = (long long)fixed_head_stride; a.S = (long long)num_series; a.T = (int)num_steps; a.N = (int)num_nodes;
  a.P = (int)num_pipes; a.W = (int)half_bandwidth; a.K = (int)num_tanks; a.M = (int)num_patterns; a.max_iter = (int)max_iter;
  a.warm = warm_start != 0 ? 1 : 0; a.dt = dt; a.accuracy = accuracy;
  a.pressure = pressure; a.head = head; a.flow = flow; a.level = level; a.status = status; a.final_dq = final_dq;
  const long long wgs = num_series < HY_GRID_CAP ? (long long)num_series : HY_GRID_CAP;
  hipLaunchKernelGGL(hydraulic_series_kernel, dim3((unsigned)wgs), dim3(HY_T), (size_t)lds, gatres_stream(stream), a);
  return gatres_launch_status();
}

extern "C" int gatres_hydraulic_series_valid(const float* pressure, const int32_t* status, const uint8_t* fixed, int64_t num_series,
                                             int32_t num_steps, int32_t num_nodes, double p_lo, double p_hi, int32_t allow_limited,
                                             uint8_t* valid, void* stream) {
  if (!pressure || !status || !fixed || !valid) return GATRES_E_BADARG;
  if (num_steps < 1 || !hy_counts_ok(num_series, num_nodes, 1)) return GATRES_E_BADARG;
  if (num_series > INT64_MAX / 64 / ((int64_t)num_nodes + GATRES_HYD_STATUS) / (int64_t)num_steps) return GATRES_E_BADARG;
  if (!(p_lo <= p_hi)) return GATRES_E_BADARG;             // (a NaN fails the comparison)
  const uint64_t S = (uint64_t)num_series, T = (uint64_t)num_steps, N = (uint64_t)num_nodes;
  const void* wr[1] = {valid};
  const uint64_t wn[1] = {S};
  const void* rd[3] = {pressure, status, fixed};
  const uint64_t rn[3] = {4 * S * T * N, 4 * GATRES_HYD_STATUS * S * T, N};
  if (any_overlap(wr, wn, 1, rd, rn, 3)) return GATRES_E_BADARG;
  const long long wgs = num_series < 4096 ? (long long)num_series : 4096;
  hipLaunchKernelGGL(hydraulic_series_valid_kernel, dim3((unsigned)wgs), dim3(HV_LANES), 0, gatres_stream(stream), pressure,
                     (const int*)status, fixed, (long long)num_series, (int)num_steps, (int)num_nodes, p_lo, p_hi,
                     (int)(allow_limited != 0), valid);
  return gatres_launch_status();
}

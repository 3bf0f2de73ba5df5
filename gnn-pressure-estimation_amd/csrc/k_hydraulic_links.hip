// Pumps, check valves, closed links and minor losses in the device hydraulic solver (hydraulics.py: a HydraulicNetwork with a
// special link or a minor loss).  gatres.h states THE LINK LAW; this file restates the two solver kernels of k_hydraulics.hip
// around hy_newton<true> (k_hydraulics_dev.h), which differs from the pipe-only loop in the law alone:
//   gatres_hydraulic_solve_links    one workgroup per scenario, as gatres_hydraulic_solve;
//   gatres_hydraulic_series_links   one workgroup per series, as gatres_hydraulic_series, the pump speeds following patterns.
// With kinds 0, no flags, m = 0 and no pumps both give every bit of their pipe-only counterparts.  Every loop is bounded, every
// sum runs in a fixed order, nothing is shared between scenarios.  No atomics.
#include "k_hydraulics_dev.h"

namespace {

constexpr int HY_GRID_CAP = GATRES_HYD_GRID_CAP;
constexpr size_t HY_LDS_BUDGET = GATRES_HYD_LDS_BUDGET;
static_assert(GATRES_HYD_STATUS == 4, "status record");
static_assert(GATRES_HYD_LINK_CHECK == 1 && GATRES_HYD_LINK_CLOSED == 2 && GATRES_HYD_PIPE == 0 && GATRES_HYD_PUMP == 1, "gatres.h");

static inline uint64_t hy_series_links_lds_bytes(uint64_t N, uint64_t P, uint64_t W, uint64_t K, uint64_t Kp) {
  return hy_links_lds_bytes(N, P, W, Kp) + 8 * N + 40 * K;
}

__global__ __launch_bounds__(HY_T) void hydraulic_solve_links_kernel(const HydLinksArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hy_smem[];
  const int N = A.N, P = A.P, W = A.W, Kp = A.K.Kp, BW = W + 1, tid = threadIdx.x;
  double* band = reinterpret_cast<double*>(hy_smem);       // [N][BW]: the arrays of the Newton loop are described at HyLds
  double* y = band + (size_t)N * BW;
  double* H = y + N;
  double* q = H + N;
  double* rr = q + P;
  double* pinv = rr + P;
  double* yv = pinv + P;
  double* red = yv + P;                                    // [4]
  double* minor = red + 4;                                 // [P]
  double* pump = minor + P;                                // [Kp][HY_PUMP_REC]
  int* sa = reinterpret_cast<int*>(pump + (size_t)Kp * HY_PUMP_REC);     // [P]
  int* sb = sa + P;                                        // [P]
  int* fx = sb + P;                                        // [N]
  int* code = fx + N;                                      // [P]
  int* flag = code + P;                                    // [4]: [0] static arrays refused, [1] scenario failed
  const HyLds L = {band, y, H, q, rr, pinv, yv, red, sa, sb, fx, minor, pump, code};

  bool static_bad = hy_check_static(L, A.position, A.order, A.fixed, A.pipe_a, A.pipe_b, N, P, W, flag, tid);
  static_bad = hy_check_links(L, A.K, A.coef, P, flag, tid) || static_bad;
  const double nan = __longlong_as_double(0x7FF8000000000000ll);

  for (long long s = blockIdx.x; s < A.S; s += gridDim.x) {
    const double* dem = A.demand + s * N;
    const double* rough = A.roughness + s * P;
    const double* fh = A.fixed_head + s * A.fh_stride;
    const uint8_t* closed = A.K.closed ? A.K.closed + s * A.K.closed_stride : nullptr;
    if (tid == 0) flag[1] = static_bad ? 1 : 0;
    __syncthreads();
    if (!static_bad) {
      for (int k = tid; k < Kp; k += HY_T) hy_set_speed(pump + (size_t)k * HY_PUMP_REC, A.K.speed[s * A.K.speed_stride + k], &flag[1]);
      for (int n = tid; n < N; n += HY_T) {
        const int r = A.position[n];
        const bool fixed = fx[r] != 0;
        const double v = fixed ? fh[n] : dem[n];
        if (!hy_finite(v)) flag[1] = 1;
        H[r] = fixed ? v : 0.0;
      }
      __syncthreads();                                     // (a link's code reads its pump's speed)
      for (int p = tid; p < P; p += HY_T) {
        const int c = hy_link_code(L, p, closed, &flag[1]);
        const double q0 = A.q_start[p];
        double r = 0.0;
        if (!(c & HY_PUMP)) {                              // (a pump has no resistance: its roughness is not read)
          const double cr = rough[p];
          r = A.coef[p] / pow(cr, 1.852);
          if (!(cr > 0.0) || !hy_finite(cr) || !(r >= 0.0) || !hy_finite(r) || (r == 0.0 && !(minor[p] > 0.0))) flag[1] = 1;
        }
        if (!hy_finite(q0)) flag[1] = 1;
        code[p] = c;
        rr[p] = r;
        q[p] = (c & HY_SHUT) ? 0.0 : q0;
      }
    }
    __syncthreads();
    bool failed = flag[1] != 0, converged = false;         // (read from LDS after a barrier: the same in every thread)
    int iters = 0;
    double rel = 0.0;
    if (!failed) {
      const HyNewton nw = hy_newton<true>(L, A.position, dem, N, P, W, A.max_iter, A.accuracy, tid);
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
    for (int p = tid; p < P; p += HY_T) {
      if (A.flow) A.flow[s * P + p] = failed ? nan : q[p];
      A.K.link_state[s * P + p] = failed ? (uint8_t)0 : hy_link_state(code[p], q[p]);
    }
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

// ---- the series ------------------------------------------------------------------------------------------------------------------------
struct HydSeriesLinksArgs {
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
  HydLinkArgs L;
  const double* speed_mult;                                // [Ms][T]
  const int* speed_pattern;                                // [Kp]
  int Ms;
};

__global__ __launch_bounds__(HY_T) void hydraulic_series_links_kernel(const HydSeriesLinksArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hy_smem[];
  const int N = A.N, P = A.P, W = A.W, K = A.K, M = A.M, T = A.T, Kp = A.L.Kp, Ms = A.Ms, BW = W + 1, tid = threadIdx.x;
  double* band = reinterpret_cast<double*>(hy_smem);       // the arrays of the Newton loop are described at HyLds
  double* y = band + (size_t)N * BW;
  double* H = y + N;
  double* q = H + N;
  double* rr = q + P;
  double* pinv = rr + P;
  double* yv = pinv + P;
  double* red = yv + P;                                    // [4]
  double* dem = red + 4;                                   // [N] the step's demand by node
  double* lev = dem + N;                                   // [K] the tank levels of the present step
  double* area = lev + K;                                  // [K]
  double* lmin = area + K;                                 // [K]
  double* lmax = lmin + K;                                 // [K]
  double* minor = lmax + K;                                // [P]
  double* pump = minor + P;                                // [Kp][HY_PUMP_REC]
  int* sa = reinterpret_cast<int*>(pump + (size_t)Kp * HY_PUMP_REC);     // [P]
  int* sb = sa + P;                                        // [P]
  int* fx = sb + P;                                        // [N]
  int* tnode = fx + N;                                     // [K]
  int* trow = tnode + K;                                   // [K]
  int* code = trow + K;                                    // [P]
  int* flag = code + P;                                    // [4]: [0] static arrays refused, [1] step failed, [2] a level clamped
  const HyLds L = {band, y, H, q, rr, pinv, yv, red, sa, sb, fx, minor, pump, code};

  bool perm_ok = false;
  bool static_bad = hy_check_static(L, A.position, A.order, A.fixed, A.pipe_a, A.pipe_b, N, P, W, flag, tid, &perm_ok);
  static_bad = hy_check_links(L, A.L, A.coef, P, flag, tid) || static_bad;
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
  for (int k = tid; k < Kp; k += HY_T) {
    const int m = A.speed_pattern[k];
    if (m < 0 || m >= Ms) flag[0] = 1;
  }
  __syncthreads();
  static_bad = flag[0] != 0;
  const double nan = __longlong_as_double(0x7FF8000000000000ll);

  for (long long s = blockIdx.x; s < A.S; s += gridDim.x) {
    const double* base = A.demand + s * N;
    const double* rough = A.roughness + s * P;
    const double* fh = A.fixed_head + s * A.fh_stride;
    const double* mult = A.mult + s * A.mult_stride;
    const double* speed = A.L.speed + s * A.L.speed_stride;
    const uint8_t* closed = A.L.closed ? A.L.closed + s * A.L.closed_stride : nullptr;
    if (tid == 0) flag[1] = static_bad ? 1 : 0;
    __syncthreads();
    if (!static_bad) {
      for (int p = tid; p < P; p += HY_T) {
        const double q0 = A.q_start[p];
        double r = 0.0;
        if (!(code[p] & HY_PUMP)) {
          const double cr = rough[p];
          r = A.coef[p] / pow(cr, 1.852);
          if (!(cr > 0.0) || !hy_finite(cr) || !(r >= 0.0) || !hy_finite(r) || (r == 0.0 && !(minor[p] > 0.0))) flag[1] = 1;
        }
        if (!hy_finite(q0)) flag[1] = 1;
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
        // the step's inputs: one rounded product per junction and per pump, the tank heads, the start of the flows
        for (int m = tid; m < M; m += HY_T) {
          const double v = mult[(long long)m * T + t];
          if (!(v >= 0.0) || !hy_finite(v)) flag[1] = 1;
        }
        for (int m = tid; m < Ms; m += HY_T) {
          const double v = A.speed_mult[(long long)m * T + t];
          if (!(v >= 0.0) || !hy_finite(v)) flag[1] = 1;
        }
        for (int k = tid; k < Kp; k += HY_T)
          hy_set_speed(pump + (size_t)k * HY_PUMP_REC, speed[k] * A.speed_mult[(long long)A.speed_pattern[k] * T + t], &flag[1]);
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
        __syncthreads();                                   // (a link's code reads its pump's speed)
        for (int p = tid; p < P; p += HY_T) {
          const int c = hy_link_code(L, p, closed, &flag[1]);
          code[p] = c;
          if (c & HY_SHUT) q[p] = 0.0;                     // a shut link starts at rest, warm or cold
          else if (t > 0 && !A.warm) q[p] = A.q_start[p];
        }
        __syncthreads();
        dead = flag[1] != 0;
        if (!dead) {
          const HyNewton nw = hy_newton<true>(L, A.position, dem, N, P, W, A.max_iter, A.accuracy, tid);
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
      for (int p = tid; p < P; p += HY_T) {
        if (A.flow) A.flow[st_i * P + p] = dead ? nan : q[p];
        A.L.link_state[st_i * P + p] = dead ? (uint8_t)0 : hy_link_state(code[p], q[p]);
      }
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

}  // namespace

extern "C" int gatres_hydraulic_solve_links(const int32_t* pipe_a, const int32_t* pipe_b, const double* coef, const double* q_start,
                                            const uint8_t* fixed, const double* elevation, const int32_t* order,
                                            const int32_t* position, int32_t half_bandwidth, const double* demand,
                                            const double* roughness, const double* fixed_head, int64_t fixed_head_stride,
                                            int64_t num_scenarios, int32_t num_nodes, int32_t num_pipes, double accuracy,
                                            int32_t max_iter, float* pressure, double* head, double* flow, int32_t* status,
                                            double* final_dq, const uint8_t* link_kind, const uint8_t* link_flags,
                                            const double* minor, const int32_t* pump_link, const double* pump_h0,
                                            const double* pump_r, const double* pump_n, int32_t num_pumps, const double* speed,
                                            int64_t speed_stride, const uint8_t* closed, int64_t closed_stride, uint8_t* link_state,
                                            void* stream) {
  if (!pipe_a || !pipe_b || !coef || !q_start || !fixed || !elevation || !order || !position) return GATRES_E_BADARG;
  if (!demand || !roughness || !fixed_head || !pressure || !status || !final_dq) return GATRES_E_BADARG;
  if (!hy_counts_ok(num_scenarios, num_nodes, num_pipes) || num_nodes < 2) return GATRES_E_BADARG;
  if (!hy_link_args_ok(link_kind, link_flags, minor, pump_link, pump_h0, pump_r, pump_n, num_pumps, speed, speed_stride, closed,
                       closed_stride, link_state, num_pipes))
    return GATRES_E_BADARG;
  if (half_bandwidth < 1 || half_bandwidth > num_nodes - 1) return GATRES_E_BADARG;
  if (max_iter < 1 || !(accuracy > 0.0) || !(accuracy <= DBL_MAX)) return GATRES_E_BADARG;
  if (fixed_head_stride != 0 && fixed_head_stride != (int64_t)num_nodes) return GATRES_E_BADARG;
  const uint64_t S = (uint64_t)num_scenarios, N = (uint64_t)num_nodes, P = (uint64_t)num_pipes, Kp = (uint64_t)num_pumps;
  const uint64_t lds = hy_links_lds_bytes(N, P, (uint64_t)half_bandwidth, Kp);
  if (lds > HY_LDS_BUDGET) return GATRES_E_BADARG;
  const void* wr[6] = {pressure, head, flow, status, final_dq, link_state};
  const uint64_t wn[6] = {4 * S * N, 8 * S * N, 8 * S * P, 4 * GATRES_HYD_STATUS * S, 8 * S, S * P};
  const void* rd[20] = {pipe_a, pipe_b, coef, q_start, fixed, elevation, order, position, demand, roughness, fixed_head,
                        link_kind, link_flags, minor, Kp ? pump_link : nullptr, Kp ? pump_h0 : nullptr, Kp ? pump_r : nullptr,
                        Kp ? pump_n : nullptr, Kp ? speed : nullptr, closed};
  const uint64_t rn[20] = {4 * P, 4 * P, 8 * P, 8 * P, N, 8 * N, 4 * N, 4 * N, 8 * S * N, 8 * S * P,
                           fixed_head_stride ? 8 * S * N : 8 * N, P, P, 8 * P, 4 * Kp, 8 * Kp, 8 * Kp, 8 * Kp,
                           speed_stride ? 8 * S * Kp : 8 * Kp, closed_stride ? S * P : P};
  if (any_overlap(wr, wn, 6, rd, rn, 20)) return GATRES_E_BADARG;
  if (lds > 64 * 1024) {                                   // (past the 64 KB a kernel gets unasked; per device)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&hydraulic_solve_links_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return (int)e;
    }
  }
  HydLinksArgs a;
  a.pipe_a = pipe_a; a.pipe_b = pipe_b; a.coef = coef; a.q_start = q_start; a.fixed = fixed; a.elevation = elevation;
  a.order = order; a.position = position; a.demand = demand; a.roughness = roughness; a.fixed_head = fixed_head;
  a.fh_stride = (long long)fixed_head_stride; a.S = (long long)num_scenarios;
  a.N = (int)num_nodes; a.P = (int)num_pipes; a.W = (int)half_bandwidth; a.max_iter = (int)max_iter; a.accuracy = accuracy;
  a.pressure = pressure; a.head = head; a.flow = flow; a.status = status; a.final_dq = final_dq;
  a.K = hy_link_args(link_kind, link_flags, minor, pump_link, pump_h0, pump_r, pump_n, num_pumps, speed, speed_stride, closed,
                     closed_stride, link_state);
  const long long wgs = num_scenarios < HY_GRID_CAP ? (long long)num_scenarios : HY_GRID_CAP;
  hipLaunchKernelGGL(hydraulic_solve_links_kernel, dim3((unsigned)wgs), dim3(HY_T), (size_t)lds, gatres_stream(stream), a);
  return gatres_launch_status();
}

extern "C" int gatres_hydraulic_series_links(
    const int32_t* pipe_a, const int32_t* pipe_b, const double* coef, const double* q_start, const uint8_t* fixed,
    const double* elevation, const int32_t* order, const int32_t* position, int32_t half_bandwidth, const int32_t* tank_node,
    const double* tank_area, const double* tank_min_level, const double* tank_max_level, int32_t num_tanks,
    const int32_t* pattern_of_node, const double* mult, int64_t mult_stride, int32_t num_patterns, const double* demand,
    const double* roughness, const double* fixed_head, int64_t fixed_head_stride, const double* initial_level, int64_t num_series,
    int32_t num_steps, int32_t num_nodes, int32_t num_pipes, double dt, int32_t warm_start, double accuracy, int32_t max_iter,
    float* pressure, double* head, double* flow, double* level, int32_t* status, double* final_dq, const uint8_t* link_kind,
    const uint8_t* link_flags, const double* minor, const int32_t* pump_link, const double* pump_h0, const double* pump_r,
    const double* pump_n, int32_t num_pumps, const double* speed, int64_t speed_stride, const uint8_t* closed,
    int64_t closed_stride, const double* speed_mult, const int32_t* speed_pattern_of_pump, int32_t num_speed_patterns,
    uint8_t* link_state, void* stream) {
  if (!pipe_a || !pipe_b || !coef || !q_start || !fixed || !elevation || !order || !position) return GATRES_E_BADARG;
  if (!pattern_of_node || !mult || !demand || !roughness || !fixed_head || !pressure || !status || !final_dq) return GATRES_E_BADARG;
  if (num_tanks < 0 || num_steps < 1 || num_patterns < 1) return GATRES_E_BADARG;
  if (num_tanks > 0 && (!tank_node || !tank_area || !tank_min_level || !tank_max_level || !initial_level || !level))
    return GATRES_E_BADARG;
  if (!hy_counts_ok(num_series, num_nodes, num_pipes) || num_nodes < 2) return GATRES_E_BADARG;
  if (!hy_link_args_ok(link_kind, link_flags, minor, pump_link, pump_h0, pump_r, pump_n, num_pumps, speed, speed_stride, closed,
                       closed_stride, link_state, num_pipes))
    return GATRES_E_BADARG;
  if (num_speed_patterns < 0 || (num_pumps > 0 && (num_speed_patterns < 1 || !speed_mult || !speed_pattern_of_pump)))
    return GATRES_E_BADARG;
  // every byte count below fits: S * (T + 1) * (N + P + K) * 64, S * M * T * 64 and Ms * T * 64
  const int64_t per_step = (int64_t)num_nodes + (int64_t)num_pipes + (int64_t)num_tanks + GATRES_HYD_STATUS;
  if (num_series > INT64_MAX / 64 / per_step / ((int64_t)num_steps + 1)) return GATRES_E_BADARG;
  if ((int64_t)num_patterns > INT64_MAX / 64 / num_series / (int64_t)num_steps) return GATRES_E_BADARG;
  if ((int64_t)num_speed_patterns > INT64_MAX / 64 / (int64_t)num_steps) return GATRES_E_BADARG;
  if (half_bandwidth < 1 || half_bandwidth > num_nodes - 1) return GATRES_E_BADARG;
  if (max_iter < 1 || !(accuracy > 0.0) || !(accuracy <= DBL_MAX)) return GATRES_E_BADARG;
  if (!(dt > 0.0) || !(dt <= DBL_MAX)) return GATRES_E_BADARG;
  if (fixed_head_stride != 0 && fixed_head_stride != (int64_t)num_nodes) return GATRES_E_BADARG;
  if (mult_stride != 0 && mult_stride != (int64_t)num_patterns * (int64_t)num_steps) return GATRES_E_BADARG;
  const uint64_t S = (uint64_t)num_series, T = (uint64_t)num_steps, N = (uint64_t)num_nodes, P = (uint64_t)num_pipes,
                 K = (uint64_t)num_tanks, M = (uint64_t)num_patterns, Kp = (uint64_t)num_pumps,
                 Ms = Kp ? (uint64_t)num_speed_patterns : 0;
  const uint64_t lds = hy_series_links_lds_bytes(N, P, (uint64_t)half_bandwidth, K, Kp);
  if (lds > HY_LDS_BUDGET) return GATRES_E_BADARG;
  const void* wr[7] = {pressure, head, flow, K ? level : nullptr, status, final_dq, link_state};
  const uint64_t wn[7] = {4 * S * T * N, 8 * S * T * N, 8 * S * T * P, 8 * S * (T + 1) * K, 4 * GATRES_HYD_STATUS * S * T, 8 * S * T,
                          S * T * P};
  const void* rd[29] = {pipe_a, pipe_b, coef, q_start, fixed, elevation, order, position, K ? tank_node : nullptr,
                        K ? tank_area : nullptr, K ? tank_min_level : nullptr, K ? tank_max_level : nullptr, pattern_of_node, mult,
                        demand, roughness, fixed_head, K ? initial_level : nullptr, link_kind, link_flags, minor,
                        Kp ? pump_link : nullptr, Kp ? pump_h0 : nullptr, Kp ? pump_r : nullptr, Kp ? pump_n : nullptr,
                        Kp ? speed : nullptr, closed, Kp ? speed_mult : nullptr, Kp ? speed_pattern_of_pump : nullptr};
  const uint64_t rn[29] = {4 * P, 4 * P, 8 * P, 8 * P, N, 8 * N, 4 * N, 4 * N, 4 * K, 8 * K, 8 * K, 8 * K, 4 * N,
                           mult_stride ? 8 * S * M * T : 8 * M * T, 8 * S * N, 8 * S * P, fixed_head_stride ? 8 * S * N : 8 * N,
                           8 * S * K, P, P, 8 * P, 4 * Kp, 8 * Kp, 8 * Kp, 8 * Kp, speed_stride ? 8 * S * Kp : 8 * Kp,
                           closed_stride ? S * P : P, 8 * Ms * T, 4 * Kp};
  if (any_overlap(wr, wn, 7, rd, rn, 29)) return GATRES_E_BADARG;
  if (lds > 64 * 1024) {                                   // (past the 64 KB a kernel gets unasked; per device)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&hydraulic_series_links_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return (int)e;
    }
  }
  HydSeriesLinksArgs a;
  a.pipe_a = pipe_a; a.pipe_b = pipe_b; a.coef = coef; a.q_start = q_start; a.fixed = fixed; a.elevation = elevation;
  a.order = order; a.position = position; a.tank_node = tank_node; a.tank_area = tank_area; a.tank_min = tank_min_level;
  a.tank_max = tank_max_level; a.pattern = pattern_of_node; a.mult = mult; a.demand = demand; a.roughness = roughness;
  a.fixed_head = fixed_head; a.level0 = initial_level; a.mult_stride = (long long)mult_stride;
  a.fh_stride = (long long)fixed_head_stride; a.S = (long long)num_series; a.T = (int)num_steps; a.N = (int)num_nodes;
  a.P = (int)num_pipes; a.W = (int)half_bandwidth; a.K = (int)num_tanks; a.M = (int)num_patterns; a.max_iter = (int)max_iter;
  a.warm = warm_start != 0 ? 1 : 0; a.dt = dt; a.accuracy = accuracy;
  a.pressure = pressure; a.head = head; a.flow = flow; a.level = level; a.status = status; a.final_dq = final_dq;
  a.L = hy_link_args(link_kind, link_flags, minor, pump_link, pump_h0, pump_r, pump_n, num_pumps, speed, speed_stride, closed,
                     closed_stride, link_state);
  a.speed_mult = speed_mult; a.speed_pattern = speed_pattern_of_pump; a.Ms = (int)Ms;
  const long long wgs = num_series < HY_GRID_CAP ? (long long)num_series : HY_GRID_CAP;
  hipLaunchKernelGGL(hydraulic_series_links_kernel, dim3((unsigned)wgs), dim3(HY_T), (size_t)lds, gatres_stream(stream), a);
  return gatres_launch_status();
}

// First-order sensitivities of the device hydraulic solver and leak localisation (hydraulics.py: HydraulicNetwork.sensitivity,
// localize_leaks).  gatres.h states THE SENSITIVITIES; this file is the kernel of gatres_hydraulic_solve_links with a tail:
//   gatres_hydraulic_sensitivity   one workgroup per scenario runs hy_newton<true>, writes what the links launch writes, then
//                                  evaluates the law's g at the returned flows, assembles and factorises A once more and solves
//                                  the K unit right-hand sides at the sensors' rows, Kc at a time, against the resident factor.
// dh_ddemand = -A^-1 at the sensor rows, dh_droughness follows from it link by link, and the leak scores are sums over the
// sensors that never leave the LDS.  Every loop is bounded, every sum runs in a fixed order (k ascending), nothing is shared
// between scenarios.  No atomics.
#include "k_hydraulics_dev.h"

namespace {

constexpr int HY_GRID_CAP = GATRES_HYD_GRID_CAP;
constexpr size_t HY_LDS_BUDGET = GATRES_HYD_LDS_BUDGET;
static_assert(GATRES_HYD_STATUS == 4, "status record");

struct HydSensArgs {
  HydLinksArgs A;
  const int* sensor_node;                                  // [K]
  const double* readings;                                  // [S][K] or NULL
  int K, Kc;                                               // sensors; right-hand sides of a chunk
  double *dh_ddemand, *dh_droughness;                      // [S][K][N], [S][K][P]
  double *residual, *leak_flow, *score;                    // [S][K], [S][N], [S][N]
  int* best;                                               // [S]
};

// LDS of a workgroup, as gatres.h states it: the links arrays, the two score accumulators per row, and per right-hand side of
// a chunk its column and its residual
static inline uint64_t hy_sens_lds_bytes(uint64_t N, uint64_t P, uint64_t W, uint64_t Kp, uint64_t Kc) {
  return hy_links_lds_bytes(N, P, W, Kp) + 16 * N + 8 * Kc * (N + 1);
}

// WZ, WC, WL: the launch writes dh_ddemand, dh_droughness, the localisation outputs
template <bool WZ, bool WC, bool WL>
__global__ __launch_bounds__(HY_T) void hydraulic_sensitivity_kernel(const HydSensArgs B) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hy_smem[];
  const HydLinksArgs& A = B.A;
  const int N = A.N, P = A.P, W = A.W, Kp = A.K.Kp, BW = W + 1, K = B.K, Kc = B.Kc, tid = threadIdx.x;
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
  double* X = pump + (size_t)Kp * HY_PUMP_REC;             // [N][Kc] the chunk's right-hand sides by solver row, then Z
  double* rho = X + (size_t)N * Kc;                        // [Kc] the chunk's residuals (NaN: the sensor is missing)
  double* num = rho + Kc;                                  // [N] <z_n, rho> by solver row, at the end the score
  double* den = num + N;                                   // [N] <z_n, z_n> by solver row
  int* sa = reinterpret_cast<int*>(den + N);               // [P]
  int* sb = sa + P;                                        // [P]
  int* fx = sb + P;                                        // [N]
  int* code = fx + N;                                      // [P]
  int* flag = code + P;                                    // [4]: [0] static arrays refused, [1] scenario failed
  const HyLds L = {band, y, H, q, rr, pinv, yv, red, sa, sb, fx, minor, pump, code};

  bool static_bad = hy_check_static(L, A.position, A.order, A.fixed, A.pipe_a, A.pipe_b, N, P, W, flag, tid);
  static_bad = hy_check_links(L, A.K, A.coef, P, flag, tid) || static_bad;
  for (int k = tid; k < K; k += HY_T) {                    // a sensor outside the network fails the launch, as a bad static array
    const int n = B.sensor_node[k];
    if (n < 0 || n >= N) flag[0] = 1;
  }
  __syncthreads();
  static_bad = flag[0] != 0;
  const double nan = __longlong_as_double(0x7FF8000000000000ll);

  for (long long s = blockIdx.x; s < A.S; s += gridDim.x) {
    const double* dem = A.demand + s * N;
    const double* rough = A.roughness + s * P;
    const double* fh = A.fixed_head + s * A.fh_stride;
    const uint8_t* closed = A.K.closed ? A.K.closed + s * A.K.closed_stride : nullptr;
    if (tid == 0) flag[1] = static_bad ? 1 : 0;
    __syncthreads();
    if (!static_bad) {                                     // the scenario's inputs, as hydraulic_solve_links_kernel forms them
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
    // the outputs of the links launch, in the caller's order
    for (int n = tid; n < N; n += HY_T) {
      const double hv = failed ? nan : H[A.position[n]];   // (position was checked unless static_bad, which is failed)
      if (A.pressure) A.pressure[s * N + n] = (float)(hv - A.elevation[n]);
      if (A.head) A.head[s * N + n] = hv;
    }
    for (int p = tid; p < P; p += HY_T) {
      if (A.flow) A.flow[s * P + p] = failed ? nan : q[p];
      if (A.K.link_state) A.K.link_state[s * P + p] = failed ? (uint8_t)0 : hy_link_state(code[p], q[p]);
    }
    if (tid == 0) {
      if (A.status) {
        int* st = A.status + s * GATRES_HYD_STATUS;
        st[0] = iters;
        st[1] = converged && !failed ? 1 : 0;
        st[2] = failed ? 1 : 0;
        st[3] = 0;
      }
      if (A.final_dq) A.final_dq[s] = failed ? nan : rel;
    }

    if constexpr (WZ || WC || WL) {
      // the factor of A at the returned flows; H and q stay as they are
      bool dead = failed;                                  // (the same in every thread)
      if (!dead) {
        hy_law_gradients(L, rough, P, tid);
        __syncthreads();
        hy_assemble_matrix(L, A.position, N, P, W, tid);
        dead = hy_factorise(L, N, W, tid);
      }
      if constexpr (WL) {
        for (int r = tid; r < N; r += HY_T) num[r] = den[r] = 0.0;
        if (tid == 0) red[0] = red[1] = 0.0;               // |rho|^2 and the number of available sensors
      }
      for (int k0 = 0; k0 < K; k0 += Kc) {
        const int kc = K - k0 < Kc ? K - k0 : Kc;
        __syncthreads();                                   // (the chunk before has been read)
        if (!dead) {
          for (int e = tid; e < N * kc; e += HY_T) {
            const int r = e / kc, c = e - r * kc;
            X[(size_t)r * Kc + c] = 0.0;
          }
          __syncthreads();
          for (int c = tid; c < kc; c += HY_T) {
            const int r = A.position[B.sensor_node[k0 + c]];
            if (!fx[r]) X[(size_t)r * Kc + c] = 1.0;       // (a fixed-head sensor keeps a row of zeros)
          }
          __syncthreads();
          hy_substitute_multi(band, X, N, W, kc, Kc, tid);
          for (int e = tid; e < N * kc; e += HY_T) {       // Z by solver row: -(A^-1), exactly 0 at a fixed-head row
            const int r = e / kc, c = e - r * kc;
            const double v = X[(size_t)r * Kc + c] / band[(size_t)r * BW];
            X[(size_t)r * Kc + c] = fx[r] ? 0.0 : 0.0 - v;             // (0.0 - v: a zero stays +0.0)
          }
        }
        if constexpr (WL) {
          for (int c = tid; c < kc; c += HY_T) {
            const int n = B.sensor_node[k0 + c];
            const double rd = B.readings[s * K + k0 + c];
            const double v = failed ? nan : rd - (H[A.position[n]] - A.elevation[n]);
            rho[c] = v;
            if (B.residual) B.residual[s * K + k0 + c] = v;
          }
        }
        __syncthreads();
        if constexpr (WZ) {
          for (long long e = tid; e < (long long)kc * N; e += HY_T) {
            const int c = (int)(e / N), n = (int)(e - (long long)c * N);
            B.dh_ddemand[(s * K + k0 + c) * N + n] = dead ? nan : X[(size_t)A.position[n] * Kc + c];
          }
        }
        if constexpr (WC) {
          for (long long e = tid; e < (long long)kc * P; e += HY_T) {
            const int c = (int)(e / P), p = (int)(e - (long long)c * P);
            B.dh_droughness[(s * K + k0 + c) * P + p] =
                dead ? nan : (X[(size_t)sa[p] * Kc + c] - X[(size_t)sb[p] * Kc + c]) * yv[p];
          }
        }
        if constexpr (WL) {
          if (!dead) {
            for (int r = tid; r < N; r += HY_T) {          // one thread per row, over the chunk's sensors in order
              double a = num[r], b = den[r];
              for (int c = 0; c < kc; ++c) {
                const double rc = rho[c], z = X[(size_t)r * Kc + c];
                if (rc != rc) continue;                    // (a missing sensor)
                a += z * rc;
                b += z * z;
              }
              num[r] = a;
              den[r] = b;
            }
            if (tid == 0) {
              double r2 = red[0], cnt = red[1];
              for (int c = 0; c < kc; ++c) {
                const double rc = rho[c];
                if (rc != rc) continue;
                r2 += rc * rc;
                cnt += 1.0;
              }
              red[0] = r2;
              red[1] = cnt;
            }
          }
        }
      }
      if constexpr (WL) {
        __syncthreads();
        const bool none = !(red[1] > 0.0) || red[0] == 0.0;     // (the same in every thread)
        const double rn = sqrt(red[0]);
        for (int n = tid; n < N; n += HY_T) {
          double lf = nan, sc = nan;
          if (!dead) {                                     // (position was checked unless static_bad, which is dead)
            const int r = A.position[n];
            const double a = num[r], b = den[r];
            if (fx[r] == 0 && b != 0.0) {
              lf = a / b;
              if (!none) sc = a / (sqrt(b) * rn);
            }
            y[n] = sc;                                     // (y is free behind the Newton loop: the scores by node)
          }
          if (B.leak_flow) B.leak_flow[s * N + n] = lf;
          if (B.score) B.score[s * N + n] = sc;
        }
        __syncthreads();
        if (tid == 0 && B.best) {                          // the lowest node among those holding the largest score written
          int at = -1;
          double top = 0.0;
          if (!dead)
            for (int n = 0; n < N; ++n) {
              const double v = y[n];
              if (v == v && (at < 0 || v > top)) {
                at = n;
                top = v;
              }
            }
          B.best[s] = at;
        }
      }
    }
    __syncthreads();                                       // (the next scenario writes the shared arrays again)
  }
}

template <bool WZ, bool WC, bool WL>
static int hy_sens_launch(const HydSensArgs& a, uint64_t lds, void* stream) {
  const void* kernel = reinterpret_cast<const void*>(&hydraulic_sensitivity_kernel<WZ, WC, WL>);
  if (lds > 64 * 1024) {                                   // (past the 64 KB a kernel gets unasked; per device)
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return (int)e;
    }
  }
  const long long wgs = a.A.S < HY_GRID_CAP ? a.A.S : HY_GRID_CAP;
  hipLaunchKernelGGL((hydraulic_sensitivity_kernel<WZ, WC, WL>), dim3((unsigned)wgs), dim3(HY_T), (size_t)lds, gatres_stream(stream), a);
  return gatres_launch_status();
}

// The right-hand sides of a chunk: as many of the K as fit beside the links arrays and the accumulators; 0 where none does
static int32_t hy_sens_chunk(int32_t num_nodes, int32_t num_pipes, int32_t half_bandwidth, int32_t num_pumps, int32_t num_sensors) {
  if (num_nodes < 1 || num_pipes < 1 || half_bandwidth < 1 || num_pumps < 0 || num_sensors < 1) return 0;
  const uint64_t N = (uint64_t)num_nodes, base = hy_links_lds_bytes(N, (uint64_t)num_pipes, (uint64_t)half_bandwidth, (uint64_t)num_pumps) + 16 * N;
  if (base >= HY_LDS_BUDGET) return 0;
  const uint64_t fit = (HY_LDS_BUDGET - base) / (8 * (N + 1));
  return (int32_t)(fit < (uint64_t)num_sensors ? fit : (uint64_t)num_sensors);
}

}  // namespace

extern "C" int gatres_hydraulic_sensitivity(
    const int32_t* pipe_a, const int32_t* pipe_b, const double* coef, const double* q_start, const uint8_t* fixed,
    const double* elevation, const int32_t* order, const int32_t* position, int32_t half_bandwidth, const double* demand,
    const double* roughness, const double* fixed_head, int64_t fixed_head_stride, int64_t num_scenarios, int32_t num_nodes,
    int32_t num_pipes, double accuracy, int32_t max_iter, float* pressure, double* head, double* flow, int32_t* status,
    double* final_dq, const uint8_t* link_kind, const uint8_t* link_flags, const double* minor, const int32_t* pump_link,
    const double* pump_h0, const double* pump_r, const double* pump_n, int32_t num_pumps, const double* speed, int64_t speed_stride,
    const uint8_t* closed, int64_t closed_stride, uint8_t* link_state, const int32_t* sensor_node, int32_t num_sensors,
    int32_t chunk, const double* readings, double* dh_ddemand, double* dh_droughness, double* residual, double* leak_flow,
    double* score, int32_t* best, void* stream) {
  if (!pipe_a || !pipe_b || !coef || !q_start || !fixed || !elevation || !order || !position) return GATRES_E_BADARG;
  if (!demand || !roughness || !fixed_head || !sensor_node) return GATRES_E_BADARG;
  if (!hy_counts_ok(num_scenarios, num_nodes, num_pipes) || num_nodes < 2 || num_sensors < 1 || chunk < 0) return GATRES_E_BADARG;
  // (link_state may be NULL here: link_kind stands in for it in the shared check)
  if (!hy_link_args_ok(link_kind, link_flags, minor, pump_link, pump_h0, pump_r, pump_n, num_pumps, speed, speed_stride, closed,
                       closed_stride, link_state ? link_state : link_kind, num_pipes))
    return GATRES_E_BADARG;
  if (half_bandwidth < 1 || half_bandwidth > num_nodes - 1) return GATRES_E_BADARG;
  if (max_iter < 1 || !(accuracy > 0.0) || !(accuracy <= DBL_MAX)) return GATRES_E_BADARG;
  if (fixed_head_stride != 0 && fixed_head_stride != (int64_t)num_nodes) return GATRES_E_BADARG;
  // every byte count below fits: S * K * (N + P) * 64
  if ((int64_t)num_sensors > INT64_MAX / 64 / num_scenarios / ((int64_t)num_nodes + (int64_t)num_pipes)) return GATRES_E_BADARG;
  const bool localise = residual || leak_flow || score || best;
  if (localise != (readings != nullptr)) return GATRES_E_BADARG;
  const uint64_t S = (uint64_t)num_scenarios, N = (uint64_t)num_nodes, P = (uint64_t)num_pipes, Kp = (uint64_t)num_pumps,
                 K = (uint64_t)num_sensors;
  int32_t kc = hy_sens_chunk(num_nodes, num_pipes, half_bandwidth, num_pumps, num_sensors);
  if (kc < 1) return GATRES_E_BADARG;                      // (no room for one right-hand side beside the band)
  if (chunk > 0 && chunk < kc) kc = chunk;
  const uint64_t lds = hy_sens_lds_bytes(N, P, (uint64_t)half_bandwidth, Kp, (uint64_t)kc);
  if (lds > HY_LDS_BUDGET) return GATRES_E_BADARG;
  const void* wr[12] = {pressure, head, flow, status, final_dq, link_state, dh_ddemand, dh_droughness, residual, leak_flow, score, best};
  const uint64_t wn[12] = {4 * S * N, 8 * S * N, 8 * S * P, 4 * GATRES_HYD_STATUS * S, 8 * S, S * P, 8 * S * K * N, 8 * S * K * P,
                           8 * S * K, 8 * S * N, 8 * S * N, 4 * S};
  const void* rd[22] = {pipe_a, pipe_b, coef, q_start, fixed, elevation, order, position, demand, roughness, fixed_head,
                        link_kind, link_flags, minor, Kp ? pump_link : nullptr, Kp ? pump_h0 : nullptr, Kp ? pump_r : nullptr,
                        Kp ? pump_n : nullptr, Kp ? speed : nullptr, closed, sensor_node, readings};
  const uint64_t rn[22] = {4 * P, 4 * P, 8 * P, 8 * P, N, 8 * N, 4 * N, 4 * N, 8 * S * N, 8 * S * P,
                           fixed_head_stride ? 8 * S * N : 8 * N, P, P, 8 * P, 4 * Kp, 8 * Kp, 8 * Kp, 8 * Kp,
                           speed_stride ? 8 * S * Kp : 8 * Kp, closed_stride ? S * P : P, 4 * K, 8 * S * K};
  if (any_overlap(wr, wn, 12, rd, rn, 22)) return GATRES_E_BADARG;
  HydSensArgs b;
  HydLinksArgs& a = b.A;
  a.pipe_a = pipe_a; a.pipe_b = pipe_b; a.coef = coef; a.q_start = q_start; a.fixed = fixed; a.elevation = elevation;
  a.order = order; a.position = position; a.demand = demand; a.roughness = roughness; a.fixed_head = fixed_head;
  a.fh_stride = (long long)fixed_head_stride; a.S = (long long)num_scenarios;
  a.N = (int)num_nodes; a.P = (int)num_pipes; a.W = (int)half_bandwidth; a.max_iter = (int)max_iter; a.accuracy = accuracy;
  a.pressure = pressure; a.head = head; a.flow = flow; a.status = status; a.final_dq = final_dq;
  a.K = hy_link_args(link_kind, link_flags, minor, pump_link, pump_h0, pump_r, pump_n, num_pumps, speed, speed_stride, closed,
                     closed_stride, link_state);
  b.sensor_node = sensor_node; b.readings = readings; b.K = (int)num_sensors; b.Kc = (int)kc;
  b.dh_ddemand = dh_ddemand; b.dh_droughness = dh_droughness; b.residual = residual; b.leak_flow = leak_flow; b.score = score;
  b.best = best;
  // what the launch computes is a compile-time fact of the instantiation
  const int which = (dh_ddemand ? 1 : 0) | (dh_droughness ? 2 : 0) | (localise ? 4 : 0);
  switch (which) {
    case 0: return hy_sens_launch<false, false, false>(b, lds, stream);
    case 1: return hy_sens_launch<true, false, false>(b, lds, stream);
    case 2: return hy_sens_launch<false, true, false>(b, lds, stream);
    case 3: return hy_sens_launch<true, true, false>(b, lds, stream);
    case 4: return hy_sens_launch<false, false, true>(b, lds, stream);
    case 5: return hy_sens_launch<true, false, true>(b, lds, stream);
    case 6: return hy_sens_launch<false, true, true>(b, lds, stream);
    default: return hy_sens_launch<true, true, true>(b, lds, stream);
  }
}

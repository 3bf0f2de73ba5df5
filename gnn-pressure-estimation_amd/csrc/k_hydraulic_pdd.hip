// Pressure-driven demand in the device hydraulic solver (hydraulics.py: simulate(demand_model="pda")).  gatres.h states THE
// PRESSURE-DRIVEN DEMAND; this file restates the two kernels of k_hydraulic_emitters.hip around hy_newton_valves<true, PDD>
// (k_hydraulics_dev.h), the Newton loop of the emitters launches with the node term of the demand at every junction that draws:
//   gatres_hydraulic_solve_pdd    one workgroup per scenario, as gatres_hydraulic_solve_emitters;
//   gatres_hydraulic_series_pdd   one workgroup per series, as gatres_hydraulic_series_emitters, the delivered flows carried along
//                                 a warm series while a junction stays pressure-driven.
// With demand_model 0 both run hy_newton_valves<true, false> and give every bit of their emitters counterparts.  Every loop is
// bounded, every sum runs in a fixed order, nothing is shared between scenarios.  No atomics.
#include "k_hydraulics_dev.h"

namespace {

constexpr int HY_GRID_CAP = GATRES_HYD_GRID_CAP;
constexpr size_t HY_LDS_BUDGET = GATRES_HYD_LDS_BUDGET;
static_assert(GATRES_HYD_STATUS == 4, "status record");
static_assert(GATRES_HYD_LINK_CHECK == 1 && GATRES_HYD_LINK_CLOSED == 2 && GATRES_HYD_PIPE == 0 && GATRES_HYD_PUMP == 1 &&
                  GATRES_HYD_PRV == 2 && GATRES_HYD_PSV == 3, "gatres.h");

// the link and valve arrays of a launch, shared by both kernels
struct HydValveArgs {
  const uint8_t *link_kind, *link_flags;
  const double* minor;
  const int* pump_link;
  const double *pump_h0, *pump_r, *pump_n;
  const double* speed;
  const uint8_t* closed;
  long long speed_stride, closed_stride;
  int Kp;
  uint8_t* link_state;
  const int* valve_link;
  const uint8_t* valve_kind;
  const double* setting;
  long long setting_stride;
  int Kv;
  int* valve_changes;
};

// the emitter arrays of a launch, shared by both kernels
struct HydEmitterArgs {
  const int* node;
  const double* coef;
  const int* onset;                                        // (the series alone; NULL: every emitter is on from step 0)
  long long coef_stride, onset_stride;
  double exponent;
  int Ke;
  double* flow;
};

// the demand model of a launch, shared by both kernels
struct HydPddArgs {
  double pmin, preq, exponent;
  double* delivered;                                       // [S][N] (series [S][T][N]); may be NULL with demand_model 0
};

struct HydSolvePddArgs {
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
  HydValveArgs K;
  HydEmitterArgs E;
  HydPddArgs D;
};

constexpr uint64_t HY_EMITTER_LDS = 48;                    // per emitter: ce, z, q, 1 / g, h / g, its row and its node

// LDS of a workgroup, as gatres.h states it: the arrays of the valves launch, and per emitter the record above
static inline uint64_t hy_emitters_lds_bytes(uint64_t N, uint64_t P, uint64_t W, uint64_t Kp, uint64_t Kv, uint64_t Ke) {
  return 8 * (N * (W + 1) + 2 * N + 4 * P) + 4 * (2 * P + N) + 64 + 12 * P + 8 * HY_PUMP_REC * Kp + 24 * Kv + HY_EMITTER_LDS * Ke;
}

static inline uint64_t hy_series_emitters_lds_bytes(uint64_t N, uint64_t P, uint64_t W, uint64_t K, uint64_t Kp, uint64_t Kv,
                                                    uint64_t Ke) {
  return hy_emitters_lds_bytes(N, P, W, Kp, Kv, Ke) + 8 * N + 40 * K;
}

constexpr uint64_t HY_PDD_LDS = 32;                        // per node with demand_model 1: D, q_d, 1 / g, h / g

// The three scalars of the demand model, checked before anything uses them: Pmin and Preq finite, Preq - Pmin at least 0.1 m
// (EPANET's MINPDIFF), the exponent finite and positive with a finite 1 / exponent.
__device__ __forceinline__ bool hy_pdd_bad(const HydPddArgs& A) {
  const double dp = A.preq - A.pmin;
  return !hy_finite(A.pmin) || !hy_finite(A.preq) || !(dp >= 0.1) || !(A.exponent > 0.0) || !hy_finite(A.exponent) ||
         !hy_finite(1.0 / A.exponent);
}

// A node's record of the scenario or step: pressure-driven where it is a junction whose full demand d is positive; q_d starts at
// d unless it is kept (a warm series in which the junction was pressure-driven in the step before).  The elevation of such a
// junction must be finite, or *bad is set.
__device__ __forceinline__ void hy_pdd_start(const HyPdd& D, int n, bool fixed, double d, bool keep, int* bad) {
  const bool on = !fixed && d > 0.0, was_on = D.dd[n] > 0.0;
  if (on && !hy_finite(D.elevation[n] + D.pmin)) *bad = 1;
  D.dd[n] = on ? d : 0.0;
  if (!on) D.q[n] = 0.0;
  else if (!(keep && was_on)) D.q[n] = d;
  D.dinv[n] = 0.0;
  D.dy[n] = 0.0;
}

// The static emitter array and the exponent, checked, after hy_check_valve_links (flag[0] keeps the verdict; V.node holds the
// controlled nodes): an emitter's node in [0, N), listed once, a junction, not the controlled node of a regulating valve; the
// exponent finite and positive with a finite 1 / exponent.  Fills E.row, E.node and E.z; nothing indexes with an emitter's node
// that was not checked here.  Ends behind a barrier; returns true where something is not what gatres.h states.
__device__ __forceinline__ bool hy_check_emitters(const HyLds& L, const HyValves& V, const HyEmitters& E, const HydEmitterArgs& A,
                                                  const int* __restrict__ position, const double* __restrict__ elevation, int N,
                                                  bool perm_ok, int* flag, int tid) {
  if (tid == 0 && (!(A.exponent > 0.0) || !hy_finite(A.exponent) || !hy_finite(1.0 / A.exponent))) flag[0] = 1;
  for (int k = tid; k < E.Ke; k += HY_T) {
    const int node = A.node[k];
    bool ok = perm_ok && node >= 0 && node < N;
    for (int j = 0; ok && j < k; ++j) ok = A.node[j] != node;
    int row = 0;
    if (ok) {
      row = position[node];                                // (in [0, N): perm_ok)
      if (L.fx[row] != 0) ok = false;
      for (int j = 0; ok && j < V.Kv; ++j) ok = V.node[j] != node;      // (V.node holds 0 for a valve that was refused)
    }
    E.row[k] = ok ? row : 0;
    E.node[k] = ok ? node : 0;
    E.z[k] = ok ? elevation[node] : 0.0;
    E.ce[k] = -1.0;
    E.q[k] = 0.0;
    E.einv[k] = 0.0;
    E.ey[k] = 0.0;
    if (!ok) flag[0] = 1;
  }
  __syncthreads();
  return flag[0] != 0;
}

// An emitter's record of the scenario or step: C == 0 switches it off (ce = -1, q = +0.0); otherwise ce = C^(-n), and the flow
// starts at C unless it is kept (a warm series in which the emitter was on in the step before).  A bad C sets *bad.
__device__ __forceinline__ void hy_emitter_start(const HyEmitters& E, int k, double C, bool keep, int* bad) {
  if (!(C >= 0.0) || !hy_finite(C)) {
    *bad = 1;
    C = 0.0;
  }
  if (C == 0.0) {
    E.ce[k] = -1.0;
    E.q[k] = 0.0;
    return;
  }
  const bool was_on = E.ce[k] >= 0.0;
  E.ce[k] = pow(C, -E.n);                                  // (+inf and 0 are legal: the law's caps take them)
  if (!(keep && was_on)) E.q[k] = C;
}

// The static link and valve arrays, checked, after hy_check_static (flag[0] keeps the verdict; L.fx, L.sa and L.sb are filled, and
// are what they should be exactly where flag[0] is 0): fills L.minor, L.code (without HY_SHUT and without a status), the constants
// of L.pump, and V.link, V.row and V.node.  Nothing indexes with a pump index, a pump's link, a valve's link or a controlled node
// that was not checked here.  Ends behind a barrier; returns true where an array is not what gatres.h states.
__device__ __forceinline__ bool hy_check_valve_links(const HyLds& L, const HyValves& V, const HydValveArgs& K,
                                                     const double* __restrict__ coef, const int* __restrict__ pipe_a,
                                                     const int* __restrict__ pipe_b, int N, int P, int* flag, int tid) {
  const int Kp = K.Kp, Kv = K.Kv;
  const bool pipes_ok = flag[0] == 0;                      // (read behind hy_check_static's barrier: the same in every thread)
  __syncthreads();
  for (int p = tid; p < P; p += HY_T) {
    const int kind = K.link_kind[p], fl = K.link_flags[p];
    const double m = K.minor[p], cf = coef[p];
    const bool valve = kind == GATRES_HYD_PRV || kind == GATRES_HYD_PSV;
    bool ok = kind <= GATRES_HYD_PSV && fl <= (GATRES_HYD_LINK_CHECK | GATRES_HYD_LINK_CLOSED) && m >= 0.0 && hy_finite(m);
    if (kind == GATRES_HYD_PIPE && !(cf >= 0.0 && hy_finite(cf) && (cf > 0.0 || m > 0.0))) ok = false;
    if (valve && (fl & GATRES_HYD_LINK_CHECK)) ok = false;
    int code = 0;
    if (ok) {
      if (kind == GATRES_HYD_PUMP) code |= HY_PUMP | HY_CHECK;
      if (fl & GATRES_HYD_LINK_CHECK) code |= HY_CHECK;
      if (fl & GATRES_HYD_LINK_CLOSED) code |= HY_CLOSED;
    } else {
      flag[0] = 1;
    }
    L.code[p] = code;                                      // (a valve's bits come with its record, below)
    L.minor[p] = ok ? m : 0.0;
  }
  __syncthreads();
  for (int k = tid; k < Kp; k += HY_T) {
    const int link = K.pump_link[k];
    const double h0 = K.pump_h0[k], rp = K.pump_r[k], n = K.pump_n[k];
    bool ok = link >= 0 && link < P;
    if (ok) ok = K.link_kind[link] == GATRES_HYD_PUMP;
    for (int j = 0; ok && j < k; ++j) ok = K.pump_link[j] != link;
    if (!(h0 >= 0.0) || !hy_finite(h0) || !(rp > 0.0) || !hy_finite(rp) || !(n >= 1.0) || !hy_finite(n)) ok = false;
    double* rec = L.pump + (size_t)k * HY_PUMP_REC;
    rec[0] = ok ? h0 : 0.0;
    rec[1] = ok ? rp : 1.0;
    rec[2] = ok ? n : 1.0;
    rec[3] = rec[4] = rec[5] = 0.0;
    if (ok) L.code[link] |= k << HY_PUMP_SHIFT;            // (one pump per link: checked above)
    else flag[0] = 1;
  }
  // a valve: its link in range and of its kind, listed once, sharing no node with another valve, its controlled node a junction
  for (int k = tid; k < Kv; k += HY_T) {
    const int link = K.valve_link[k], kind = K.valve_kind[k];
    bool ok = pipes_ok && link >= 0 && link < P && (kind == GATRES_HYD_PRV || kind == GATRES_HYD_PSV);
    if (ok) ok = K.link_kind[link] == kind;
    int row = 0, node = 0;
    if (ok) {
      const int a = pipe_a[link], b = pipe_b[link];        // (in [0, N): pipes_ok)
      for (int j = 0; ok && j < k; ++j) {
        const int lj = K.valve_link[j];
        if (lj == link) ok = false;
        else if (lj >= 0 && lj < P) {
          const int aj = pipe_a[lj], bj = pipe_b[lj];
          if (aj == a || aj == b || bj == a || bj == b) ok = false;
        }
      }
      node = kind == GATRES_HYD_PRV ? b : a;
      row = kind == GATRES_HYD_PRV ? L.sb[link] : L.sa[link];
      if (L.fx[row] != 0) ok = false;
    }
    V.link[k] = ok ? link : 0;
    V.row[k] = ok ? row : 0;
    V.node[k] = ok ? node : 0;
    V.chg[k] = 0;
    V.hset[k] = 0.0;
    if (!ok) flag[0] = 1;
  }
  __syncthreads();
  for (int k = tid; k < Kv; k += HY_T)                     // (one valve per link: checked above; no pump's link is a valve's)
    if (flag[0] == 0) L.code[V.link[k]] |= HY_VALVE | (K.valve_kind[k] == GATRES_HYD_PSV ? HY_VALVE_PSV : 0);
  __syncthreads();
  for (int p = tid; p < P; p += HY_T) {                    // every pump link has its record, every valve link its valve
    const int code = L.code[p], kind = K.link_kind[p];
    bool ok = true;
    if (code & HY_PUMP) {
      const int k = code >> HY_PUMP_SHIFT;
      ok = k < Kp;
      if (ok) ok = K.pump_link[k] == p;
    } else if (kind == GATRES_HYD_PRV || kind == GATRES_HYD_PSV) {
      ok = (code & HY_VALVE) != 0;
    }
    if (!ok) {
      L.code[p] = 0;
      flag[0] = 1;
    }
  }
  __syncthreads();
  return flag[0] != 0;
}

// A pump's speed of the scenario or step: w^2 and w^(2-n), formed once.  Bad speeds set *bad.
__device__ __forceinline__ void hy_set_speed(double* rec, double w, int* bad) {
  const double w2 = w * w, w2n = w > 0.0 ? pow(w, 2.0 - rec[2]) : 0.0;
  if (!(w >= 0.0) || !hy_finite(w) || !hy_finite(w2) || !hy_finite(w2n)) *bad = 1;
  rec[3] = w2;                                             // (a bad speed fails the scenario before the law reads the record, and
  rec[4] = w2n;                                            //  the next scenario or step rewrites all three)
  rec[5] = w;
}

// A link's code of the scenario or step: HY_SHUT where the static flag, the scenario's byte or a pump speed of zero shuts it.  A
// valve's bits stay.
__device__ __forceinline__ int hy_link_code(const HyLds& L, int p, const uint8_t* closed, int* bad) {
  int code = L.code[p] & ~HY_SHUT;
  const int cl = closed ? closed[p] : 0;
  if (cl > 1) *bad = 1;
  if ((code & HY_CLOSED) || cl == 1 || ((code & HY_PUMP) && L.pump[(size_t)(code >> HY_PUMP_SHIFT) * HY_PUMP_REC + 5] == 0.0))
    code |= HY_SHUT;
  return code;
}

// link_state of gatres.h at the returned flow and status
__device__ __forceinline__ uint8_t hy_link_state(int code, double q) {
  if (code & HY_SHUT) return 2;
  if (code & HY_VALVE) return (uint8_t)hy_valve_status(code);
  return (code & HY_CHECK) && q < 0.0 ? 1 : 0;
}

// A valve's target head of the scenario, and its status at the start: ACTIVE unless its input shuts it, or kept (a warm series).
__device__ __forceinline__ void hy_valve_start(const HyLds& L, const HyValves& V, int k, double setting, const double* elevation,
                                               bool keep, int* bad) {
  const double hset = elevation[V.node[k]] + setting;
  if (!hy_finite(hset)) *bad = 1;
  V.hset[k] = hset;
  const int p = V.link[k];
  int c = L.code[p];
  if (c & HY_SHUT) c &= ~(HY_VALVE_ACTIVE | HY_VALVE_CLOSED);
  else if (!keep) c = (c & ~HY_VALVE_CLOSED) | HY_VALVE_ACTIVE;
  L.code[p] = c;
}

template <bool PDD>
__global__ __launch_bounds__(HY_T) void hydraulic_solve_pdd_kernel(const HydSolvePddArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hy_smem[];
  const int N = A.N, P = A.P, W = A.W, Kp = A.K.Kp, Kv = A.K.Kv, Ke = A.E.Ke, BW = W + 1, tid = threadIdx.x;
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
  double* hset = pump + (size_t)Kp * HY_PUMP_REC;          // [Kv]
  double* ece = hset + Kv;                                 // [Ke] each: the emitters' records are described at HyEmitters
  double* ez = ece + Ke;
  double* eq = ez + Ke;
  double* einv = eq + Ke;
  double* ey = einv + Ke;
  double* pdd = ey + Ke;                                   // [N] each, with PDD alone: the record is described at HyPdd
  const int Nd = PDD ? N : 0;
  int* sa = reinterpret_cast<int*>(pdd + 4 * (size_t)Nd);  // [P]
  int* sb = sa + P;                                        // [P]
  int* fx = sb + P;                                        // [N]
  int* code = fx + N;                                      // [P]
  int* vlink = code + P;                                   // [Kv] each
  int* vrow = vlink + Kv;
  int* vnode = vrow + Kv;
  int* vchg = vnode + Kv;
  int* erow = vchg + Kv;                                   // [Ke] each
  int* enode = erow + Ke;
  int* flag = enode + Ke;                                  // [4]: [0] static arrays refused, [1] scenario failed
  const HyLds L = {band, y, H, q, rr, pinv, yv, red, sa, sb, fx, minor, pump, code};
  const HyValves V = {hset, vlink, vrow, vnode, vchg, Kv};
  const HyEmitters E = {ece, ez, eq, einv, ey, erow, enode, Ke, 1.0 / A.E.exponent};
  HyPdd D;
  if constexpr (PDD) {
    D.dd = pdd;
    D.q = pdd + Nd;
    D.dinv = pdd + 2 * (size_t)Nd;
    D.dy = pdd + 3 * (size_t)Nd;
    D.elevation = A.elevation;
    D.pmin = A.D.pmin;
    D.dp = A.D.preq - A.D.pmin;
    D.n = 1.0 / A.D.exponent;
  }

  bool perm_ok = false;
  bool static_bad = hy_check_static(L, A.position, A.order, A.fixed, A.pipe_a, A.pipe_b, N, P, W, flag, tid, &perm_ok);
  static_bad = hy_check_valve_links(L, V, A.K, A.coef, A.pipe_a, A.pipe_b, N, P, flag, tid) || static_bad;
  static_bad = hy_check_emitters(L, V, E, A.E, A.position, A.elevation, N, perm_ok, flag, tid) || static_bad;
  if constexpr (PDD) {
    static_bad = hy_pdd_bad(A.D) || static_bad;            // (the launch's scalars: the same in every thread)
    for (int n = tid; n < N; n += HY_T) D.dd[n] = 0.0;     // (node n is always this thread's)
  }
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
        const bool fixed = A.fixed[n] != 0;                // (fx[r] of a controlled node still holds the last scenario's status)
        const double v = fixed ? fh[n] : dem[n];
        if (!hy_finite(v)) flag[1] = 1;
        H[r] = fixed ? v : 0.0;
        if constexpr (PDD) hy_pdd_start(D, n, fixed, v, false, &flag[1]);
      }
      __syncthreads();                                     // (a link's code reads its pump's speed)
      for (int p = tid; p < P; p += HY_T) {
        const int c = hy_link_code(L, p, closed, &flag[1]);
        const double q0 = A.q_start[p];
        double r = 0.0;
        if (!(c & (HY_PUMP | HY_VALVE))) {                 // (a pump and a valve have no resistance: their roughness is not read)
          const double cr = rough[p];
          r = A.coef[p] / pow(cr, 1.852);
          if (!(cr > 0.0) || !hy_finite(cr) || !(r >= 0.0) || !hy_finite(r) || (r == 0.0 && !(minor[p] > 0.0))) flag[1] = 1;
        }
        if (!hy_finite(q0)) flag[1] = 1;
        code[p] = c;
        rr[p] = r;
        q[p] = (c & HY_SHUT) ? 0.0 : q0;
      }
      __syncthreads();
      for (int k = tid; k < Kv; k += HY_T)
        hy_valve_start(L, V, k, A.K.setting[s * A.K.setting_stride + k], A.elevation, false, &flag[1]);
      for (int k = tid; k < Ke; k += HY_T) hy_emitter_start(E, k, A.E.coef[s * A.E.coef_stride + k], false, &flag[1]);
    }
    __syncthreads();
    bool failed = flag[1] != 0, converged = false;         // (read from LDS after a barrier: the same in every thread)
    int iters = 0, changes = 0;
    double rel = 0.0;
    if (!failed) {
      const HyNewtonValves nw = hy_newton_valves<true, PDD>(L, V, A.position, dem, N, P, W, A.max_iter, A.accuracy, tid, E, D);
      iters = nw.n.iters;
      converged = nw.n.converged;
      failed = nw.n.failed;
      rel = nw.n.rel;
      changes = nw.changes;
    }
    // outputs, in the caller's order
    for (int n = tid; n < N; n += HY_T) {
      const double hv = failed ? nan : H[A.position[n]];   // (position was checked unless static_bad, which is failed)
      A.pressure[s * N + n] = (float)(hv - A.elevation[n]);
      if (A.head) A.head[s * N + n] = hv;
      if (A.D.delivered) {                                 // q_d where the junction is pressure-driven, else the demand itself
        double dv = A.fixed[n] ? 0.0 : dem[n];
        if constexpr (PDD) {
          if (D.dd[n] > 0.0) dv = D.q[n];
        }
        A.D.delivered[s * N + n] = failed ? nan : dv;
      }
    }
    for (int p = tid; p < P; p += HY_T) {
      if (A.flow) A.flow[s * P + p] = failed ? nan : q[p];
      A.K.link_state[s * P + p] = failed ? (uint8_t)0 : hy_link_state(code[p], q[p]);
    }
    for (int k = tid; k < Ke; k += HY_T) A.E.flow[s * Ke + k] = failed ? nan : eq[k];
    if (tid == 0) {
      int* st = A.status + s * GATRES_HYD_STATUS;
      st[0] = iters;
      st[1] = converged && !failed ? 1 : 0;
      st[2] = failed ? 1 : 0;
      st[3] = 0;
      A.final_dq[s] = failed ? nan : rel;
      A.K.valve_changes[s] = failed ? 0 : changes;
    }
    __syncthreads();                                       // (the next scenario writes the shared arrays again)
  }
}

// ---- the series ------------------------------------------------------------------------------------------------------------------------
struct HydSeriesPddArgs {
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
  HydValveArgs L;
  HydEmitterArgs E;
  const double* speed_mult;                                // [Ms][T]
  const int* speed_pattern;                                // [Kp]
  int Ms;
  HydPddArgs D;
};

template <bool PDD>
__global__ __launch_bounds__(HY_T) void hydraulic_series_pdd_kernel(const HydSeriesPddArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hy_smem[];
  const int N = A.N, P = A.P, W = A.W, K = A.K, M = A.M, T = A.T, Kp = A.L.Kp, Kv = A.L.Kv, Ke = A.E.Ke, Ms = A.Ms, BW = W + 1,
            tid = threadIdx.x;
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
  double* hset = pump + (size_t)Kp * HY_PUMP_REC;          // [Kv]
  double* ece = hset + Kv;                                 // [Ke] each: the emitters' records are described at HyEmitters
  double* ez = ece + Ke;
  double* eq = ez + Ke;
  double* einv = eq + Ke;
  double* ey = einv + Ke;
  double* pdd = ey + Ke;                                   // [N] each, with PDD alone: the record is described at HyPdd
  const int Nd = PDD ? N : 0;
  int* sa = reinterpret_cast<int*>(pdd + 4 * (size_t)Nd);  // [P]
  int* sb = sa + P;                                        // [P]
  int* fx = sb + P;                                        // [N]
  int* tnode = fx + N;                                     // [K]
  int* trow = tnode + K;                                   // [K]
  int* code = trow + K;                                    // [P]
  int* vlink = code + P;                                   // [Kv] each
  int* vrow = vlink + Kv;
  int* vnode = vrow + Kv;
  int* vchg = vnode + Kv;
  int* erow = vchg + Kv;                                   // [Ke] each
  int* enode = erow + Ke;
  int* flag = enode + Ke;                                  // [4]: [0] static arrays refused, [1] step failed, [2] a level clamped
  const HyLds L = {band, y, H, q, rr, pinv, yv, red, sa, sb, fx, minor, pump, code};
  const HyValves V = {hset, vlink, vrow, vnode, vchg, Kv};
  const HyEmitters E = {ece, ez, eq, einv, ey, erow, enode, Ke, 1.0 / A.E.exponent};
  HyPdd D;
  if constexpr (PDD) {
    D.dd = pdd;
    D.q = pdd + Nd;
    D.dinv = pdd + 2 * (size_t)Nd;
    D.dy = pdd + 3 * (size_t)Nd;
    D.elevation = A.elevation;
    D.pmin = A.D.pmin;
    D.dp = A.D.preq - A.D.pmin;
    D.n = 1.0 / A.D.exponent;
  }

  bool perm_ok = false;
  bool static_bad = hy_check_static(L, A.position, A.order, A.fixed, A.pipe_a, A.pipe_b, N, P, W, flag, tid, &perm_ok);
  static_bad = hy_check_valve_links(L, V, A.L, A.coef, A.pipe_a, A.pipe_b, N, P, flag, tid) || static_bad;
  static_bad = hy_check_emitters(L, V, E, A.E, A.position, A.elevation, N, perm_ok, flag, tid) || static_bad;
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
  if constexpr (PDD) static_bad = hy_pdd_bad(A.D) || static_bad;       // (the launch's scalars: the same in every thread)
  const double nan = __longlong_as_double(0x7FF8000000000000ll);

  for (long long s = blockIdx.x; s < A.S; s += gridDim.x) {
    const double* base = A.demand + s * N;
    const double* rough = A.roughness + s * P;
    const double* fh = A.fixed_head + s * A.fh_stride;
    const double* mult = A.mult + s * A.mult_stride;
    const double* speed = A.L.speed + s * A.L.speed_stride;
    const uint8_t* closed = A.L.closed ? A.L.closed + s * A.L.closed_stride : nullptr;
    const double* ecoef = A.E.coef + s * A.E.coef_stride;
    const int* onset = A.E.onset ? A.E.onset + s * A.E.onset_stride : nullptr;
    if (tid == 0) flag[1] = static_bad ? 1 : 0;
    __syncthreads();
    if (!static_bad) {
      for (int k = tid; k < Ke; k += HY_T) {               // a bad coefficient fails the series from step 0 on, whatever its onset
        const double C = ecoef[k];
        if (!(C >= 0.0) || !hy_finite(C)) flag[1] = 1;
        ece[k] = -1.0;                                     // (off until a step switches it on)
        eq[k] = 0.0;
      }
      for (int p = tid; p < P; p += HY_T) {
        const double q0 = A.q_start[p];
        double r = 0.0;
        if (!(code[p] & (HY_PUMP | HY_VALVE))) {
          const double cr = rough[p];
          r = A.coef[p] / pow(cr, 1.852);
          if (!(cr > 0.0) || !hy_finite(cr) || !(r >= 0.0) || !hy_finite(r) || (r == 0.0 && !(minor[p] > 0.0))) flag[1] = 1;
        }
        if (!hy_finite(q0)) flag[1] = 1;
        rr[p] = r;
        q[p] = q0;
      }
      for (int n = tid; n < N; n += HY_T) {                // the reservoirs keep their heads; a tank's row is set at every step
        const bool fixed = A.fixed[n] != 0;
        const double v = fixed ? fh[n] : 0.0;
        if (!hy_finite(v)) flag[1] = 1;
        H[A.position[n]] = v;
        if constexpr (PDD) D.dd[n] = 0.0;                  // (no junction is pressure-driven before step 0)
      }
      for (int k = tid; k < K; k += HY_T) lev[k] = A.level0[s * K + k];
    }
    for (int k = tid; k < K; k += HY_T) A.level[(s * (T + 1)) * K + k] = A.level0[s * K + k];       // row 0: as given
    __syncthreads();
    bool dead = flag[1] != 0;                              // (the same in every thread; once set, every later step is failed)

    for (int t = 0; t < T; ++t) {
      const long long st_i = s * T + t;
      int iters = 0, changes = 0;
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
          if (A.fixed[n] == 0) {
            v = base[n] * mult[(long long)A.pattern[n] * T + t];
            if (!hy_finite(v)) flag[1] = 1;
          }
          dem[n] = v;
          if constexpr (PDD)                               // a warm series carries q_d along while the junction stays pressure-driven
            hy_pdd_start(D, n, A.fixed[n] != 0, v, t > 0 && A.warm, &flag[1]);
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
        for (int k = tid; k < Kv; k += HY_T)               // a warm series carries the statuses along with the flows
          hy_valve_start(L, V, k, A.L.setting[s * A.L.setting_stride + k], A.elevation, t > 0 && A.warm, &flag[1]);
        for (int k = tid; k < Ke; k += HY_T)               // a warm series carries an emitter's flow along while it stays on
          hy_emitter_start(E, k, onset && t < onset[k] ? 0.0 : ecoef[k], t > 0 && A.warm, &flag[1]);
        __syncthreads();
        dead = flag[1] != 0;
        if (!dead) {
          const HyNewtonValves nw = hy_newton_valves<true, PDD>(L, V, A.position, dem, N, P, W, A.max_iter, A.accuracy, tid, E, D);
          iters = nw.n.iters;
          converged = nw.n.converged;
          dead = nw.n.failed;
          rel = nw.n.rel;
          changes = nw.changes;
        }
      }
      // outputs, in the caller's order
      for (int n = tid; n < N; n += HY_T) {
        const double hv = dead ? nan : H[A.position[n]];   // (position was checked unless static_bad, which is dead)
        A.pressure[st_i * N + n] = (float)(hv - A.elevation[n]);
        if (A.head) A.head[st_i * N + n] = hv;
        if (A.D.delivered) {                               // q_d where the junction is pressure-driven, else the step's demand
          double dv = dead ? nan : dem[n];                 // (0 at a fixed node; not read where dead: a NaN either way)
          if constexpr (PDD) {
            if (!dead && D.dd[n] > 0.0) dv = D.q[n];
          }
          A.D.delivered[st_i * N + n] = dv;
        }
      }
      for (int p = tid; p < P; p += HY_T) {
        if (A.flow) A.flow[st_i * P + p] = dead ? nan : q[p];
        A.L.link_state[st_i * P + p] = dead ? (uint8_t)0 : hy_link_state(code[p], q[p]);
      }
      for (int k = tid; k < Ke; k += HY_T) A.E.flow[st_i * Ke + k] = dead ? nan : eq[k];
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
        A.L.valve_changes[st_i] = dead ? 0 : changes;
      }
    }
    __syncthreads();                                       // (the next series writes the shared arrays again)
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

// the link and valve arguments both entry points share; num_pipes is known to be >= 1
static bool hy_valve_args_ok(const uint8_t* link_kind, const uint8_t* link_flags, const double* minor, const int32_t* pump_link,
                             const double* pump_h0, const double* pump_r, const double* pump_n, int32_t num_pumps,
                             const double* speed, int64_t speed_stride, const uint8_t* closed, int64_t closed_stride,
                             const uint8_t* link_state, const int32_t* valve_link, const uint8_t* valve_kind,
                             const double* valve_setting, int64_t setting_stride, int32_t num_valves, const int32_t* valve_changes,
                             int32_t num_pipes) {
  if (!link_kind || !link_flags || !minor || !link_state || !valve_changes) return false;
  if (num_pumps < 0 || num_pumps > num_pipes || num_valves < 0 || num_valves > num_pipes) return false;
  if (num_pumps > 0 && (!pump_link || !pump_h0 || !pump_r || !pump_n || !speed)) return false;
  if (num_valves > 0 && (!valve_link || !valve_kind || !valve_setting)) return false;
  if (speed_stride != 0 && speed_stride != (int64_t)num_pumps) return false;
  if (setting_stride != 0 && setting_stride != (int64_t)num_valves) return false;
  if (closed_stride != 0 && (closed_stride != (int64_t)num_pipes || !closed)) return false;
  return true;
}

static HydValveArgs hy_valve_args(const uint8_t* link_kind, const uint8_t* link_flags, const double* minor, const int32_t* pump_link,
                                  const double* pump_h0, const double* pump_r, const double* pump_n, int32_t num_pumps,
                                  const double* speed, int64_t speed_stride, const uint8_t* closed, int64_t closed_stride,
                                  uint8_t* link_state, const int32_t* valve_link, const uint8_t* valve_kind,
                                  const double* valve_setting, int64_t setting_stride, int32_t num_valves, int32_t* valve_changes) {
  HydValveArgs k;
  k.link_kind = link_kind; k.link_flags = link_flags; k.minor = minor; k.pump_link = pump_link; k.pump_h0 = pump_h0;
  k.pump_r = pump_r; k.pump_n = pump_n; k.speed = speed; k.closed = closed; k.speed_stride = (long long)speed_stride;
  k.closed_stride = (long long)closed_stride; k.Kp = (int)num_pumps; k.link_state = link_state;
  k.valve_link = valve_link; k.valve_kind = valve_kind; k.setting = valve_setting; k.setting_stride = (long long)setting_stride;
  k.Kv = (int)num_valves; k.valve_changes = valve_changes;
  return k;
}

// the emitter arguments both entry points share; num_nodes is known to be >= 2
static bool hy_emitter_args_ok(const int32_t* emitter_node, const double* emitter_coef, int64_t coef_stride, int32_t num_emitters,
                               const double* emitter_flow, int32_t num_nodes) {
  if (num_emitters < 0 || num_emitters > num_nodes) return false;
  if (num_emitters > 0 && (!emitter_node || !emitter_coef || !emitter_flow)) return false;
  if (coef_stride != 0 && coef_stride != (int64_t)num_emitters) return false;
  return true;
}

}  // namespace

extern "C" int gatres_hydraulic_solve_pdd(const int32_t* pipe_a, const int32_t* pipe_b, const double* coef, const double* q_start,
                                             const uint8_t* fixed, const double* elevation, const int32_t* order,
                                             const int32_t* position, int32_t half_bandwidth, const double* demand,
                                             const double* roughness, const double* fixed_head, int64_t fixed_head_stride,
                                             int64_t num_scenarios, int32_t num_nodes, int32_t num_pipes, double accuracy,
                                             int32_t max_iter, float* pressure, double* head, double* flow, int32_t* status,
                                             double* final_dq, const uint8_t* link_kind, const uint8_t* link_flags,
                                             const double* minor, const int32_t* pump_link, const double* pump_h0,
                                             const double* pump_r, const double* pump_n, int32_t num_pumps, const double* speed,
                                             int64_t speed_stride, const uint8_t* closed, int64_t closed_stride, uint8_t* link_state,
                                             const int32_t* valve_link, const uint8_t* valve_kind, const double* valve_setting,
                                             int64_t valve_setting_stride, int32_t num_valves, int32_t* valve_changes,
                                             const int32_t* emitter_node, const double* emitter_coef, int64_t emitter_coef_stride,
                                             int32_t num_emitters, double emitter_exponent, double* emitter_flow, int32_t demand_model,
                                             double minimum_pressure, double required_pressure, double pressure_exponent,
                                             double* demand_delivered, void* stream) {
  if (demand_model != 0 && demand_model != 1) return GATRES_E_BADARG;
  if (demand_model == 1 && !demand_delivered) return GATRES_E_BADARG;
  if (!pipe_a || !pipe_b || !coef || !q_start || !fixed || !elevation || !order || !position) return GATRES_E_BADARG;
  if (!demand || !roughness || !fixed_head || !pressure || !status || !final_dq) return GATRES_E_BADARG;
  if (!hy_counts_ok(num_scenarios, num_nodes, num_pipes) || num_nodes < 2) return GATRES_E_BADARG;
  if (!hy_emitter_args_ok(emitter_node, emitter_coef, emitter_coef_stride, num_emitters, emitter_flow, num_nodes))
    return GATRES_E_BADARG;
  if (!hy_valve_args_ok(link_kind, link_flags, minor, pump_link, pump_h0, pump_r, pump_n, num_pumps, speed, speed_stride, closed,
                        closed_stride, link_state, valve_link, valve_kind, valve_setting, valve_setting_stride, num_valves,
                        valve_changes, num_pipes))
    return GATRES_E_BADARG;
  if (half_bandwidth < 1 || half_bandwidth > num_nodes - 1) return GATRES_E_BADARG;
  if (max_iter < 1 || !(accuracy > 0.0) || !(accuracy <= DBL_MAX)) return GATRES_E_BADARG;
  if (fixed_head_stride != 0 && fixed_head_stride != (int64_t)num_nodes) return GATRES_E_BADARG;
  const uint64_t S = (uint64_t)num_scenarios, N = (uint64_t)num_nodes, P = (uint64_t)num_pipes, Kp = (uint64_t)num_pumps,
                 Kv = (uint64_t)num_valves, Ke = (uint64_t)num_emitters;
  const uint64_t lds = hy_emitters_lds_bytes(N, P, (uint64_t)half_bandwidth, Kp, Kv, Ke) + (demand_model ? HY_PDD_LDS * N : 0);
  if (lds > HY_LDS_BUDGET) return GATRES_E_BADARG;
  const void* wr[9] = {pressure, head, flow, status, final_dq, link_state, valve_changes, Ke ? emitter_flow : nullptr,
                       demand_delivered};
  const uint64_t wn[9] = {4 * S * N, 8 * S * N, 8 * S * P, 4 * GATRES_HYD_STATUS * S, 8 * S, S * P, 4 * S, 8 * S * Ke, 8 * S * N};
  const void* rd[25] = {pipe_a, pipe_b, coef, q_start, fixed, elevation, order, position, demand, roughness, fixed_head,
                        link_kind, link_flags, minor, Kp ? pump_link : nullptr, Kp ? pump_h0 : nullptr, Kp ? pump_r : nullptr,
                        Kp ? pump_n : nullptr, Kp ? speed : nullptr, closed, Kv ? valve_link : nullptr, Kv ? valve_kind : nullptr,
                        Kv ? valve_setting : nullptr, Ke ? emitter_node : nullptr, Ke ? emitter_coef : nullptr};
  const uint64_t rn[25] = {4 * P, 4 * P, 8 * P, 8 * P, N, 8 * N, 4 * N, 4 * N, 8 * S * N, 8 * S * P,
                           fixed_head_stride ? 8 * S * N : 8 * N, P, P, 8 * P, 4 * Kp, 8 * Kp, 8 * Kp, 8 * Kp,
                           speed_stride ? 8 * S * Kp : 8 * Kp, closed_stride ? S * P : P, 4 * Kv, Kv,
                           valve_setting_stride ? 8 * S * Kv : 8 * Kv, 4 * Ke, emitter_coef_stride ? 8 * S * Ke : 8 * Ke};
  if (any_overlap(wr, wn, 9, rd, rn, 25)) return GATRES_E_BADARG;
  if (lds > 64 * 1024) {                                   // (past the 64 KB a kernel gets unasked; per device)
    const void* kernel = demand_model ? reinterpret_cast<const void*>(&hydraulic_solve_pdd_kernel<true>)
                                      : reinterpret_cast<const void*>(&hydraulic_solve_pdd_kernel<false>);
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return (int)e;
    }
  }
  HydSolvePddArgs a;
  a.pipe_a = pipe_a; a.pipe_b = pipe_b; a.coef = coef; a.q_start = q_start; a.fixed = fixed; a.elevation = elevation;
  a.order = order; a.position = position; a.demand = demand; a.roughness = roughness; a.fixed_head = fixed_head;
  a.fh_stride = (long long)fixed_head_stride; a.S = (long long)num_scenarios;
  a.N = (int)num_nodes; a.P = (int)num_pipes; a.W = (int)half_bandwidth; a.max_iter = (int)max_iter; a.accuracy = accuracy;
  a.pressure = pressure; a.head = head; a.flow = flow; a.status = status; a.final_dq = final_dq;
  a.K = hy_valve_args(link_kind, link_flags, minor, pump_link, pump_h0, pump_r, pump_n, num_pumps, speed, speed_stride, closed,
                      closed_stride, link_state, valve_link, valve_kind, valve_setting, valve_setting_stride, num_valves,
                      valve_changes);
  a.E.node = emitter_node; a.E.coef = emitter_coef; a.E.onset = nullptr; a.E.coef_stride = (long long)emitter_coef_stride;
  a.E.onset_stride = 0; a.E.exponent = emitter_exponent; a.E.Ke = (int)num_emitters; a.E.flow = emitter_flow;
  a.D.pmin = demand_model ? minimum_pressure : 0.0; a.D.preq = demand_model ? required_pressure : 0.0;
  a.D.exponent = demand_model ? pressure_exponent : 1.0; a.D.delivered = demand_delivered;
  const long long wgs = num_scenarios < HY_GRID_CAP ? (long long)num_scenarios : HY_GRID_CAP;
  if (demand_model)
    hipLaunchKernelGGL(hydraulic_solve_pdd_kernel<true>, dim3((unsigned)wgs), dim3(HY_T), (size_t)lds, gatres_stream(stream), a);
  else
    hipLaunchKernelGGL(hydraulic_solve_pdd_kernel<false>, dim3((unsigned)wgs), dim3(HY_T), (size_t)lds, gatres_stream(stream), a);
  return gatres_launch_status();
}

extern "C" int gatres_hydraulic_series_pdd(
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
    uint8_t* link_state, const int32_t* valve_link, const uint8_t* valve_kind, const double* valve_setting,
    int64_t valve_setting_stride, int32_t num_valves, int32_t* valve_changes, const int32_t* emitter_node,
    const double* emitter_coef, int64_t emitter_coef_stride, int32_t num_emitters, double emitter_exponent,
    const int32_t* emitter_onset, int64_t emitter_onset_stride, double* emitter_flow, int32_t demand_model,
    double minimum_pressure, double required_pressure, double pressure_exponent, double* demand_delivered, void* stream) {
  if (demand_model != 0 && demand_model != 1) return GATRES_E_BADARG;
  if (demand_model == 1 && !demand_delivered) return GATRES_E_BADARG;
  if (!pipe_a || !pipe_b || !coef || !q_start || !fixed || !elevation || !order || !position) return GATRES_E_BADARG;
  if (!hy_emitter_args_ok(emitter_node, emitter_coef, emitter_coef_stride, num_emitters, emitter_flow, num_nodes))
    return GATRES_E_BADARG;
  if (emitter_onset_stride != 0 && (emitter_onset_stride != (int64_t)num_emitters || !emitter_onset)) return GATRES_E_BADARG;
  if (!pattern_of_node || !mult || !demand || !roughness || !fixed_head || !pressure || !status || !final_dq) return GATRES_E_BADARG;
  if (num_tanks < 0 || num_steps < 1 || num_patterns < 1) return GATRES_E_BADARG;
  if (num_tanks > 0 && (!tank_node || !tank_area || !tank_min_level || !tank_max_level || !initial_level || !level))
    return GATRES_E_BADARG;
  if (!hy_counts_ok(num_series, num_nodes, num_pipes) || num_nodes < 2) return GATRES_E_BADARG;
  if (!hy_valve_args_ok(link_kind, link_flags, minor, pump_link, pump_h0, pump_r, pump_n, num_pumps, speed, speed_stride, closed,
                        closed_stride, link_state, valve_link, valve_kind, valve_setting, valve_setting_stride, num_valves,
                        valve_changes, num_pipes))
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
                 K = (uint64_t)num_tanks, M = (uint64_t)num_patterns, Kp = (uint64_t)num_pumps, Kv = (uint64_t)num_valves,
                 Ms = Kp ? (uint64_t)num_speed_patterns : 0, Ke = (uint64_t)num_emitters;
  const uint64_t lds = hy_series_emitters_lds_bytes(N, P, (uint64_t)half_bandwidth, K, Kp, Kv, Ke) +
                       (demand_model ? HY_PDD_LDS * N : 0);
  if (lds > HY_LDS_BUDGET) return GATRES_E_BADARG;
  const void* wr[10] = {pressure, head, flow, K ? level : nullptr, status, final_dq, link_state, valve_changes,
                        Ke ? emitter_flow : nullptr, demand_delivered};
  const uint64_t wn[10] = {4 * S * T * N, 8 * S * T * N, 8 * S * T * P, 8 * S * (T + 1) * K, 4 * GATRES_HYD_STATUS * S * T, 8 * S * T,
                           S * T * P, 4 * S * T, 8 * S * T * Ke, 8 * S * T * N};
  const void* rd[35] = {pipe_a, pipe_b, coef, q_start, fixed, elevation, order, position, K ? tank_node : nullptr,
                        K ? tank_area : nullptr, K ? tank_min_level : nullptr, K ? tank_max_level : nullptr, pattern_of_node, mult,
                        demand, roughness, fixed_head, K ? initial_level : nullptr, link_kind, link_flags, minor,
                        Kp ? pump_link : nullptr, Kp ? pump_h0 : nullptr, Kp ? pump_r : nullptr, Kp ? pump_n : nullptr,
                        Kp ? speed : nullptr, closed, Kp ? speed_mult : nullptr, Kp ? speed_pattern_of_pump : nullptr,
                        Kv ? valve_link : nullptr, Kv ? valve_kind : nullptr, Kv ? valve_setting : nullptr,
                        Ke ? emitter_node : nullptr, Ke ? emitter_coef : nullptr, Ke ? emitter_onset : nullptr};
  const uint64_t rn[35] = {4 * P, 4 * P, 8 * P, 8 * P, N, 8 * N, 4 * N, 4 * N, 4 * K, 8 * K, 8 * K, 8 * K, 4 * N,
                           mult_stride ? 8 * S * M * T : 8 * M * T, 8 * S * N, 8 * S * P, fixed_head_stride ? 8 * S * N : 8 * N,
                           8 * S * K, P, P, 8 * P, 4 * Kp, 8 * Kp, 8 * Kp, 8 * Kp, speed_stride ? 8 * S * Kp : 8 * Kp,
                           closed_stride ? S * P : P, 8 * Ms * T, 4 * Kp, 4 * Kv, Kv, valve_setting_stride ? 8 * S * Kv : 8 * Kv,
                           4 * Ke, emitter_coef_stride ? 8 * S * Ke : 8 * Ke, emitter_onset_stride ? 4 * S * Ke : 4 * Ke};
  if (any_overlap(wr, wn, 10, rd, rn, 35)) return GATRES_E_BADARG;
  if (lds > 64 * 1024) {                                   // (past the 64 KB a kernel gets unasked; per device)
    const void* kernel = demand_model ? reinterpret_cast<const void*>(&hydraulic_series_pdd_kernel<true>)
                                      : reinterpret_cast<const void*>(&hydraulic_series_pdd_kernel<false>);
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return (int)e;
    }
  }
  HydSeriesPddArgs a;
  a.pipe_a = pipe_a; a.pipe_b = pipe_b; a.coef = coef; a.q_start = q_start; a.fixed = fixed; a.elevation = elevation;
  a.order = order; a.position = position; a.tank_node = tank_node; a.tank_area = tank_area; a.tank_min = tank_min_level;
  a.tank_max = tank_max_level; a.pattern = pattern_of_node; a.mult = mult; a.demand = demand; a.roughness = roughness;
  a.fixed_head = fixed_head; a.level0 = initial_level; a.mult_stride = (long long)mult_stride;
  a.fh_stride = (long long)fixed_head_stride; a.S = (long long)num_series; a.T = (int)num_steps; a.N = (int)num_nodes;
  a.P = (int)num_pipes; a.W = (int)half_bandwidth; a.K = (int)num_tanks; a.M = (int)num_patterns; a.max_iter = (int)max_iter;
  a.warm = warm_start != 0 ? 1 : 0; a.dt = dt; a.accuracy = accuracy;
  a.pressure = pressure; a.head = head; a.flow = flow; a.level = level; a.status = status; a.final_dq = final_dq;
  a.L = hy_valve_args(link_kind, link_flags, minor, pump_link, pump_h0, pump_r, pump_n, num_pumps, speed, speed_stride, closed,
                      closed_stride, link_state, valve_link, valve_kind, valve_setting, valve_setting_stride, num_valves,
                      valve_changes);
  a.E.node = emitter_node; a.E.coef = emitter_coef; a.E.onset = Ke ? emitter_onset : nullptr;
  a.E.coef_stride = (long long)emitter_coef_stride; a.E.onset_stride = (long long)emitter_onset_stride;
  a.E.exponent = emitter_exponent; a.E.Ke = (int)num_emitters; a.E.flow = emitter_flow;
  a.D.pmin = demand_model ? minimum_pressure : 0.0; a.D.preq = demand_model ? required_pressure : 0.0;
  a.D.exponent = demand_model ? pressure_exponent : 1.0; a.D.delivered = demand_delivered;
  a.speed_mult = speed_mult; a.speed_pattern = speed_pattern_of_pump; a.Ms = (int)Ms;
  const long long wgs = num_series < HY_GRID_CAP ? (long long)num_series : HY_GRID_CAP;
  if (demand_model)
    hipLaunchKernelGGL(hydraulic_series_pdd_kernel<true>, dim3((unsigned)wgs), dim3(HY_T), (size_t)lds, gatres_stream(stream), a);
  else
    hipLaunchKernelGGL(hydraulic_series_pdd_kernel<false>, dim3((unsigned)wgs), dim3(HY_T), (size_t)lds, gatres_stream(stream), a);
  return gatres_launch_status();
}

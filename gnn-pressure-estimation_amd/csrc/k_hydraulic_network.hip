// Regulating valves, emitters and pressure-driven demand in the device hydraulic solver (hydraulics.py: a HydraulicNetwork with
// valve_links or emitter_nodes; simulate(demand_model="pda")).  gatres.h states THE REGULATING VALVES, THE EMITTERS and THE
// PRESSURE-DRIVEN DEMAND.  Two kernels, stated once around hy_newton_valves<EMIT, PDD> (k_hydraulics_dev.h) and instantiated per
// level LV, each level holding the one below:
//   LV 0  valves     the Newton loop of the link law with the valves' status machine, the statuses carried along a warm series;
//   LV 1  emitters   EMIT: the emitters' node term, their flows carried along a warm series, each emitter off before its onset step;
//   LV 2  pdd        PDD: the node term of the demand at every junction that draws, the delivered flows carried along a warm series
//                    while a junction stays pressure-driven.
//   hydraulic_solve_network_kernel<LV>    one workgroup per scenario   gatres_hydraulic_solve_{valves,emitters,pdd}
//   hydraulic_series_network_kernel<LV, CTL>  one workgroup per series  gatres_hydraulic_series_{valves,emitters,pdd} (CTL false)
//                    CTL: THE CONTROLS of gatres.h, a pass at the start of every step; gatres_hydraulic_series_controls, LV 1 and 2
// The pdd entry points with demand_model 0 launch LV 1.  With no valve LV 0 gives every bit of the links launches
// (k_hydraulic_links.hip), with no emitter LV 1 every bit of LV 0.  Every loop is bounded, every sum runs in a fixed order, nothing
// is shared between scenarios.  No atomics.
#include "k_hydraulics_dev.h"

#include <type_traits>

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

// the emitter arrays of a launch, shared by both kernels (LV 0: all zero)
struct HydEmitterArgs {
  const int* node;
  const double* coef;
  const int* onset;                                        // (the series alone; NULL: every emitter is on from step 0)
  long long coef_stride, onset_stride;
  double exponent;
  int Ke;
  double* flow;
};

// the demand model of a launch, shared by both kernels (below LV 2 the scalars are not read)
struct HydPddArgs {
  double pmin, preq, exponent;
  double* delivered;                                       // [S][N] (series [S][T][N]); NULL at LV 0, may be NULL at LV 1
};

// the control table of a series launch with THE CONTROLS (gatres.h); all zero in every other launch
struct HydControlArgs {
  const int* link;
  const uint8_t* action;
  const double* value;
  const uint8_t* kind;
  const int* target;
  const double* threshold;
  long long threshold_stride;
  int Kc;
  int* changes;                                            // [S][T]
};

struct HydNetSolveArgs {
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
  HydValveArgs L;
  HydEmitterArgs E;
  HydPddArgs D;
};

struct HydNetSeriesArgs {
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
  const double* speed_mult;                                // [Ms][T]
  const int* speed_pattern;                                // [Kp]
  int Ms;
  HydEmitterArgs E;                                        // (the levels' own members last: a lower level reads none behind its own)
  HydPddArgs D;
};

// the arguments of the series kernels with THE CONTROLS: the table comes behind everything the other instantiations take
struct HydNetSeriesCtlArgs : HydNetSeriesArgs {
  HydControlArgs C;
};

constexpr uint64_t HY_EMITTER_LDS = 48;                   // per emitter: ce, z, q, 1 / g, h / g, its row and its node
constexpr uint64_t HY_PDD_LDS = 32;                        // per node at LV 2: D, q_d, 1 / g, h / g

// LDS of a workgroup, as gatres.h states it: the arrays of the links launch, per valve hset, link, row, node and change flag, per
// emitter and (Nd = N at LV 2, else 0) per node the records above; a series adds the step's demands and the tanks' records
static inline uint64_t hy_network_lds_bytes(uint64_t N, uint64_t P, uint64_t W, uint64_t Kp, uint64_t Kv, uint64_t Ke, uint64_t Nd) {
  return 8 * (N * (W + 1) + 2 * N + 4 * P) + 4 * (2 * P + N) + 64 + 12 * P + 8 * HY_PUMP_REC * Kp + 24 * Kv + HY_EMITTER_LDS * Ke +
         HY_PDD_LDS * Nd;
}

static inline uint64_t hy_series_network_lds_bytes(uint64_t N, uint64_t P, uint64_t W, uint64_t K, uint64_t Kp, uint64_t Kv,
                                                   uint64_t Ke, uint64_t Nd) {
  return hy_network_lds_bytes(N, P, W, Kp, Kv, Ke, Nd) + 8 * N + 40 * K;
}

// what a series with THE CONTROLS adds: per link the override value and the state word, and the four waves' change counts
static inline uint64_t hy_controls_lds_bytes(uint64_t P) { return 12 * P + 16; }

// A workgroup's LDS, carved for both kernels: the arrays of the Newton loop (HyLds, HyValves, HyEmitters, HyPdd describe them; the
// scalars of E and D are the kernel's to set), the series' arrays (a steady launch has K = 0 and no dem) and the flag words.  With a
// null base `bytes` is all the host wants: where the carve ends, which no launch may place past the bytes it asks for.
struct HyCarve {
  HyLds L;
  HyValves V;
  HyEmitters E;
  HyPdd D;
  double* dem;                                             // [N] the step's demand by node (series)
  double *lev, *area, *lmin, *lmax;                        // [K] the tank levels of the present step, and the tanks' constants
  int *tnode, *trow;                                       // [K] a tank's node and its solver row
  double* cval;                                            // [Pc] a link's override of THE CONTROLS (Pc = P with controls, else 0)
  int *cst, *ccnt;                                         // [Pc] a link's state word (HY_CS_*); [4 with controls] a wave's changes
  int* flag;                                              // [4]: [0] static arrays refused, [1] scenario or step failed, [2] a level clamped
  uint64_t bytes;
};

__host__ __device__ __forceinline__ HyCarve hy_carve(unsigned char* base, int N, int P, int W, int K, int Kp, int Kv, int Ke, int Nd,
                                                     bool series, int Pc = 0) {
  HyCarve C;
  const int BW = W + 1, Ns = series ? N : 0;
  C.L.band = reinterpret_cast<double*>(base);              // [N][BW]
  C.L.y = C.L.band + (size_t)N * BW;
  C.L.H = C.L.y + N;
  C.L.q = C.L.H + N;
  C.L.rr = C.L.q + P;
  C.L.pinv = C.L.rr + P;
  C.L.yv = C.L.pinv + P;
  C.L.red = C.L.yv + P;                                    // [4]
  C.dem = C.L.red + 4;                                     // [Ns]
  C.lev = C.dem + Ns;                                      // [K] each
  C.area = C.lev + K;
  C.lmin = C.area + K;
  C.lmax = C.lmin + K;
  C.L.minor = C.lmax + K;                                  // [P]
  C.L.pump = C.L.minor + P;                                // [Kp][HY_PUMP_REC]
  C.V.hset = C.L.pump + (size_t)Kp * HY_PUMP_REC;          // [Kv]
  C.E.ce = C.V.hset + Kv;                                  // [Ke] each
  C.E.z = C.E.ce + Ke;
  C.E.q = C.E.z + Ke;
  C.E.einv = C.E.q + Ke;
  C.E.ey = C.E.einv + Ke;
  C.D.dd = C.E.ey + Ke;                                    // [Nd] each
  C.D.q = C.D.dd + Nd;
  C.D.dinv = C.D.q + Nd;
  C.D.dy = C.D.dinv + Nd;
  C.cval = C.D.dy + Nd;                                    // [Pc]
  C.L.sa = reinterpret_cast<int*>(C.cval + Pc);            // [P]
  C.L.sb = C.L.sa + P;                                     // [P]
  C.L.fx = C.L.sb + P;                                     // [N]
  C.tnode = C.L.fx + N;                                    // [K]
  C.trow = C.tnode + K;                                    // [K]
  C.L.code = C.trow + K;                                   // [P]
  C.V.link = C.L.code + P;                                 // [Kv] each
  C.V.row = C.V.link + Kv;
  C.V.node = C.V.row + Kv;
  C.V.chg = C.V.node + Kv;
  C.E.row = C.V.chg + Kv;                                  // [Ke] each
  C.E.node = C.E.row + Ke;
  C.cst = C.E.node + Ke;                                   // [Pc]
  C.ccnt = C.cst + Pc;                                     // [Pc ? 4 : 0]
  C.flag = C.ccnt + (Pc ? 4 : 0);                          // [4]
  C.V.Kv = Kv;
  C.E.Ke = Ke;
  C.bytes = (uint64_t)(reinterpret_cast<unsigned char*>(C.flag + 4) - base);
  return C;
}

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

// The kernel's own scalars of the carved records: 1 / gamma of the emitters, and the demand model with the elevations by node
template <bool EMIT, bool PDD>
__device__ __forceinline__ void hy_carve_scalars(HyCarve& C, const HydEmitterArgs& E, const HydPddArgs& D, const double* elevation) {
  if constexpr (EMIT) C.E.n = 1.0 / E.exponent;
  if constexpr (PDD) {
    C.D.elevation = elevation;
    C.D.pmin = D.pmin;
    C.D.dp = D.preq - D.pmin;
    C.D.n = 1.0 / D.exponent;
  }
}

template <int LV>
__global__ __launch_bounds__(HY_T) void hydraulic_solve_network_kernel(const HydNetSolveArgs A) {
  constexpr bool EMIT = LV >= 1, PDD = LV >= 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char hy_smem[];
  const int N = A.N, P = A.P, W = A.W, Kp = A.L.Kp, Kv = A.L.Kv, Ke = EMIT ? A.E.Ke : 0, tid = threadIdx.x;
  HyCarve C = hy_carve(hy_smem, N, P, W, 0, Kp, Kv, Ke, PDD ? N : 0, false);
  hy_carve_scalars<EMIT, PDD>(C, A.E, A.D, A.elevation);
  const HyLds& L = C.L;
  const HyValves& V = C.V;
  const HyEmitters& E = C.E;
  const HyPdd& D = C.D;
  double *H = L.H, *q = L.q, *rr = L.rr, *minor = L.minor, *pump = L.pump;
  int *code = L.code, *flag = C.flag;                      // flag: [0] static arrays refused, [1] scenario failed

  bool perm_ok = false;
  bool static_bad = hy_check_static(L, A.position, A.order, A.fixed, A.pipe_a, A.pipe_b, N, P, W, flag, tid, &perm_ok);
  static_bad = hy_check_valve_links(L, V, A.L, A.coef, A.pipe_a, A.pipe_b, N, P, flag, tid) || static_bad;
  if constexpr (EMIT) static_bad = hy_check_emitters(L, V, E, A.E, A.position, A.elevation, N, perm_ok, flag, tid) || static_bad;
  if constexpr (PDD) {
    static_bad = hy_pdd_bad(A.D) || static_bad;            // (the launch's scalars: the same in every thread)
    for (int n = tid; n < N; n += HY_T) D.dd[n] = 0.0;     // (node n is always this thread's)
  }
  const double nan = __longlong_as_double(0x7FF8000000000000ll);

  for (long long s = blockIdx.x; s < A.S; s += gridDim.x) {
    const double* dem = A.demand + s * N;
    const double* rough = A.roughness + s * P;
    const double* fh = A.fixed_head + s * A.fh_stride;
    const uint8_t* closed = A.L.closed ? A.L.closed + s * A.L.closed_stride : nullptr;
    if (tid == 0) flag[1] = static_bad ? 1 : 0;
    __syncthreads();
    if (!static_bad) {
      for (int k = tid; k < Kp; k += HY_T) hy_set_speed(pump + (size_t)k * HY_PUMP_REC, A.L.speed[s * A.L.speed_stride + k], &flag[1]);
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
        hy_valve_start(L, V, k, A.L.setting[s * A.L.setting_stride + k], A.elevation, false, &flag[1]);
      if constexpr (EMIT)
        for (int k = tid; k < Ke; k += HY_T) hy_emitter_start(E, k, A.E.coef[s * A.E.coef_stride + k], false, &flag[1]);
    }
    __syncthreads();
    bool failed = flag[1] != 0, converged = false;         // (read from LDS after a barrier: the same in every thread)
    int iters = 0, changes = 0;
    double rel = 0.0;
    if (!failed) {
      const HyNewtonValves nw = hy_newton_valves<EMIT, PDD>(L, V, A.position, dem, N, P, W, A.max_iter, A.accuracy, tid, E, D);
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
      if constexpr (EMIT) {
        if (A.D.delivered) {                               // q_d where the junction is pressure-driven, else the demand itself
          double dv = A.fixed[n] ? 0.0 : dem[n];
          if constexpr (PDD) {
            if (D.dd[n] > 0.0) dv = D.q[n];
          }
          A.D.delivered[s * N + n] = failed ? nan : dv;
        }
      }
    }
    for (int p = tid; p < P; p += HY_T) {
      if (A.flow) A.flow[s * P + p] = failed ? nan : q[p];
      A.L.link_state[s * P + p] = failed ? (uint8_t)0 : hy_link_state(code[p], q[p]);
    }
    if constexpr (EMIT)
      for (int k = tid; k < Ke; k += HY_T) A.E.flow[s * Ke + k] = failed ? nan : E.q[k];
    if (tid == 0) {
      int* st = A.status + s * GATRES_HYD_STATUS;
      st[0] = iters;
      st[1] = converged && !failed ? 1 : 0;
      st[2] = failed ? 1 : 0;
      st[3] = 0;
      A.final_dq[s] = failed ? nan : rel;
      A.L.valve_changes[s] = failed ? 0 : changes;
    }
    __syncthreads();                                       // (the next scenario writes the shared arrays again)
  }
}

// ---- THE CONTROLS of a series (gatres.h) ------------------------------------------------------------------------------------------------
// A link's state word: the control state (HY_CTL_MASK), whether it carries an override, whether a control changed it in the
// present step, and whether the step restarts the link (its flow at q_start, its valve ACTIVE).
constexpr int HY_CS_VALUE = 4, HY_CS_CHANGED = 8, HY_CS_RESTART = 16;
static_assert(GATRES_HYD_CTL_OPEN == 0 && GATRES_HYD_CTL_CLOSED == 1 && GATRES_HYD_CTL_SETTING == 2 && GATRES_HYD_CTL_TANK_BELOW == 0 &&
                  GATRES_HYD_CTL_TANK_ABOVE == 1 && GATRES_HYD_CTL_NODE_BELOW == 2 && GATRES_HYD_CTL_NODE_ABOVE == 3 &&
                  GATRES_HYD_CTL_AT_STEP == 4, "gatres.h");

// The static control table, checked, after hy_check_valve_links (L.code holds the links' kinds; flag[0] keeps the verdict): what
// gatres.h refuses.  Nothing indexes with a control's link, tank or node that was not checked here.  No barrier of its own.
__device__ __forceinline__ void hy_check_controls(const HyLds& L, const HydControlArgs& A, const uint8_t* __restrict__ fixed, int N,
                                                  int P, int K, int* flag, int tid) {
  for (int k = tid; k < A.Kc; k += HY_T) {
    const int link = A.link[k], action = A.action[k], kind = A.kind[k], target = A.target[k];
    const double v = A.value[k];
    bool ok = link >= 0 && link < P && action <= GATRES_HYD_CTL_SETTING && kind <= GATRES_HYD_CTL_AT_STEP && target >= 0;
    if (ok) {
      const int code = L.code[link];
      if ((code & HY_CHECK) && !(code & HY_PUMP)) ok = false;
      if (action == GATRES_HYD_CTL_SETTING) {
        if (!(code & (HY_PUMP | HY_VALVE)) || !hy_finite(v) || ((code & HY_PUMP) && !(v >= 0.0))) ok = false;
      }
      if (kind <= GATRES_HYD_CTL_TANK_ABOVE) {
        if (target >= K) ok = false;
      } else if (kind <= GATRES_HYD_CTL_NODE_ABOVE) {
        if (target >= N) ok = false;
        else if (fixed[target] != 0) ok = false;
      }
    }
    if (!ok) flag[0] = 1;
  }
}

// The control pass of step t, one thread per link scanning the table in order (so the last control that fires wins, without
// atomics): reads lev[] (the levels the step starts with) and H[] (the solution of step t - 1), writes the link's state word and
// override, and leaves the changes of a wave's links in ccnt[wave].  The caller puts a barrier behind it.
__device__ __forceinline__ void hy_control_pass(const HyCarve& C, const HydControlArgs& A, const double* __restrict__ thr,
                                                const int* __restrict__ position, const double* __restrict__ elevation, int P, int t,
                                                int tid) {
  int n = 0;
  for (int p = tid; p < P; p += HY_T) {
    int st = C.cst[p] & ~(HY_CS_CHANGED | HY_CS_RESTART);
    double val = C.cval[p];
    for (int k = 0; k < A.Kc; ++k) {
      if (A.link[k] != p) continue;
      const int kind = A.kind[k], target = A.target[k];
      bool fire;
      if (kind == GATRES_HYD_CTL_AT_STEP) {
        fire = t == target;
      } else if (kind <= GATRES_HYD_CTL_TANK_ABOVE) {
        const double lv = C.lev[target], th = thr[k];
        fire = kind == GATRES_HYD_CTL_TANK_BELOW ? lv <= th : lv >= th;
      } else if (t == 0) {
        fire = false;
      } else {
        const double pr = C.L.H[position[target]] - elevation[target], th = thr[k];
        fire = kind == GATRES_HYD_CTL_NODE_BELOW ? pr <= th : pr >= th;
      }
      if (!fire) continue;
      const int action = A.action[k];
      int ns = (st & ~HY_CTL_MASK) | (action == GATRES_HYD_CTL_CLOSED ? HY_CTL_CLOSED : HY_CTL_OPEN);
      double nv = val;
      if (action == GATRES_HYD_CTL_SETTING) {
        ns |= HY_CS_VALUE;
        nv = A.value[k];
      }
      const int same = HY_CTL_MASK | HY_CS_VALUE;
      if ((ns & same) != (st & same) || __double_as_longlong(nv) != __double_as_longlong(val)) {
        st = ns | HY_CS_CHANGED;
        val = nv;
        ++n;
      }
    }
    C.cst[p] = st;
    C.cval[p] = val;
  }
  for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off, 64);
  if ((tid & 63) == 0) C.ccnt[tid >> 6] = n;
}

// ---- the series ------------------------------------------------------------------------------------------------------------------------
template <int LV, bool CTL>
__global__ __launch_bounds__(HY_T) void hydraulic_series_network_kernel(const std::conditional_t<CTL, HydNetSeriesCtlArgs, HydNetSeriesArgs> A) {
  constexpr bool EMIT = LV >= 1, PDD = LV >= 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char hy_smem[];
  const int N = A.N, P = A.P, W = A.W, K = A.K, M = A.M, T = A.T, Kp = A.L.Kp, Kv = A.L.Kv, Ke = EMIT ? A.E.Ke : 0, Ms = A.Ms,
            tid = threadIdx.x;
  HyCarve C = hy_carve(hy_smem, N, P, W, K, Kp, Kv, Ke, PDD ? N : 0, true, CTL ? P : 0);
  hy_carve_scalars<EMIT, PDD>(C, A.E, A.D, A.elevation);
  const HyLds& L = C.L;
  const HyValves& V = C.V;
  const HyEmitters& E = C.E;
  const HyPdd& D = C.D;
  double *H = L.H, *q = L.q, *rr = L.rr, *minor = L.minor, *pump = L.pump;
  double *dem = C.dem, *lev = C.lev, *area = C.area, *lmin = C.lmin, *lmax = C.lmax;
  int *sa = L.sa, *sb = L.sb, *code = L.code, *tnode = C.tnode, *trow = C.trow;
  int* flag = C.flag;                                      // [0] static arrays refused, [1] step failed, [2] a level clamped
  __builtin_assume(N >= 2);                                // (the entry point refuses anything else; without these words the LV 0
                                                           //  instantiation reserves 68 bytes of scratch that no instruction touches)

  bool perm_ok = false;
  bool static_bad = hy_check_static(L, A.position, A.order, A.fixed, A.pipe_a, A.pipe_b, N, P, W, flag, tid, &perm_ok);
  static_bad = hy_check_valve_links(L, V, A.L, A.coef, A.pipe_a, A.pipe_b, N, P, flag, tid) || static_bad;
  if constexpr (EMIT) static_bad = hy_check_emitters(L, V, E, A.E, A.position, A.elevation, N, perm_ok, flag, tid) || static_bad;
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
  if constexpr (CTL) hy_check_controls(L, A.C, A.fixed, N, P, K, flag, tid);
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
    const double* ecoef = EMIT ? A.E.coef + s * A.E.coef_stride : nullptr;
    const int* onset = EMIT && A.E.onset ? A.E.onset + s * A.E.onset_stride : nullptr;
    [[maybe_unused]] const double* thr = nullptr;
    if constexpr (CTL) thr = A.C.threshold + s * A.C.threshold_stride;
    if (tid == 0) flag[1] = static_bad ? 1 : 0;
    __syncthreads();
    if (!static_bad) {
      if constexpr (EMIT) {
        for (int k = tid; k < Ke; k += HY_T) {             // a bad coefficient fails the series from step 0 on, whatever its onset
          const double Cf = ecoef[k];
          if (!(Cf >= 0.0) || !hy_finite(Cf)) flag[1] = 1;
          E.ce[k] = -1.0;                                  // (off until a step switches it on)
          E.q[k] = 0.0;
        }
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
        if constexpr (CTL) {                               // no control has touched a link before step 0
          C.cst[p] = 0;
          C.cval[p] = 0.0;
        }
      }
      if constexpr (CTL) {
        for (int k = tid; k < A.C.Kc; k += HY_T)           // a threshold that is not finite fails the series from step 0 on
          if (A.C.kind[k] != GATRES_HYD_CTL_AT_STEP && !hy_finite(thr[k])) flag[1] = 1;
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
      [[maybe_unused]] int ctl_changes = 0;
      bool converged = false;
      double rel = 0.0;
      if (!dead) {
        if constexpr (CTL) {                               // THE CONTROLS: before the step's inputs are formed
          hy_control_pass(C, A.C, thr, A.position, A.elevation, P, t, tid);
          __syncthreads();                                 // (a pump's speed and a valve's start read their link's state)
          ctl_changes = C.ccnt[0] + C.ccnt[1] + C.ccnt[2] + C.ccnt[3];     // (rewritten two barriers on at the earliest)
        }
        // the step's inputs: one rounded product per junction and per pump, the tank heads, the start of the flows
        for (int m = tid; m < M; m += HY_T) {
          const double v = mult[(long long)m * T + t];
          if (!(v >= 0.0) || !hy_finite(v)) flag[1] = 1;
        }
        for (int m = tid; m < Ms; m += HY_T) {
          const double v = A.speed_mult[(long long)m * T + t];
          if (!(v >= 0.0) || !hy_finite(v)) flag[1] = 1;
        }
        for (int k = tid; k < Kp; k += HY_T) {
          if constexpr (CTL) {                             // a SETTING control's value stands in place of the base speed
            const int pl = A.L.pump_link[k];               // (checked by hy_check_valve_links)
            const double w = (C.cst[pl] & HY_CS_VALUE) ? C.cval[pl] : speed[k];
            hy_set_speed(pump + (size_t)k * HY_PUMP_REC, w * A.speed_mult[(long long)A.speed_pattern[k] * T + t], &flag[1]);
          } else {
            hy_set_speed(pump + (size_t)k * HY_PUMP_REC, speed[k] * A.speed_mult[(long long)A.speed_pattern[k] * T + t], &flag[1]);
          }
        }
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
          if constexpr (CTL) {                             // a link that a control has touched: reopened, it starts anew
            const int cs = C.cst[p];
            const bool touched = (cs & HY_CTL_MASK) != HY_CTL_NONE, was_shut = t > 0 && (code[p] & HY_SHUT) != 0;
            const int c = hy_link_code(L, p, closed, &flag[1], cs & HY_CTL_MASK);
            if (touched && t > 0 && ((cs & HY_CS_CHANGED) || was_shut)) C.cst[p] = cs | HY_CS_RESTART;
            code[p] = c;
            if (c & HY_SHUT) q[p] = 0.0;
            else if ((t > 0 && !A.warm) || (touched && was_shut)) q[p] = A.q_start[p];
          } else {
            const int c = hy_link_code(L, p, closed, &flag[1]);
            code[p] = c;
            if (c & HY_SHUT) q[p] = 0.0;                   // a shut link starts at rest, warm or cold
            else if (t > 0 && !A.warm) q[p] = A.q_start[p];
          }
        }
        __syncthreads();
        for (int k = tid; k < Kv; k += HY_T) {             // a warm series carries the statuses along with the flows
          if constexpr (CTL) {                             // (V.link was checked; 0 where the launch is refused)
            const int cs = C.cst[V.link[k]];
            const double setting = (cs & HY_CS_VALUE) ? C.cval[V.link[k]] : A.L.setting[s * A.L.setting_stride + k];
            hy_valve_start(L, V, k, setting, A.elevation, t > 0 && A.warm && !(cs & HY_CS_RESTART), &flag[1]);
          } else {
            hy_valve_start(L, V, k, A.L.setting[s * A.L.setting_stride + k], A.elevation, t > 0 && A.warm, &flag[1]);
          }
        }
        if constexpr (EMIT)
          for (int k = tid; k < Ke; k += HY_T)             // a warm series carries an emitter's flow along while it stays on
            hy_emitter_start(E, k, onset && t < onset[k] ? 0.0 : ecoef[k], t > 0 && A.warm, &flag[1]);
        __syncthreads();
        dead = flag[1] != 0;
        if (!dead) {
          const HyNewtonValves nw = hy_newton_valves<EMIT, PDD>(L, V, A.position, dem, N, P, W, A.max_iter, A.accuracy, tid, E, D);
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
        if constexpr (EMIT) {
          if (A.D.delivered) {                             // q_d where the junction is pressure-driven, else the step's demand
            double dv = dead ? nan : dem[n];               // (0 at a fixed node; not read where dead: a NaN either way)
            if constexpr (PDD) {
              if (!dead && D.dd[n] > 0.0) dv = D.q[n];
            }
            A.D.delivered[st_i * N + n] = dv;
          }
        }
      }
      for (int p = tid; p < P; p += HY_T) {
        if (A.flow) A.flow[st_i * P + p] = dead ? nan : q[p];
        A.L.link_state[st_i * P + p] = dead ? (uint8_t)0 : hy_link_state(code[p], q[p]);
      }
      if constexpr (EMIT)
        for (int k = tid; k < Ke; k += HY_T) A.E.flow[st_i * Ke + k] = dead ? nan : E.q[k];
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
        if constexpr (CTL) A.C.changes[st_i] = dead ? 0 : ctl_changes;
      }
    }
    __syncthreads();                                       // (the next series writes the shared arrays again)
  }
}

// ---- the host side: one function per kernel does every check; the six entry points fill the struct and name their level ----------------
// the link and valve arguments; P is known to be >= 1
static bool hy_valve_args_ok(const HydValveArgs& k, int32_t P) {
  if (!k.link_kind || !k.link_flags || !k.minor || !k.link_state || !k.valve_changes) return false;
  if (k.Kp < 0 || k.Kp > P || k.Kv < 0 || k.Kv > P) return false;
  if (k.Kp > 0 && (!k.pump_link || !k.pump_h0 || !k.pump_r || !k.pump_n || !k.speed)) return false;
  if (k.Kv > 0 && (!k.valve_link || !k.valve_kind || !k.setting)) return false;
  if (k.speed_stride != 0 && k.speed_stride != (long long)k.Kp) return false;
  if (k.setting_stride != 0 && k.setting_stride != (long long)k.Kv) return false;
  if (k.closed_stride != 0 && (k.closed_stride != (long long)P || !k.closed)) return false;
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

// the emitter arguments (all zero at LV 0, which passes); N is known to be >= 2
static bool hy_emitter_args_ok(const HydEmitterArgs& e, int32_t N) {
  if (e.Ke < 0 || e.Ke > N) return false;
  if (e.Ke > 0 && (!e.node || !e.coef || !e.flow)) return false;
  if (e.coef_stride != 0 && e.coef_stride != (long long)e.Ke) return false;
  if (e.onset_stride != 0 && (e.onset_stride != (long long)e.Ke || !e.onset)) return false;
  return true;
}

static HydEmitterArgs hy_emitter_args(const int32_t* node, const double* coef, int64_t coef_stride, int32_t num_emitters,
                                      double exponent, const int32_t* onset, int64_t onset_stride, double* flow) {
  HydEmitterArgs e;
  e.node = node; e.coef = coef; e.onset = onset; e.coef_stride = (long long)coef_stride; e.onset_stride = (long long)onset_stride;
  e.exponent = exponent; e.Ke = (int)num_emitters; e.flow = flow;
  return e;
}

static HydPddArgs hy_pdd_args(int32_t demand_model, double pmin, double preq, double exponent, double* delivered) {
  HydPddArgs d;
  d.pmin = demand_model ? pmin : 0.0; d.preq = demand_model ? preq : 0.0; d.exponent = demand_model ? exponent : 1.0;
  d.delivered = delivered;
  return d;
}

// Raise the dynamic-LDS attribute of the kernel where the launch needs it (past the 64 KB a kernel gets unasked; per device)
static int hy_raise_lds(const void* kernel, uint64_t lds) {
  if (lds <= 64 * 1024) return 0;
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) (void)hipGetLastError();
  return (int)e;
}

// Every check of a steady launch at level lv (0 valves, 1 emitters, 2 pdd), and the launch.  A null pointer is no range of the
// overlap lists, so the arrays a lower level does not have drop out of them.
static int hy_solve_network(const HydNetSolveArgs& a, int lv, void* stream) {
  if (lv == 2 && !a.D.delivered) return GATRES_E_BADARG;
  if (!a.pipe_a || !a.pipe_b || !a.coef || !a.q_start || !a.fixed || !a.elevation || !a.order || !a.position) return GATRES_E_BADARG;
  if (!a.demand || !a.roughness || !a.fixed_head || !a.pressure || !a.status || !a.final_dq) return GATRES_E_BADARG;
  if (!hy_counts_ok(a.S, a.N, a.P) || a.N < 2) return GATRES_E_BADARG;
  if (!hy_emitter_args_ok(a.E, a.N) || !hy_valve_args_ok(a.L, a.P)) return GATRES_E_BADARG;
  if (a.W < 1 || a.W > a.N - 1) return GATRES_E_BADARG;
  if (a.max_iter < 1 || !(a.accuracy > 0.0) || !(a.accuracy <= DBL_MAX)) return GATRES_E_BADARG;
  if (a.fh_stride != 0 && a.fh_stride != (long long)a.N) return GATRES_E_BADARG;
  const uint64_t S = (uint64_t)a.S, N = (uint64_t)a.N, P = (uint64_t)a.P, Kp = (uint64_t)a.L.Kp, Kv = (uint64_t)a.L.Kv,
                 Ke = (uint64_t)a.E.Ke, Nd = lv == 2 ? N : 0;
  const uint64_t lds = hy_network_lds_bytes(N, P, (uint64_t)a.W, Kp, Kv, Ke, Nd);
  if (lds > HY_LDS_BUDGET) return GATRES_E_BADARG;
  if (hy_carve(nullptr, a.N, a.P, a.W, 0, a.L.Kp, a.L.Kv, a.E.Ke, (int)Nd, false).bytes > lds) return GATRES_E_BADARG;
  const void* wr[9] = {a.pressure, a.head, a.flow, a.status, a.final_dq, a.L.link_state, a.L.valve_changes,
                       Ke ? a.E.flow : nullptr, a.D.delivered};
  const uint64_t wn[9] = {4 * S * N, 8 * S * N, 8 * S * P, 4 * GATRES_HYD_STATUS * S, 8 * S, S * P, 4 * S, 8 * S * Ke, 8 * S * N};
  const void* rd[25] = {a.pipe_a, a.pipe_b, a.coef, a.q_start, a.fixed, a.elevation, a.order, a.position, a.demand, a.roughness,
                        a.fixed_head, a.L.link_kind, a.L.link_flags, a.L.minor, Kp ? a.L.pump_link : nullptr,
                        Kp ? a.L.pump_h0 : nullptr, Kp ? a.L.pump_r : nullptr, Kp ? a.L.pump_n : nullptr, Kp ? a.L.speed : nullptr,
                        a.L.closed, Kv ? a.L.valve_link : nullptr, Kv ? a.L.valve_kind : nullptr, Kv ? a.L.setting : nullptr,
                        Ke ? a.E.node : nullptr, Ke ? a.E.coef : nullptr};
  const uint64_t rn[25] = {4 * P, 4 * P, 8 * P, 8 * P, N, 8 * N, 4 * N, 4 * N, 8 * S * N, 8 * S * P,
                           a.fh_stride ? 8 * S * N : 8 * N, P, P, 8 * P, 4 * Kp, 8 * Kp, 8 * Kp, 8 * Kp,
                           a.L.speed_stride ? 8 * S * Kp : 8 * Kp, a.L.closed_stride ? S * P : P, 4 * Kv, Kv,
                           a.L.setting_stride ? 8 * S * Kv : 8 * Kv, 4 * Ke, a.E.coef_stride ? 8 * S * Ke : 8 * Ke};
  if (any_overlap(wr, wn, 9, rd, rn, 25)) return GATRES_E_BADARG;
  void (*const kernels[3])(const HydNetSolveArgs) = {hydraulic_solve_network_kernel<0>, hydraulic_solve_network_kernel<1>,
                                                  hydraulic_solve_network_kernel<2>};
  const int e = hy_raise_lds(reinterpret_cast<const void*>(kernels[lv]), lds);
  if (e != 0) return e;
  const long long wgs = a.S < HY_GRID_CAP ? a.S : HY_GRID_CAP;
  hipLaunchKernelGGL(kernels[lv], dim3((unsigned)wgs), dim3(HY_T), (size_t)lds, gatres_stream(stream), a);
  return gatres_launch_status();
}

// The same for a series; num_speed_patterns is the caller's count (a.Ms: 0 where there is no pump).  With ctl the launch has
// THE CONTROLS: the table *ctl is checked like every other array, and its LDS is added in closed form.
static int hy_series_network(HydNetSeriesArgs a, int32_t num_speed_patterns, int lv, void* stream, const HydControlArgs* ctl = nullptr) {
  if (lv == 2 && !a.D.delivered) return GATRES_E_BADARG;
  const HydControlArgs C = ctl ? *ctl : HydControlArgs{};
  if (ctl) {
    const HydControlArgs& c = C;
    if (!c.changes || c.Kc < 0) return GATRES_E_BADARG;
    if (c.Kc > 0 && (!c.link || !c.action || !c.value || !c.kind || !c.target || !c.threshold)) return GATRES_E_BADARG;
    if (c.threshold_stride != 0 && c.threshold_stride != (long long)c.Kc) return GATRES_E_BADARG;
    if (a.S >= 1 && c.Kc > 0 && a.S > INT64_MAX / 64 / (int64_t)c.Kc) return GATRES_E_BADARG;
  }
  if (!a.pipe_a || !a.pipe_b || !a.coef || !a.q_start || !a.fixed || !a.elevation || !a.order || !a.position) return GATRES_E_BADARG;
  if (!a.pattern || !a.mult || !a.demand || !a.roughness || !a.fixed_head || !a.pressure || !a.status || !a.final_dq)
    return GATRES_E_BADARG;
  if (a.K < 0 || a.T < 1 || a.M < 1) return GATRES_E_BADARG;
  if (a.K > 0 && (!a.tank_node || !a.tank_area || !a.tank_min || !a.tank_max || !a.level0 || !a.level)) return GATRES_E_BADARG;
  if (!hy_counts_ok(a.S, a.N, a.P) || a.N < 2) return GATRES_E_BADARG;
  if (!hy_emitter_args_ok(a.E, a.N) || !hy_valve_args_ok(a.L, a.P)) return GATRES_E_BADARG;
  if (num_speed_patterns < 0 || (a.L.Kp > 0 && (num_speed_patterns < 1 || !a.speed_mult || !a.speed_pattern))) return GATRES_E_BADARG;
  // every byte count below fits: S * (T + 1) * (N + P + K) * 64, S * M * T * 64 and Ms * T * 64
  const int64_t per_step = (int64_t)a.N + (int64_t)a.P + (int64_t)a.K + GATRES_HYD_STATUS;
  if (a.S > INT64_MAX / 64 / per_step / ((int64_t)a.T + 1)) return GATRES_E_BADARG;
  if ((int64_t)a.M > INT64_MAX / 64 / a.S / (int64_t)a.T) return GATRES_E_BADARG;
  if ((int64_t)num_speed_patterns > INT64_MAX / 64 / (int64_t)a.T) return GATRES_E_BADARG;
  if (a.W < 1 || a.W > a.N - 1) return GATRES_E_BADARG;
  if (a.max_iter < 1 || !(a.accuracy > 0.0) || !(a.accuracy <= DBL_MAX)) return GATRES_E_BADARG;
  if (!(a.dt > 0.0) || !(a.dt <= DBL_MAX)) return GATRES_E_BADARG;
  if (a.fh_stride != 0 && a.fh_stride != (long long)a.N) return GATRES_E_BADARG;
  if (a.mult_stride != 0 && a.mult_stride != (long long)a.M * (long long)a.T) return GATRES_E_BADARG;
  const uint64_t S = (uint64_t)a.S, T = (uint64_t)a.T, N = (uint64_t)a.N, P = (uint64_t)a.P, K = (uint64_t)a.K, M = (uint64_t)a.M,
                 Kp = (uint64_t)a.L.Kp, Kv = (uint64_t)a.L.Kv, Ms = Kp ? (uint64_t)num_speed_patterns : 0, Ke = (uint64_t)a.E.Ke,
                 Nd = lv == 2 ? N : 0, Kc = (uint64_t)C.Kc;
  const uint64_t lds = hy_series_network_lds_bytes(N, P, (uint64_t)a.W, K, Kp, Kv, Ke, Nd) + (ctl ? hy_controls_lds_bytes(P) : 0);
  if (lds > HY_LDS_BUDGET) return GATRES_E_BADARG;
  if (hy_carve(nullptr, a.N, a.P, a.W, a.K, a.L.Kp, a.L.Kv, a.E.Ke, (int)Nd, true, ctl ? a.P : 0).bytes > lds) return GATRES_E_BADARG;
  const void* wr[11] = {a.pressure, a.head, a.flow, K ? a.level : nullptr, a.status, a.final_dq, a.L.link_state, a.L.valve_changes,
                        Ke ? a.E.flow : nullptr, a.D.delivered, C.changes};
  const uint64_t wn[11] = {4 * S * T * N, 8 * S * T * N, 8 * S * T * P, 8 * S * (T + 1) * K, 4 * GATRES_HYD_STATUS * S * T, 8 * S * T,
                           S * T * P, 4 * S * T, 8 * S * T * Ke, 8 * S * T * N, 4 * S * T};
  const void* rd[41] = {a.pipe_a, a.pipe_b, a.coef, a.q_start, a.fixed, a.elevation, a.order, a.position, K ? a.tank_node : nullptr,
                        K ? a.tank_area : nullptr, K ? a.tank_min : nullptr, K ? a.tank_max : nullptr, a.pattern, a.mult,
                        a.demand, a.roughness, a.fixed_head, K ? a.level0 : nullptr, a.L.link_kind, a.L.link_flags, a.L.minor,
                        Kp ? a.L.pump_link : nullptr, Kp ? a.L.pump_h0 : nullptr, Kp ? a.L.pump_r : nullptr,
                        Kp ? a.L.pump_n : nullptr, Kp ? a.L.speed : nullptr, a.L.closed, Kp ? a.speed_mult : nullptr,
                        Kp ? a.speed_pattern : nullptr, Kv ? a.L.valve_link : nullptr, Kv ? a.L.valve_kind : nullptr,
                        Kv ? a.L.setting : nullptr, Ke ? a.E.node : nullptr, Ke ? a.E.coef : nullptr, Ke ? a.E.onset : nullptr,
                        Kc ? C.link : nullptr, Kc ? C.action : nullptr, Kc ? C.value : nullptr, Kc ? C.kind : nullptr,
                        Kc ? C.target : nullptr, Kc ? C.threshold : nullptr};
  const uint64_t rn[41] = {4 * P, 4 * P, 8 * P, 8 * P, N, 8 * N, 4 * N, 4 * N, 4 * K, 8 * K, 8 * K, 8 * K, 4 * N,
                           a.mult_stride ? 8 * S * M * T : 8 * M * T, 8 * S * N, 8 * S * P, a.fh_stride ? 8 * S * N : 8 * N,
                           8 * S * K, P, P, 8 * P, 4 * Kp, 8 * Kp, 8 * Kp, 8 * Kp, a.L.speed_stride ? 8 * S * Kp : 8 * Kp,
                           a.L.closed_stride ? S * P : P, 8 * Ms * T, 4 * Kp, 4 * Kv, Kv, a.L.setting_stride ? 8 * S * Kv : 8 * Kv,
                           4 * Ke, a.E.coef_stride ? 8 * S * Ke : 8 * Ke, a.E.onset_stride ? 4 * S * Ke : 4 * Ke,
                           4 * Kc, Kc, 8 * Kc, Kc, 4 * Kc, C.threshold_stride ? 8 * S * Kc : 8 * Kc};
  if (any_overlap(wr, wn, 11, rd, rn, 41)) return GATRES_E_BADARG;
  void (*const kernels[3])(const HydNetSeriesArgs) = {hydraulic_series_network_kernel<0, false>, hydraulic_series_network_kernel<1, false>,
                                                   hydraulic_series_network_kernel<2, false>};
  void (*const ctl_kernels[3])(const HydNetSeriesCtlArgs) = {nullptr, hydraulic_series_network_kernel<1, true>,
                                                          hydraulic_series_network_kernel<2, true>};       // (no entry point takes LV 0)
  const int e = hy_raise_lds(ctl ? reinterpret_cast<const void*>(ctl_kernels[lv]) : reinterpret_cast<const void*>(kernels[lv]), lds);
  if (e != 0) return e;
  if (!Ke) a.E.onset = nullptr;
  a.Ms = (int)Ms;
  const long long wgs = a.S < HY_GRID_CAP ? a.S : HY_GRID_CAP;
  if (ctl) {
    HydNetSeriesCtlArgs ac;
    static_cast<HydNetSeriesArgs&>(ac) = a;
    ac.C = C;
    hipLaunchKernelGGL(ctl_kernels[lv], dim3((unsigned)wgs), dim3(HY_T), (size_t)lds, gatres_stream(stream), ac);
  } else {
    hipLaunchKernelGGL(kernels[lv], dim3((unsigned)wgs), dim3(HY_T), (size_t)lds, gatres_stream(stream), a);
  }
  return gatres_launch_status();
}

// the arguments every steady entry point begins with (valves, emitters and demand model: zero until the entry point sets them)
static HydNetSolveArgs hy_solve_args(const int32_t* pipe_a, const int32_t* pipe_b, const double* coef, const double* q_start,
                                  const uint8_t* fixed, const double* elevation, const int32_t* order, const int32_t* position,
                                  int32_t half_bandwidth, const double* demand, const double* roughness, const double* fixed_head,
                                  int64_t fixed_head_stride, int64_t num_scenarios, int32_t num_nodes, int32_t num_pipes,
                                  double accuracy, int32_t max_iter, float* pressure, double* head, double* flow, int32_t* status,
                                  double* final_dq) {
  HydNetSolveArgs a = {};
  a.pipe_a = pipe_a; a.pipe_b = pipe_b; a.coef = coef; a.q_start = q_start; a.fixed = fixed; a.elevation = elevation;
  a.order = order; a.position = position; a.demand = demand; a.roughness = roughness; a.fixed_head = fixed_head;
  a.fh_stride = (long long)fixed_head_stride; a.S = (long long)num_scenarios;
  a.N = (int)num_nodes; a.P = (int)num_pipes; a.W = (int)half_bandwidth; a.max_iter = (int)max_iter; a.accuracy = accuracy;
  a.pressure = pressure; a.head = head; a.flow = flow; a.status = status; a.final_dq = final_dq;
  return a;
}

// the arguments every series entry point begins with
static HydNetSeriesArgs hy_series_args(const int32_t* pipe_a, const int32_t* pipe_b, const double* coef, const double* q_start,
                                    const uint8_t* fixed, const double* elevation, const int32_t* order, const int32_t* position,
                                    int32_t half_bandwidth, const int32_t* tank_node, const double* tank_area,
                                    const double* tank_min_level, const double* tank_max_level, int32_t num_tanks,
                                    const int32_t* pattern_of_node, const double* mult, int64_t mult_stride, int32_t num_patterns,
                                    const double* demand, const double* roughness, const double* fixed_head,
                                    int64_t fixed_head_stride, const double* initial_level, int64_t num_series, int32_t num_steps,
                                    int32_t num_nodes, int32_t num_pipes, double dt, int32_t warm_start, double accuracy,
                                    int32_t max_iter, float* pressure, double* head, double* flow, double* level, int32_t* status,
                                    double* final_dq, const double* speed_mult, const int32_t* speed_pattern_of_pump) {
  HydNetSeriesArgs a = {};
  a.pipe_a = pipe_a; a.pipe_b = pipe_b; a.coef = coef; a.q_start = q_start; a.fixed = fixed; a.elevation = elevation;
  a.order = order; a.position = position; a.tank_node = tank_node; a.tank_area = tank_area; a.tank_min = tank_min_level;
  a.tank_max = tank_max_level; a.pattern = pattern_of_node; a.mult = mult; a.demand = demand; a.roughness = roughness;
  a.fixed_head = fixed_head; a.level0 = initial_level; a.mult_stride = (long long)mult_stride;
  a.fh_stride = (long long)fixed_head_stride; a.S = (long long)num_series; a.T = (int)num_steps; a.N = (int)num_nodes;
  a.P = (int)num_pipes; a.W = (int)half_bandwidth; a.K = (int)num_tanks; a.M = (int)num_patterns; a.max_iter = (int)max_iter;
  a.warm = warm_start != 0 ? 1 : 0; a.dt = dt; a.accuracy = accuracy;
  a.pressure = pressure; a.head = head; a.flow = flow; a.level = level; a.status = status; a.final_dq = final_dq;
  a.speed_mult = speed_mult; a.speed_pattern = speed_pattern_of_pump;
  return a;
}

}  // namespace

extern "C" int gatres_hydraulic_solve_valves(const int32_t* pipe_a, const int32_t* pipe_b, const double* coef, const double* q_start,
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
                                             int64_t valve_setting_stride, int32_t num_valves, int32_t* valve_changes, void* stream) {
  HydNetSolveArgs a = hy_solve_args(pipe_a, pipe_b, coef, q_start, fixed, elevation, order, position, half_bandwidth, demand, roughness,
                                 fixed_head, fixed_head_stride, num_scenarios, num_nodes, num_pipes, accuracy, max_iter, pressure,
                                 head, flow, status, final_dq);
  a.L = hy_valve_args(link_kind, link_flags, minor, pump_link, pump_h0, pump_r, pump_n, num_pumps, speed, speed_stride, closed,
                      closed_stride, link_state, valve_link, valve_kind, valve_setting, valve_setting_stride, num_valves,
                      valve_changes);
  return hy_solve_network(a, 0, stream);
}

extern "C" int gatres_hydraulic_solve_emitters(const int32_t* pipe_a, const int32_t* pipe_b, const double* coef, const double* q_start,
                                               const uint8_t* fixed, const double* elevation, const int32_t* order,
                                               const int32_t* position, int32_t half_bandwidth, const double* demand,
                                               const double* roughness, const double* fixed_head, int64_t fixed_head_stride,
                                               int64_t num_scenarios, int32_t num_nodes, int32_t num_pipes, double accuracy,
                                               int32_t max_iter, float* pressure, double* head, double* flow, int32_t* status,
                                               double* final_dq, const uint8_t* link_kind, const uint8_t* link_flags,
                                               const double* minor, const int32_t* pump_link, const double* pump_h0,
                                               const double* pump_r, const double* pump_n, int32_t num_pumps, const double* speed,
                                               int64_t speed_stride, const uint8_t* closed, int64_t closed_stride,
                                               uint8_t* link_state, const int32_t* valve_link, const uint8_t* valve_kind,
                                               const double* valve_setting, int64_t valve_setting_stride, int32_t num_valves,
                                               int32_t* valve_changes, const int32_t* emitter_node, const double* emitter_coef,
                                               int64_t emitter_coef_stride, int32_t num_emitters, double emitter_exponent,
                                               double* emitter_flow, void* stream) {
  HydNetSolveArgs a = hy_solve_args(pipe_a, pipe_b, coef, q_start, fixed, elevation, order, position, half_bandwidth, demand, roughness,
                                 fixed_head, fixed_head_stride, num_scenarios, num_nodes, num_pipes, accuracy, max_iter, pressure,
                                 head, flow, status, final_dq);
  a.L = hy_valve_args(link_kind, link_flags, minor, pump_link, pump_h0, pump_r, pump_n, num_pumps, speed, speed_stride, closed,
                      closed_stride, link_state, valve_link, valve_kind, valve_setting, valve_setting_stride, num_valves,
                      valve_changes);
  a.E = hy_emitter_args(emitter_node, emitter_coef, emitter_coef_stride, num_emitters, emitter_exponent, nullptr, 0, emitter_flow);
  return hy_solve_network(a, 1, stream);
}

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
  HydNetSolveArgs a = hy_solve_args(pipe_a, pipe_b, coef, q_start, fixed, elevation, order, position, half_bandwidth, demand, roughness,
                                 fixed_head, fixed_head_stride, num_scenarios, num_nodes, num_pipes, accuracy, max_iter, pressure,
                                 head, flow, status, final_dq);
  a.L = hy_valve_args(link_kind, link_flags, minor, pump_link, pump_h0, pump_r, pump_n, num_pumps, speed, speed_stride, closed,
                      closed_stride, link_state, valve_link, valve_kind, valve_setting, valve_setting_stride, num_valves,
                      valve_changes);
  a.E = hy_emitter_args(emitter_node, emitter_coef, emitter_coef_stride, num_emitters, emitter_exponent, nullptr, 0, emitter_flow);
  a.D = hy_pdd_args(demand_model, minimum_pressure, required_pressure, pressure_exponent, demand_delivered);
  return hy_solve_network(a, demand_model ? 2 : 1, stream);
}

extern "C" int gatres_hydraulic_series_valves(
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
    int64_t valve_setting_stride, int32_t num_valves, int32_t* valve_changes, void* stream) {
  HydNetSeriesArgs a = hy_series_args(pipe_a, pipe_b, coef, q_start, fixed, elevation, order, position, half_bandwidth, tank_node,
                                   tank_area, tank_min_level, tank_max_level, num_tanks, pattern_of_node, mult, mult_stride,
                                   num_patterns, demand, roughness, fixed_head, fixed_head_stride, initial_level, num_series,
                                   num_steps, num_nodes, num_pipes, dt, warm_start, accuracy, max_iter, pressure, head, flow, level,
                                   status, final_dq, speed_mult, speed_pattern_of_pump);
  a.L = hy_valve_args(link_kind, link_flags, minor, pump_link, pump_h0, pump_r, pump_n, num_pumps, speed, speed_stride, closed,
                      closed_stride, link_state, valve_link, valve_kind, valve_setting, valve_setting_stride, num_valves,
                      valve_changes);
  return hy_series_network(a, num_speed_patterns, 0, stream);
}

extern "C" int gatres_hydraulic_series_emitters(
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
    const int32_t* emitter_onset, int64_t emitter_onset_stride, double* emitter_flow, void* stream) {
  HydNetSeriesArgs a = hy_series_args(pipe_a, pipe_b, coef, q_start, fixed, elevation, order, position, half_bandwidth, tank_node,
                                   tank_area, tank_min_level, tank_max_level, num_tanks, pattern_of_node, mult, mult_stride,
                                   num_patterns, demand, roughness, fixed_head, fixed_head_stride, initial_level, num_series,
                                   num_steps, num_nodes, num_pipes, dt, warm_start, accuracy, max_iter, pressure, head, flow, level,
                                   status, final_dq, speed_mult, speed_pattern_of_pump);
  a.L = hy_valve_args(link_kind, link_flags, minor, pump_link, pump_h0, pump_r, pump_n, num_pumps, speed, speed_stride, closed,
                      closed_stride, link_state, valve_link, valve_kind, valve_setting, valve_setting_stride, num_valves,
                      valve_changes);
  a.E = hy_emitter_args(emitter_node, emitter_coef, emitter_coef_stride, num_emitters, emitter_exponent, emitter_onset,
                        emitter_onset_stride, emitter_flow);
  return hy_series_network(a, num_speed_patterns, 1, stream);
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
  HydNetSeriesArgs a = hy_series_args(pipe_a, pipe_b, coef, q_start, fixed, elevation, order, position, half_bandwidth, tank_node,
                                   tank_area, tank_min_level, tank_max_level, num_tanks, pattern_of_node, mult, mult_stride,
                                   num_patterns, demand, roughness, fixed_head, fixed_head_stride, initial_level, num_series,
                                   num_steps, num_nodes, num_pipes, dt, warm_start, accuracy, max_iter, pressure, head, flow, level,
                                   status, final_dq, speed_mult, speed_pattern_of_pump);
  a.L = hy_valve_args(link_kind, link_flags, minor, pump_link, pump_h0, pump_r, pump_n, num_pumps, speed, speed_stride, closed,
                      closed_stride, link_state, valve_link, valve_kind, valve_setting, valve_setting_stride, num_valves,
                      valve_changes);
  a.E = hy_emitter_args(emitter_node, emitter_coef, emitter_coef_stride, num_emitters, emitter_exponent, emitter_onset,
                        emitter_onset_stride, emitter_flow);
  a.D = hy_pdd_args(demand_model, minimum_pressure, required_pressure, pressure_exponent, demand_delivered);
  return hy_series_network(a, num_speed_patterns, demand_model ? 2 : 1, stream);
}

extern "C" int gatres_hydraulic_series_controls(
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
    double minimum_pressure, double required_pressure, double pressure_exponent, double* demand_delivered,
    const int32_t* control_link, const uint8_t* control_action, const double* control_value, const uint8_t* control_kind,
    const int32_t* control_target, const double* control_threshold, int64_t control_threshold_stride, int32_t num_controls,
    int32_t* control_changes, void* stream) {
  if (demand_model != 0 && demand_model != 1) return GATRES_E_BADARG;
  HydNetSeriesArgs a = hy_series_args(pipe_a, pipe_b, coef, q_start, fixed, elevation, order, position, half_bandwidth, tank_node,
                                   tank_area, tank_min_level, tank_max_level, num_tanks, pattern_of_node, mult, mult_stride,
                                   num_patterns, demand, roughness, fixed_head, fixed_head_stride, initial_level, num_series,
                                   num_steps, num_nodes, num_pipes, dt, warm_start, accuracy, max_iter, pressure, head, flow, level,
                                   status, final_dq, speed_mult, speed_pattern_of_pump);
  a.L = hy_valve_args(link_kind, link_flags, minor, pump_link, pump_h0, pump_r, pump_n, num_pumps, speed, speed_stride, closed,
                      closed_stride, link_state, valve_link, valve_kind, valve_setting, valve_setting_stride, num_valves,
                      valve_changes);
  a.E = hy_emitter_args(emitter_node, emitter_coef, emitter_coef_stride, num_emitters, emitter_exponent, emitter_onset,
                        emitter_onset_stride, emitter_flow);
  a.D = hy_pdd_args(demand_model, minimum_pressure, required_pressure, pressure_exponent, demand_delivered);
  HydControlArgs c;
  c.link = control_link; c.action = control_action; c.value = control_value; c.kind = control_kind; c.target = control_target;
  c.threshold = control_threshold; c.threshold_stride = (long long)control_threshold_stride; c.Kc = (int)num_controls;
  c.changes = control_changes;
  return hy_series_network(a, num_speed_patterns, demand_model ? 2 : 1, stream, &c);
}

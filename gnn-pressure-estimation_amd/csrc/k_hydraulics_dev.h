// The hydraulic Newton loop, stated once for the two kernels of k_hydraulics.hip (hydraulic_solve_kernel: one steady scenario per
// workgroup; hydraulic_series_kernel: one series of steps per workgroup) and their two counterparts with pumps, check valves,
// closed links and minor losses in k_hydraulic_links.hip; and, at the end, with the status machine of the regulating valves and,
// by compile-time arguments of that loop, with the node terms of the emitters and of the pressure-driven demand, for the two
// kernel templates of k_hydraulic_network.hip (one instantiation per level: valves, emitters, pressure-driven demand).  Behind the
// loops stand the helpers the link and network kernels share, and the host checks of every hydraulic entry point.
// gatres.h states the model, the law at low flow, the link law, the valves, the emitters, the pressure-driven demand and the solver.  Everything here works on one workgroup's LDS arrays; every sum runs in a fixed order.
#pragma once
#include "gatres_common.h"

#include <float.h>
#include <math.h>

namespace {

constexpr int HY_T = 256;                                  // threads of a solve workgroup
constexpr double HY_LINEAR_G = 1e-7;                       // the law at low flow (gatres.h)

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

// THE LINK LAW of gatres.h (pumps, check valves, closed links, minor losses), link_headloss of hydraulics.py.  code: HY_PUMP,
// HY_CHECK (set for every pump), HY_SHUT (shut in this scenario or step: by the static flag HY_CLOSED, by the scenario's byte
// or by a pump speed of zero); pump: the pump's {h0, rp, n, w^2, w^(2-n), w}, read where HY_PUMP is set and HY_SHUT is not.
// With code 0 and m = 0 it is pipe_headloss in every bit: ra + 0 is ra, and 1.852 ra + 0 is 1.852 ra.
constexpr int HY_PUMP = 1, HY_CHECK = 2, HY_SHUT = 4, HY_CLOSED = 8;
constexpr int HY_PUMP_SHIFT = 4;                           // a link's code holds its pump's index above the four bits
constexpr int HY_PUMP_REC = 6;                             // doubles of a pump's record
constexpr double HY_SHUT_G = 1e8;                          // the gradient of a shut link and of a CHECK link's reverse branch

__device__ __forceinline__ void link_headloss(double q, double r, double m, int code, const double* pump, double* h, double* g) {
  if (code & HY_SHUT) {
    *g = HY_SHUT_G;
    *h = HY_SHUT_G * q;
    return;
  }
  double lift = 0.0;                                       // -h(0): w^2 h0 of a pump
  if (code & HY_PUMP) lift = pump[3] * pump[0];
  if ((code & HY_CHECK) && q < 0.0) {
    *g = HY_SHUT_G;
    *h = HY_SHUT_G * q - lift;
    return;
  }
  double gg, hh;
  if (code & HY_PUMP) {
    const double n = pump[2], ca = (pump[4] * pump[1]) * pow(q, n - 1.0);      // (q >= 0 here; pow(0, 0) is 1)
    gg = n * ca;
    hh = ca * q;
  } else {
    const double aq = fabs(q), ra = r * pow(aq, 0.852), ma = m * aq;
    gg = 1.852 * ra + 2.0 * ma;
    hh = (ra + ma) * q;
  }
  if (gg < HY_LINEAR_G) {
    gg = HY_LINEAR_G;
    hh = HY_LINEAR_G * q;
  }
  *h = hh - lift;
  *g = gg;
}

// The LDS arrays of the Newton loop (a workgroup's own; the kernels lay them out)
struct HyLds {
  double* band;                                            // [N][W + 1]: band[r * BW + k] = A[r][r - k], rows in solver order
  double* y;                                               // [N] the right-hand side, then the substitutions' vector
  double* H;                                               // [N] heads by solver row; the fixed rows are set by the caller
  double* q;                                               // [P] flows: the start on entry, the result on return
  double* rr;                                              // [P] resistance r_p
  double* pinv;                                            // [P] 1 / g_p; after the flow update |dq_p|
  double* yv;                                              // [P] h_p / g_p; after the flow update |q_p|
  double* red;                                             // [4] the two sums of the stop rule
  int *sa, *sb;                                            // [P] solver rows of a pipe's ends
  int* fx;                                                 // [N] fixed flag by solver row
  // the link law's arrays (hy_newton<true> alone reads them; the pipe-only kernels leave them out)
  double* minor = nullptr;                                 // [P] minor-loss coefficient m_p
  double* pump = nullptr;                                  // [Kp][HY_PUMP_REC] h0, rp, n, w^2, w^(2-n), w
  int* code = nullptr;                                     // [P] HY_PUMP | HY_CHECK | HY_SHUT | HY_CLOSED | pump index << HY_PUMP_SHIFT
};

// The static arrays of a launch, checked: nothing in the kernels indexes with a value that was not checked here.  Fills L.fx,
// L.sa and L.sb; flag[0] is the workgroup's word for the verdict.  Returns true where an array is not what gatres.h states; the
// permutation is good (position may index L.fx) exactly where *perm_ok.  Ends behind a barrier.
__device__ __forceinline__ bool hy_check_static(const HyLds& L, const int* __restrict__ position, const int* __restrict__ order,
                                                const uint8_t* __restrict__ fixed, const int* __restrict__ pipe_a,
                                                const int* __restrict__ pipe_b, int N, int P, int W, int* flag, int tid,
                                                bool* perm_good = nullptr) {
  int *sa = L.sa, *sb = L.sb, *fx = L.fx;
  if (tid == 0) flag[0] = 0;
  __syncthreads();
  for (int n = tid; n < N; n += HY_T) {
    const int r = position[n];
    bool ok = r >= 0 && r < N;
    if (ok) ok = order[r] == n;                            // (holds for every n: position is a permutation, order its inverse)
    if (ok) fx[r] = fixed[n] ? 1 : 0;
    else flag[0] = 1;
  }
  __syncthreads();
  const bool perm_ok = flag[0] == 0;
  if (perm_good) *perm_good = perm_ok;
  for (int p = tid; p < P; p += HY_T) {
    const int a = pipe_a[p], b = pipe_b[p];
    bool ok = perm_ok && a >= 0 && a < N && b >= 0 && b < N && a != b;
    int ra = 0, rb = 0;
    if (ok) {
      ra = position[a];
      rb = position[b];
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
  return flag[0] != 0;
}

struct HyNewton {
  int iters;
  bool converged, failed;
  double rel;                                              // the last sum |dq| / sum |q|
};

// The whole Newton loop of one scenario, run by all HY_T threads of the workgroup.  position: node -> solver row (checked by the
// caller); dem: the demands by node, in global memory or in LDS.  The caller has put a barrier behind its writes to L; the loop
// ends behind a barrier or with values that are the same in every thread.  LINKS chooses the law at compile time: pipe_headloss
// (the default: the loop the pipe-only kernels have always had) or link_headloss; nothing else differs.
template <bool LINKS = false>
__device__ __forceinline__ HyNewton hy_newton(const HyLds& L, const int* __restrict__ position, const double* dem, int N, int P,
                                              int W, int max_iter, double accuracy, int tid) {
  const int BW = W + 1;
  double *band = L.band, *y = L.y, *H = L.H, *q = L.q, *rr = L.rr, *pinv = L.pinv, *yv = L.yv, *red = L.red;
  const int *sa = L.sa, *sb = L.sb, *fx = L.fx;
  HyNewton out;
  out.iters = 0;
  out.converged = false;
  out.failed = false;
  out.rel = 0.0;
  for (int it = 1; it <= max_iter; ++it) {
    out.iters = it;
    // the law at the present flows
    for (int p = tid; p < P; p += HY_T) {
      double h, g;
      if constexpr (LINKS) {
        const int code = L.code[p];
        link_headloss(q[p], rr[p], L.minor[p], code, L.pump + (size_t)(code >> HY_PUMP_SHIFT) * HY_PUMP_REC, &h, &g);
      } else {
        pipe_headloss(q[p], rr[p], &h, &g);
      }
      pinv[p] = 1.0 / g;
      yv[p] = h / g;
    }
    __syncthreads();
    // assembly: one thread per row, over the pipes in pipe order
    for (int n = tid; n < N; n += HY_T) {
      const int r = position[n];
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
          else if (o < r) row[r - o] -= pi;                // (r - o <= W: checked by the caller)
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
      if (!(d > 0.0) || !hy_finite(d)) {                   // (the same value in every thread)
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
      out.failed = true;
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
    if (tid == 0 || tid == 64) {                           // one thread per sum, in pipe order
      const double* v = tid == 0 ? pinv : yv;
      double sum = 0.0;
      for (int p = 0; p < P; ++p) sum += v[p];
      red[tid == 0 ? 0 : 1] = sum;
    }
    __syncthreads();
    const double dqs = red[0], qs = red[1];
    if (!hy_finite(dqs) || !hy_finite(qs)) {
      out.failed = true;
      break;
    }
    out.rel = qs > 0.0 ? dqs / qs : (dqs > 0.0 ? __longlong_as_double(0x7FF0000000000000ll) : 0.0);
    out.converged = dqs <= accuracy * qs;
    if (out.converged) break;
  }
  return out;
}

// ---- THE REGULATING VALVES of gatres.h (k_hydraulic_network.hip) -------------------------------------------------------------------
// A regulating valve's link keeps, above the bits of the link law, what it is and where its status machine stands; a valve is
// never a pump, so the bits of a pump's index are free.  OPEN is neither status bit.  fx[row] of a valve's controlled node is
// HY_FX_VALVE while the valve is ACTIVE and 0 otherwise; a fixed-head node has 1 and is never a controlled node.
constexpr int HY_VALVE = 1 << 30, HY_VALVE_ACTIVE = 1 << 29, HY_VALVE_CLOSED = 1 << 28, HY_VALVE_PSV = 1 << 27;
constexpr int HY_FX_VALVE = 2;
constexpr int HY_ST_OPEN = 0, HY_ST_ACTIVE = 3, HY_ST_CLOSED = 4;      // link_state of a regulating valve
constexpr double HY_HTOL = 1.524e-4, HY_QTOL = 2.8316846592e-6;        // EPANET's 0.0005 ft and 0.0001 cfs

struct HyValves {
  double* hset;                                            // [Kv] the target head elevation[c] + setting of the scenario
  int* link;                                               // [Kv] the valve's link
  int* row;                                                // [Kv] solver row of the controlled node c
  int* node;                                               // [Kv] c itself
  int* chg;                                                // [Kv] 1 where the status changed in this iteration
  int Kv;
};

__device__ __forceinline__ int hy_valve_status(int code) {
  return (code & HY_VALVE_ACTIVE) ? HY_ST_ACTIVE : ((code & HY_VALVE_CLOSED) ? HY_ST_CLOSED : HY_ST_OPEN);
}

// The six rules of gatres.h: the next status from the old one, the new heads at the valve's ends and its new flow.
__device__ __forceinline__ int hy_valve_next(bool psv, int st, double Ha, double Hb, double q, double hml, double hset) {
  if (st != HY_ST_CLOSED) {
    if (q < -HY_QTOL) return HY_ST_CLOSED;
    if (!psv) {
      if (st == HY_ST_ACTIVE) return Ha - hml < hset - HY_HTOL ? HY_ST_OPEN : HY_ST_ACTIVE;
      return Hb >= hset + HY_HTOL ? HY_ST_ACTIVE : HY_ST_OPEN;
    }
    if (st == HY_ST_ACTIVE) return Hb + hml > hset + HY_HTOL ? HY_ST_OPEN : HY_ST_ACTIVE;
    return Ha < hset - HY_HTOL ? HY_ST_ACTIVE : HY_ST_OPEN;
  }
  if (!psv) {
    if (Ha >= hset + HY_HTOL && Hb < hset - HY_HTOL) return HY_ST_ACTIVE;
    if (Ha < hset - HY_HTOL && Ha > Hb + HY_HTOL) return HY_ST_OPEN;
    return HY_ST_CLOSED;
  }
  if (Hb > hset + HY_HTOL && Ha > Hb + HY_HTOL) return HY_ST_OPEN;
  if (Ha >= hset + HY_HTOL && Ha > Hb + HY_HTOL) return HY_ST_ACTIVE;
  return HY_ST_CLOSED;
}

struct HyNewtonValves {
  HyNewton n;
  int changes;                                             // status changes over all iterations
};

// ---- THE EMITTERS of gatres.h (k_hydraulic_network.hip) ----------------------------------------------------------------------------
// An emitter is a virtual link from its junction to the fixed head z = elevation, with a flow of its own, positive out of the
// network.  ce < 0 marks an emitter that is off in this scenario or step (C == 0): its row gets nothing and its flow is +0.0.
struct HyEmitters {
  double* ce = nullptr;                                    // [Ke] C^(-n) of the scenario or step, -1 where the emitter is off
  double* z = nullptr;                                     // [Ke] elevation of the emitter's junction
  double* q = nullptr;                                     // [Ke] the emitter's flow: the start on entry, the result on return
  double* einv = nullptr;                                  // [Ke] 1 / g; after the flow update |dq|
  double* ey = nullptr;                                    // [Ke] h / g; after the flow update |q|
  int* row = nullptr;                                      // [Ke] solver row of the junction
  int* node = nullptr;                                     // [Ke] the junction itself
  int Ke = 0;
  double n = 2.0;                                          // 1 / gamma, one value per launch
};

// emitter_headloss of gatres.h / hydraulics.py
__device__ __forceinline__ void emitter_headloss(double q, double ce, double n, double* h, double* g) {
  if (q < 0.0) {                                           // a leak takes no water in: the reverse branch of a CHECK link
    *g = HY_SHUT_G;
    *h = HY_SHUT_G * q;
    return;
  }
  const double ca = ce * pow(q, n - 1.0);                  // (pow(0, 0) is 1; pow(0, n - 1 < 0) is +inf)
  double gg = n * ca, hh = ca * q;
  if (gg < HY_LINEAR_G) {
    gg = HY_LINEAR_G;
    hh = HY_LINEAR_G * q;
  } else if (!(gg <= HY_SHUT_G)) {                         // (also where g is not finite)
    gg = HY_SHUT_G;
    hh = HY_SHUT_G * q;
  }
  *h = hh;
  *g = gg;
}

// ---- THE PRESSURE-DRIVEN DEMAND of gatres.h (k_hydraulic_network.hip) ----------------------------------------------------------------
// A junction whose full demand D is positive is a virtual link from the junction to the fixed head z = elevation + Pmin, with a
// flow q_d of its own, positive out of the network.  The record is indexed by NODE: there are up to N of these, and no thread
// walks a list.  dd[n] == 0 marks a node that is not pressure-driven (a fixed-head node, a junction with D <= 0): it keeps the
// fixed draw -dem[n], its 1 / g and h / g stay +0.0, and adding them to the sums of the stop rule changes no bit.
struct HyPdd {
  double* dd = nullptr;                                    // [N] the full demand D of a pressure-driven junction, 0 elsewhere
  double* q = nullptr;                                     // [N] q_d: the start on entry, the result on return
  double* dinv = nullptr;                                  // [N] 1 / g; after the flow update |dq|
  double* dy = nullptr;                                    // [N] h / g; after the flow update |q_d|
  const double* elevation = nullptr;                       // [N] by node (global memory)
  double pmin = 0.0, dp = 0.0, n = 2.0;                    // Pmin, Preq - Pmin, 1 / exponent: one value each per launch
};

// demand_headloss of gatres.h / hydraulics.py (D > 0)
__device__ __forceinline__ void demand_headloss(double q, double D, double dp, double n, double* h, double* g) {
  if (q < 0.0) {                                           // no demand node feeds the network
    *g = HY_SHUT_G;
    *h = HY_SHUT_G * q;
    return;
  }
  if (q > D) {                                             // above the required pressure: the full demand, and a shut link's leak
    *g = HY_SHUT_G;
    *h = dp + HY_SHUT_G * (q - D);
    return;
  }
  double gg = ((n * dp) * pow(q / D, n - 1.0)) / D, hh = (gg * q) / n;       // (pow(0, 0) is 1; pow(0, n - 1 < 0) is +inf)
  if (gg < HY_LINEAR_G) {
    gg = HY_LINEAR_G;
    hh = HY_LINEAR_G * q;
  } else if (!(gg <= HY_SHUT_G)) {                         // (also where g is not finite)
    gg = HY_SHUT_G;
    hh = HY_SHUT_G * q;
  }
  *h = hh;
  *g = gg;
}

// hy_newton<true> with the status machine of the regulating valves; with Kv == 0 every operation on a double is the one of
// hy_newton<true>, in the same order.  L.code carries the valves' bits (set by the caller: a valve that its input does not shut
// starts with a status bit or none), L.fx the fixed-head nodes as 1; red[2] takes the iteration's count of changes.  EMIT adds
// the node term of the emitters E at compile time (the default: the loop the valves kernels have always had); an emitter's
// junction is never a fixed row nor a valve's controlled node (checked by the caller).  PDD adds the node term of the
// pressure-driven demand D at compile time (the default: the loop as it was); such a junction may be a valve's controlled node.
template <bool EMIT = false, bool PDD = false>
__device__ __forceinline__ HyNewtonValves hy_newton_valves(const HyLds& L, const HyValves& V, const int* __restrict__ position,
                                                           const double* dem, int N, int P, int W, int max_iter, double accuracy,
                                                           int tid, const HyEmitters& E = HyEmitters(),
                                                           const HyPdd& D = HyPdd()) {
  const int BW = W + 1, Kv = V.Kv;
  double *band = L.band, *y = L.y, *H = L.H, *q = L.q, *rr = L.rr, *pinv = L.pinv, *yv = L.yv, *red = L.red;
  const int *sa = L.sa, *sb = L.sb;
  int *fx = L.fx, *code = L.code;
  HyNewtonValves out;
  out.n.iters = 0;
  out.n.converged = false;
  out.n.failed = false;
  out.n.rel = 0.0;
  out.changes = 0;
  for (int it = 1; it <= max_iter; ++it) {
    out.n.iters = it;
    // the law at the present flows and statuses; an ACTIVE valve is not in the matrix, and its controlled node is a fixed row
    for (int p = tid; p < P; p += HY_T) {
      int c = code[p];
      if (c & HY_VALVE_ACTIVE) {
        pinv[p] = 0.0;
        yv[p] = 0.0;
        continue;
      }
      if (c & HY_VALVE_CLOSED) c |= HY_SHUT;
      double h, g;
      link_headloss(q[p], rr[p], L.minor[p], c, L.pump + (size_t)((c & HY_PUMP) ? c >> HY_PUMP_SHIFT : 0) * HY_PUMP_REC, &h, &g);
      pinv[p] = 1.0 / g;
      yv[p] = h / g;
    }
    for (int k = tid; k < Kv; k += HY_T) {
      const bool active = (code[V.link[k]] & HY_VALVE_ACTIVE) != 0;
      fx[V.row[k]] = active ? HY_FX_VALVE : 0;
      if (active) H[V.row[k]] = V.hset[k];
    }
    if constexpr (EMIT) {                                  // one thread per emitter evaluates the law
      for (int k = tid; k < E.Ke; k += HY_T) {
        double h = 0.0, g = 1.0;
        const bool on = E.ce[k] >= 0.0;
        if (on) emitter_headloss(E.q[k], E.ce[k], E.n, &h, &g);
        E.einv[k] = on ? 1.0 / g : 0.0;
        E.ey[k] = on ? h / g : 0.0;
      }
    }
    if constexpr (PDD) {                                   // one thread per node evaluates the demand's law
      for (int n = tid; n < N; n += HY_T) {
        double h = 0.0, g = 1.0;
        const bool on = D.dd[n] > 0.0;
        if (on) demand_headloss(D.q[n], D.dd[n], D.dp, D.n, &h, &g);
        D.dinv[n] = on ? 1.0 / g : 0.0;
        D.dy[n] = on ? h / g : 0.0;
      }
    }
    __syncthreads();
    // assembly: one thread per row, over the pipes in pipe order; an ACTIVE valve's flow is a fixed draw at its two ends
    for (int n = tid; n < N; n += HY_T) {
      const int r = position[n];
      double* row = band + (size_t)r * BW;
      for (int k = 0; k < BW; ++k) row[k] = 0.0;
      if (fx[r]) {
        row[0] = 1.0;
        y[r] = H[r];
      } else {
        double diag = 0.0, f = -dem[n];
        if constexpr (PDD) {                               // a pressure-driven row has no fixed draw
          if (D.dd[n] > 0.0) f = 0.0;
        }
        for (int p = 0; p < P; ++p) {
          const int a = sa[p], b = sb[p];
          if (a != r && b != r) continue;
          if (code[p] & HY_VALVE_ACTIVE) {
            f = b == r ? f + q[p] : f - q[p];
            continue;
          }
          const int o = a == r ? b : a;
          const double pi = pinv[p], t = q[p] - yv[p];
          diag += pi;
          f = b == r ? f + t : f - t;
          if (fx[o]) f += pi * H[o];
          else if (o < r) row[r - o] -= pi;                // (r - o <= W: checked by the caller)
        }
        if constexpr (EMIT) {                              // the row's thread adds its emitter's term, after the links
          for (int k = 0; k < E.Ke; ++k) {
            if (E.row[k] != r || !(E.ce[k] >= 0.0)) continue;
            const double ei = E.einv[k];
            diag += ei;
            f -= E.q[k] - E.ey[k];
            f += E.z[k] * ei;
          }
        }
        if constexpr (PDD) {                               // then its own demand's term
          if (D.dd[n] > 0.0) {
            const double di = D.dinv[n];
            diag += di;
            f -= D.q[n] - D.dy[n];
            f += (D.elevation[n] + D.pmin) * di;
          }
        }
        row[0] = diag;
        y[r] = f;
      }
    }
    __syncthreads();
    // banded LDL^T and the substitutions, as in hy_newton
    bool bad = false;
    for (int j = 0; j < N; ++j) {
      const double d = band[(size_t)j * BW];
      if (!(d > 0.0) || !hy_finite(d)) {                   // (the same value in every thread)
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
      out.n.failed = true;
      break;
    }
    for (int k = N - 1; k >= 0; --k) {
      const double xk = y[k] / band[(size_t)k * BW];
      const int m = W < k ? W : k;
      for (int t = tid + 1; t <= m; t += HY_T) y[k - t] -= band[(size_t)k * BW + t] * xk;
      if (tid == 0) H[k] = xk;
      __syncthreads();
    }
    // the flows of every link that is not an ACTIVE valve
    for (int p = tid; p < P; p += HY_T) {
      if (code[p] & HY_VALVE_ACTIVE) continue;
      const double dq = yv[p] - (H[sa[p]] - H[sb[p]]) * pinv[p], qn = q[p] - dq;
      q[p] = qn;
      pinv[p] = fabs(dq);
      yv[p] = fabs(qn);
    }
    if constexpr (EMIT) {                                  // the emitters' flows, after the links'
      for (int k = tid; k < E.Ke; k += HY_T) {
        if (!(E.ce[k] >= 0.0)) continue;
        const double dq = E.ey[k] - (H[E.row[k]] - E.z[k]) * E.einv[k], qn = E.q[k] - dq;
        E.q[k] = qn;
        E.einv[k] = fabs(dq);
        E.ey[k] = fabs(qn);
      }
    }
    if constexpr (PDD) {                                   // the delivered flows, after the emitters'; an ACTIVE valve's controlled
      for (int n = tid; n < N; n += HY_T) {                // node has its target head here
        if (!(D.dd[n] > 0.0)) continue;
        const double dq = D.dy[n] - (H[position[n]] - (D.elevation[n] + D.pmin)) * D.dinv[n], qn = D.q[n] - dq;
        D.q[n] = qn;
        D.dinv[n] = fabs(dq);
        D.dy[n] = fabs(qn);
      }
    }
    __syncthreads();
    // one thread per valve: an ACTIVE valve's flow closes the mass balance at its controlled node over the other links in pipe
    // order; then the status from the new heads and the valve's own new flow.  No valve shares a node with another (checked by
    // the caller), so no thread reads a flow that another writes here.
    for (int k = tid; k < Kv; k += HY_T) {
      const int p = V.link[k], c = code[p];
      V.chg[k] = 0;
      if (c & HY_SHUT) continue;                           // shut by its input: a shut link, without a status
      const int st = hy_valve_status(c), cr = V.row[k];
      const bool psv = (c & HY_VALVE_PSV) != 0;
      double qv = q[p];
      if (st == HY_ST_ACTIVE) {
        double inflow = 0.0;
        for (int o = 0; o < P; ++o) {
          if (o == p) continue;
          if (sb[o] == cr) inflow += q[o];
          if (sa[o] == cr) inflow -= q[o];
        }
        double d = dem[V.node[k]];
        if constexpr (PDD) {                               // the junction's new q_d (written before the barrier above)
          if (D.dd[V.node[k]] > 0.0) d = D.q[V.node[k]];
        }
        const double qn = psv ? inflow - d : d - inflow;
        pinv[p] = fabs(qv - qn);
        yv[p] = fabs(qn);
        q[p] = qn;
        qv = qn;
      }
      const double hml = (L.minor[p] * fabs(qv)) * qv;
      const int ns = hy_valve_next(psv, st, H[sa[p]], H[sb[p]], qv, hml, V.hset[k]);
      if (ns != st) {
        V.chg[k] = 1;
        code[p] = (c & ~(HY_VALVE_ACTIVE | HY_VALVE_CLOSED)) | (ns == HY_ST_ACTIVE ? HY_VALVE_ACTIVE : 0) |
                  (ns == HY_ST_CLOSED ? HY_VALVE_CLOSED : 0);
        if (ns == HY_ST_CLOSED) {                          // (its |dq| stays the one from before)
          q[p] = 0.0;
          yv[p] = 0.0;
        }
      }
    }
    __syncthreads();
    if (tid == 0 || tid == 64) {                           // one thread per sum, in pipe order
      const double* v = tid == 0 ? pinv : yv;
      double sum = 0.0;
      for (int p = 0; p < P; ++p) sum += v[p];
      if constexpr (EMIT) {                                // then the emitters that are on, in emitter order
        const double* w = tid == 0 ? E.einv : E.ey;
        for (int k = 0; k < E.Ke; ++k)
          if (E.ce[k] >= 0.0) sum += w[k];
      }
      if constexpr (PDD) {                                 // then the pressure-driven junctions in node order (+0.0 at the others)
        const double* w = tid == 0 ? D.dinv : D.dy;
        for (int n = 0; n < N; ++n) sum += w[n];
      }
      red[tid == 0 ? 0 : 1] = sum;
    } else if (tid == 128) {
      int n = 0;
      for (int k = 0; k < Kv; ++k) n += V.chg[k];
      red[2] = (double)n;
    }
    __syncthreads();
    const double dqs = red[0], qs = red[1];
    const int changed = (int)red[2];
    out.changes += changed;
    if (!hy_finite(dqs) || !hy_finite(qs)) {
      out.n.failed = true;
      break;
    }
    out.n.rel = qs > 0.0 ? dqs / qs : (dqs > 0.0 ? __longlong_as_double(0x7FF0000000000000ll) : 0.0);
    out.n.converged = dqs <= accuracy * qs && changed == 0;
    if (out.n.converged) break;
  }
  return out;
}

// ---- what the link, valve, emitter and demand kernels share around the loop (k_hydraulic_links.hip, k_hydraulic_network.hip) --------
// A pump's speed of the scenario or step: w^2 and w^(2-n), formed once.  Bad speeds set *bad.
__device__ __forceinline__ void hy_set_speed(double* rec, double w, int* bad) {
  const double w2 = w * w, w2n = w > 0.0 ? pow(w, 2.0 - rec[2]) : 0.0;
  if (!(w >= 0.0) || !hy_finite(w) || !hy_finite(w2) || !hy_finite(w2n)) *bad = 1;
  rec[3] = w2;                                             // (a bad speed fails the scenario before the law reads the record, and
  rec[4] = w2n;                                            //  the next scenario or step rewrites all three)
  rec[5] = w;
}

// A link's control state of a series with THE CONTROLS (gatres.h): the two low bits of its state word; 0 where no control has
// touched the link in this series, and in every launch without controls.
constexpr int HY_CTL_NONE = 0, HY_CTL_OPEN = 1, HY_CTL_CLOSED = 2, HY_CTL_MASK = 3;

// A link's code of the scenario or step: HY_SHUT where the static flag, the scenario's byte or a pump speed of zero shuts it.  A
// valve's bits stay.  A control state other than HY_CTL_NONE stands in place of the static flag and the byte: HY_CTL_CLOSED shuts
// the link, HY_CTL_OPEN leaves it to its pump's speed alone.
__device__ __forceinline__ int hy_link_code(const HyLds& L, int p, const uint8_t* closed, int* bad, int ctl = HY_CTL_NONE) {
  int code = L.code[p] & ~HY_SHUT;
  const int cl = closed ? closed[p] : 0;
  if (cl > 1) *bad = 1;
  if (ctl != HY_CTL_NONE) {
    if (ctl == HY_CTL_CLOSED || ((code & HY_PUMP) && L.pump[(size_t)(code >> HY_PUMP_SHIFT) * HY_PUMP_REC + 5] == 0.0)) code |= HY_SHUT;
    return code;
  }
  if ((code & HY_CLOSED) || cl == 1 || ((code & HY_PUMP) && L.pump[(size_t)(code >> HY_PUMP_SHIFT) * HY_PUMP_REC + 5] == 0.0))
    code |= HY_SHUT;
  return code;
}

// link_state of gatres.h at the returned flow and status (a code of the links kernels never carries HY_VALVE)
__device__ __forceinline__ uint8_t hy_link_state(int code, double q) {
  if (code & HY_SHUT) return 2;
  if (code & HY_VALVE) return (uint8_t)hy_valve_status(code);
  return (code & HY_CHECK) && q < 0.0 ? 1 : 0;
}

// ---- what the links launches share (k_hydraulic_links.hip, k_hydraulic_sensitivity.hip) -----------------------------------------------
// the link arrays of a launch
struct HydLinkArgs {
  const uint8_t *link_kind, *link_flags;
  const double* minor;
  const int* pump_link;
  const double *pump_h0, *pump_r, *pump_n;
  const double* speed;
  const uint8_t* closed;
  long long speed_stride, closed_stride;
  int Kp;
  uint8_t* link_state;
};

struct HydLinksArgs {
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
  HydLinkArgs K;
};

// LDS of a workgroup, as gatres.h states it: the pipe-only arrays, and per link m and the code, per pump its record
static inline uint64_t hy_links_lds_bytes(uint64_t N, uint64_t P, uint64_t W, uint64_t Kp) {
  return 8 * (N * (W + 1) + 2 * N + 4 * P) + 4 * (2 * P + N) + 64 + 12 * P + 8 * HY_PUMP_REC * Kp;
}

// The static link arrays, checked, after hy_check_static (flag[0] keeps the verdict): fills L.minor, L.code (without HY_SHUT)
// and the constants of L.pump.  Nothing indexes with a pump index or a pump's link that was not checked here.  Ends behind a
// barrier; returns true where an array is not what gatres.h states.
__device__ __forceinline__ bool hy_check_links(const HyLds& L, const HydLinkArgs& K, const double* __restrict__ coef, int P,
                                               int* flag, int tid) {
  const int Kp = K.Kp;
  for (int p = tid; p < P; p += HY_T) {
    const int kind = K.link_kind[p], fl = K.link_flags[p];
    const double m = K.minor[p], cf = coef[p];
    bool ok = kind <= GATRES_HYD_PUMP && fl <= (GATRES_HYD_LINK_CHECK | GATRES_HYD_LINK_CLOSED) && m >= 0.0 && hy_finite(m);
    if (kind == GATRES_HYD_PIPE && !(cf >= 0.0 && hy_finite(cf) && (cf > 0.0 || m > 0.0))) ok = false;
    int code = 0;
    if (ok) {
      if (kind == GATRES_HYD_PUMP) code |= HY_PUMP | HY_CHECK;
      if (fl & GATRES_HYD_LINK_CHECK) code |= HY_CHECK;
      if (fl & GATRES_HYD_LINK_CLOSED) code |= HY_CLOSED;
    } else {
      flag[0] = 1;
    }
    L.code[p] = code;
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
  __syncthreads();
  for (int p = tid; p < P; p += HY_T) {                    // every pump link has its record
    const int code = L.code[p];
    if (code & HY_PUMP) {
      const int k = code >> HY_PUMP_SHIFT;
      bool ok = k < Kp;
      if (ok) ok = K.pump_link[k] == p;
      if (!ok) {
        L.code[p] = 0;
        flag[0] = 1;
      }
    }
  }
  __syncthreads();
  return flag[0] != 0;
}

// ---- THE SENSITIVITIES of gatres.h (k_hydraulic_sensitivity.hip) -------------------------------------------------------------------
// The law's 1 / g at the flows in L.q, into L.pinv, and into L.yv what a link's roughness moves: -h_C / g, the factor of
// dh_droughness (0 for a pump, on a 1e8 branch and on the low-flow floor); rough: the scenario's coefficients.  The caller puts
// a barrier behind it.
__device__ __forceinline__ void hy_law_gradients(const HyLds& L, const double* __restrict__ rough, int P, int tid) {
  for (int p = tid; p < P; p += HY_T) {
    const int code = L.code[p];
    const double q = L.q[p], r = L.rr[p], m = L.minor[p];
    double h, g;
    link_headloss(q, r, m, code, L.pump + (size_t)(code >> HY_PUMP_SHIFT) * HY_PUMP_REC, &h, &g);
    double gain = 0.0;
    if (!(code & (HY_SHUT | HY_PUMP)) && !((code & HY_CHECK) && q < 0.0)) {
      const double aq = fabs(q), ra = r * pow(aq, 0.852);
      if (!(1.852 * ra + 2.0 * (m * aq) < HY_LINEAR_G)) gain = ((1.852 * ra) * q) / (rough[p] * g);
    }
    L.pinv[p] = 1.0 / g;
    L.yv[p] = gain;
  }
}

// The matrix of hy_newton's assembly alone, from the 1 / g in L.pinv: one thread per row, over the pipes in pipe order, unit
// rows for the fixed nodes.  Ends behind a barrier.
__device__ __forceinline__ void hy_assemble_matrix(const HyLds& L, const int* __restrict__ position, int N, int P, int W, int tid) {
  const int BW = W + 1;
  const int *sa = L.sa, *sb = L.sb, *fx = L.fx;
  for (int n = tid; n < N; n += HY_T) {
    const int r = position[n];
    double* row = L.band + (size_t)r * BW;
    for (int k = 0; k < BW; ++k) row[k] = 0.0;
    if (fx[r]) {
      row[0] = 1.0;
    } else {
      double diag = 0.0;
      for (int p = 0; p < P; ++p) {
        const int a = sa[p], b = sb[p];
        if (a != r && b != r) continue;
        const int o = a == r ? b : a;
        const double pi = L.pinv[p];
        diag += pi;
        if (!fx[o] && o < r) row[r - o] -= pi;             // (r - o <= W: checked by the caller)
      }
      row[0] = diag;
    }
  }
  __syncthreads();
}

// hy_newton's banded LDL^T without a right-hand side: the factor stays in L.band.  Returns true on a bad pivot (the same value
// in every thread); ends behind a barrier.
__device__ __forceinline__ bool hy_factorise(const HyLds& L, int N, int W, int tid) {
  const int BW = W + 1;
  double* band = L.band;
  for (int j = 0; j < N; ++j) {
    const double d = band[(size_t)j * BW];
    if (!(d > 0.0) || !hy_finite(d)) return true;
    const int m = W < N - 1 - j ? W : N - 1 - j;
    for (int e = tid; e < m * m; e += HY_T) {
      const int r = e / m + 1, c = e - (r - 1) * m + 1;
      if (c <= r) {
        const double vr = band[(size_t)(j + r) * BW + r], vc = band[(size_t)(j + c) * BW + c];
        band[(size_t)(j + r) * BW + (r - c)] -= vr * (vc / d);
      }
    }
    __syncthreads();
  }
  return false;
}

// hy_newton's two substitutions for kc right-hand sides at once against the factor in L.band.  X is [N][stride], the right-hand
// side's index fastest; the work items of a column step are the (band offset, right-hand side) pairs, one barrier per column, and
// every right-hand side takes the operations of the loop's single vector in the same order.  On return X[r][c] holds the
// solution's row r times the pivot d_r: the caller divides (no thread writes the row that the others read).  The caller has put
// a barrier behind its writes to X; ends behind a barrier.
__device__ __forceinline__ void hy_substitute_multi(const double* band, double* X, int N, int W, int kc, int stride, int tid) {
  const int BW = W + 1;
  for (int j = 0; j < N; ++j) {
    const double d = band[(size_t)j * BW];
    const int m = W < N - 1 - j ? W : N - 1 - j;
    for (int e = tid; e < m * kc; e += HY_T) {
      const int t = e / kc, c = e - t * kc;
      const double zj = X[(size_t)j * stride + c] / d;
      X[(size_t)(j + 1 + t) * stride + c] -= band[(size_t)(j + 1 + t) * BW + (t + 1)] * zj;
    }
    __syncthreads();
  }
  for (int k = N - 1; k >= 0; --k) {
    const double d = band[(size_t)k * BW];
    const int m = W < k ? W : k;
    for (int e = tid; e < m * kc; e += HY_T) {
      const int t = e / kc + 1, c = e - (t - 1) * kc;
      const double xk = X[(size_t)k * stride + c] / d;
      X[(size_t)(k - t) * stride + c] -= band[(size_t)k * BW + t] * xk;
    }
    __syncthreads();
  }
}


// ---- the host checks every hydraulic entry point makes --------------------------------------------------------------------------------
// Does one of the written ranges overlap a read range or another written range?  (A null pointer is no range.)
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
  return S >= 1 && N >= 1 && P >= 1 && S <= INT64_MAX / 64 / ((int64_t)N + (int64_t)P);    // (every byte count of a launch fits)
}

// the link arguments both entry points share; num_pipes is known to be >= 1
static bool hy_link_args_ok(const uint8_t* link_kind, const uint8_t* link_flags, const double* minor, const int32_t* pump_link,
                            const double* pump_h0, const double* pump_r, const double* pump_n, int32_t num_pumps,
                            const double* speed, int64_t speed_stride, const uint8_t* closed, int64_t closed_stride,
                            const uint8_t* link_state, int32_t num_pipes) {
  if (!link_kind || !link_flags || !minor || !link_state) return false;
  if (num_pumps < 0 || num_pumps > num_pipes) return false;
  if (num_pumps > 0 && (!pump_link || !pump_h0 || !pump_r || !pump_n || !speed)) return false;
  if (speed_stride != 0 && speed_stride != (int64_t)num_pumps) return false;
  if (closed_stride != 0 && (closed_stride != (int64_t)num_pipes || !closed)) return false;
  return true;
}

static HydLinkArgs hy_link_args(const uint8_t* link_kind, const uint8_t* link_flags, const double* minor, const int32_t* pump_link,
                                const double* pump_h0, const double* pump_r, const double* pump_n, int32_t num_pumps,
                                const double* speed, int64_t speed_stride, const uint8_t* closed, int64_t closed_stride,
                                uint8_t* link_state) {
  HydLinkArgs k;
  k.link_kind = link_kind; k.link_flags = link_flags; k.minor = minor; k.pump_link = pump_link; k.pump_h0 = pump_h0;
  k.pump_r = pump_r; k.pump_n = pump_n; k.speed = speed; k.closed = closed; k.speed_stride = (long long)speed_stride;
  k.closed_stride = (long long)closed_stride; k.Kp = (int)num_pumps; k.link_state = link_state;
  return k;
}

}  // namespace

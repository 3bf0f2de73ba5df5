// Device side of the drift monitor of sensor readings (estimation.PressureEstimator.monitor / estimate_monitored): a sensor that
// is off by a fraction of its screening bound for a long time.  The leave-one-out residuals resid[S][K] of k_screen.hip are read
// as E series of T consecutive rows; then
//   gatres_cusum_scan     a two-sided CUSUM per (series, sensor) along time, in int64 fixed point (units of 2^-16 sigma): the
//                         state after the last row, the first alarm with its onset, and optionally both paths;
//   gatres_monitor_latch  one latching round: per series the sensor that alarmed first is taken out of the availability matrix
//                         from its onset (or its alarm) on.
// Integer addition and max are associative, so the parallel scan gives the bits of the sequential loop (monitoring.cusum_scan_ref)
// whatever the launch geometry.  No atomics.
#include "gatres_common.h"

namespace {

// ---- the CUSUM scan ----------------------------------------------------------------------------------------------------------------
constexpr int CS_T = 256;                      // one workgroup per (series, sensor); every thread owns a contiguous slice of rows
constexpr int CS_LANES = 64;
constexpr int CS_WAVES = 4;
constexpr int CS_NONE = 2147483647;            // "no alarm in this slice"
static_assert(CS_WAVES * CS_LANES == CS_T, "whole waves");

constexpr long long CS_FLOOR = -(1ll << 62);   // C of the identity map
constexpr long long CS_STATE_MAX = 1ll << 61;  // P and M of a carried state are clamped into [0, 2^61]
constexpr long long CS_ARG_MAX = 1ll << 31;    // kappa_q and h_q lie in [0, 2^31]

// The map g -> max(C, g + A).  One counted step of a side is (a, 0); a slice's steps compose to one such map.
struct CusumOp {
  long long A, C;
};
__device__ __forceinline__ CusumOp cusum_identity() { return {0ll, CS_FLOOR}; }
// x first, then y
__device__ __forceinline__ CusumOp cusum_compose(CusumOp x, CusumOp y) {
  const long long c = x.C + y.A;
  return {x.A + y.A, y.C > c ? y.C : c};
}
__device__ __forceinline__ CusumOp cusum_shfl_up(CusumOp x, int d) {
  return {__shfl_up(x.A, d, CS_LANES), __shfl_up(x.C, d, CS_LANES)};
}
__device__ __forceinline__ long long ll_max(long long a, long long b) { return a > b ? a : b; }

// Entry `idx` of the residuals: is it counted, and its q.
__device__ __forceinline__ bool cusum_entry(const float* __restrict__ resid, const uint8_t* __restrict__ available, long long idx,
                                            float mu, float inv_sigma, long long* q) {
  if (available && available[idx] == 0) return false;
  const float r = resid[idx];
  float z = __fmul_rn(__fsub_rn(r, mu), inv_sigma);
  if (r != r || z != z) return false;
  z = fminf(fmaxf(z, -32768.0f), 32768.0f);
  *q = llrintf(z * 65536.0f);                  // (the product is exact)
  return true;
}

// Local row index of the first row with global index >= tau, in [0, T].
__device__ __forceinline__ int rows_from(long long tau, long long t0, int T) {
  if (tau <= t0) return 0;
  const long long d = tau - t0;                // (tau > t0 >= 0: no overflow)
  return d > (long long)T ? T : (int)d;
}

template <bool PATHS>
__global__ __launch_bounds__(CS_T) void cusum_scan_kernel(const float* __restrict__ resid, const float* __restrict__ mu,
                                                          const float* __restrict__ inv_sigma,
                                                          const uint8_t* __restrict__ available, long long pairs, int K, int T,
                                                          long long t0, long long kappa_q, long long h_q, const long long* state_in,
                                                          long long* state_out, long long* __restrict__ records,
                                                          float* __restrict__ stat_pos, float* __restrict__ stat_neg) {
  __shared__ long long s_op[CS_WAVES][4];
  __shared__ long long s_zero[CS_WAVES][2];
  __shared__ long long s_sum[CS_WAVES][2];
  __shared__ long long s_onset;
  __shared__ int s_alarm[CS_WAVES];
  const int tid = threadIdx.x, lane = tid & (CS_LANES - 1), wave = tid / CS_LANES;
  const int per = (T + CS_T - 1) / CS_T;       // (T < 2^30: tid * per fits an int)
  const int lo = tid * per < T ? tid * per : T;
  const int hi = lo + per < T ? lo + per : T;
  for (long long pair = blockIdx.x; pair < pairs; pair += gridDim.x) {
    const long long e = pair / K;
    const int k = (int)(pair - e * K);
    const float m = mu[k], is = inv_sigma[k];
    const long long base = e * (long long)T * K + k;             // row t of the series is entry base + t * K
    long long P0 = 0, M0 = 0, zP0 = t0, zM0 = t0;
    if (state_in) {
      const long long* st = state_in + pair * 4;
      P0 = st[0] < 0 ? 0 : (st[0] > CS_STATE_MAX ? CS_STATE_MAX : st[0]);
      M0 = st[1] < 0 ? 0 : (st[1] > CS_STATE_MAX ? CS_STATE_MAX : st[1]);
      zP0 = st[2];
      zM0 = st[3];
    }
    // sweep 1: the slice as one map per side
    CusumOp fp = cusum_identity(), fm = cusum_identity();
    for (int t = lo; t < hi; ++t) {
      long long q;
      if (cusum_entry(resid, available, base + (long long)t * K, m, is, &q)) {
        fp = cusum_compose(fp, {q - kappa_q, 0ll});
        fm = cusum_compose(fm, {-q - kappa_q, 0ll});
      }
    }
    // exclusive scan of the maps over the workgroup: what came before the slice
#pragma unroll
    for (int d = 1; d < CS_LANES; d <<= 1) {
      const CusumOp op = cusum_shfl_up(fp, d), om = cusum_shfl_up(fm, d);
      if (lane >= d) {
        fp = cusum_compose(op, fp);
        fm = cusum_compose(om, fm);
      }
    }
    if (lane == CS_LANES - 1) {
      s_op[wave][0] = fp.A; s_op[wave][1] = fp.C; s_op[wave][2] = fm.A; s_op[wave][3] = fm.C;
    }
    CusumOp xp = cusum_shfl_up(fp, 1), xm = cusum_shfl_up(fm, 1);
    if (lane == 0) xp = xm = cusum_identity();
    __syncthreads();
    CusumOp wp = cusum_identity(), wm = cusum_identity();
    for (int w = 0; w < wave; ++w) {
      wp = cusum_compose(wp, {s_op[w][0], s_op[w][1]});
      wm = cusum_compose(wm, {s_op[w][2], s_op[w][3]});
    }
    xp = cusum_compose(wp, xp);
    xm = cusum_compose(wm, xm);
    long long P = ll_max(xp.C, P0 + xp.A), M = ll_max(xm.C, M0 + xm.A);
    // sweep 2: the slice with the true values
    long long lzP = -1, lzM = -1;              // the slice's last zero per side (tau + 1 >= 1), -1: none
    int at = CS_NONE, a_side = 0;              // the slice's first alarm, with the last zero of its side seen before it
    long long a_stat = 0, a_zero = -1;
    for (int t = lo; t < hi; ++t) {
      const long long idx = base + (long long)t * K;
      long long q;
      if (cusum_entry(resid, available, idx, m, is, &q)) {
        const long long tau = t0 + t;
        P = ll_max(0ll, P + (q - kappa_q));
        M = ll_max(0ll, M + (-q - kappa_q));
        if (P == 0) lzP = tau + 1;
        if (M == 0) lzM = tau + 1;
        if (at == CS_NONE && (P > h_q || M > h_q)) {
          const bool pos = P > h_q && (!(M > h_q) || P >= M);
          at = t;
          a_side = pos ? 1 : -1;
          a_stat = pos ? P : M;
          a_zero = pos ? lzP : lzM;
        }
      }
      if (PATHS) {
        stat_pos[idx] = __ll2float_rn(P) * (1.0f / 65536.0f);
        stat_neg[idx] = __ll2float_rn(M) * (1.0f / 65536.0f);
      }
    }
    // exclusive max-scan of the last zeros, min-reduce of the alarms
    long long zp = lzP, zm = lzM;
    int first = at;
#pragma unroll
    for (int d = 1; d < CS_LANES; d <<= 1) {
      const long long op = __shfl_up(zp, d, CS_LANES), om = __shfl_up(zm, d, CS_LANES);
      const int oa = __shfl_xor(first, d, CS_LANES);
      if (lane >= d) {
        zp = ll_max(zp, op);
        zm = ll_max(zm, om);
      }
      first = oa < first ? oa : first;
    }
    if (lane == CS_LANES - 1) {
      s_zero[wave][0] = zp; s_zero[wave][1] = zm;
      s_alarm[wave] = first;
    }
    long long xzp = __shfl_up(zp, 1, CS_LANES), xzm = __shfl_up(zm, 1, CS_LANES);
    if (lane == 0) xzp = xzm = -1;
    __syncthreads();
    for (int w = 0; w < wave; ++w) {
      xzp = ll_max(xzp, s_zero[w][0]);
      xzm = ll_max(xzm, s_zero[w][1]);
    }
    first = s_alarm[0];
#pragma unroll
    for (int w = 1; w < CS_WAVES; ++w) first = s_alarm[w] < first ? s_alarm[w] : first;
    long long* rec = records + pair * 6;
    if (first == CS_NONE) {
      if (tid < 6) rec[tid] = tid == 0 ? -1ll : 0ll;
    } else if (at == first) {                  // (the slices are disjoint: one thread)
      const long long before = a_side > 0 ? xzp : xzm, given = a_side > 0 ? zP0 : zM0;
      const long long onset = a_zero >= 0 ? a_zero : (before >= 0 ? before : given);
      rec[0] = t0 + first;
      rec[1] = a_side;
      rec[2] = onset;
      rec[5] = a_stat;
      s_onset = onset;
    }
    if (tid == CS_T - 1 && state_out) {        // (its slice ends at row T: P and M are the state after the last row)
      const long long endP = ll_max(xzp, lzP), endM = ll_max(xzm, lzM);
      long long* st = state_out + pair * 4;
      st[0] = P;
      st[1] = M;
      st[2] = endP >= 0 ? endP : zP0;
      st[3] = endM >= 0 ? endM : zM0;
    }
    __syncthreads();
    // sweep 3: the counted entries of the excursion that alarmed
    if (first != CS_NONE) {
      const int from = rows_from(s_onset, t0, T);
      const int a = lo > from ? lo : from, b = hi < first + 1 ? hi : first + 1;
      long long n = 0, sq = 0;
      for (int t = a; t < b; ++t) {
        long long q;
        if (cusum_entry(resid, available, base + (long long)t * K, m, is, &q)) {
          n += 1;
          sq += q;
        }
      }
#pragma unroll
      for (int d = CS_LANES / 2; d > 0; d >>= 1) {
        n += __shfl_xor(n, d, CS_LANES);
        sq += __shfl_xor(sq, d, CS_LANES);
      }
      if (lane == 0) {
        s_sum[wave][0] = n; s_sum[wave][1] = sq;
      }
      __syncthreads();
      if (tid == 0) {
        n = sq = 0;
        for (int w = 0; w < CS_WAVES; ++w) {
          n += s_sum[w][0];
          sq += s_sum[w][1];
        }
        rec[3] = n;
        rec[4] = sq;
      }
    }
    __syncthreads();                           // (the next pair writes the shared arrays again)
  }
}

// ---- one latching round ------------------------------------------------------------------------------------------------------------
constexpr int ML_T = 256;                      // one workgroup per series
constexpr int ML_LANES = 64;

// The order of the candidates: the smaller alarm index, then the larger statistic, then the smaller k.  As one unsigned key,
// larger is better: the alarm index (>= 0) complemented, the statistic with its sign bit flipped (so that unsigned order is the
// signed order), k complemented.  Three words, compared in turn: an int64 index, an int64 statistic and k do not fit in 64 bits.
// k == -1 is "no candidate" and loses against every candidate.
struct LatchKey {
  unsigned long long alarm, stat;
  int k;
};
__device__ __forceinline__ LatchKey latch_key(long long alarm, long long stat, int k) {
  return {~(unsigned long long)alarm, (unsigned long long)stat ^ 0x8000000000000000ull, k};
}
__device__ __forceinline__ bool latch_better(const LatchKey& x, const LatchKey& y) {
  if (y.k < 0 || x.k < 0) return x.k >= 0 && y.k < 0;
  if (x.alarm != y.alarm) return x.alarm > y.alarm;
  if (x.stat != y.stat) return x.stat > y.stat;
  return x.k < y.k;
}

__global__ __launch_bounds__(ML_T) void monitor_latch_kernel(const long long* __restrict__ records, uint8_t* __restrict__ available,
                                                             long long series, int K, int T, long long t0, int since,
                                                             int min_sensors, int round, int max_rounds, int* latched,
                                                             long long* __restrict__ latched_rec) {
  const int lane = threadIdx.x & (ML_LANES - 1);
  for (long long e = blockIdx.x; e < series; e += gridDim.x) {
    // (every wave of the workgroup forms the same choice: nothing to exchange)
    const int* mine = latched + e * max_rounds;
    int taken = 0;
    for (int r = 0; r < round; ++r) taken += mine[r] >= 0 ? 1 : 0;
    LatchKey best = {0ull, 0ull, -1};
    for (int k = lane; k < K; k += ML_LANES) {
      const long long* rec = records + (e * K + k) * 6;
      bool cand = rec[0] >= 0;
      for (int r = 0; r < round; ++r) cand = cand && mine[r] != k;
      if (cand) {
        const LatchKey key = latch_key(rec[0], rec[5], k);
        if (latch_better(key, best)) best = key;
      }
    }
#pragma unroll
    for (int d = ML_LANES / 2; d > 0; d >>= 1) {
      const LatchKey other = {__shfl_xor(best.alarm, d, ML_LANES), __shfl_xor(best.stat, d, ML_LANES),
                              __shfl_xor(best.k, d, ML_LANES)};
      if (latch_better(other, best)) best = other;
    }
    const int k_star = (best.k >= 0 && K - taken - 1 >= min_sensors) ? best.k : -1;
    long long rec[6] = {0, 0, 0, 0, 0, 0};
    if (k_star >= 0)
      for (int i = 0; i < 6; ++i) rec[i] = records[(e * K + k_star) * 6 + i];
    if (threadIdx.x == 0) latched[e * max_rounds + round] = k_star;
    if (threadIdx.x < 6) latched_rec[(e * max_rounds + round) * 6 + threadIdx.x] = rec[threadIdx.x];
    if (k_star >= 0) {
      const int from = rows_from(since == 0 ? rec[2] : rec[0], t0, T);
      uint8_t* col = available + e * (long long)T * K + k_star;
      for (int t = from + (int)threadIdx.x; t < T; t += ML_T) col[(long long)t * K] = 0;
    }
  }
}

}  // namespace

extern "C" int gatres_cusum_scan(const float* resid, const float* mu, const float* inv_sigma, const uint8_t* available,
                                 int64_t num_snapshots, int32_t num_observed, int64_t series_length, int64_t first_index,
                                 int64_t kappa_q, int64_t h_q, const int64_t* state_in, int64_t* state_out, int64_t* records,
                                 float* stat_pos, float* stat_neg, void* stream) {
  if (!resid || !mu || !inv_sigma || !records) return GATRES_E_BADARG;
  if (num_snapshots < 1 || num_observed < 1 || series_length < 1 || series_length >= (1ll << 30)) return GATRES_E_BADARG;
  if (num_snapshots % series_length != 0 || first_index < 0 || first_index > INT64_MAX / 4) return GATRES_E_BADARG;
  if (num_snapshots > INT64_MAX / 64 / num_observed) return GATRES_E_BADARG;           // (every byte count below fits)
  if (kappa_q < 0 || kappa_q > CS_ARG_MAX || h_q < 0 || h_q > CS_ARG_MAX) return GATRES_E_BADARG;
  if ((stat_pos == nullptr) != (stat_neg == nullptr)) return GATRES_E_BADARG;
  const uint64_t cells = (uint64_t)num_snapshots * (uint64_t)num_observed, k_bytes = 4 * (uint64_t)num_observed;
  const uint64_t pairs = (uint64_t)(num_snapshots / series_length) * (uint64_t)num_observed;
  // (what the launch writes -- state_out, records, the paths -- against what it reads and against each other)
  const void* wr[4] = {state_out, records, stat_pos, stat_neg};
  const uint64_t wn[4] = {32 * pairs, 48 * pairs, 4 * cells, 4 * cells};
  for (int i = 0; i < 4; ++i) {
    if (bytes_overlap(wr[i], wn[i], resid, 4 * cells) || bytes_overlap(wr[i], wn[i], mu, k_bytes) ||
        bytes_overlap(wr[i], wn[i], inv_sigma, k_bytes) || bytes_overlap(wr[i], wn[i], available, cells))
      return GATRES_E_BADARG;
    if (!(i == 0 && state_out == state_in) && bytes_overlap(wr[i], wn[i], state_in, 32 * pairs)) return GATRES_E_BADARG;
    for (int j = i + 1; j < 4; ++j)
      if (bytes_overlap(wr[i], wn[i], wr[j], wn[j])) return GATRES_E_BADARG;
  }
  long long wgs = (long long)pairs;
  if (wgs > 1024) wgs = 1024;
  const dim3 grid((unsigned)wgs), block(CS_T);
  if (stat_pos)
    hipLaunchKernelGGL(cusum_scan_kernel<true>, grid, block, 0, gatres_stream(stream), resid, mu, inv_sigma, available,
                       (long long)pairs, (int)num_observed, (int)series_length, (long long)first_index, (long long)kappa_q,
                       (long long)h_q, (const long long*)state_in, (long long*)state_out, (long long*)records, stat_pos, stat_neg);
  else
    hipLaunchKernelGGL(cusum_scan_kernel<false>, grid, block, 0, gatres_stream(stream), resid, mu, inv_sigma, available,
                       (long long)pairs, (int)num_observed, (int)series_length, (long long)first_index, (long long)kappa_q,
                       (long long)h_q, (const long long*)state_in, (long long*)state_out, (long long*)records, stat_pos, stat_neg);
  return gatres_launch_status();
}

extern "C" int gatres_monitor_latch(const int64_t* records, uint8_t* available, int64_t num_snapshots, int32_t num_observed,
                                    int64_t series_length, int64_t first_index, int32_t since, int32_t min_sensors, int32_t round,
                                    int32_t max_rounds, int32_t* latched, int64_t* latched_rec, void* stream) {
  if (!records || !available || !latched || !latched_rec) return GATRES_E_BADARG;
  if (num_snapshots < 1 || num_observed < 1 || series_length < 1 || series_length >= (1ll << 30)) return GATRES_E_BADARG;
  if (num_snapshots % series_length != 0 || first_index < 0 || first_index > INT64_MAX / 4) return GATRES_E_BADARG;
  if (since != 0 && since != 1) return GATRES_E_BADARG;
  if (min_sensors < 1 || max_rounds < 1 || round < 0 || round >= max_rounds) return GATRES_E_BADARG;
  if (num_snapshots > INT64_MAX / 64 / num_observed || num_snapshots > INT64_MAX / 64 / max_rounds) return GATRES_E_BADARG;
  const uint64_t series = (uint64_t)(num_snapshots / series_length);
  const uint64_t cells = (uint64_t)num_snapshots * (uint64_t)num_observed, rec_bytes = 48 * series * (uint64_t)num_observed;
  // (what the launch writes -- available, latched, latched_rec -- against what it reads and against each other)
  const void* wr[3] = {available, latched, latched_rec};
  const uint64_t wn[3] = {cells, 4 * series * (uint64_t)max_rounds, 48 * series * (uint64_t)max_rounds};
  for (int i = 0; i < 3; ++i) {
    if (bytes_overlap(wr[i], wn[i], records, rec_bytes)) return GATRES_E_BADARG;
    for (int j = i + 1; j < 3; ++j)
      if (bytes_overlap(wr[i], wn[i], wr[j], wn[j])) return GATRES_E_BADARG;
  }
  long long wgs = (long long)series;
  if (wgs > 1024) wgs = 1024;
  hipLaunchKernelGGL(monitor_latch_kernel, dim3((unsigned)wgs), dim3(ML_T), 0, gatres_stream(stream), (const long long*)records,
                     available, (long long)series, (int)num_observed, (int)series_length, (long long)first_index, (int)since,
                     (int)min_sensors, (int)round, (int)max_rounds, latched, (long long*)latched_rec);
  return gatres_launch_status();
}

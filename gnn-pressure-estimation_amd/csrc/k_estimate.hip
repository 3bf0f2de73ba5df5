// Device side of pressure estimation with a FIXED sensor set (estimation.PressureEstimator): what a deployed model does with the
// readings of its sensors, and the back-test report over a snapshot store.
//   gatres_stage_observed      one batch's input: zero and mask = 1 at every node but the observed ones, which carry their value;
//   gatres_estimate_write      one batch's result into the pass's [S][stride] matrix in physical units;
//   gatres_node_error_moments  per-node error moments of an estimate matrix against the truth, one fp64 record per node.
// gatres_stage_observed_available and gatres_node_error_moments_available are the same two kernels compiled with AVAIL = true:
// a sensor without a reading in a snapshot is one more hidden node there (x = 0, mask = 1; its error counts as a hidden entry's).
// The first two are memory-bound element passes over one batch (16-byte accesses on the batch's flat arrays, which are aligned
// whatever the graph size); the third streams two [S][N] matrices once with the lanes of a wave on consecutive nodes and sums in
// fp64 in a fixed order, without atomics: the same bits on every run.
// Measurement noise (estimate_ensemble, noise_report):
//   gatres_stage_observed_noisy   the staging kernel with NOISE = true: graph g is one (snapshot, member) pair and every present
//                                 reading gets sigma[k] * z, z drawn in the launch from (seed, member, source row, k);
//   gatres_ensemble_reduce        mean and sample standard deviation over the members of each snapshot, one element pass;
//   gatres_node_spread_moments    per-node moments of a [S][N] matrix of standard deviations: the traversal of the error moments.
// Sensor placement (layout_errors, place_sensors): one long pass over (snapshot, layout) pairs, as the ensemble's over members:
//   gatres_stage_observed_layouts the staging kernel with LAYOUTS = true: graph g is one (snapshot, layout) pair and a sensor
//                                 counts only where the pair's layout installs it;
//   gatres_layout_pair_errors     one batch's error against the truth, one fp64 record per graph, from the forward's buffers;
//   gatres_layout_error_reduce    the pairs' records folded into one record per layout, in snapshot order.
#include "gatres_common.h"

namespace {

// ---- staging -------------------------------------------------------------------------------------------------------------------
constexpr int OBS_T = 256;                     // threads of a workgroup: one 4-element chunk each
constexpr int OBS_TILE = 4 * OBS_T + 4;        // nodes a workgroup's chunks can touch: 4 * OBS_T plus the alignment shift
constexpr int OBS_MAX_GY = 256;                // workgroups that share the graphs of one tile

// (v - offset) / factor as torch forms it on fp32 tensors with Python-float scalars: the subtraction rounded to fp32, then a
// division (mode 1) or the product with the fp32 reciprocal (mode 2: `scale` is then 1.0f / (float)factor, formed on the host)
__device__ __forceinline__ float obs_normalise(float v, int mode, float offset, float scale) {
  if (mode == GATRES_NORMALISE_NONE) return v;
  const float c = __fsub_rn(v, offset);
  return mode == GATRES_NORMALISE_DIVIDE ? __fdiv_rn(c, scale) : __fmul_rn(c, scale);
}

// (by the bits: the test holds whatever the compiler may assume about floating-point comparisons)
__device__ __forceinline__ bool obs_is_nan(float v) { return (__float_as_uint(v) & 0x7fffffffu) > 0x7f800000u; }

// Workgroup (tile, y): chunk j = tile * OBS_T + thread of graph g covers the nodes [shift + 4 (j - 1), shift + 4 j) of the graph,
// shift = (-g * N) mod 4 -- so every whole chunk starts at a multiple of four in the batch's flat arrays (one float4 and one
// 32-bit mask store), whatever N is; the first and the last chunk of a graph may be partial and store element by element.  The
// inverse of observed[] over the tile's nodes is built ONCE in LDS (k + 1, 0: not observed) and serves every graph this
// workgroup takes (g = y, y + gridDim.y, ...).  Every node of every graph is written exactly once.
// AVAIL (a compile-time fact of the launch; gatres_stage_observed is the instantiation without it and reads neither argument):
// the reading of sensor k in source row r counts only where available[r * K + k] != 0 (available == NULL: everywhere) and, with
// nan_missing in the readings layout, is no NaN; a missing reading is not loaded, its node gets x = 0 and mask = 1.
// NOISE (gatres_stage_observed_noisy; always with AVAIL): graph g is pair p = first_row + g of a snapshot-major list of
// (source row, member) pairs -- source row p / members, member member0 + p % members -- and a PRESENT reading r of sensor k is
// staged as normalise(r + sigma[k] * z).  z = obs_noise(...) is a pure function of (seed, member, source row, k): the launch,
// the batch and the graph's place in it do not enter.  A missing reading draws nothing.  The draws are taken in a loop of their
// own, one trip per present sensor of the lane's chunk: the wave runs the division, the hashes and logf / sqrtf / cosf as often as
// its busiest lane holds sensors (once, as a rule), not once per element of the chunk.
struct ObsNoise {
  const float* sigma;      // [K], in the units of src
  uint64_t seed;
  long long member0;
  int members;
};
// LAYOUTS (gatres_stage_observed_layouts; always with AVAIL, never with NOISE): graph g is pair p = first_row + g of a
// snapshot-major list of (source row, layout) pairs -- source row p / count, layout p % count -- and sensor k is read only where
// on[(p % count) * K + k] != 0; a sensor the layout leaves out is staged as a missing reading.  As with NOISE the 64-bit division
// is left to the lanes that hold a sensor.
struct ObsLayouts {
  const uint8_t* on;       // [count][K]
  int count;
};

// TARGETS (gatres_stage_observed_targets; always with AVAIL, never with NOISE or LAYOUTS): graph g is pair p = first_row + g of a
// snapshot-major list of (source row, target) pairs -- source row p / count, target p % count -- staged as the launch with AVAIL
// alone stages that row, and g_out gets the pair's seed: 1.0f at the target's node (nodes[p % count]; nodes == NULL: node
// p % count), 0.0f at every other node, from the chunks that x_dst and mask are written from.  Every lane writes seeds, so the
// division is taken once per graph by everyone (it is uniform over the workgroup).
struct ObsTargets {
  const int* nodes;        // [count] or NULL
  float* g_out;            // [G * N]
  int count;
  int vec;                 // g_out is 16-byte aligned: whole chunks are one float4 store where x_dst's are
};

// (obs_noise_stream / obs_noise, the generator: gatres_common.h -- the layout staging launch of k_stage.hip draws from it too)

template <bool AVAIL, bool NOISE, bool LAYOUTS, bool TARGETS>
__global__ __launch_bounds__(OBS_T) void stage_observed_kernel(const float* __restrict__ src, int readings, long long src_rows,
                                                               const long long* __restrict__ rows, long long first_row, int N,
                                                               int G, const int* __restrict__ observed, int K, int mode,
                                                               float offset, float scale, float* __restrict__ x_dst,
                                                               uint8_t* __restrict__ mask, int vec,
                                                               const uint8_t* __restrict__ available, int nan_missing,
                                                               ObsNoise nz, ObsLayouts lay, ObsTargets tg) {
  static_assert(AVAIL || !(NOISE || LAYOUTS || TARGETS), "the noisy, the layouts and the targets launch carry the availability arguments");
  static_assert(!(NOISE && LAYOUTS), "noise combined with layouts is not built");
  static_assert(!(TARGETS && (NOISE || LAYOUTS)), "targets combined with noise or layouts are not built");
  __shared__ int slot[OBS_TILE];
  const int tid = threadIdx.x;
  const int j = blockIdx.x * OBS_T + tid;
  const int tile_lo = blockIdx.x * (4 * OBS_T) - 4;          // first node slot[] speaks of
  for (int i = tid; i < OBS_TILE; i += OBS_T) slot[i] = 0;
  __syncthreads();
  for (int k = tid; k < K; k += OBS_T) {
    const int v = observed[k];
    if (v >= 0 && v < N && v >= tile_lo && v < tile_lo + OBS_TILE) slot[v - tile_lo] = k + 1;
  }
  __syncthreads();
  for (int g = blockIdx.y; g < G; g += gridDim.y) {
    const long long base = (long long)g * N;
    const int shift = vec ? (int)((4 - (base & 3)) & 3) : 0;
    const int v0 = shift + 4 * (j - 1);
    if (v0 >= N || v0 + 4 <= 0) continue;
    // (NOISE: the pair's row lies inside the matrix, the host checked the pair range; the 64-bit division is left to the lanes
    //  that hold a sensor)
    long long row = (NOISE || LAYOUTS || TARGETS) ? 0 : (rows ? rows[g] : first_row + g);
    const bool row_ok = NOISE || LAYOUTS || TARGETS || (row >= 0 && row < src_rows);   // (a row outside the matrix is not read: its nodes get 0)
    int target = -1;                                                    // TARGETS: the node of the pair's seed
    if (TARGETS) {
      const long long pair = first_row + g;
      row = pair / tg.count;
      const int t = (int)(pair - row * tg.count);
      target = tg.nodes ? tg.nodes[t] : t;
    }
    uint64_t noise_stream = 0;
    unsigned draw = 0;                                                  // NOISE: the elements that hold a present reading
    const uint8_t* installed = nullptr;                                 // LAYOUTS: the pair's row of lay.on
    if (NOISE || LAYOUTS) {
      bool any = false;
#pragma unroll
      for (int e = 0; e < 4; ++e) any |= v0 + e >= 0 && v0 + e < N && slot[v0 + e - tile_lo] != 0;
      if (any) {
        const long long pair = first_row + g;
        row = pair / (NOISE ? nz.members : lay.count);
        if (NOISE) noise_stream = obs_noise_stream(nz.seed, (uint64_t)(nz.member0 + (pair - row * nz.members)));
        else installed = lay.on + (pair - row * lay.count) * K;
      }
    }
    float val[4];
    uint8_t mk[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int v = v0 + e;
      const int s = (v >= 0 && v < N) ? slot[v - tile_lo] : 0;
      mk[e] = s ? 0 : 1;
      val[e] = 0.f;
      if (s && row_ok) {
        bool have = true;
        if (LAYOUTS) have = installed[s - 1] != 0;
        if (AVAIL && have && available) have = available[row * K + (s - 1)] != 0;
        if (have) {
          const float r = readings ? src[row * K + (s - 1)] : src[row * N + v];
          if (AVAIL && nan_missing && readings && obs_is_nan(r)) have = false;
          else if (NOISE) {
            val[e] = r;                                                 // (raw: the loop below adds the noise and normalises)
            draw |= 1u << e;
          } else val[e] = obs_normalise(r, readings ? mode : GATRES_NORMALISE_NONE, offset, scale);
        }
        if (AVAIL && !have) mk[e] = 1;
      }
    }
    if (NOISE) {
      while (draw) {
        const int e = __ffs(draw) - 1;
        draw &= draw - 1;
        const int k = slot[v0 + e - tile_lo] - 1;
        float r = e == 0 ? val[0] : e == 1 ? val[1] : e == 2 ? val[2] : val[3];
        r = __fadd_rn(r, __fmul_rn(nz.sigma[k], obs_noise(noise_stream, row, K, k)));
        r = obs_normalise(r, readings ? mode : GATRES_NORMALISE_NONE, offset, scale);
#pragma unroll
        for (int f = 0; f < 4; ++f)
          if (f == e) val[f] = r;
      }
    }
    if (vec && v0 >= 0 && v0 + 4 <= N) {
      st4(x_dst + base + v0, make_float4(val[0], val[1], val[2], val[3]));
      *reinterpret_cast<uint32_t*>(mask + base + v0) =
          (uint32_t)mk[0] | ((uint32_t)mk[1] << 8) | ((uint32_t)mk[2] << 16) | ((uint32_t)mk[3] << 24);
      if (TARGETS) {
        if (tg.vec) {
          st4(tg.g_out + base + v0, make_float4(v0 == target ? 1.f : 0.f, v0 + 1 == target ? 1.f : 0.f,
                                                v0 + 2 == target ? 1.f : 0.f, v0 + 3 == target ? 1.f : 0.f));
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) tg.g_out[base + v0 + e] = v0 + e == target ? 1.f : 0.f;
        }
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int v = v0 + e;
        if (v >= 0 && v < N) {
          x_dst[base + v] = val[e];
          mask[base + v] = mk[e];
          if (TARGETS) tg.g_out[base + v] = v == target ? 1.f : 0.f;
        }
      }
    }
  }
}

// ---- write-back ----------------------------------------------------------------------------------------------------------------
constexpr int EW_T = 256;

// One 4-element chunk of the batch's flat arrays per thread per trip (16-byte loads of out and x, one 32-bit load of the mask).
// The destination rows are dst_stride apart: a chunk is stored as one float4 when `vec_store` says that every chunk lies inside
// one row at a 16-byte boundary (N and dst_stride multiples of four, dst aligned), element by element otherwise.
__global__ __launch_bounds__(EW_T) void estimate_write_kernel(const float* __restrict__ out, const float* __restrict__ x,
                                                              const uint8_t* __restrict__ mask, int N, long long total,
                                                              float scale, float offset, int keep_observed,
                                                              float* __restrict__ dst, long long dst_stride, long long first_row,
                                                              int vec_load, int vec_store) {
  for (long long i0 = 4 * ((long long)blockIdx.x * EW_T + threadIdx.x); i0 < total; i0 += 4LL * gridDim.x * EW_T) {
    float o[4], xv[4] = {0.f, 0.f, 0.f, 0.f};
    uint8_t mk[4] = {1, 1, 1, 1};
    const int n = total - i0 < 4 ? (int)(total - i0) : 4;
    if (vec_load && n == 4) {
      const float4 a = ld4(out + i0);
      o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
      if (keep_observed) {
        const float4 b = ld4(x + i0);
        const uint32_t m = *reinterpret_cast<const uint32_t*>(mask + i0);
        xv[0] = b.x; xv[1] = b.y; xv[2] = b.z; xv[3] = b.w;
        mk[0] = m & 0xff; mk[1] = (m >> 8) & 0xff; mk[2] = (m >> 16) & 0xff; mk[3] = m >> 24;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o[e] = e < n ? out[i0 + e] : 0.f;
        if (keep_observed && e < n) {
          xv[e] = x[i0 + e];
          mk[e] = mask[i0 + e];
        }
      }
    }
    float r[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = gatres_descale(mk[e] ? o[e] : xv[e], scale, offset);
    const long long g = i0 / N;
    const int v = (int)(i0 - g * N);
    if (vec_store && n == 4) {
      st4(dst + (first_row + g) * dst_stride + v, make_float4(r[0], r[1], r[2], r[3]));
    } else {
      long long ge = g;
      int ve = v;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (e < n) dst[(first_row + ge) * dst_stride + ve] = r[e];
        if (++ve == N) { ve = 0; ++ge; }
      }
    }
  }
}

// ---- per-node error moments ----------------------------------------------------------------------------------------------------
constexpr int NE_WAVES = 8;
constexpr int NE_T = NE_WAVES * GATRES_WAVE;
constexpr int NE_U = 8;                        // rows in flight per wave and trip
constexpr int NE_F = 6;                        // accumulated fields: the record's slots [1..6] (AVAIL: and the hidden count)

// The end of both moments kernels: the waves' partial records go through LDS and wave 0 combines them in wave order, field
// MAXF by fmax and every other field by addition.  True in the lanes of wave 0, which then hold the combined record in r[].
template <int NF, int MAXF>
__device__ __forceinline__ bool ne_combine(double (*part)[NF][GATRES_WAVE], const double (&a)[NF], int lane, int wave,
                                           double (&r)[NF]) {
#pragma unroll
  for (int f = 0; f < NF; ++f) part[wave][f][lane] = a[f];
  __syncthreads();
  if (wave != 0) return false;
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    double s = part[0][f][lane];
    for (int w = 1; w < NE_WAVES; ++w) s = f == MAXF ? fmax(s, part[w][f][lane]) : s + part[w][f][lane];
    r[f] = s;
  }
  return true;
}

// Workgroup b takes the 64 nodes [64 b, 64 b + 64): lane l of every wave is node 64 b + l, so a wave reads 256 consecutive bytes
// of a row.  Wave w takes the rows w, w + NE_WAVES, ... in ascending order (NE_U of them in flight per trip: a chunk of
// GATRES_NODE_ERROR_CHUNK = NE_WAVES * NE_U rows per workgroup), each lane adding its node's terms in that order; the waves'
// partials go through LDS and are added in wave order.  The association depends on S alone.
// AVAIL: seen[] holds k + 1 for the sensor observed[k]; a sensor lane reads available[s * K + k] with its rows and skips the
// entries it was observed in (they add nothing, so a lane that skips none forms the sums of the kernel without AVAIL, bit for
// bit); the hidden entries are counted as a seventh field.  Record: [0] hidden entries, [1..6] over them, [7] S - [0].
template <bool AVAIL>
__global__ __launch_bounds__(NE_T) void node_error_moments_kernel(const float* __restrict__ est, const float* __restrict__ truth,
                                                                  long long S, int N, float scale, float offset,
                                                                  const int* __restrict__ observed, int K,
                                                                  double* __restrict__ table,
                                                                  const uint8_t* __restrict__ available) {
  constexpr int NF = AVAIL ? NE_F + 1 : NE_F;
  __shared__ double part[NE_WAVES][NF][GATRES_WAVE];
  __shared__ int seen[GATRES_WAVE];
  const int lane = threadIdx.x % GATRES_WAVE, wave = threadIdx.x / GATRES_WAVE;
  const int v_lo = blockIdx.x * GATRES_WAVE, v = v_lo + lane;
  if (threadIdx.x < GATRES_WAVE) seen[threadIdx.x] = 0;
  __syncthreads();
  for (int k = threadIdx.x; k < K; k += NE_T) {
    const int o = observed[k];
    if (o >= v_lo && o < v_lo + GATRES_WAVE) seen[o - v_lo] = AVAIL ? k + 1 : 1;
  }
  if (AVAIL) __syncthreads();
  const int sensor = AVAIL ? seen[lane] - 1 : -1;          // (AVAIL: this lane's column of available[], -1: not a sensor)
  double a[NF] = {};                                        // sum e, sum |e|, sum e^2, max |e|, #kept, sum |e| / |t| (, #hidden)
  float amax = 0.f;
  if (v < N) {
    for (long long s0 = wave; s0 < S; s0 += (long long)NE_U * NE_WAVES) {
      float p[NE_U], t[NE_U];
      uint8_t av[NE_U] = {};
#pragma unroll
      for (int u = 0; u < NE_U; ++u) {
        const long long s = s0 + (long long)u * NE_WAVES;
        p[u] = s < S ? est[s * N + v] : 0.f;
        t[u] = s < S ? truth[s * N + v] : 0.f;
      }
      // (one region for the sensor lanes, so that the trip's NE_U bytes are in flight together with its rows; a row past the
      //  end reads the last row's byte, which the loop below skips)
      if (AVAIL && sensor >= 0) {
#pragma unroll
        for (int u = 0; u < NE_U; ++u) {
          const long long s = s0 + (long long)u * NE_WAVES;
          av[u] = available[(s < S ? s : S - 1) * K + sensor];
        }
      }
#pragma unroll
      for (int u = 0; u < NE_U; ++u) {           // (in row order: the same association as a plain loop)
        if (s0 + (long long)u * NE_WAVES >= S) continue;
        if (AVAIL) {
          if (av[u]) continue;
          a[NF - 1] += 1.0;
        }
        const float tr = gatres_descale(t[u], scale, offset);
        const float e = __fsub_rn(p[u], tr);
        const float ae = fabsf(e), at = fabsf(tr);
        a[0] += (double)e;
        a[1] += (double)ae;
        a[2] += (double)e * (double)e;
        amax = fmaxf(amax, ae);
        if (at > 0.01f) {
          a[4] += 1.0;
          a[5] += (double)ae / (double)at;
        }
      }
    }
  }
  a[3] = (double)amax;
  double r[NF];
  if (ne_combine<NF, 3>(part, a, lane, wave, r) && v < N) {
    double* rec = table + (size_t)v * (AVAIL ? GATRES_NODE_ERROR_AVAIL_RECORD : GATRES_NODE_ERROR_RECORD);
    rec[0] = AVAIL ? r[NF - 1] : (double)S;
    rec[1] = r[0]; rec[2] = r[1]; rec[3] = r[2]; rec[4] = r[3]; rec[5] = r[4]; rec[6] = r[5];
    rec[7] = AVAIL ? (double)S - r[NF - 1] : (seen[lane] ? 1.0 : 0.0);
  }
}

// ---- per-node spread moments ---------------------------------------------------------------------------------------------------
// The traversal of node_error_moments_kernel over ONE matrix: workgroup b takes the nodes [64 b, 64 b + 64), wave w the rows
// w, w + NE_WAVES, ... in ascending order with NE_U of them in flight, each lane adding its node's terms in that order, the
// waves' partials combined in wave order.  Record: [0] S, [1] sum (double)sd * (double)sd, [2] max sd, [3] sum sd.
__global__ __launch_bounds__(NE_T) void node_spread_moments_kernel(const float* __restrict__ sd, long long S, int N,
                                                                   double* __restrict__ table) {
  constexpr int NF = 3;                                     // sum sd^2, max sd, sum sd
  __shared__ double part[NE_WAVES][NF][GATRES_WAVE];
  const int lane = threadIdx.x % GATRES_WAVE, wave = threadIdx.x / GATRES_WAVE;
  const int v = blockIdx.x * GATRES_WAVE + lane;
  double a[NF] = {};
  float smax = 0.f;
  if (v < N) {
    for (long long s0 = wave; s0 < S; s0 += (long long)NE_U * NE_WAVES) {
      float p[NE_U];
#pragma unroll
      for (int u = 0; u < NE_U; ++u) {
        const long long s = s0 + (long long)u * NE_WAVES;
        p[u] = s < S ? sd[s * N + v] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < NE_U; ++u) {           // (in row order: the same association as a plain loop)
        if (s0 + (long long)u * NE_WAVES >= S) continue;
        a[0] += (double)p[u] * (double)p[u];
        smax = fmaxf(smax, p[u]);
        a[2] += (double)p[u];
      }
    }
  }
  a[1] = (double)smax;
  double r[NF];
  if (ne_combine<NF, 1>(part, a, lane, wave, r) && v < N) {
    double* rec = table + (size_t)v * GATRES_NODE_SPREAD_RECORD;
    rec[0] = (double)S; rec[1] = r[0]; rec[2] = r[1]; rec[3] = r[2];
  }
}

// ---- ensemble reduce -----------------------------------------------------------------------------------------------------------
constexpr int ER_T = 256;

// One chunk of W consecutive nodes of one snapshot per thread and trip (W = 4: 16-byte accesses, when the host found N, both
// strides and the three pointers fit; W = 1 otherwise); the chunks of all snapshots are numbered row by row, so the lanes of a
// wave read consecutive bytes of a member's row whatever N is, and the grid is capped and strides over them.  Two passes over the snapshot's M member rows in member order, both in fp64: the sum for the mean, then the sum of the
// squared deviations from the fp64 mean (the second pass finds the rows in L2; M rows of registers would bound M).  No
// contraction (the library is compiled with -ffp-contract=off), no atomics.
template <int W>
__global__ __launch_bounds__(ER_T) void ensemble_reduce_kernel(const float* __restrict__ mem, long long C, int M, int N,
                                                               long long stride, float* __restrict__ mean,
                                                               float* __restrict__ sd, long long out_stride,
                                                               long long first_row) {
  const int per_row = (N + W - 1) / W;
  for (long long i = (long long)blockIdx.x * ER_T + threadIdx.x; i < C * per_row; i += (long long)gridDim.x * ER_T) {
    const long long s = i / per_row;
    const int v0 = W * (int)(i - s * per_row);
    const float* row0 = mem + s * M * stride + v0;
    double sum[W], m64[W], sq[W];
#pragma unroll
    for (int e = 0; e < W; ++e) sum[e] = sq[e] = 0.0;
    for (int m = 0; m < M; ++m) {
      float x[W];
      if constexpr (W == 4) { const float4 t = ld4(row0 + m * stride); x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w; }
      else x[0] = row0[m * stride];
#pragma unroll
      for (int e = 0; e < W; ++e) sum[e] += (double)x[e];
    }
#pragma unroll
    for (int e = 0; e < W; ++e) m64[e] = sum[e] / (double)M;
    for (int m = 0; m < M; ++m) {
      float x[W];
      if constexpr (W == 4) { const float4 t = ld4(row0 + m * stride); x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w; }
      else x[0] = row0[m * stride];
#pragma unroll
      for (int e = 0; e < W; ++e) {
        const double d = (double)x[e] - m64[e];
        sq[e] += d * d;
      }
    }
    float om[W], os[W];
#pragma unroll
    for (int e = 0; e < W; ++e) {
      om[e] = (float)m64[e];
      os[e] = M > 1 ? (float)sqrt(sq[e] / (double)(M - 1)) : 0.f;
    }
    const long long o = (first_row + s) * out_stride + v0;
    if constexpr (W == 4) {
      st4(mean + o, make_float4(om[0], om[1], om[2], om[3]));
      st4(sd + o, make_float4(os[0], os[1], os[2], os[3]));
    } else {
      mean[o] = om[0];
      sd[o] = os[0];
    }
  }
}

// ---- layout errors -------------------------------------------------------------------------------------------------------------
constexpr int PE_WAVES = 4;                    // graphs per workgroup: one wave each
constexpr int PE_T = PE_WAVES * GATRES_WAVE;

// The sum of a over the lanes of a wave by a butterfly (xor 32, 16, ... 1): every lane ends with the same bits, and the
// association is fixed.
__device__ __forceinline__ double pe_wave_sum(double a) {
#pragma unroll
  for (int off = GATRES_WAVE / 2; off > 0; off >>= 1) a += __shfl_xor(a, off, GATRES_WAVE);
  return a;
}

// Wave w of workgroup b takes graph g = b * PE_WAVES + w: pair p = first_pair + g, truth row s = p / L.  Lane l takes the chunks
// l, l + 64, ... of four consecutive nodes [4 j, 4 j + 4) of the graph, in ascending order, and adds the terms of a chunk's
// counted nodes in node order; the lanes' partials go through the butterfly above.  The association depends on N alone: not on
// g, on the alignment or on which loads were taken.  A whole chunk is one 16-byte load of out, one 32-bit load of mask and of
// score and one 16-byte load of truth where g * N, resp. s * N, is a multiple of four and the pointer is aligned (out_vec,
// mask_vec, score_vec, truth_vec: facts of the pointers, the rest is uniform over the wave); element loads otherwise.
__global__ __launch_bounds__(PE_T) void layout_pair_errors_kernel(const float* __restrict__ out, const uint8_t* __restrict__ mask,
                                                                  const float* __restrict__ truth, int N, int G,
                                                                  long long first_pair, int L, float scale, float offset,
                                                                  const uint8_t* __restrict__ score, double* __restrict__ rec,
                                                                  int out_vec, int mask_vec, int truth_vec, int score_vec) {
  const int lane = threadIdx.x % GATRES_WAVE, wave = threadIdx.x / GATRES_WAVE;
  const int g = blockIdx.x * PE_WAVES + wave;
  if (g >= G) return;                                       // (no barrier below: a wave works alone)
  const long long s = (first_pair + g) / L;
  const long long base = (long long)g * N, tbase = s * N;
  const bool ov = out_vec && (base & 3) == 0, mv = mask_vec && (base & 3) == 0, tv = truth_vec && (tbase & 3) == 0;
  double sum_abs = 0.0, sum_sq = 0.0;
  float amax = 0.f;
  int count = 0;
  for (int v0 = 4 * lane; v0 < N; v0 += 4 * GATRES_WAVE) {
    const bool whole = v0 + 4 <= N;
    float o[4], t[4];
    uint8_t mk[4], sc[4] = {1, 1, 1, 1};
    if (whole && ov) {
      const float4 a = ld4(out + base + v0);
      o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = v0 + e < N ? out[base + v0 + e] : 0.f;
    }
    if (whole && tv) {
      const float4 a = ld4(truth + tbase + v0);
      t[0] = a.x; t[1] = a.y; t[2] = a.z; t[3] = a.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) t[e] = v0 + e < N ? truth[tbase + v0 + e] : 0.f;
    }
    if (whole && mv) {
      const uint32_t m = *reinterpret_cast<const uint32_t*>(mask + base + v0);
      mk[0] = m & 0xff; mk[1] = (m >> 8) & 0xff; mk[2] = (m >> 16) & 0xff; mk[3] = m >> 24;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) mk[e] = v0 + e < N ? mask[base + v0 + e] : 0;
    }
    if (score) {
      if (whole && score_vec) {
        const uint32_t m = *reinterpret_cast<const uint32_t*>(score + v0);
        sc[0] = m & 0xff; sc[1] = (m >> 8) & 0xff; sc[2] = (m >> 16) & 0xff; sc[3] = m >> 24;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) sc[e] = v0 + e < N ? score[v0 + e] : 0;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {                           // (in node order; a node past N has mk = 0)
      if (!mk[e] || !sc[e]) continue;
      const float err = __fsub_rn(gatres_descale(o[e], scale, offset), gatres_descale(t[e], scale, offset));
      const float ae = fabsf(err);
      ++count;
      sum_abs += (double)ae;
      sum_sq += (double)err * (double)err;
      amax = fmaxf(amax, ae);
    }
  }
  const double r_abs = pe_wave_sum(sum_abs), r_sq = pe_wave_sum(sum_sq);
#pragma unroll
  for (int off = GATRES_WAVE / 2; off > 0; off >>= 1) {
    count += __shfl_xor(count, off, GATRES_WAVE);
    amax = fmaxf(amax, __shfl_xor(amax, off, GATRES_WAVE));
  }
  if (lane == 0) {
    double* r = rec + (size_t)g * GATRES_LAYOUT_PAIR_RECORD;
    r[0] = (double)count; r[1] = r_abs; r[2] = r_sq; r[3] = (double)amax;
  }
}

// ---- layout error reduce -------------------------------------------------------------------------------------------------------
constexpr int LR_T = 64;

// Lane l is layout l: it folds the records rec[s * L + l], s = 0 .. S - 1, strictly in that order (so the table's bits do not
// depend on how a pass was cut into launches), starting from the table's record when `accumulate`.  The lanes of a wave read
// consecutive records; LR_U of a lane's records are in flight per trip.
constexpr int LR_U = 8;
__global__ __launch_bounds__(LR_T) void layout_error_reduce_kernel(const double* __restrict__ rec, long long S, int L,
                                                                   double* __restrict__ table, int accumulate) {
  const int l = blockIdx.x * LR_T + threadIdx.x;
  if (l >= L) return;
  double* t = table + (size_t)l * GATRES_LAYOUT_ERROR_RECORD;
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  if (accumulate) {
#pragma unroll
    for (int f = 0; f < 4; ++f) a[f] = t[f];
  }
  for (long long s0 = 0; s0 < S; s0 += LR_U) {
    double r[LR_U][4];
#pragma unroll
    for (int u = 0; u < LR_U; ++u) {
      const long long s = s0 + u < S ? s0 + u : S - 1;      // (a row past the end reads the last one, which the loop below skips)
      const double* p = rec + ((size_t)s * L + l) * GATRES_LAYOUT_PAIR_RECORD;
#pragma unroll
      for (int f = 0; f < 4; ++f) r[u][f] = p[f];
    }
#pragma unroll
    for (int u = 0; u < LR_U; ++u) {                        // (in snapshot order: the same association as a plain loop)
      if (s0 + u >= S) continue;
      a[0] += r[u][0]; a[1] += r[u][1]; a[2] += r[u][2];
      a[3] = fmax(a[3], r[u][3]);
    }
  }
#pragma unroll
  for (int f = 0; f < 4; ++f) t[f] = a[f];
}

// The checks and the launch of the staging entry points (AVAIL: with the availability arguments; NOISE / LAYOUTS / TARGETS:
// first_row is the first pair, rows is NULL and nz / lay / tg holds the noise / layout / target arguments).
template <bool AVAIL, bool NOISE = false, bool LAYOUTS = false, bool TARGETS = false>
int stage_observed(const float* src, int32_t layout, int64_t src_rows, const int64_t* rows, int64_t first_row,
                   int32_t nodes_per_graph, int32_t num_graphs, const int32_t* observed, int32_t num_observed, int32_t normalise,
                   double offset, double factor, float* x_dst, uint8_t* mask, const uint8_t* available, int32_t nan_is_missing,
                   void* stream, ObsNoise nz = ObsNoise{nullptr, 0, 0, 1}, ObsLayouts lay = ObsLayouts{nullptr, 1},
                   ObsTargets tg = ObsTargets{nullptr, nullptr, 1, 0}) {
  if (!src || !observed || !x_dst || !mask || src == x_dst) return GATRES_E_BADARG;
  if (nodes_per_graph <= 0 || num_graphs <= 0 || num_observed <= 0 || num_observed > nodes_per_graph) return GATRES_E_BADARG;
  if ((int64_t)nodes_per_graph * num_graphs > INT32_MAX) return GATRES_E_BADARG;
  if (layout != GATRES_OBSERVED_FULL_ROWS && layout != GATRES_OBSERVED_READINGS) return GATRES_E_BADARG;
  if (layout == GATRES_OBSERVED_READINGS && rows) return GATRES_E_BADARG;
  if (NOISE) {
    // (pairs [first_row, first_row + num_graphs) of the src_rows * members there are)
    if (!nz.sigma || nz.members < 1 || nz.member0 < 0 || src_rows <= 0 || src_rows > INT64_MAX / nz.members) return GATRES_E_BADARG;
    if (first_row < 0 || first_row > src_rows * nz.members - num_graphs) return GATRES_E_BADARG;
    const uint64_t total = (uint64_t)nodes_per_graph * (uint64_t)num_graphs;
    if (bytes_overlap(nz.sigma, 4 * (uint64_t)num_observed, x_dst, 4 * total) ||
        bytes_overlap(nz.sigma, 4 * (uint64_t)num_observed, mask, total)) return GATRES_E_BADARG;
  } else if (LAYOUTS) {
    // (pairs [first_row, first_row + num_graphs) of the src_rows * count there are)
    if (!lay.on || lay.count < 1 || src_rows <= 0 || src_rows > INT64_MAX / lay.count) return GATRES_E_BADARG;
    if (first_row < 0 || first_row > src_rows * lay.count - num_graphs) return GATRES_E_BADARG;
    const uint64_t total = (uint64_t)nodes_per_graph * (uint64_t)num_graphs;
    const uint64_t lay_bytes = (uint64_t)lay.count * (uint64_t)num_observed;
    if (bytes_overlap(lay.on, lay_bytes, x_dst, 4 * total) || bytes_overlap(lay.on, lay_bytes, mask, total)) return GATRES_E_BADARG;
  } else if (TARGETS) {
    // (pairs [first_row, first_row + num_graphs) of the src_rows * count there are; without nodes[] target t is node t)
    if (!tg.g_out || tg.count < 1 || src_rows <= 0 || src_rows > INT64_MAX / tg.count) return GATRES_E_BADARG;
    if (!tg.nodes && tg.count > nodes_per_graph) return GATRES_E_BADARG;
    if (first_row < 0 || first_row > src_rows * tg.count - num_graphs) return GATRES_E_BADARG;
    const uint64_t total = (uint64_t)nodes_per_graph * (uint64_t)num_graphs;
    const uint64_t width = layout == GATRES_OBSERVED_READINGS ? (uint64_t)num_observed : (uint64_t)nodes_per_graph;
    const uint64_t src_bytes = (uint64_t)src_rows > (uint64_t)INT64_MAX / 4 / width ? (uint64_t)INT64_MAX : 4 * (uint64_t)src_rows * width;
    if (bytes_overlap(tg.g_out, 4 * total, x_dst, 4 * total) || bytes_overlap(tg.g_out, 4 * total, mask, total) ||
        bytes_overlap(tg.g_out, 4 * total, src, src_bytes) ||
        (tg.nodes && (bytes_overlap(tg.g_out, 4 * total, tg.nodes, 4 * (uint64_t)tg.count) ||
                      bytes_overlap(tg.nodes, 4 * (uint64_t)tg.count, x_dst, 4 * total) ||
                      bytes_overlap(tg.nodes, 4 * (uint64_t)tg.count, mask, total)))) return GATRES_E_BADARG;
  } else if (src_rows <= 0 || (!rows && (first_row < 0 || first_row > src_rows - num_graphs))) return GATRES_E_BADARG;
  if (normalise < GATRES_NORMALISE_NONE || normalise > GATRES_NORMALISE_RECIPROCAL) return GATRES_E_BADARG;
  if (AVAIL) {
    if (!NOISE && !LAYOUTS && !TARGETS && !available && !nan_is_missing) return GATRES_E_BADARG;
    // (available[src_rows][num_observed] must not overlap the bytes this launch writes)
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(available), a1 = a0 + (uintptr_t)src_rows * (uintptr_t)num_observed;
    const uintptr_t total = (uintptr_t)nodes_per_graph * (uintptr_t)num_graphs;
    const uintptr_t x0 = reinterpret_cast<uintptr_t>(x_dst), m0 = reinterpret_cast<uintptr_t>(mask);
    if (available && ((a0 < x0 + 4 * total && x0 < a1) || (a0 < m0 + total && m0 < a1))) return GATRES_E_BADARG;
  }
  float scale = 1.f;
  if (normalise != GATRES_NORMALISE_NONE) {
    if (!((float)factor != 0.f)) return GATRES_E_BADARG;
    scale = normalise == GATRES_NORMALISE_RECIPROCAL ? 1.0f / (float)factor : (float)factor;
  }
  const int vec = gatres_aligned16(x_dst) && (reinterpret_cast<uintptr_t>(mask) & 3u) == 0;
  const int chunks = (nodes_per_graph + 3) / 4 + 1;
  const dim3 grid((chunks + OBS_T - 1) / OBS_T, num_graphs < OBS_MAX_GY ? num_graphs : OBS_MAX_GY);
  tg.vec = vec && gatres_aligned16(tg.g_out);
  hipLaunchKernelGGL((stage_observed_kernel<AVAIL, NOISE, LAYOUTS, TARGETS>), grid, dim3(OBS_T), 0, gatres_stream(stream), src,
                     (int)(layout == GATRES_OBSERVED_READINGS), (long long)src_rows, reinterpret_cast<const long long*>(rows),
                     (long long)first_row, (int)nodes_per_graph, (int)num_graphs, observed, (int)num_observed, (int)normalise,
                     (float)offset, scale, x_dst, mask, vec, available, (int)(nan_is_missing != 0), nz, lay, tg);
  return gatres_launch_status();
}

}  // namespace

extern "C" int gatres_stage_observed(const float* src, int32_t layout, int64_t src_rows, const int64_t* rows, int64_t first_row,
                                     int32_t nodes_per_graph, int32_t num_graphs, const int32_t* observed, int32_t num_observed,
                                     int32_t normalise, double offset, double factor, float* x_dst, uint8_t* mask,
                                     void* stream) {
  return stage_observed<false>(src, layout, src_rows, rows, first_row, nodes_per_graph, num_graphs, observed, num_observed,
                               normalise, offset, factor, x_dst, mask, nullptr, 0, stream);
}

extern "C" int gatres_stage_observed_available(const float* src, int32_t layout, int64_t src_rows, const int64_t* rows,
                                               int64_t first_row, int32_t nodes_per_graph, int32_t num_graphs,
                                               const int32_t* observed, int32_t num_observed, int32_t normalise, double offset,
                                               double factor, float* x_dst, uint8_t* mask, const uint8_t* available,
                                               int32_t nan_is_missing, void* stream) {
  return stage_observed<true>(src, layout, src_rows, rows, first_row, nodes_per_graph, num_graphs, observed, num_observed,
                              normalise, offset, factor, x_dst, mask, available, nan_is_missing, stream);
}

extern "C" int gatres_stage_observed_noisy(const float* src, int32_t layout, int64_t src_rows, int64_t first_pair, int32_t members,
                                           int64_t member0, int32_t nodes_per_graph, int32_t num_graphs, const int32_t* observed,
                                           int32_t num_observed, int32_t normalise, double offset, double factor, float* x_dst,
                                           uint8_t* mask, const uint8_t* available, int32_t nan_is_missing, const float* sigma,
                                           uint64_t seed, void* stream) {
  return stage_observed<true, true>(src, layout, src_rows, nullptr, first_pair, nodes_per_graph, num_graphs, observed,
                                    num_observed, normalise, offset, factor, x_dst, mask, available, nan_is_missing, stream,
                                    ObsNoise{sigma, seed, (long long)member0, (int)members});
}

extern "C" int gatres_estimate_write(const float* out, const float* x, const uint8_t* mask, int32_t nodes_per_graph,
                                     int32_t num_graphs, double scale, double offset, int32_t keep_observed, float* dst,
                                     int64_t dst_rows, int64_t dst_stride, int64_t first_row, void* stream) {
  if (!out || !dst || out == dst || nodes_per_graph <= 0 || num_graphs <= 0) return GATRES_E_BADARG;
  if (keep_observed && (!x || !mask || x == dst)) return GATRES_E_BADARG;
  if ((int64_t)nodes_per_graph * num_graphs > INT32_MAX) return GATRES_E_BADARG;
  if (dst_stride < nodes_per_graph || dst_rows <= 0 || first_row < 0 || first_row > dst_rows - num_graphs) return GATRES_E_BADARG;
  const long long total = (long long)nodes_per_graph * num_graphs;
  const int vec_load = gatres_aligned16(out) && (!keep_observed || (gatres_aligned16(x) && (reinterpret_cast<uintptr_t>(mask) & 3u) == 0));
  const int vec_store = gatres_aligned16(dst) && nodes_per_graph % 4 == 0 && dst_stride % 4 == 0;
  long long wgs = (total + 4LL * EW_T - 1) / (4LL * EW_T);
  if (wgs > 4096) wgs = 4096;
  hipLaunchKernelGGL(estimate_write_kernel, dim3((unsigned)wgs), dim3(EW_T), 0, gatres_stream(stream), out, x, mask,
                     (int)nodes_per_graph, total, (float)scale, (float)offset, (int)(keep_observed != 0), dst,
                     (long long)dst_stride, (long long)first_row, vec_load, vec_store);
  return gatres_launch_status();
}

extern "C" int gatres_node_error_moments(const float* est, const float* truth, int64_t num_snapshots, int32_t nodes_per_graph,
                                         double scale, double offset, const int32_t* observed, int32_t num_observed,
                                         double* table, void* stream) {
  if (!est || !truth || !observed || !table || num_snapshots <= 0 || nodes_per_graph <= 0) return GATRES_E_BADARG;
  if (num_observed <= 0 || num_observed > nodes_per_graph) return GATRES_E_BADARG;
  static_assert(GATRES_NODE_ERROR_CHUNK == NE_WAVES * NE_U, "gatres.h states the chunk of the moments kernel");
  static_assert(GATRES_NODE_ERROR_RECORD == 8, "record layout");
  hipLaunchKernelGGL(node_error_moments_kernel<false>, dim3((nodes_per_graph + GATRES_WAVE - 1) / GATRES_WAVE), dim3(NE_T), 0,
                     gatres_stream(stream), est, truth, (long long)num_snapshots, (int)nodes_per_graph, (float)scale,
                     (float)offset, observed, (int)num_observed, table, (const uint8_t*)nullptr);
  return gatres_launch_status();
}

extern "C" int gatres_node_error_moments_available(const float* est, const float* truth, int64_t num_snapshots,
                                                   int32_t nodes_per_graph, double scale, double offset, const int32_t* observed,
                                                   int32_t num_observed, const uint8_t* available, double* table, void* stream) {
  if (!est || !truth || !observed || !available || !table || num_snapshots <= 0 || nodes_per_graph <= 0) return GATRES_E_BADARG;
  if (num_observed <= 0 || num_observed > nodes_per_graph) return GATRES_E_BADARG;
  if (reinterpret_cast<const void*>(available) == reinterpret_cast<const void*>(table)) return GATRES_E_BADARG;
  static_assert(GATRES_NODE_ERROR_AVAIL_RECORD == 8, "record layout");
  hipLaunchKernelGGL(node_error_moments_kernel<true>, dim3((nodes_per_graph + GATRES_WAVE - 1) / GATRES_WAVE), dim3(NE_T), 0,
                     gatres_stream(stream), est, truth, (long long)num_snapshots, (int)nodes_per_graph, (float)scale,
                     (float)offset, observed, (int)num_observed, table, available);
  return gatres_launch_status();
}

extern "C" int gatres_ensemble_reduce(const float* members_mat, int64_t num_snapshots, int32_t members, int32_t nodes_per_graph,
                                      int64_t stride, float* mean, float* std_dev, int64_t out_rows, int64_t out_stride,
                                      int64_t first_row, void* stream) {
  if (!members_mat || !mean || !std_dev || num_snapshots <= 0 || members < 1 || nodes_per_graph <= 0) return GATRES_E_BADARG;
  if (stride < nodes_per_graph || out_stride < nodes_per_graph) return GATRES_E_BADARG;
  if (out_rows <= 0 || first_row < 0 || first_row > out_rows - num_snapshots) return GATRES_E_BADARG;
  if (num_snapshots > INT64_MAX / 4 / members / stride || out_rows > INT64_MAX / 4 / out_stride) return GATRES_E_BADARG;
  // (the rows of the source and the rows [first_row, first_row + num_snapshots) of either destination, strides included)
  const uint64_t src_bytes = 4 * (uint64_t)num_snapshots * (uint64_t)members * (uint64_t)stride;
  const uint64_t dst_bytes = 4 * (uint64_t)num_snapshots * (uint64_t)out_stride;
  const float* m0 = mean + first_row * out_stride;
  const float* s0 = std_dev + first_row * out_stride;
  if (bytes_overlap(members_mat, src_bytes, m0, dst_bytes) || bytes_overlap(members_mat, src_bytes, s0, dst_bytes) ||
      bytes_overlap(m0, dst_bytes, s0, dst_bytes)) return GATRES_E_BADARG;
  const bool vec = nodes_per_graph % 4 == 0 && stride % 4 == 0 && out_stride % 4 == 0 && gatres_aligned16(members_mat) &&
                   gatres_aligned16(mean) && gatres_aligned16(std_dev);
  const int per = vec ? 4 : 1;
  long long wgs = (num_snapshots * ((nodes_per_graph + per - 1) / per) + ER_T - 1) / ER_T;
  if (wgs > 2048) wgs = 2048;
  const dim3 grid((unsigned)wgs);
  if (vec)
    hipLaunchKernelGGL(ensemble_reduce_kernel<4>, grid, dim3(ER_T), 0, gatres_stream(stream), members_mat, (long long)num_snapshots,
                       (int)members, (int)nodes_per_graph, (long long)stride, mean, std_dev, (long long)out_stride, (long long)first_row);
  else
    hipLaunchKernelGGL(ensemble_reduce_kernel<1>, grid, dim3(ER_T), 0, gatres_stream(stream), members_mat, (long long)num_snapshots,
                       (int)members, (int)nodes_per_graph, (long long)stride, mean, std_dev, (long long)out_stride, (long long)first_row);
  return gatres_launch_status();
}

extern "C" int gatres_node_spread_moments(const float* std_dev, int64_t num_snapshots, int32_t nodes_per_graph, double* table,
                                          void* stream) {
  if (!std_dev || !table || num_snapshots <= 0 || nodes_per_graph <= 0) return GATRES_E_BADARG;
  if (reinterpret_cast<const void*>(std_dev) == reinterpret_cast<const void*>(table)) return GATRES_E_BADARG;
  static_assert(GATRES_NODE_SPREAD_RECORD == 4, "record layout");
  hipLaunchKernelGGL(node_spread_moments_kernel, dim3((nodes_per_graph + GATRES_WAVE - 1) / GATRES_WAVE), dim3(NE_T), 0,
                     gatres_stream(stream), std_dev, (long long)num_snapshots, (int)nodes_per_graph, table);
  return gatres_launch_status();
}

extern "C" int gatres_stage_observed_layouts(const float* src, int32_t layout, int64_t src_rows, int64_t first_pair,
                                             int32_t num_layouts, int32_t nodes_per_graph, int32_t num_graphs,
                                             const int32_t* observed, int32_t num_observed, int32_t normalise, double offset,
                                             double factor, float* x_dst, uint8_t* mask, const uint8_t* available,
                                             int32_t nan_is_missing, const uint8_t* layouts, void* stream) {
  return stage_observed<true, false, true>(src, layout, src_rows, nullptr, first_pair, nodes_per_graph, num_graphs, observed,
                                           num_observed, normalise, offset, factor, x_dst, mask, available, nan_is_missing, stream,
                                           ObsNoise{nullptr, 0, 0, 1}, ObsLayouts{layouts, (int)num_layouts});
}

extern "C" int gatres_stage_observed_targets(const float* src, int32_t layout, int64_t src_rows, int64_t first_pair,
                                             int32_t num_targets, const int32_t* targets, int32_t nodes_per_graph,
                                             int32_t num_graphs, const int32_t* observed, int32_t num_observed, int32_t normalise,
                                             double offset, double factor, float* x_dst, uint8_t* mask, float* g_out,
                                             const uint8_t* available, int32_t nan_is_missing, void* stream) {
  return stage_observed<true, false, false, true>(src, layout, src_rows, nullptr, first_pair, nodes_per_graph, num_graphs, observed,
                                                  num_observed, normalise, offset, factor, x_dst, mask, available, nan_is_missing,
                                                  stream, ObsNoise{nullptr, 0, 0, 1}, ObsLayouts{nullptr, 1},
                                                  ObsTargets{targets, g_out, (int)num_targets, 0});
}

extern "C" int gatres_layout_pair_errors(const float* out, const uint8_t* mask, const float* truth, int64_t truth_rows,
                                         int32_t nodes_per_graph, int32_t num_graphs, int64_t first_pair, int32_t num_layouts,
                                         double scale, double offset, const uint8_t* score, double* rec, int64_t rec_rows,
                                         int64_t rec_first, void* stream) {
  if (!out || !mask || !truth || !rec || nodes_per_graph <= 0 || num_graphs <= 0 || num_layouts < 1) return GATRES_E_BADARG;
  if ((int64_t)nodes_per_graph * num_graphs > INT32_MAX) return GATRES_E_BADARG;
  if (truth_rows <= 0 || truth_rows > INT64_MAX / num_layouts || truth_rows > INT64_MAX / 4 / nodes_per_graph) return GATRES_E_BADARG;
  if (first_pair < 0 || first_pair > truth_rows * num_layouts - num_graphs) return GATRES_E_BADARG;
  static_assert(GATRES_LAYOUT_PAIR_RECORD == 4, "record layout");
  if (rec_rows <= 0 || rec_rows > INT64_MAX / 32 || rec_first < 0 || rec_first > rec_rows - num_graphs) return GATRES_E_BADARG;
  const uint64_t total = (uint64_t)nodes_per_graph * (uint64_t)num_graphs, rec_bytes = 32 * (uint64_t)rec_rows;
  if (bytes_overlap(rec, rec_bytes, out, 4 * total) || bytes_overlap(rec, rec_bytes, mask, total) ||
      bytes_overlap(rec, rec_bytes, truth, 4 * (uint64_t)truth_rows * (uint64_t)nodes_per_graph) ||
      (score && bytes_overlap(rec, rec_bytes, score, (uint64_t)nodes_per_graph))) return GATRES_E_BADARG;
  hipLaunchKernelGGL(layout_pair_errors_kernel, dim3((num_graphs + PE_WAVES - 1) / PE_WAVES), dim3(PE_T), 0, gatres_stream(stream),
                     out, mask, truth, (int)nodes_per_graph, (int)num_graphs, (long long)first_pair, (int)num_layouts, (float)scale,
                     (float)offset, score, rec + rec_first * GATRES_LAYOUT_PAIR_RECORD, (int)gatres_aligned16(out),
                     (int)((reinterpret_cast<uintptr_t>(mask) & 3u) == 0), (int)gatres_aligned16(truth),
                     (int)((reinterpret_cast<uintptr_t>(score) & 3u) == 0));
  return gatres_launch_status();
}

extern "C" int gatres_layout_error_reduce(const double* rec, int64_t num_snapshots, int32_t num_layouts, double* table,
                                          int32_t accumulate, void* stream) {
  if (!rec || !table || num_snapshots <= 0 || num_layouts < 1 || num_snapshots > INT64_MAX / 32 / num_layouts) return GATRES_E_BADARG;
  static_assert(GATRES_LAYOUT_ERROR_RECORD == 4 && GATRES_LAYOUT_PAIR_RECORD == 4, "record layout");
  if (bytes_overlap(rec, 32 * (uint64_t)num_snapshots * (uint64_t)num_layouts, table, 32 * (uint64_t)num_layouts)) return GATRES_E_BADARG;
  hipLaunchKernelGGL(layout_error_reduce_kernel, dim3((num_layouts + LR_T - 1) / LR_T), dim3(LR_T), 0, gatres_stream(stream), rec,
                     (long long)num_snapshots, (int)num_layouts, table, (int)(accumulate != 0));
  return gatres_launch_status();
}

// The epoch boundary of the reference's training loop (train.py:426-511 `internal_train`) on the device, for
// GATResTrainer.fit: the decision of one epoch -- losses, best bookkeeping, EarlyStopping, ReduceLROnPlateau -- as ONE
// single-wave launch behind the epoch's last validation launch (gatres_epoch_control), and the best checkpoint kept in device
// memory (gatres_snapshot_if).  The host reads one history record per epoch and learns from it whether to stop.
//
// Number formats, as the reference runs them:
//   losses, best_loss and the scheduler: fp64 -- Python floats (train.py:426 `val_loss < best_loss`, torch's
//     ReduceLROnPlateau.step: `float(metrics)`, `best * (1 - threshold)`, `max(old_lr * factor, min_lr)`);
//   EarlyStopping: fp32 -- train.py:506 hands it `torch.tensor(val_loss)`, a float32 tensor, and `a < best - min_delta`
//     is then an fp32 subtraction (min_delta rounded to fp32 first) and an fp32 comparison.
// The epoch's validation loss is accumulated batch by batch in the host loop's order (evaluation.metrics_from_moments:
// `acc += loss_b * g_b`, then `acc / n`): a product and a sum, each rounded -- never an fma -- so the bits are numpy's.
#include "gatres_common.h"

#pragma clang fp contract(off)

namespace {

// sum_b loss_b * g_b in batch order and n = sum_b g_b; every lane of the (single) wave returns the same two values.
// loss_b = table[b][1] / table[b][0] (the moment record's masked MSE) or (double)losses[b].  The wave loads and multiplies 64
// batches at a time; the additions go one by one, in order.
__device__ __forceinline__ void epoch_val_sums(const double* __restrict__ table, const float* __restrict__ losses,
                                               const int* __restrict__ graphs, int B, double& acc_out, double& n_out) {
  const int lane = threadIdx.x % GATRES_WAVE;
  double acc = 0.0;
  long long n = 0;
  for (int b0 = 0; b0 < B; b0 += GATRES_WAVE) {
    const int b = b0 + lane;
    double prod = 0.0;
    int g = 0;
    if (b < B) {
      g = graphs[b];
      const double v = table ? table[(size_t)b * GATRES_METRICS_RECORD + 1] / table[(size_t)b * GATRES_METRICS_RECORD]
                             : (double)losses[b];
      prod = __dmul_rn(v, (double)g);
    }
    const int cnt = B - b0 < GATRES_WAVE ? B - b0 : GATRES_WAVE;
    for (int i = 0; i < cnt; ++i) {
      acc = __dadd_rn(acc, __shfl(prod, i));
      n += __shfl(g, i);
    }
  }
  acc_out = acc;
  n_out = (double)n;
}

__global__ __launch_bounds__(GATRES_WAVE) void epoch_val_sums_kernel(const double* __restrict__ table,
                                                                     const float* __restrict__ losses,
                                                                     const int* __restrict__ graphs, int B,
                                                                     double* __restrict__ out) {
  double acc, n;
  epoch_val_sums(table, losses, graphs, B, acc, n);
  if (threadIdx.x == 0) {
    out[0] = acc;
    out[1] = n;
  }
}

__global__ __launch_bounds__(GATRES_WAVE) void epoch_control_kernel(const double* __restrict__ train_sums,
                                                                    const double* __restrict__ val_table,
                                                                    const float* __restrict__ val_losses,
                                                                    const int* __restrict__ val_graphs, int B,
                                                                    const double* __restrict__ val_sums, gatres_epoch_config_t cfg,
                                                                    double* __restrict__ hp, double* __restrict__ state,
                                                                    double* __restrict__ history, int history_capacity) {
  double acc, n;
  if (B > 0) {
    epoch_val_sums(val_table, val_losses, val_graphs, B, acc, n);
  } else {
    acc = val_sums[0];
    n = val_sums[1];
  }
  if (threadIdx.x != 0) return;
  double* s = state;
  // 1. the epoch's two losses
  const double tr_loss = train_sums[0] / train_sums[1];
  const double val_loss = acc / n;
  const double epoch = s[GATRES_EPOCH_S_EPOCH] + 1.0;
  // 2. best bookkeeping (train.py:426-430): fp64, strict
  double best_loss = s[GATRES_EPOCH_S_BEST_LOSS], best_epoch = s[GATRES_EPOCH_S_BEST_EPOCH];
  const bool improved = val_loss < best_loss;
  if (improved) {
    best_loss = val_loss;
    best_epoch = epoch;
  }
  // 3. EarlyStopping(mode="min", min_delta, patience).step(torch.tensor(val_loss)): fp32
  bool stop = false;
  double es_has = s[GATRES_EPOCH_S_ES_HAS_BEST], es_bad = s[GATRES_EPOCH_S_ES_BAD];
  float es_best = (float)s[GATRES_EPOCH_S_ES_BEST];
  if (cfg.patience != 0) {
    const float m = (float)val_loss;
    if (es_has == 0.0) {                 // the first epoch only stores its metric, whatever it is
      es_best = m;
      es_has = 1.0;
    } else if (m != m) {                 // a NaN metric stops (and counts nothing)
      stop = true;
    } else {
      if (m < __fsub_rn(es_best, (float)cfg.min_delta)) {
        es_bad = 0.0;
        es_best = m;
      } else {
        es_bad += 1.0;
      }
      stop = es_bad >= (double)cfg.patience;
    }
  }
  // 4. ReduceLROnPlateau(mode="min", threshold_mode="rel", cooldown=0).step(val_loss) -- not on the epoch that stops
  const double lr_used = hp[0];
  double lr = lr_used, sc_best = s[GATRES_EPOCH_S_SCHED_BEST], sc_bad = s[GATRES_EPOCH_S_SCHED_BAD];
  if (!stop && cfg.use_scheduler) {
    if (val_loss < __dmul_rn(sc_best, __dsub_rn(1.0, cfg.threshold))) {
      sc_best = val_loss;
      sc_bad = 0.0;
    } else {
      sc_bad += 1.0;
    }
    if (sc_bad > (double)cfg.scheduler_patience) {
      const double scaled = __dmul_rn(lr_used, cfg.factor);
      const double new_lr = cfg.min_lr > scaled ? cfg.min_lr : scaled;       // Python's max(scaled, min_lr)
      if (__dsub_rn(lr_used, new_lr) > cfg.eps) lr = new_lr;
      sc_bad = 0.0;
    }
    if (lr != lr_used) hp[0] = lr;       // the update kernels of the next epoch read it from here
  }
  s[GATRES_EPOCH_S_EPOCH] = epoch;
  s[GATRES_EPOCH_S_BEST_LOSS] = best_loss;
  s[GATRES_EPOCH_S_BEST_EPOCH] = best_epoch;
  s[GATRES_EPOCH_S_ES_HAS_BEST] = es_has;
  s[GATRES_EPOCH_S_ES_BEST] = (double)es_best;
  s[GATRES_EPOCH_S_ES_BAD] = es_bad;
  s[GATRES_EPOCH_S_SCHED_BEST] = sc_best;
  s[GATRES_EPOCH_S_SCHED_BAD] = sc_bad;
  s[GATRES_EPOCH_S_IMPROVED] = improved ? 1.0 : 0.0;
  s[GATRES_EPOCH_S_STOPPED] = stop ? 1.0 : 0.0;
  // 5. the epoch's history record
  const long long slot = (long long)epoch - 1;
  if (slot >= 0 && slot < history_capacity) {
    double* r = history + (size_t)slot * GATRES_EPOCH_RECORD;
    r[GATRES_EPOCH_R_EPOCH] = epoch;
    r[GATRES_EPOCH_R_TR_LOSS] = tr_loss;
    r[GATRES_EPOCH_R_VAL_LOSS] = val_loss;
    r[GATRES_EPOCH_R_LR_USED] = lr_used;
    r[GATRES_EPOCH_R_LR_AFTER] = lr;
    r[GATRES_EPOCH_R_IMPROVED] = improved ? 1.0 : 0.0;
    r[GATRES_EPOCH_R_BEST_LOSS] = best_loss;
    r[GATRES_EPOCH_R_BEST_EPOCH] = best_epoch;
    r[GATRES_EPOCH_R_ES_BAD] = es_bad;
    r[GATRES_EPOCH_R_STOP] = stop ? 1.0 : 0.0;
    r[GATRES_EPOCH_R_SCHED_BAD] = sc_bad;
    r[GATRES_EPOCH_R_SCHED_BEST] = sc_best;
    r[GATRES_EPOCH_R_ES_BEST] = (double)es_best;
    r[GATRES_EPOCH_R_VAL_GRAPHS] = n;
    r[14] = 0.0;
    r[15] = 0.0;
  }
}

// ---- the best checkpoint on the device ---------------------------------------------------------------------------------------
constexpr int SNAP_T = 256;
constexpr int SNAP_U = 4;                              // 16-byte vectors per thread and trip
constexpr int SNAP_WG_FLOATS = SNAP_T * SNAP_U * 4;    // 16 KB per workgroup and trip
constexpr int SNAP_MAX_WGS = 2048;

struct snap_arrays_t {
  const float* src[3];
  float* dst[3];
};

// blockIdx.y names the array (parameters, exp_avg, exp_avg_sq), blockIdx.x strides over its 16 KB pieces.  Per array: a
// scalar head up to the destination's first 16-byte boundary, the aligned body as float4 (if the source is aligned there
// too; float by float otherwise), a scalar tail.
__global__ __launch_bounds__(SNAP_T) void snapshot_if_kernel(const double* __restrict__ flag, snap_arrays_t a,
                                                             const unsigned long long* __restrict__ step_src,
                                                             unsigned long long* __restrict__ step_dst, long long count) {
  if (flag && !(flag[0] != 0.0)) return;
  // (selects, not an index: a dynamically indexed kernel-argument struct becomes a private array)
  const float* __restrict__ src = blockIdx.y == 0 ? a.src[0] : blockIdx.y == 1 ? a.src[1] : a.src[2];
  float* __restrict__ dst = blockIdx.y == 0 ? a.dst[0] : blockIdx.y == 1 ? a.dst[1] : a.dst[2];
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && step_src && step_dst) step_dst[0] = step_src[0];
  long long head = (long long)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) / 4u);
  if (head > count) head = count;
  const bool vec = (reinterpret_cast<uintptr_t>(src + head) & 15u) == 0;
  const long long nvec = vec ? (count - head) / 4 : 0;
  const long long tail0 = head + 4 * nvec;
  if (blockIdx.x == 0) {
    for (long long i = threadIdx.x; i < head; i += SNAP_T) dst[i] = src[i];
    if (vec)
      for (long long i = tail0 + threadIdx.x; i < count; i += SNAP_T) dst[i] = src[i];
  }
  if (vec) {
    const float4* __restrict__ s4 = reinterpret_cast<const float4*>(src + head);
    float4* __restrict__ d4 = reinterpret_cast<float4*>(dst + head);
    for (long long v0 = (long long)blockIdx.x * (SNAP_T * SNAP_U); v0 < nvec; v0 += (long long)gridDim.x * (SNAP_T * SNAP_U)) {
      float4 r[SNAP_U];
#pragma unroll
      for (int u = 0; u < SNAP_U; ++u) {
        const long long v = v0 + u * SNAP_T + threadIdx.x;
        if (v < nvec) r[u] = s4[v];
      }
#pragma unroll
      for (int u = 0; u < SNAP_U; ++u) {
        const long long v = v0 + u * SNAP_T + threadIdx.x;
        if (v < nvec) d4[v] = r[u];
      }
    }
  } else {
    for (long long i = head + (long long)blockIdx.x * SNAP_T + threadIdx.x; i < count; i += (long long)gridDim.x * SNAP_T)
      dst[i] = src[i];
  }
}

bool epoch_config_ok(const gatres_epoch_config_t* c) {
  return c && c->patience >= 0 && c->scheduler_patience >= 0;
}

}  // namespace

extern "C" int gatres_epoch_val_sums(const double* val_table, const float* val_losses, const int32_t* val_graphs,
                                     int32_t num_batches, double* out, void* stream) {
  if ((!val_table) == (!val_losses) || !val_graphs || num_batches <= 0 || !out) return GATRES_E_BADARG;
  hipLaunchKernelGGL(epoch_val_sums_kernel, dim3(1), dim3(GATRES_WAVE), 0, gatres_stream(stream), val_table, val_losses,
                     val_graphs, (int)num_batches, out);
  return gatres_launch_status();
}

extern "C" int gatres_epoch_control(const double* train_sums, const double* val_table, const float* val_losses,
                                    const int32_t* val_graphs, int32_t num_batches, const double* val_sums,
                                    const gatres_epoch_config_t* config_host, double* hp, double* state, double* history,
                                    int32_t history_capacity, void* stream) {
  if (!train_sums || !epoch_config_ok(config_host) || !hp || !state || !history || history_capacity <= 0 || num_batches < 0)
    return GATRES_E_BADARG;
  if (num_batches > 0 ? ((!val_table) == (!val_losses) || !val_graphs) : !val_sums) return GATRES_E_BADARG;
  hipLaunchKernelGGL(epoch_control_kernel, dim3(1), dim3(GATRES_WAVE), 0, gatres_stream(stream), train_sums, val_table,
                     val_losses, val_graphs, (int)num_batches, val_sums, *config_host, hp, state, history, (int)history_capacity);
  return gatres_launch_status();
}

extern "C" int gatres_snapshot_if(const double* flag, const float* params, const float* exp_avg, const float* exp_avg_sq,
                                  const uint64_t* step_counter, float* dst_params, float* dst_exp_avg, float* dst_exp_avg_sq,
                                  uint64_t* dst_step_counter, int64_t count, void* stream) {
  if (!params || !exp_avg || !exp_avg_sq || !dst_params || !dst_exp_avg || !dst_exp_avg_sq || count <= 0) return GATRES_E_BADARG;
  if ((!step_counter) != (!dst_step_counter)) return GATRES_E_BADARG;
  for (const void* p : {(const void*)params, (const void*)exp_avg, (const void*)exp_avg_sq, (const void*)dst_params,
                        (const void*)dst_exp_avg, (const void*)dst_exp_avg_sq})
    if (reinterpret_cast<uintptr_t>(p) & 3u) return GATRES_E_BADARG;
  snap_arrays_t a{{params, exp_avg, exp_avg_sq}, {dst_params, dst_exp_avg, dst_exp_avg_sq}};
  long long wgs = ((long long)count + SNAP_WG_FLOATS - 1) / SNAP_WG_FLOATS;        // sized to the bytes, not to the chip
  if (wgs > SNAP_MAX_WGS) wgs = SNAP_MAX_WGS;
  hipLaunchKernelGGL(snapshot_if_kernel, dim3((unsigned)wgs, 3), dim3(SNAP_T), 0, gatres_stream(stream), flag, a,
                     reinterpret_cast<const unsigned long long*>(step_counter),
                     reinterpret_cast<unsigned long long*>(dst_step_counter), (long long)count);
  return gatres_launch_status();
}

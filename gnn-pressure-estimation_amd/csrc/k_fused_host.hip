// Host side of the fused per-snapshot path: launch geometry, the deferred parameter-gradient launch, the slab reduction +
// Adam launch, and the C-ABI entry points (include/gatres.h: gatres_fused_*).
#include <atomic>
#include <vector>
#include "k_fused_dev.h"
#include "k_mask.h"
#include "k_autoclip.h"
#include "k_update.h"

namespace {

static unsigned long long* g_stamps = nullptr;      // gatres_fused_set_stamps (diagnostic build)
static int g_stamp_cap = 0;

// What the slab sum is given; the update behind it: UpdateArgs (a.count = the length of a slab row that is summed; a.g is
// not read: the update takes the sum)
struct SlabSumArgs {
  const float* slabs;            // num_slabs rows, `stride` floats apart
  int num_slabs, num_loss;
  long long stride;
  float* grads;                  // receives the sum (NaN on a faulted step)
  const float* loss_part;        // num_loss partial sums and the masked-node count behind them, or null
  float* loss;
  int do_adam, use_snap, reduce_blocks;
  unsigned* status;              // the status block (fused_status), or null: the plan has no split launches
  double* ac_partials;           // NORM only
  unsigned long long* ac_ctl;
};

// grads = sum of segment slabs (fixed order) ; optionally the Adam update and the loss finalisation in the same pass.
// NORM (AutoClip, with do_adam == 0): each workgroup also leaves the fp64 sum of squares of its slice of grads * grad_scale
// in ac_partials[blockIdx.x], and block 0 snapshots the words the AutoClip update launch reads (k_autoclip.hip).  NORM == false
// is the kernel of the step without clipping, unchanged.
template <bool NORM>
__global__ __launch_bounds__(256) void reduce_adam_kernel(const UpdateArgs a, const SlabSumArgs r) {
  __shared__ float s_step_size, s_bc2_sqrt;
  __shared__ unsigned s_fault;
  // The device mask of the NEXT step (utils/auxil.py:166-182), sampled by the workgroups behind the reduction's: the
  // sampler's own launch (5.9 us + a launch boundary per step) disappears from the captured step.  Its key uses the step
  // count this update leaves behind -- exactly what gatres_mask_generate would read at the start of the next step: the
  // count and the fault word as the parameter-gradient launch in front of this one snapshotted them (mask_snap: this
  // launch changes both, and 512 more tickets on the one counter address would cost 10 us).
  if (a.mask_next && (int)blockIdx.x >= r.reduce_blocks) {
    const int mb = (int)blockIdx.x - r.reduce_blocks;
    const unsigned long long next_step = a.mask_snap[1] == 0ULL ? a.mask_snap[0] + 1ULL : a.mask_snap[0];      // (dropped: unchanged)
    mask_sample_graph<256, MASK_WGS_UPDATE>(a.mask_node_ptr, a.mask_rate, a.mask_seed, next_step, a.mask_next,
                                            mb / MASK_WGS_UPDATE, mb % MASK_WGS_UPDATE);
    return;
  }
  double lr = a.lr, b1 = a.b1, b2 = a.b2, eps = a.eps, wd = a.wd;
  if (a.hp) { lr = a.hp[0]; b1 = a.hp[1]; b2 = a.hp[2]; eps = a.hp[3]; wd = a.hp[4]; }      // (gatres_train_step_t.hparams)
  // The status block's FAULT word (gatres_layout.h): a split launch of this step gave up waiting for a partner workgroup (its
  // results are poisoned).  The step is then DROPPED: no Adam update, no step count, loss = NaN, gradients = NaN; the last
  // block clears the word and counts the event in FAULT_COUNT, so one transient stall costs one step instead of the whole run.
  // snap: the parameter-gradient launch in front of this one left the step count and the fault word in mask_snap (the training
  // step's sequence, gatres_train_step).  Every block then reads THOSE -- stable words -- and block 0 alone counts the step:
  // no tickets (258 read-modify-writes on one address serialise in the L2 at ~20 ns each: 5 of this launch's 8 us).
  const bool snap = r.use_snap != 0;
  if (threadIdx.x == 0)
    s_fault = snap ? (unsigned)a.mask_snap[1]
                   : (r.status ? __hip_atomic_load(r.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u);
  if (r.do_adam && threadIdx.x == 0) {
    const unsigned long long t =
        (snap ? a.mask_snap[0] : __hip_atomic_load(a.step_counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) + 1ULL;
    s_step_size = (float)(lr / (1.0 - gatres_powi(b1, t)));
    s_bc2_sqrt = (float)sqrt(1.0 - gatres_powi(b2, t));
    if (snap && s_fault == 0u && blockIdx.x == 0) a.step_counter[0] = t;      // (nobody reads the counter in this launch)
    // The step is counted once every block has READ the counter: a ticket drawn right after this block's read (its value is
    // in a register: the wait below), the last ticket increments.  Nothing orders the count behind the parameter stores --
    // the next launch is -- so no fence: the ticket used to follow the block's stores behind a __threadfence(), an L2
    // write-back + invalidate of ~3.5 us at the end of every block of a 14-us launch.
    if (!snap) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    if (!snap && s_fault == 0u) {
      const unsigned long long done = atomicAdd(&a.step_counter[1], 1ULL);
      if (done == (unsigned long long)r.reduce_blocks - 1ULL) {
        a.step_counter[1] = 0ULL;
        atomicAdd(&a.step_counter[0], 1ULL);
      }
    }
  }
  if (r.loss_part && blockIdx.x == 0 && threadIdx.x < 64) {
    // the loss: sum of the per-(segment, part) squared errors / masked-node count.  One wave, strided partial sums
    // and a fixed-order butterfly (a single thread walking 128 dependent loads made block 0 the kernel's critical path)
    float s = 0.f;
    for (int k = threadIdx.x; k < r.num_loss; k += 64) s += r.loss_part[k];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (threadIdx.x == 0) r.loss[0] = s / r.loss_part[r.num_loss];
  }
  __syncthreads();
  const bool fault = s_fault != 0u;
  if (fault && r.loss && blockIdx.x == 0 && threadIdx.x == 0) r.loss[0] = NAN;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  [[maybe_unused]] double sq = 0.0;
  if (idx < a.count && (int)blockIdx.x < r.reduce_blocks) {
    float acc = 0.f;
    int s0 = 0;
    // the parameter and its moments are requested together with the first slab rows: one memory round trip for a
    // 32-snapshot batch instead of five dependent ones (this launch is pure latency: 258 workgroups x 4 waves)
    float pv = 0.f, mv0 = 0.f, vv0 = 0.f;
    if (r.do_adam && !fault) { pv = a.p[idx]; mv0 = a.m[idx]; vv0 = a.v[idx]; }
    for (; s0 + 32 <= r.num_slabs; s0 += 32) {          // 32 loads in flight, summed in slab order
      float v32[32];
#pragma unroll
      for (int u = 0; u < 32; ++u) v32[u] = r.slabs[(size_t)(s0 + u) * r.stride + idx];
#pragma unroll
      for (int u = 0; u < 32; ++u) acc += v32[u];
    }
    for (; s0 + 8 <= r.num_slabs; s0 += 8) {
      float v8[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v8[u] = r.slabs[(size_t)(s0 + u) * r.stride + idx];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += v8[u];
    }
    for (; s0 < r.num_slabs; ++s0) acc += r.slabs[(size_t)s0 * r.stride + idx];
    r.grads[idx] = fault ? NAN : acc;
    if constexpr (NORM) {
      const double x = (double)(acc * a.grad_scale);
      sq = fault ? 0.0 : x * x;
    }
    if (r.do_adam && !fault) {
      float gv = acc * a.grad_scale;
      gv = gv + (float)wd * pv;
      float mv = mv0;
      mv = mv + (float)(1.0 - b1) * (gv - mv);
      const float vv = (float)b2 * vv0 + (float)(1.0 - b2) * gv * gv;
      const float denom = sqrtf(vv) / s_bc2_sqrt + (float)eps;
      const float pn = pv + (-s_step_size * mv) / denom;
      a.p[idx] = pn;
      a.m[idx] = mv;
      a.v[idx] = vv;
      if (a.wt) {                 // keep the transposed conv weights of the next backward current (k_misc.hip layout)
        const long long per = 2LL * a.nc * a.nc, stride = 9LL * a.nc + 2 * per, off = idx - 2LL * a.nc;
        if (off >= 0 && off < (long long)a.nb * stride) {
          const long long b = off / stride, o = off % stride;
          if (o >= 6LL * a.nc && o < 6LL * a.nc + per) {                    // W1 [2nc][nc] -> [nc][2nc]
            const long long e = o - 6LL * a.nc, row = e / a.nc, col = e % a.nc;
            a.wt[b * 2 * per + col * 2 * a.nc + row] = pn;
          } else if (o >= 9LL * a.nc + per) {                               // W2 [nc][2nc] -> [2nc][nc]
            const long long e = o - 9LL * a.nc - per, row = e / (2 * a.nc), col = e % (2 * a.nc);
            a.wt[b * 2 * per + per + col * a.nc + row] = pn;
          }
        }
      }
    }
  }
  if constexpr (NORM) {
    __shared__ double lds4[4];
    sq = ac_block_sum(sq, lds4);
    if (threadIdx.x == 0) {
      r.ac_partials[blockIdx.x] = sq;
      if (blockIdx.x == 0) ac_snapshot(r.ac_ctl, a.step_counter, fault);      // (every block has read the fault word: s_fault)
    }
  }
  if (fault && snap && blockIdx.x == 0 && threadIdx.x == 0) {      // (the other blocks read the snapshot, not the word)
    r.status[FUSED_STATUS_FAULT_COUNT] += 1u;
    __hip_atomic_store(r.status, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (fault && !snap && threadIdx.x == 0) {      // every block has read the fault word before the last ticket is drawn
    __threadfence();
    if (atomicAdd(r.status + FUSED_STATUS_FAULT_TICKETS, 1u) == (unsigned)r.reduce_blocks - 1u) {
      r.status[FUSED_STATUS_FAULT_TICKETS] = 0u;
      r.status[FUSED_STATUS_FAULT_COUNT] += 1u;
      __hip_atomic_store(r.status, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Parameter gradients of a RANGE of blocks, summed over the segments, in ONE launch: what the data-parallel step of the
// fused path forms its gradient buckets with (gatres_train_step: GATRES_FLAG_GRADS_ONLY) -- the upper blocks' bucket goes on
// the wire while the lower blocks' launch runs.
// A COLUMN is one (block, conv): the S = num_segments items of a column (one workgroup each, param_grads_reg_kernel's
// items) write the column's range of S slab rows with agent-scope stores (sc1: written through), acknowledged (every wave's
// s_waitcnt vmcnt(0)) before the item counts itself at the column's counter; the item that ARRIVES LAST reads the rows
// back with agent-scope loads (never served from its L1 or a stale L2 line: the granule protocol's pair of accesses,
// k_fused_dev.h), sums them in slab order -- reduce_adam_kernel's association: the same bits, whoever arrives last --,
// writes grads and, if asked (do_adam: the whole model only), applies Adam to those parameters.  lin0's range rides on
// column (block 0, conv1), lin1's on (last block, conv2).
// As a replacement of the single-GPU step's two launches (round 4's item launch 37.6 us + reduce_adam_kernel 8.7 us
// inside the captured step) it was measured and is NOT used: 53 us with everything in it (47.7 without Adam) -- the column
// sums are a serial tail of dependent memory round trips on the workgroups that finish last; a release fence per arriver
// instead of agent-scope stores 73 us (960 L2 write-back walks); dedicated reducer workgroups behind the items 60 us
// (a third round of workgroups): profiles/r04_param_grads_finish_probe.txt, tests/micro/pgf_probe.py.
// A faulted split launch (the status block's FAULT word) turns grads and loss into NaN and skips the update, as gatres_fused_finish;
// `final_launch`: this launch holds block 0 (it clears the fault).
struct FinishArgs {
  UpdateArgs u;                  // (u.g is not read: the update takes the column sums; no sampling ahead, no drop count)
  float* grads;
  const float* loss_part;
  float* loss;
  int num_loss, do_adam;
  unsigned* status;
  unsigned* colcnt;
  int S, b_lo, b_hi, final_launch;
};

template <int NC>
__global__ __launch_bounds__(PGR_THREADS) void param_grads_finish_kernel(const ParamGradArgs a, const FinishArgs f) {
  __shared__ __attribute__((aligned(16))) float lds[PGR_LDS_FLOATS(NC)];
  __shared__ int s_last;
  __shared__ float s_step_size, s_bc2_sqrt;
  __shared__ unsigned s_fault;
  const Layout& L = a.L;
  const int S = f.S, tid = threadIdx.x;
  // segment-major: a segment's items are adjacent workgroups, every column completes with the launch's last segment
  // (column-major measured 56 us against 53)
  const int ncol = 2 * (f.b_hi - f.b_lo);
  const int col = (int)(blockIdx.x % ncol), seg = (int)(blockIdx.x / ncol);
  const int b = f.b_hi - 1 - (col >> 1), conv = 1 - (col & 1);          // production order: upper blocks first, conv2 before conv1
  if (f.loss_part && blockIdx.x == 0 && tid < 64) {                      // the loss (as reduce_adam_kernel)
    float s = 0.f;
    for (int k = tid; k < f.num_loss; k += 64) s += f.loss_part[k];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    const bool flt = f.status && __hip_atomic_load(f.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
    if (tid == 0) f.loss[0] = flt ? NAN : s / f.loss_part[f.num_loss];
  }
  if (conv == 0) param_grads_item_reg<NC, 0, true>(a, seg, b, lds);
  else           param_grads_item_reg<NC, 1, true>(a, seg, b, lds);
  const bool has_lin0 = b == 0 && conv == 0, has_lin1 = b == L.nb - 1 && conv == 1;
  if (a.M > 1) {                                                         // lin0 / lin1 partials of a split segment
    if (has_lin0) fold_parts<PGR_THREADS, true>(a, seg, L.p_lin0_w, 2 * NC);
    if (has_lin1) fold_parts<PGR_THREADS, true>(a, seg, L.p_lin1_w, NC + 1);
  }
  // ---- arrive at the column's counter (no fence: see above)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  unsigned* cnt = f.colcnt + (2 * b + conv);
  if (tid == 0) {
    const unsigned prev = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = prev == (unsigned)(S - 1) ? 1 : 0;
  }
  __syncthreads();
  if (!s_last) return;
  double lr = f.u.lr, b1 = f.u.b1, b2 = f.u.b2, eps = f.u.eps, wd = f.u.wd;
  if (f.u.hp) { lr = f.u.hp[0]; b1 = f.u.hp[1]; b2 = f.u.hp[2]; eps = f.u.hp[3]; wd = f.u.hp[4]; }
  if (tid == 0) {
    __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);           // (the next launch starts from zero)
    s_fault = f.status ? __hip_atomic_load(f.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    if (f.do_adam) {
      const unsigned long long t = __hip_atomic_load(f.u.step_counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1ULL;
      s_step_size = (float)(lr / (1.0 - gatres_powi(b1, t)));
      s_bc2_sqrt = (float)sqrt(1.0 - gatres_powi(b2, t));
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");          // (the step count and the fault word are in registers)
  }
  __syncthreads();
  const bool fault = s_fault != 0u;
  const int64_t po = L.p_block0 + (int64_t)b * L.p_block_stride;
  const __amdgpu_buffer_rsrc_t slab_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(a.slabs, 0, (int)((size_t)S * L.slab_stride * 4), 0x00020000);
  typedef float v4f __attribute__((ext_vector_type(4)));
  auto slab4 = [&](int srow, int64_t idx) -> float4 {                   // 16 bytes of slab row srow, agent scope (sc1)
    const v4f v = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(
        slab_rsrc, (unsigned)(((size_t)srow * L.slab_stride + idx) * 4), 0, 16));
    return make_float4(v.x, v.y, v.z, v.w);
  };
  // one parameter: Adam on the summed gradient (the arithmetic of reduce_adam_kernel, statement for statement)
  auto update = [&](int64_t idx, float acc, float pv, float mv0, float vv0) {
    f.grads[idx] = fault ? NAN : acc;
    if (f.do_adam && !fault) {
      float gv = acc * f.u.grad_scale;
      gv = gv + (float)wd * pv;
      float mv = mv0;
      mv = mv + (float)(1.0 - b1) * (gv - mv);
      const float vv = (float)b2 * vv0 + (float)(1.0 - b2) * gv * gv;
      const float denom = sqrtf(vv) / s_bc2_sqrt + (float)eps;
      const float pn = pv + (-s_step_size * mv) / denom;
      f.u.p[idx] = pn;
      f.u.m[idx] = mv;
      f.u.v[idx] = vv;
      if (f.u.wt) {               // keep the transposed conv weights of the next backward current (k_misc.hip layout)
        const long long per = 2LL * NC * NC, o = idx - po;
        if (o >= 6LL * NC && o < 6LL * NC + per) {                          // W1 [2nc][nc] -> [nc][2nc]
          const long long e = o - 6LL * NC, row = e / NC, cl = e % NC;
          f.u.wt[(long long)b * 2 * per + cl * 2 * NC + row] = pn;
        } else if (o >= 9LL * NC + per && o < 9LL * NC + 2 * per) {         // W2 [nc][2nc] -> [2nc][nc]
          const long long e = o - 9LL * NC - per, row = e / (2 * NC), cl = e % (2 * NC);
          f.u.wt[(long long)b * 2 * per + per + cl * NC + row] = pn;
        }
      }
    }
  };
  // [lo, hi) of the flat vector, lo % 4 == 0: 16 bytes per thread and slab row, twelve rows in flight (sixteen spill at the
  // 128 VGPRs that two workgroups per CU leave), every element summed in slab order
  auto finish_range = [&](int64_t lo, int64_t hi) {
    const int64_t n4 = (hi - lo) >> 2;
    for (int64_t q = tid; q < n4; q += PGR_THREADS) {
      const int64_t idx = lo + 4 * q;
      float4 pv = f4zero(), mv0 = f4zero(), vv0 = f4zero();
      if (f.do_adam && !fault) { pv = ld4(f.u.p + idx); mv0 = ld4(f.u.m + idx); vv0 = ld4(f.u.v + idx); }
      float4 acc = f4zero();
      int s0 = 0;
      for (; s0 + 12 <= S; s0 += 12) {
        float4 v12[12];
#pragma unroll
        for (int u = 0; u < 12; ++u) v12[u] = slab4(s0 + u, idx);
#pragma unroll
        for (int u = 0; u < 12; ++u) { acc.x += v12[u].x; acc.y += v12[u].y; acc.z += v12[u].z; acc.w += v12[u].w; }
      }
      for (; s0 + 8 <= S; s0 += 8) {
        float4 v8[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v8[u] = slab4(s0 + u, idx);
#pragma unroll
        for (int u = 0; u < 8; ++u) { acc.x += v8[u].x; acc.y += v8[u].y; acc.z += v8[u].z; acc.w += v8[u].w; }
      }
      for (; s0 < S; ++s0) {
        const float4 v1 = slab4(s0, idx);
        acc.x += v1.x; acc.y += v1.y; acc.z += v1.z; acc.w += v1.w;
      }
      update(idx, acc.x, pv.x, mv0.x, vv0.x);
      update(idx + 1, acc.y, pv.y, mv0.y, vv0.y);
      update(idx + 2, acc.z, pv.z, mv0.z, vv0.z);
      update(idx + 3, acc.w, pv.w, mv0.w, vv0.w);
    }
    for (int64_t idx = lo + 4 * n4 + tid; idx < hi; idx += PGR_THREADS) {      // (lin1's odd element)
      float pv = 0.f, mv0 = 0.f, vv0 = 0.f;
      if (f.do_adam && !fault) { pv = f.u.p[idx]; mv0 = f.u.m[idx]; vv0 = f.u.v[idx]; }
      float acc = 0.f;
      for (int s0 = 0; s0 < S; ++s0)
        acc += __hip_atomic_load(a.slabs + (size_t)s0 * L.slab_stride + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      update(idx, acc, pv, mv0, vv0);
    }
  };
  if (conv == 0) finish_range(po, po + L.c2_as);
  else           finish_range(po + L.c2_as, po + L.p_block_stride);
  if (has_lin0) finish_range(L.p_lin0_w, L.p_block0);
  if (has_lin1) finish_range(L.p_lin1_w, L.P);
  if (tid == 0) {
    const unsigned ncols = (unsigned)ncol;
    if (f.do_adam && !fault) {
      // counted by the column that finishes last; every column has read the count before it draws
      const unsigned long long done = atomicAdd(&f.u.step_counter[1], 1ULL);
      if (done == (unsigned long long)ncols - 1ULL) {
        f.u.step_counter[1] = 0ULL;
        atomicAdd(&f.u.step_counter[0], 1ULL);
      }
    }
    if (fault && f.final_launch) {                 // every column of this launch has read the fault word before the last ticket
      __threadfence();
      if (atomicAdd(f.status + FUSED_STATUS_FAULT_TICKETS, 1u) == ncols - 1u) {
        f.status[FUSED_STATUS_FAULT_TICKETS] = 0u;
        f.status[FUSED_STATUS_FAULT_COUNT] += 1u;
        __hip_atomic_store(f.status, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

// gatres_probe_xcd_dispatch: one workgroup per CU (the whole LDS, 1024 threads: the shape of the split launches), each records
// the XCD it runs on.
__global__ __launch_bounds__(1024) void xcd_probe_kernel(unsigned* __restrict__ out) {
  __shared__ unsigned char lds[LDS_BYTES];
  lds[threadIdx.x] = (unsigned char)threadIdx.x;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = xcc_id() | ((unsigned)(lds[1] & 0u) << 8);
}

// The same bookkeeping after a split launch that no gatres_fused_finish follows (forward / inference launches)
__global__ __launch_bounds__(64) void fused_status_kernel(unsigned* __restrict__ status) {
  if (threadIdx.x == 0 && __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
    status[FUSED_STATUS_FAULT_COUNT] += 1u;
    __hip_atomic_store(status, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Two split launches must never be in flight on one device at the same time: each needs its whole grid resident, and
// each could hold CUs the other waits for (the bounded spins would then poison both).  Launches on ONE stream are
// ordered anyway; when the stream changes, the new stream first waits for everything enqueued on the previous one.
// Skipped while `st` is being captured: the host that replays the graph calls gatres_fused_serialize before the replay.
static std::mutex g_split_mu;
static hipStream_t g_split_stream[64];
static bool g_split_seen[64] = {};
static int serialize_split_launch(hipStream_t st) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
  std::lock_guard<std::mutex> lk(g_split_mu);
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); return 0; }
  if (cs != hipStreamCaptureStatusNone) return 0;
  if (g_split_seen[dev] && g_split_stream[dev] != st) {
    hipStream_t prev = g_split_stream[dev];
    hipStreamCaptureStatus ps = hipStreamCaptureStatusNone;
    hipEvent_t ev;
    if (hipStreamIsCapturing(prev, &ps) == hipSuccess && ps == hipStreamCaptureStatusNone &&
        hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess) {
      if (hipEventRecord(ev, prev) == hipSuccess) (void)hipStreamWaitEvent(st, ev, 0);
      (void)hipEventDestroy(ev);
    }
    (void)hipGetLastError();                     // (a stream the caller has destroyed meanwhile: nothing left to wait for)
  }
  // ... and for what the per-op backward may still have in flight on the library's side stream (its parameter-gradient
  // launches): they hold CUs a split launch needs resident
  if (gatres_side_t* side = gatres_side_peek()) {
    hipStreamCaptureStatus ss = hipStreamCaptureStatusNone;
    hipEvent_t ev;
    if (side->stream != st && hipStreamIsCapturing(side->stream, &ss) == hipSuccess && ss == hipStreamCaptureStatusNone &&
        hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess) {
      if (hipEventRecord(ev, side->stream) == hipSuccess) (void)hipStreamWaitEvent(st, ev, 0);
      (void)hipEventDestroy(ev);
    }
    (void)hipGetLastError();
  }
  g_split_stream[dev] = st;
  g_split_seen[dev] = true;
  return 0;
}

static int fused_threads_small() {
  return gatres_knobs()->fused_threads;
}
static int threads_for(int nc) { return nc <= 32 ? fused_threads_small() : (nc == 64 ? 512 : 256); }

// CUs of the current device (cached): every workgroup of a split launch must be resident at once, one per CU.
static int device_cus() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
      cus = v;
    else
      cus = 1;               // unknown: never split
  }
  return cus;
}

// The window kernel applies when the plan knows the parts' row windows and both LDS layouts fit with them.
static bool window_kernel_fits(const Layout& L, const gatres_graph_t* g, int M, bool keep = false) {
  if (gatres_knobs()->fused_no_window || M < 2 || M > 8 || L.nc > 32 || threads_for(L.nc) != 1024) return false;
  const int k = M - 2;
  const int wr = g->window[k][0], ge = g->window[k][1], gm = g->window[k][2], hl = g->halo[k];
  if (wr <= 0 || L.xch_stride <= 0) return false;
  const int tiles = (g->max_segment_nodes + 15) / 16;
  const int ow = 16 * ((tiles + M - 1) / M);
  const long long kb = keep ? win_keep_bytes(L.nb, ow) : 0;
  return win_fwd_bytes(L.nc, wr, ow, ge, gm, hl) + kb <= LDS_BYTES &&
         win_bwd_bytes(L.nc, 1024, wr, ow, ge, gm, hl) + kb + (keep ? 4LL * ow * L.nc + 16 : 0) <= LDS_BYTES &&
         wr <= 65535 && ge <= 65535 && gm <= 65535;
}

// CUs per segment.  B = the co-residency bound of the layout (at most 8, whole grid resident, no more parts than 16-row
// tiles).  Preferred: B parts on the window kernel; the kept gradient tables then become parameter gradients in the
// stand-alone launch that follows (gatres_fused_param_grads).  Measured on gatres_small, C-Town, bs = 32 (B = 8;
// profiles/r02_split_sweep.txt), GPU time of the two launches: 8 parts 462 + 38 us; 6 parts with the parameter gradients
// on the two CUs per snapshot left over 526 us (the part that owns a segment's last 68 rows needs two trips through every
// conv1-width sparse stage and a fifth MFMA tile -- 384-node snapshots run 22 us faster).  Otherwise the
// whole-segment-table kernel at min(B, 4).  The choice depends on the plan only, never on the phases of a launch: the
// per-part hand-off epochs persist in scratch.  GATRES_FUSED_SPLIT=1..8 overrides.
static int fused_split(const Layout& L, const gatres_graph_t* g, int cus) {
  const int tiles = (g->max_segment_nodes + 15) / 16;
  const int padded = ((g->num_segments + 7) / 8) * 8;
  // Rounds: 49 .. 96 segments fit the chip only at 4 .. 2 parts each -- whole-segment tables, where a snapshot costs MORE
  // than in a batch of 32 (bs 64: 0.99 ms = 64.7 k snapshots/s against 75.5 k at bs 32).  The window kernel is launched twice
  // instead, each round with half the segments at the parts that fit then (hand-offs only ever cross the parts of ONE
  // segment; the parameter-gradient launch and the update follow the last round): C-Town, bs 56 / 64 / 72 / 80 / 88 / 96,
  // ms per step, resident vs rounds: profiles/r03_rounds.txt.  Three rounds of 32 measured slower than the resident choice
  // (bs 72 .. 96: 1.24 .. 1.29 vs 1.14 .. 1.27).  GATRES_FUSED_NO_ROUNDS=1: the resident choice.
  if (const int rp = rounds_parts_for(g->num_segments)) {
    const int per = ((padded / 2 + 7) / 8) * 8;
    if (L.split_max == rp && tiles >= rp && L.nb > 0 && per * rp <= cus && !gatres_knobs()->fused_split &&
        !gatres_knobs()->fused_no_rounds && window_kernel_fits(L, g, rp))
      return rp;
  }
  int B = L.split_max;
  while (B > 1 && (B > tiles || L.nb == 0 || padded * B > cus)) --B;   // (a partitioned / smaller device)
  if (const int v = gatres_knobs()->fused_split) {
    if (v >= 1 && v <= B) return v;
  }
  if (B >= 2 && window_kernel_fits(L, g, B)) return B;
  int m = 1;
  while (m * 2 <= B && m < 4) m *= 2;
  return m;
}
static int fused_split(const Layout& L, const gatres_graph_t* g) { return fused_split(L, g, device_cus()); }

// Workgroups of one launch that carries seg_cnt segments at M parts each: ids of one segment are 8 apart
static unsigned fused_grid(int seg_cnt, int M) { return (unsigned)(((seg_cnt + 7) / 8) * 8 * M); }

// Everything a fused launch decides from the plan, the model and the phases, in ONE place: gatres_fused_run launches what
// this says and gatres_fused_plan reports it (include/gatres.h: GATRES_FUSED_PLAN_*), so the two cannot drift apart.
// has_saved: the launch is given a `saved` buffer (the window kernel writes the saved tables); cus: the CUs every
// workgroup of a split launch must be resident on; probed: the device's dispatch was probed (gatres_probe_xcd_dispatch).
struct FusedPlan {
  int M, window, cache, keep, facts, launches, per_launch, grid0, threads, part_rows, cus;
};
static int fused_decide(const gatres_model_t* m, const gatres_graph_t* g, const Layout& L, int32_t phases, bool has_saved,
                        int cus, bool probed, FusedPlan* p) {
  const int nc = m->nc, threads = threads_for(nc);
  p->cus = cus;
  p->threads = threads;
  p->M = fused_split(L, g, cus);
  p->window = threads == 1024 && nc <= 32 && has_saved && window_kernel_fits(L, g, p->M) ? 1 : 0;
  p->cache = !gatres_knobs()->fused_nocache &&
             cache_fits(nc, threads, g->max_segment_nodes, g->max_segment_edges_gat, g->max_segment_edges_mean) ? 1 : 0;
  const int tiles = (g->max_segment_nodes + 15) / 16;
  p->part_rows = p->M > 0 ? 16 * ((tiles + p->M - 1) / p->M) : INT32_MAX;
  p->facts = ((g->flags & GATRES_GRAPH_DEG_LE6) ? 0x400 : 0) | (p->part_rows <= 64 ? 0x1000 : 0) |
             (((m->flags & GATRES_MODEL_INFERENCE) && phases == GATRES_PHASE_FORWARD) ? 0x2000 : 0) |
             ((probed && !gatres_knobs()->window_sync_start) ? 0x4000 : 0);
  p->keep = (phases & GATRES_PHASE_FORWARD) && (phases & GATRES_PHASE_BACKWARD) && !gatres_knobs()->fused_no_keep &&
            window_kernel_fits(L, g, p->M, true) ? 1 : 0;
  // every workgroup of a split launch must be resident at once: more segments than that go round by round
  int per_round = g->num_segments;
  if (p->M > 1 && ((g->num_segments + 7) / 8) * 8 * p->M > cus) {
    const int padded = ((g->num_segments + 7) / 8) * 8, fit = (cus / p->M) & ~7;
    const int rounds = fit > 0 ? (padded + fit - 1) / fit : 0;
    per_round = rounds > 0 ? (((padded + rounds - 1) / rounds + 7) / 8) * 8 : 0;        // (equal rounds: 72 segments = 40 + 32)
  }
  p->per_launch = per_round;
  p->launches = per_round > 0 ? (g->num_segments + per_round - 1) / per_round : 0;
  p->grid0 = per_round > 0 ? (int)fused_grid(g->num_segments < per_round ? g->num_segments : per_round, p->M) : 0;
  return per_round > 0 ? 0 : GATRES_E_UNSUPPORTED;
}

static int launch_fused(int nc, const FusedPlan& p, const FusedArgs& a0, const gatres_graph_t* g, hipStream_t st) {
  const int per_round = p.per_launch;
  if (per_round <= 0) return GATRES_E_UNSUPPORTED;
  FusedArgs a = a0;
  for (int s0 = 0; s0 < g->num_segments; s0 += per_round) {
    a.seg0 = s0;
    a.seg_cnt = g->num_segments - s0 < per_round ? g->num_segments - s0 : per_round;
    const unsigned grid = fused_grid(a.seg_cnt, a.M);
    const int rc = p.window ? gatres_fused_launch_window(&a, nc, grid, st)
                            : gatres_fused_launch_whole(&a, nc, p.threads, p.cache, grid, st);
    if (rc != 0) return rc;
  }
  return 0;
}
}  // namespace

// C-ABI ------------------------------------------------------------------------------------------------------

extern "C" int gatres_fused_supported(const gatres_model_t* m, const gatres_graph_t* g) {
  if (!m || !g || g->num_segments <= 0 || !g->seg_ptr) return 0;
  if (!(m->nc >= 4 && m->nc <= 128 && gatres_is_pow2(m->nc))) return 0;
  if (m->act_dtype != GATRES_DTYPE_F32) return 0;        // the per-snapshot kernels are fp32 (the 1e-5 parity path)
  // Wide models (gatres_large, nc = 128): the per-snapshot tables do not fit the LDS, the per-snapshot kernel would
  // run without them at 256 / 512 threads, and the per-op kernels (LDS-staged persistent projections, 256 slabs) are
  // then 1.6-1.8x faster on C-Town batches of 32 .. 128 snapshots.  GATRES_FUSED_WIDE=1 keeps the fused path for them.
  if (m->nc > 32 && !gatres_knobs()->fused_wide) return 0;
  if (g->max_segment_nodes > 4096) return 0;      // beyond this a snapshot should be spread over many CUs
  return nocache_fits(m->nc, threads_for(m->nc), g->max_segment_nodes, g->max_segment_edges_gat, g->max_segment_edges_mean)
             ? 1 : 0;
}

extern "C" int gatres_fused_cus_per_segment(const gatres_model_t* m, const gatres_graph_t* g) {
  Layout L;
  if (!gatres_fused_supported(m, g) || !make_layout_g(m, g, &L)) return 0;
  return fused_split(L, g);
}

// Zero the split-segment barrier state (epochs, XCD words, column counters, error word) of a scratch buffer: what a
// freshly zeroed buffer has.  Only needed after a launch was aborted or the buffer was handed over from elsewhere.
extern "C" int gatres_fused_reset_sync(const gatres_model_t* m, const gatres_graph_t* g, float* scratch, void* stream) {
  if (!m || !g || !scratch) return GATRES_E_BADARG;
  Layout L;
  if (!make_layout_g(m, g, &L)) return GATRES_E_UNSUPPORTED;
  if (fused_nodes_of(g) == 0) return 0;
  if (L.xch_stride > 0) {      // granule tags of an aborted run must not meet a restarted epoch count
    const hipError_t e = hipMemsetAsync(scratch + L.sc_xch, 0, (size_t)g->num_segments * L.xch_stride * 4, gatres_stream(stream));
    if (e != hipSuccess) return (int)e;
  }
  return (int)hipMemsetAsync(scratch + L.sc_flags, 0, (size_t)(L.flag_words + L.col_words) * 4, gatres_stream(stream));
}

extern "C" int gatres_fused_window_kernel(const gatres_model_t* m, const gatres_graph_t* g) {
  Layout L;
  if (!gatres_fused_supported(m, g) || !make_layout_g(m, g, &L)) return 0;
  return window_kernel_fits(L, g, fused_split(L, g)) ? 1 : 0;
}

static std::atomic<int> g_xcd_rr[64];          // per device: 0 = not probed, 1 = no, 2 = workgroups 8 ids apart share an XCD
static int xcd_rr_cached() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
  return g_xcd_rr[dev].load(std::memory_order_acquire) == 2 ? 1 : 0;
}

extern "C" int gatres_fused_plan(const gatres_model_t* m, const gatres_graph_t* g, int32_t phases, int32_t num_cus,
                                 int32_t* out) {
  if (!m || !g || !out) return GATRES_E_BADARG;
  for (int k = 0; k < GATRES_FUSED_PLAN_WORDS; ++k) out[k] = 0;
  Layout L;
  if (!gatres_fused_supported(m, g) || !make_layout_g(m, g, &L)) return GATRES_E_UNSUPPORTED;
  FusedPlan p;
  const int rc = fused_decide(m, g, L, phases, true, num_cus > 0 ? num_cus : device_cus(), xcd_rr_cached() != 0, &p);
  out[GATRES_FUSED_PLAN_PARTS] = p.M;                 out[GATRES_FUSED_PLAN_WINDOW] = p.window;
  out[GATRES_FUSED_PLAN_CACHED] = p.cache;            out[GATRES_FUSED_PLAN_KEEP] = p.keep;
  out[GATRES_FUSED_PLAN_FACTS] = p.facts;             out[GATRES_FUSED_PLAN_LAUNCHES] = p.launches;
  out[GATRES_FUSED_PLAN_PER_LAUNCH] = p.per_launch;   out[GATRES_FUSED_PLAN_GRID] = p.grid0;
  out[GATRES_FUSED_PLAN_THREADS] = p.threads;         out[GATRES_FUSED_PLAN_PART_ROWS] = p.part_rows;
  out[GATRES_FUSED_PLAN_CUS] = p.cus;
  return rc;
}

// Diagnostic: segment 0 of the next fused launches writes a 100 MHz wall-clock stamp at every stage boundary into
// stamps[0..capacity) (device memory).  Pass nullptr to switch it off.
extern "C" int gatres_fused_set_stamps(uint64_t* stamps, int32_t capacity) {
  g_stamps = reinterpret_cast<unsigned long long*>(stamps);
  g_stamp_cap = stamps ? capacity : 0;
  return 0;
}

extern "C" int gatres_fused_prepare_backward(const gatres_model_t* m, const gatres_graph_t* g, const float* params,
                                             float* scratch, void* stream) {
  if (!m || !g || !params || !scratch) return GATRES_E_BADARG;
  Layout L;
  if (!make_layout_g(m, g, &L)) return GATRES_E_UNSUPPORTED;
  return gatres_transpose_conv_weights(params, scratch + L.sc_wt, L.nb, L.nc, stream);
}

extern "C" int gatres_fused_run(const gatres_model_t* m, const gatres_graph_t* g, const float* params,
                                const float* x, const uint8_t* mask, const float* y, float* out, float* g_out,
                                float* loss_part, float* g_x, float* saved, float* scratch, int32_t phases,
                                void* stream) {
  if (!m || !g || !params || !x || !scratch) return GATRES_E_BADARG;
  if (!gatres_fused_supported(m, g)) return GATRES_E_UNSUPPORTED;
  FusedArgs a;
  if (!make_layout_g(m, g, &a.L)) return GATRES_E_UNSUPPORTED;
  if ((phases & GATRES_PHASE_FORWARD) && !out) return GATRES_E_BADARG;
  if ((phases & GATRES_PHASE_LOSS) && (!mask || !y || !out || !g_out || !loss_part)) return GATRES_E_BADARG;
  const int32_t crit_bits = phases & (GATRES_PHASE_LOSS_MAE | GATRES_PHASE_LOSS_SCE);
  if (crit_bits && (!(phases & GATRES_PHASE_LOSS) || crit_bits == (GATRES_PHASE_LOSS_MAE | GATRES_PHASE_LOSS_SCE)))
    return GATRES_E_BADARG;
  if ((phases & GATRES_PHASE_BACKWARD) && (!saved || !g_out)) return GATRES_E_BADARG;
  a.seg_ptr = g->seg_ptr;
  a.rowptr = g->rowptr; a.col = g->col; a.t_rowptr = g->t_rowptr; a.t_eid = g->t_eid; a.t_dst = g->t_dst;
  a.m_rowptr = g->m_rowptr; a.m_col = g->m_col; a.mt_rowptr = g->mt_rowptr; a.mt_dst = g->mt_dst;
  a.N = g->num_nodes;
  a.perm = g->perm;
  a.params = params; a.wt = scratch + a.L.sc_wt;
  a.x = x; a.mask = mask; a.y = y; a.out = out; a.g_out = g_out; a.loss_part = loss_part; a.g_x = g_x;
  a.saved = saved; a.scratch = scratch; a.slabs = scratch + a.L.sc_slabs;
  a.num_segments = g->num_segments;
  a.seg0 = 0; a.seg_cnt = g->num_segments;
  FusedPlan plan;
  (void)fused_decide(m, g, a.L, phases, saved != nullptr, device_cus(), xcd_rr_cached() != 0, &plan);      // (launch_fused refuses)
  a.M = plan.M;
  a.safe_sync = gatres_knobs()->fused_safe_sync;
  // bits 1 / 2 (diagnostic build only, WRONG results): never-wait exchanges; dX epilogues without their global reads
  a.no_halo = gatres_knobs()->fused_no_halo | (gatres_knobs()->xch_nowait ? 2 : 0) | (gatres_knobs()->diag_nomask ? 4 : 0);
  a.sym = (g->flags & GATRES_GRAPH_SYMMETRIC) && !gatres_knobs()->fused_heartbeat ? 1 : 0;
  a.ptab = g->part_tables; a.ptab_m = g->part_tables_m; a.ptab_stride = g->part_tables_stride;
  a.facts = plan.facts;
  a.keep_lds = plan.keep;
  a.flags = reinterpret_cast<unsigned*>(scratch + a.L.sc_flags);
  a.err = reinterpret_cast<int*>(fused_status(scratch, a.L));
  a.part_slabs = scratch + a.L.sc_part_slabs;
  a.SL = make_seg_layout(a.L.nb, a.L.nc, g->max_segment_nodes, g->max_segment_edges_gat);
  a.xch = reinterpret_cast<unsigned long long*>(scratch + a.L.sc_xch);
  a.urec = reinterpret_cast<int*>(scratch + a.L.sc_urec);
  a.XL = make_xch_layout(a.L.nc, g->max_segment_nodes, g->max_segment_edges_gat);
  a.stamps = g_stamps; a.stamp_cap = g_stamp_cap;
  a.phases = (phases & (GATRES_PHASE_FORWARD | GATRES_PHASE_BACKWARD)) | ((phases & GATRES_PHASE_LOSS) ? PH_LOSS : 0);
  a.criterion = crit_bits == GATRES_PHASE_LOSS_MAE ? GATRES_LOSS_MAE : crit_bits == GATRES_PHASE_LOSS_SCE ? GATRES_LOSS_SCE
                                                                                                        : GATRES_LOSS_MSE;
  hipStream_t st = gatres_stream(stream);
  if (a.M > 1) serialize_split_launch(st);
  int rc = launch_fused(m->nc, plan, a, g, st);
  if (rc == 0 && a.M > 1 && !(phases & GATRES_PHASE_BACKWARD)) {      // (a backward launch is followed by gatres_fused_finish)
    hipLaunchKernelGGL(fused_status_kernel, dim3(1), dim3(64), 0, st, reinterpret_cast<unsigned*>(a.err));
    rc = gatres_launch_status();
  }
  return rc;
}

extern "C" int gatres_fused_serialize(void* stream) { return serialize_split_launch(gatres_stream(stream)); }

extern "C" int gatres_probe_xcd_dispatch(void* stream) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
  const int have = g_xcd_rr[dev].load(std::memory_order_acquire);
  if (have != 0) return have == 2 ? 1 : 0;
  hipStream_t st = gatres_stream(stream);
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return 0;      // (not now)
  const int cus = device_cus();
  if (cus < 16 || cus > 4096) { g_xcd_rr[dev].store(1, std::memory_order_release); return 0; }
  unsigned* d = nullptr;
  if (hipMalloc(&d, sizeof(unsigned) * cus) != hipSuccess) return 0;
  std::vector<unsigned> h((size_t)cus, 0xffu);
  bool ok = hipMemsetAsync(d, 0xff, sizeof(unsigned) * cus, st) == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL(xcd_probe_kernel, dim3((unsigned)cus), dim3(1024), 0, st, d);
    ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(st) == hipSuccess &&
         hipMemcpy(h.data(), d, sizeof(unsigned) * cus, hipMemcpyDeviceToHost) == hipSuccess;
  }
  (void)hipFree(d);
  if (!ok) return 0;
  bool rr = true;
  for (int b = 0; b < cus && rr; ++b) rr = (h[b] & 0xfu) == (h[b & 7] & 0xfu) && h[b] != 0xffffffffu;
  g_xcd_rr[dev].store(rr ? 2 : 1, std::memory_order_release);
  return rr ? 1 : 0;
}

extern "C" int64_t gatres_fused_status_offset(const gatres_model_t* m, const gatres_graph_t* g) {
  Layout L;
  if (!gatres_fused_supported(m, g) || !make_layout_g(m, g, &L)) return -1;
  return fused_status_offset(L);
}

extern "C" int gatres_fused_param_grads(const gatres_model_t* m, const gatres_graph_t* g, const float* saved,
                                        float* scratch, void* stream) {
  return gatres_fused_param_grads_ex(m, g, saved, scratch, nullptr, stream);
}
extern "C" __attribute__((visibility("hidden"))) int gatres_fused_param_grads_ex(
    const gatres_model_t* m, const gatres_graph_t* g, const float* saved, float* scratch, const uint64_t* step_counter, void* stream) {
  if (!m || !g || !saved || !scratch) return GATRES_E_BADARG;
  if (!gatres_fused_supported(m, g)) return GATRES_E_UNSUPPORTED;
  ParamGradArgs a;
  if (!make_layout_g(m, g, &a.L)) return GATRES_E_UNSUPPORTED;
  if (a.L.nb == 0) return 0;
  a.seg_ptr = g->seg_ptr; a.saved = saved; a.keep = scratch + a.L.sc_keep; a.slabs = scratch + a.L.sc_slabs;
  a.M = fused_split(a.L, g); a.part_slabs = scratch + a.L.sc_part_slabs;
  a.SL = make_seg_layout(a.L.nb, a.L.nc, g->max_segment_nodes, g->max_segment_edges_gat);
  a.wt = scratch + a.L.sc_wt;
  const dim3 grid((unsigned)(2 * a.L.nb * g->num_segments));
  hipStream_t st = gatres_stream(stream);
  if (m->nc == 16 || m->nc == 32) {
    if (step_counter) {
      unsigned* status = fused_status(scratch, a.L);
      a.step_counter = reinterpret_cast<const unsigned long long*>(step_counter);
      a.status = fused_nodes_of(g) > 0 ? status : nullptr;
      a.snap = fused_status_snapshot(status);
    }
    if (m->nc == 16) hipLaunchKernelGGL((param_grads_reg_kernel<16>), grid, dim3(PGR_THREADS), 0, st, a);
    else             hipLaunchKernelGGL((param_grads_reg_kernel<32>), grid, dim3(PGR_THREADS), 0, st, a);
    const int rc = gatres_launch_status();
    return rc ? rc : (step_counter ? 1 : 0);
  }
  switch (m->nc) {
    case 4: hipLaunchKernelGGL((param_grads_kernel<4, 256>), grid, dim3(256), 0, st, a); break;
    case 8: hipLaunchKernelGGL((param_grads_kernel<8, 256>), grid, dim3(256), 0, st, a); break;
    case 64: hipLaunchKernelGGL((param_grads_kernel<64, 512>), grid, dim3(512), 0, st, a); break;
    case 128: hipLaunchKernelGGL((param_grads_kernel<128, 512>), grid, dim3(512), 0, st, a); break;
    default: return GATRES_E_UNSUPPORTED;
  }
  return gatres_launch_status();
}

// 1 when gatres_fused_param_grads_finish applies: streamed items (nc 16 / 32) in a launch of their own
static bool finish_folds(const gatres_model_t* m, const Layout& L) {
  return (m->nc == 16 || m->nc == 32) && L.nb > 0;
}

extern "C" int gatres_fused_finish_folds(const gatres_model_t* m, const gatres_graph_t* g) {
  Layout L;
  if (!gatres_fused_supported(m, g) || !make_layout_g(m, g, &L)) return 0;
  return finish_folds(m, L) ? 1 : 0;
}

extern "C" int gatres_fused_param_grads_finish(const gatres_model_t* m, const gatres_graph_t* g, const float* saved,
                                               float* scratch, float* grads, const float* loss_part, float* loss,
                                               int32_t do_adam, float* params, float* exp_avg, float* exp_avg_sq,
                                               uint64_t* step_counter, double lr, double beta1, double beta2, double eps,
                                               double weight_decay, const double* hparams, float grad_scale,
                                               int32_t block_lo, int32_t block_hi, void* stream) {
  if (!m || !g || !saved || !scratch || !grads) return GATRES_E_BADARG;
  if (do_adam && (!params || !exp_avg || !exp_avg_sq || !step_counter)) return GATRES_E_BADARG;
  if ((loss_part == nullptr) != (loss == nullptr)) return GATRES_E_BADARG;
  if (!gatres_fused_supported(m, g)) return GATRES_E_UNSUPPORTED;
  ParamGradArgs a;
  if (!make_layout_g(m, g, &a.L)) return GATRES_E_UNSUPPORTED;
  if (!finish_folds(m, a.L)) return GATRES_E_UNSUPPORTED;
  if (block_lo < 0 || block_hi > a.L.nb || block_lo >= block_hi) return GATRES_E_BADARG;
  if (do_adam && (block_lo != 0 || block_hi != a.L.nb)) return GATRES_E_BADARG;      // (the step is counted per launch)
  a.seg_ptr = g->seg_ptr; a.saved = saved; a.keep = scratch + a.L.sc_keep; a.slabs = scratch + a.L.sc_slabs;
  a.M = fused_split(a.L, g); a.part_slabs = scratch + a.L.sc_part_slabs;
  a.SL = make_seg_layout(a.L.nb, a.L.nc, g->max_segment_nodes, g->max_segment_edges_gat);
  a.wt = scratch + a.L.sc_wt;
  FinishArgs f;
  f.u = update_args_of(params, nullptr, exp_avg, exp_avg_sq, step_counter, a.L.P, lr, beta1, beta2, eps, weight_decay, hparams,
                       grad_scale);
  f.u.wt = do_adam ? scratch + a.L.sc_wt : nullptr;      // (its blocks and width: a.L, NC)
  f.grads = grads; f.loss_part = loss_part; f.loss = loss; f.num_loss = g->num_segments * a.M; f.do_adam = do_adam ? 1 : 0;
  f.status = fused_nodes_of(g) > 0 ? fused_status(scratch, a.L) : nullptr;
  f.colcnt = reinterpret_cast<unsigned*>(scratch + a.L.sc_flags + a.L.flag_words);
  f.S = g->num_segments; f.b_lo = block_lo; f.b_hi = block_hi; f.final_launch = block_lo == 0 ? 1 : 0;
  const dim3 grid((unsigned)(2 * (block_hi - block_lo) * g->num_segments));
  hipStream_t st = gatres_stream(stream);
  if (m->nc == 16) hipLaunchKernelGGL((param_grads_finish_kernel<16>), grid, dim3(PGR_THREADS), 0, st, a, f);
  else             hipLaunchKernelGGL((param_grads_finish_kernel<32>), grid, dim3(PGR_THREADS), 0, st, a, f);
  return gatres_launch_status();
}

extern "C" int gatres_fused_finish(const gatres_model_t* m, const gatres_graph_t* g, float* scratch, float* grads,
                                   const float* loss_part, float* loss, int32_t do_adam, float* params,
                                   float* exp_avg, float* exp_avg_sq, uint64_t* step_counter, double lr, double beta1,
                                   double beta2, double eps, double weight_decay, float grad_scale, void* stream) {
  return gatres_fused_finish_hp(m, g, scratch, grads, loss_part, loss, do_adam, params, exp_avg, exp_avg_sq, step_counter,
                                lr, beta1, beta2, eps, weight_decay, nullptr, grad_scale, nullptr, 0, 0.0, 0, nullptr, stream);
}

extern "C" int gatres_fused_finish_hp(const gatres_model_t* m, const gatres_graph_t* g, float* scratch, float* grads,
                                      const float* loss_part, float* loss, int32_t do_adam, float* params,
                                      float* exp_avg, float* exp_avg_sq, uint64_t* step_counter, double lr, double beta1,
                                      double beta2, double eps, double weight_decay, const double* hparams,
                                      float grad_scale, const int32_t* mask_node_ptr, int32_t mask_graphs, double mask_rate,
                                      uint64_t mask_seed, uint8_t* mask_next, void* stream) {
  // (mask_next through the public entry: the caller vouches that gatres_fused_param_grads ran under gatres_train_step's
  //  sequence -- the snapshot it reads is only written there; without one the sampling tail is refused, and the other
  //  mask_* arguments have nothing to say)
  if (mask_next) return GATRES_E_UNSUPPORTED;
  return gatres_fused_finish_ex(m, g, scratch, grads, loss_part, loss, do_adam,
                                update_args_of(params, nullptr, exp_avg, exp_avg_sq, step_counter, 0, lr, beta1, beta2, eps,
                                               weight_decay, hparams, grad_scale), 0, stream);
}

// The slab sum's arguments for a plan and its scratch (do_adam, use_snap and the AutoClip words: the caller's)
static bool slab_sum_args(const gatres_model_t* m, const gatres_graph_t* g, float* scratch, float* grads, const float* loss_part,
                          float* loss, Layout* L, SlabSumArgs* r) {
  if (!make_layout_g(m, g, L)) return false;
  *r = SlabSumArgs{};
  r->slabs = scratch + L->sc_slabs; r->num_slabs = g->num_segments; r->num_loss = g->num_segments * fused_split(*L, g);
  r->stride = L->slab_stride;
  r->grads = grads; r->loss_part = loss_part; r->loss = loss;
  r->reduce_blocks = (int)((L->P + 255) / 256);
  r->status = fused_nodes_of(g) > 0 ? fused_status(scratch, *L) : nullptr;
  return true;
}

extern "C" __attribute__((visibility("hidden"))) int gatres_fused_finish_ex(
    const gatres_model_t* m, const gatres_graph_t* g, float* scratch, float* grads, const float* loss_part, float* loss,
    int32_t do_adam, const UpdateArgs& u, int32_t use_snap, void* stream) {
  if (!m || !g || !scratch || !grads) return GATRES_E_BADARG;
  if (u.mask_next && !use_snap) return GATRES_E_BADARG;
  if (u.mask_next && (!do_adam || !u.mask_node_ptr || u.mask_graphs <= 0 || !(u.mask_rate >= 0.0 && u.mask_rate <= 1.0)))
    return GATRES_E_BADARG;
  if (do_adam && (!u.p || !u.m || !u.v || !u.step_counter)) return GATRES_E_BADARG;
  if ((loss_part == nullptr) != (loss == nullptr)) return GATRES_E_BADARG;
  Layout L;
  SlabSumArgs r;
  if (!slab_sum_args(m, g, scratch, grads, loss_part, loss, &L, &r)) return GATRES_E_UNSUPPORTED;
  r.do_adam = do_adam; r.use_snap = (use_snap && do_adam) ? 1 : 0;
  UpdateArgs a = u;
  a.count = L.P;
  a.wt = do_adam ? scratch + L.sc_wt : nullptr; a.nb = L.nb; a.nc = L.nc;
  a.mask_snap = fused_status_snapshot(fused_status(scratch, L));
  const unsigned grid = (unsigned)(r.reduce_blocks + (a.mask_next ? a.mask_graphs * MASK_WGS_UPDATE : 0));
  hipLaunchKernelGGL(reduce_adam_kernel<false>, dim3(grid), dim3(256), 0, gatres_stream(stream), a, r);
  return gatres_launch_status();
}

// The slab sum of the clipped step: gatres_fused_finish_ex without Adam, as the norm launch of AutoClip
extern "C" __attribute__((visibility("hidden"))) int gatres_fused_finish_norm_ex(
    const gatres_model_t* m, const gatres_graph_t* g, float* scratch, float* grads, const float* loss_part, float* loss,
    const UpdateArgs& u, const gatres_autoclip_t* ac, int32_t* num_partials, void* stream) {
  if (!m || !g || !scratch || !grads || !u.step_counter || !ac || !ac->partials || !ac->ctl || !num_partials) return GATRES_E_BADARG;
  if ((loss_part == nullptr) != (loss == nullptr)) return GATRES_E_BADARG;
  Layout L;
  SlabSumArgs r;
  if (!slab_sum_args(m, g, scratch, grads, loss_part, loss, &L, &r)) return GATRES_E_UNSUPPORTED;
  if (r.reduce_blocks > ac->partials_cap) return GATRES_E_BADARG;
  r.ac_partials = ac->partials; r.ac_ctl = reinterpret_cast<unsigned long long*>(ac->ctl);
  UpdateArgs a{};
  a.step_counter = u.step_counter; a.count = L.P; a.grad_scale = u.grad_scale;
  hipLaunchKernelGGL(reduce_adam_kernel<true>, dim3((unsigned)r.reduce_blocks), dim3(256), 0, gatres_stream(stream), a, r);
  *num_partials = r.reduce_blocks;
  return gatres_launch_status();
}

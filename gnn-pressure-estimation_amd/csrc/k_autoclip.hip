// AutoClip gradient-norm clipping in front of Adam (reference utils/gradient_clipping.py, train.py:186-187): the norm launch
// and the update launch, and the C-ABI entry points (include/gatres.h: gatres_autoclip_*).
//
// An update is two launches.  The NORM launch leaves per-workgroup fp64 sum-of-squares partials of g = grads * grad_scale and
// snapshots the history count, the step count and the drop decision (block 0).  On the fused path that launch is the slab
// reduction itself (reduce_adam_kernel<true>, k_fused_host.hip); elsewhere the gradient is complete already and
// autoclip_norm_kernel below reads it.  The UPDATE launch, in every workgroup redundantly: sums the partials in a fixed
// order (n), finds the rank of n in the sorted history (rounds of a 256-way search: no atomics, no spinning), forms the
// percentile c and coef = min(1, c / (n + 1e-6)) in double (NaN where the norm is not finite, as torch's clamp), then
// applies Adam to its slice of the parameters with the clipped gradient and writes its slice of the history's next sorted copy.  Block 0 appends n to the log and stores the
// counts; every other workgroup reads the snapshot only, so nothing in the launch waits for anything.
#include "gatres_common.h"
#include "k_autoclip.h"
#include "k_mask.h"
#include "k_update.h"

namespace {

constexpr int AC_NORM_MAX_BLOCKS = 256;
constexpr int AC_UPDATE_MAX_BLOCKS = 512;

__global__ __launch_bounds__(256) void autoclip_norm_kernel(const float* __restrict__ g, long long count, float grad_scale,
                                                            double* __restrict__ partials, unsigned long long* __restrict__ ctl,
                                                            const unsigned long long* __restrict__ step_counter, int drop_nan) {
  __shared__ double lds4[4];
  double s = 0.0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
    const double x = (double)(g[i] * grad_scale);
    s += x * x;
  }
  s = ac_block_sum(s, lds4);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = s;
    // (drop_nan: the data-parallel Adam phase of the fused path -- a faulted replica marks g[0] NaN, gatres_fused_finish)
    if (blockIdx.x == 0) ac_snapshot(ctl, step_counter, drop_nan && g[0] != g[0]);
  }
}

struct AutoClipUpdate {
  UpdateArgs u;
  int update_blocks;
  int num_partials;
  const double* partials;
  double* log;
  double* sorted0;
  double* sorted1;
  unsigned long long* ctl;
  double* norm_out;
  double* clip_out;
  double* coef_out;
  long long capacity;
  double percentile;
};

// x sorts before the new norm n: np.sort order with NaN last (a NaN n goes behind everything)
__device__ __forceinline__ bool ac_before(double x, double n) { return x < n || n != n; }

// number of threads of the workgroup with pred set (lds_cnt: __shared__ int[4])
__device__ __forceinline__ int ac_block_count(bool pred, int* lds_cnt) {
  const unsigned long long b = __ballot(pred);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds_cnt[threadIdx.x >> 6] = __popcll(b);
  __syncthreads();
  return lds_cnt[0] + lds_cnt[1] + lds_cnt[2] + lds_cnt[3];
}

__global__ __launch_bounds__(256) void autoclip_adam_kernel(const AutoClipUpdate a) {
  __shared__ double lds4[4];
  __shared__ int lds_cnt[4];
  __shared__ float s_step_size, s_bc2_sqrt;
  const int tid = threadIdx.x;
  const unsigned long long cnt = a.ctl[AC_SNAP_COUNT], step = a.ctl[AC_SNAP_STEP];
  const bool overflow = cnt >= (unsigned long long)a.capacity;
  const bool drop = a.ctl[AC_SNAP_DROP] != 0ULL || overflow;
  if (a.u.mask_next && (int)blockIdx.x >= a.update_blocks) {       // (the step count this update leaves behind)
    const int mb = (int)blockIdx.x - a.update_blocks;
    mask_sample_graph<256, MASK_WGS_UPDATE>(a.u.mask_node_ptr, a.u.mask_rate, a.u.mask_seed, step + (drop ? 0ULL : 1ULL),
                                            a.u.mask_next, mb / MASK_WGS_UPDATE, mb % MASK_WGS_UPDATE);
    return;
  }
  if (drop) {                    // no update, no step count, no history entry, outputs untouched
    if (blockIdx.x == 0 && tid == 0) {
      if (overflow) a.ctl[AC_OVERFLOW] = 1ULL;
      else if (a.u.drop_count) atomicAdd(a.u.drop_count, 1u);
    }
    return;
  }
  double lr = a.u.lr, b1 = a.u.b1, b2 = a.u.b2, eps = a.u.eps, wd = a.u.wd;
  if (a.u.hp) { lr = a.u.hp[0]; b1 = a.u.hp[1]; b2 = a.u.hp[2]; eps = a.u.hp[3]; wd = a.u.hp[4]; }
  if (tid == 0) {
    const unsigned long long t = step + 1ULL;
    s_step_size = (float)(lr / (1.0 - gatres_powi(b1, t)));
    s_bc2_sqrt = (float)sqrt(1.0 - gatres_powi(b2, t));
  }
  // n: the partials in a fixed order (the same bits in every workgroup)
  double s = 0.0;
  for (int j = tid; j < a.num_partials; j += 256) s += a.partials[j];
  const double n = sqrt(ac_block_sum(s, lds4));
  // r = entries of the current sorted copy A that sort before n.  The answer lies in [lo, hi]; a round samples 256 equally
  // spaced entries, whose predicates form a prefix, and keeps the gap behind the last one that is set.
  const double* A = (cnt & 1ULL) ? a.sorted1 : a.sorted0;
  double* B = (cnt & 1ULL) ? a.sorted0 : a.sorted1;
  long long lo = 0, hi = (long long)cnt;
  while (hi - lo > 256) {
    const long long stride = (hi - lo + 255) / 256, pos = lo + (long long)tid * stride;
    const int k = ac_block_count(pos < hi && ac_before(A[pos], n), lds_cnt);
    if (k == 0) {
      hi = lo;
    } else {
      const long long nlo = lo + (long long)(k - 1) * stride + 1, nhi = lo + (long long)k * stride;
      lo = nlo;
      hi = nhi < hi ? nhi : hi;
    }
  }
  const long long r = lo + ac_block_count(lo + tid < hi && ac_before(A[lo + tid], n), lds_cnt);
  // the next sorted copy: A with n inserted at r
  const long long t = (long long)cnt + 1;
  auto sorted_at = [&](long long i) -> double { return i < r ? A[i] : (i == r ? n : A[i - 1]); };
  // c = np.percentile(history, percentile): numpy's "linear" method, virtual index (t - 1) * q, its _lerp
  const double h = (double)(t - 1) * (a.percentile / 100.0);
  long long i0 = (long long)floor(h);
  if (i0 > t - 1) i0 = t - 1;
  if (i0 < 0) i0 = 0;
  const long long i1 = i0 + 1 < t ? i0 + 1 : t - 1;
  const double gam = h - (double)i0, va = sorted_at(i0), vb = sorted_at(i1), diff = vb - va;
  const double c = gam >= 0.5 ? vb - diff * (1.0 - gam) : va + diff * gam;
  // torch.nn.utils.clip_grad_norm_(params, c): always multiplies, also by n / (n + 1e-6) when c >= n.  Its clamp(max=1) lets a
  // NaN quotient through -- a norm that is not finite (an inf or NaN gradient entry) makes EVERY entry NaN, and Adam then every
  // parameter -- which fmin(1, q) would turn into 1: an unclipped update of the finite entries
  const double q = c / (n + 1e-6);
  const double coef_d = q > 1.0 ? 1.0 : q;
  const float coef = (float)coef_d;
  if (blockIdx.x == 0 && tid == 0) {     // (nobody in this launch reads these words: the workgroups read the snapshot)
    a.log[cnt] = n;
    a.norm_out[0] = n;
    a.clip_out[0] = c;
    a.coef_out[0] = coef_d;
    a.ctl[AC_COUNT] = (unsigned long long)t;
    a.u.step_counter[0] = step + 1ULL;
  }
  __syncthreads();                       // (s_step_size, s_bc2_sqrt)
  const long long gstride = (long long)a.update_blocks * 256;
  for (long long i = (long long)blockIdx.x * 256 + tid; i < t; i += gstride) B[i] = sorted_at(i);
  // Adam on the clipped gradient: adam_kernel's arithmetic (k_misc.hip) with the one multiplication in front of weight decay
  for (long long idx = (long long)blockIdx.x * 256 + tid; idx < a.u.count; idx += gstride) {
    const float pv = a.u.p[idx];
    float gv = a.u.g[idx] * a.u.grad_scale;
    gv = gv * coef;
    gv = gv + (float)wd * pv;
    float mv = a.u.m[idx];
    mv = mv + (float)(1.0 - b1) * (gv - mv);
    const float vv = (float)b2 * a.u.v[idx] + (float)(1.0 - b2) * gv * gv;
    const float denom = sqrtf(vv) / s_bc2_sqrt + (float)eps;
    const float pn = pv + (-s_step_size * mv) / denom;
    a.u.p[idx] = pn;
    a.u.m[idx] = mv;
    a.u.v[idx] = vv;
    if (a.u.wt) {                // keep the fused kernels' transposed conv weights current (transpose_conv_weights_kernel's layout)
      const long long nc = a.u.nc, per = 2LL * nc * nc, stride = 9LL * nc + 2 * per, off = idx - 2LL * nc;
      if (off >= 0 && off < (long long)a.u.nb * stride) {
        const long long b = off / stride, o = off % stride;
        if (o >= 6LL * nc && o < 6LL * nc + per) {                        // W1 [2nc][nc] -> [nc][2nc]
          const long long e = o - 6LL * nc, row = e / nc, col = e % nc;
          a.u.wt[b * 2 * per + col * 2 * nc + row] = pn;
        } else if (o >= 9LL * nc + per) {                                 // W2 [nc][2nc] -> [2nc][nc]
          const long long e = o - 9LL * nc - per, row = e / (2 * nc), col = e % (2 * nc);
          a.u.wt[b * 2 * per + per + col * nc + row] = pn;
        }
      }
    }
  }
}

bool ac_valid(const gatres_autoclip_t* ac) {
  return ac && ac->log && ac->sorted[0] && ac->sorted[1] && ac->sorted[0] != ac->sorted[1] && ac->ctl && ac->partials &&
         ac->norm_out && ac->clip_out && ac->coef_out && ac->capacity > 0 && ac->partials_cap > 0 &&
         ac->percentile >= 0.0 && ac->percentile <= 100.0;
}

}  // namespace

extern "C" int32_t gatres_autoclip_partials(int64_t count) {
  return count <= 0 ? 0 : (int32_t)((count + 255) / 256);
}

extern "C" __attribute__((visibility("hidden"))) int gatres_autoclip_norm_ex(const UpdateArgs& u, const gatres_autoclip_t* ac,
                                                                             int32_t* num_partials, void* stream) {
  if (!u.g || !u.step_counter || u.count <= 0 || !ac_valid(ac) || !num_partials) return GATRES_E_BADARG;
  const long long need = (u.count + 255) / 256;
  const int blocks = (int)(need < AC_NORM_MAX_BLOCKS ? need : AC_NORM_MAX_BLOCKS);
  if (blocks > ac->partials_cap) return GATRES_E_BADARG;
  hipLaunchKernelGGL(autoclip_norm_kernel, dim3((unsigned)blocks), dim3(256), 0, gatres_stream(stream), u.g, u.count,
                     u.grad_scale, ac->partials, reinterpret_cast<unsigned long long*>(ac->ctl), u.step_counter,
                     u.drop_count ? 1 : 0);
  *num_partials = blocks;
  return gatres_launch_status();
}

extern "C" __attribute__((visibility("hidden"))) int gatres_autoclip_update_ex(const UpdateArgs& u, const gatres_autoclip_t* ac,
                                                                               int32_t num_partials, void* stream) {
  if (!u.p || !u.g || !u.m || !u.v || !u.step_counter || u.count <= 0 || !ac_valid(ac)) return GATRES_E_BADARG;
  if (num_partials <= 0 || num_partials > ac->partials_cap) return GATRES_E_BADARG;
  const bool sample = u.mask_next && u.mask_node_ptr && u.mask_graphs > 0;
  const long long need = (u.count + 255) / 256;
  const int ub = (int)(need < AC_UPDATE_MAX_BLOCKS ? need : AC_UPDATE_MAX_BLOCKS);
  AutoClipUpdate a;
  a.u = u;
  if (!sample) { a.u.mask_node_ptr = nullptr; a.u.mask_next = nullptr; }
  a.update_blocks = ub;
  a.num_partials = num_partials; a.partials = ac->partials;
  a.log = ac->log; a.sorted0 = ac->sorted[0]; a.sorted1 = ac->sorted[1];
  a.ctl = reinterpret_cast<unsigned long long*>(ac->ctl);
  a.norm_out = ac->norm_out; a.clip_out = ac->clip_out; a.coef_out = ac->coef_out;
  a.capacity = ac->capacity; a.percentile = ac->percentile;
  hipLaunchKernelGGL(autoclip_adam_kernel, dim3((unsigned)(ub + (sample ? u.mask_graphs * MASK_WGS_UPDATE : 0))), dim3(256), 0,
                     gatres_stream(stream), a);
  return gatres_launch_status();
}

extern "C" int gatres_autoclip_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                                         uint64_t* step_counter, int64_t count, double lr, double beta1, double beta2,
                                         double eps, double weight_decay, float grad_scale, const gatres_autoclip_t* ac,
                                         void* stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || !step_counter || count <= 0 || !ac_valid(ac)) return GATRES_E_BADARG;
  const UpdateArgs u = update_args_of(params, grads, exp_avg, exp_avg_sq, step_counter, count, lr, beta1, beta2, eps,
                                      weight_decay, nullptr, grad_scale);
  int32_t np = 0;
  int rc = gatres_autoclip_norm_ex(u, ac, &np, stream);
  if (rc) return rc;
  return gatres_autoclip_update_ex(u, ac, np, stream);
}

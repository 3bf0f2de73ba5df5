// The reference's per-epoch view into a deep network (train.py:476-504 with --log_gradient) on the device:
//   gatres_grad_flow      get_gradient_norm(model, 2) (utils/auxil.py:295-313) on the flat fp32 gradient -- the L2 norm of every
//                         parameter tensor of the blocks, and the norm of those norms;
//   gatres_mean_abs_diff  torch.abs(out - first_out).mean(), the "model update" of the epoch's last training batch.
//
// Both are fixed-order fp64 reductions without atomics: the same bits on every run.  A tensor is summed by ONE workgroup --
// thread i adds elements i, i + T, i + 2T, ... in that order, the waves reduce by a fixed butterfly, thread 0 adds the wave
// partials in wave order -- so the sum's association depends on the tensor's length alone, never on where the tensor lies or on
// which workgroup takes it.  gatres_grad_flow is one launch of 8 * num_blocks + 1 workgroups: workgroup t forms tensor t's norm,
// the last one forms EVERY tensor's sum of squares again (the same function on the same data: the same bits) and from them the
// total.  That costs one workgroup a pass over the blocks' gradient (gatres_small: 260 KB) once per epoch, and saves a second
// launch, a partials buffer or a ticket counter -- the entry point has none of them to offer.
#include "gatres_common.h"

namespace {

constexpr int GF_T = 1024;
constexpr int GF_WAVES = GF_T / GATRES_WAVE;
constexpr int GF_U = 8;                // strides per trip of the element loops (loads in flight per thread)

// Sum of v over the workgroup, the same association on every run; every thread gets the result.  `lds`: GF_WAVES + 1 doubles.
__device__ __forceinline__ double gf_block_sum(double v, double* lds) {
#pragma unroll
  for (int off = GATRES_WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
  const int lane = threadIdx.x % GATRES_WAVE, wave = threadIdx.x / GATRES_WAVE;
  // (a second call may write here at once: thread 0 read the wave partials before the previous call's last barrier, and the
  //  previous result is overwritten only behind this call's first barrier, which every thread reaches after reading it)
  if (lane == 0) lds[wave] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int w = 0; w < GF_WAVES; ++w) s += lds[w];
    lds[GF_WAVES] = s;
  }
  __syncthreads();
  return lds[GF_WAVES];
}

// sum_i (double)g[i]^2 over n floats.  The product of two fp32 values is exact in fp64.
__device__ __forceinline__ double gf_sumsq(const float* __restrict__ g, long long n, double* lds) {
  double a = 0.0;
  for (long long i0 = threadIdx.x; i0 < n; i0 += (long long)GF_U * GF_T) {
    float v[GF_U];
#pragma unroll
    for (int u = 0; u < GF_U; ++u) {
      const long long i = i0 + (long long)u * GF_T;
      v[u] = i < n ? g[i] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < GF_U; ++u)     // (in stride order: the same association as a plain loop)
      if (i0 + (long long)u * GF_T < n) a += (double)v[u] * (double)v[u];
  }
  return gf_block_sum(a, lds);
}

// Tensor t of the blocks' part of the flat parameter layout (gatres.h): its first float and its length.  Per block:
// conv1.att_src, conv1.att_dst, conv1.bias [2nc each], conv1.lin.weight [2nc x nc], conv2.att_src, conv2.att_dst, conv2.bias
// [nc each], conv2.lin.weight [nc x 2nc] -- the order of named_parameters().
__device__ __forceinline__ void gf_tensor(int t, int nc, long long* first, long long* count) {
  const long long c = nc, w = 2LL * c * c;
  const int b = t >> 3, k = t & 7;
  long long o, n;
  if (k < 3) { o = 2 * c * k; n = 2 * c; }
  else if (k == 3) { o = 6 * c; n = w; }
  else if (k < 7) { o = 6 * c + w + c * (k - 4); n = c; }
  else { o = 9 * c + w; n = w; }
  *first = 2 * c + (long long)b * (9 * c + 2 * w) + o;
  *count = n;
}

// factor: |scale|
__global__ __launch_bounds__(GF_T) void grad_flow_kernel(const float* __restrict__ grads, int num_tensors, int nc, double factor,
                                                         const double* __restrict__ coef, double* __restrict__ out) {
  __shared__ double lds[GF_WAVES + 1];
  const double c = coef ? coef[0] : 1.0;
  const int wg = blockIdx.x;
  long long first, count;
  if (wg < num_tensors) {
    gf_tensor(wg, nc, &first, &count);
    const double s = gf_sumsq(grads + first, count, lds);
    if (threadIdx.x == 0) out[1 + wg] = sqrt(s) * factor * c;
    return;
  }
  double total = 0.0;                  // sum_t sumsq_t in tensor order (every thread holds the same value)
  for (int t = 0; t < num_tensors; ++t) {
    gf_tensor(t, nc, &first, &count);
    total += gf_sumsq(grads + first, count, lds);
  }
  if (threadIdx.x == 0) out[0] = sqrt(total) * factor * c;
}

__global__ __launch_bounds__(GF_T) void mean_abs_diff_kernel(const float* __restrict__ a, const float* __restrict__ b, long long n,
                                                             double* __restrict__ out) {
  __shared__ double lds[GF_WAVES + 1];
  double s = 0.0;
  for (long long i0 = threadIdx.x; i0 < n; i0 += (long long)GF_U * GF_T) {
    float va[GF_U], vb[GF_U];
#pragma unroll
    for (int u = 0; u < GF_U; ++u) {
      const long long i = i0 + (long long)u * GF_T;
      va[u] = i < n ? a[i] : 0.f;
      vb[u] = i < n ? b[i] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < GF_U; ++u)     // difference and absolute value in fp32, as torch forms torch.abs(out - first_out)
      if (i0 + (long long)u * GF_T < n) s += (double)fabsf(__fsub_rn(va[u], vb[u]));
  }
  s = gf_block_sum(s, lds);
  if (threadIdx.x == 0) out[0] = s / (double)n;
}

}  // namespace

extern "C" int32_t gatres_grad_flow_count(int32_t num_blocks, int32_t nc) {
  (void)nc;
  return num_blocks <= 0 ? 0 : 8 * num_blocks;
}

extern "C" int gatres_grad_flow(const gatres_model_t* m, const float* grads, double scale, const double* coef, double* out,
                                void* stream) {
  if (!m || !grads || !out || m->num_blocks <= 0 || m->num_blocks > (1 << 24)) return GATRES_E_BADARG;
  if (m->nc < 4 || m->nc > 128 || !gatres_is_pow2(m->nc)) return GATRES_E_UNSUPPORTED;
  const int T = 8 * m->num_blocks;
  hipLaunchKernelGGL(grad_flow_kernel, dim3(T + 1), dim3(GF_T), 0, gatres_stream(stream), grads, T, (int)m->nc, fabs(scale), coef,
                     out);
  return gatres_launch_status();
}

extern "C" int gatres_mean_abs_diff(const float* a, const float* b, int64_t n, double* out, void* stream) {
  if (!a || !b || !out || n <= 0) return GATRES_E_BADARG;
  hipLaunchKernelGGL(mean_abs_diff_kernel, dim3(1), dim3(GF_T), 0, gatres_stream(stream), a, b, (long long)n, out);
  return gatres_launch_status();
}

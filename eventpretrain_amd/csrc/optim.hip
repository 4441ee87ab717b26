// K21: fused multi-tensor AdamW (torch.optim.AdamW semantics, main_pretrain.py:341-343) and the global gradient
// norm (utils/misc.py:303-315). One launch covers every parameter: a host-built chunk table maps each workgroup
// to (tensor, offset); weight decay / lr scale are per tensor. The step also writes the bf16 shadow of each weight
// that the next forward's MFMA GEMMs read, so no separate cast pass touches the 112 M parameters.
// Gradient clipping (torch.nn.utils.clip_grad_norm_, utils/misc.py:289-290) stays on the device: evp_grad_clip_multi
// reads every gradient once (16 B per lane), reduces wave -> LDS -> one partial per chunk -> one workgroup, and the thread
// that finishes the reduction multiplies the coefficient into dev_hyper[2], which adamw_kernel applies as it reads each
// gradient. No pass writes the gradients, no float atomics (bit-identical from replay to replay), no host decision:
// the clipped step can live in a captured HIP graph.
// Skipping the update on a non-finite gradient (GradScaler.step, utils/misc.py:290) is the same single pass: evp_grad_guard_multi
// tests every element it sums, its final stage leaves the verdict and Adam's applied-step count in a device int64 table, and
// evp_adamw_guarded_multi returns before it touches anything when the verdict says skip.
#include "evp_common.h"

namespace {

struct AdamArgs {
  float *const *params; const float *const *grads; float *const *exp_avg; float *const *exp_avg_sq;
  uint16_t *const *lp; const int64_t *numel; const float *wd; const float *lr_scale;
  const int32_t *chunk_tensor; const int64_t *chunk_offset; int chunk_elems;
  float lr, beta1, beta2, eps, bc1, bc2_sqrt, grad_scale;
  const float *dev_hyper;  // optional device-resident {bc1, bc2_sqrt, grad_scale, lr_mult}: graph-replay safe
  const int64_t *guard;    // optional verdict of evp_grad_guard_multi: guard[0] != 0 = skip this step (null: always update)
};

__global__ __launch_bounds__(256) void adamw_kernel(const AdamArgs a) {
  if (a.guard && a.guard[0] != 0) return;      // uniform across the workgroup: a skipped step writes nothing at all
  const int t = a.chunk_tensor[blockIdx.x];
  const int64_t off = a.chunk_offset[blockIdx.x];
  const int64_t n = a.numel[t];
  int64_t cnt = n - off; if (cnt > a.chunk_elems) cnt = a.chunk_elems;
  float *p = a.params[t] + off; const float *g = a.grads[t] + off;
  float *m = a.exp_avg[t] + off; float *v = a.exp_avg_sq[t] + off;
  uint16_t *lp = a.lp && a.lp[t] ? a.lp[t] + off : nullptr;
  float bc1 = a.bc1, bc2_sqrt = a.bc2_sqrt, grad_scale = a.grad_scale, lr_mult = 1.0f;
  if (a.dev_hyper) { bc1 = a.dev_hyper[0]; bc2_sqrt = a.dev_hyper[1]; grad_scale = a.dev_hyper[2]; lr_mult = a.dev_hyper[3]; }
  const float lr = a.lr * lr_mult * a.lr_scale[t], wd = a.wd[t];
  const float decay = 1.0f - lr * wd, step_size = lr / bc1;
  const bool vec = ((off & 3) == 0);
  const int64_t c4 = vec ? (cnt >> 2) : 0;
  for (int64_t i = threadIdx.x; i < c4; i += 256) {
    float4 pp = reinterpret_cast<float4 *>(p)[i];
    float4 gg = reinterpret_cast<const float4 *>(g)[i];
    float4 mm = reinterpret_cast<float4 *>(m)[i];
    float4 vv = reinterpret_cast<float4 *>(v)[i];
    float *P = &pp.x, *G = &gg.x, *M = &mm.x, *V = &vv.x;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float gr = G[e] * grad_scale;
      P[e] *= decay;
      M[e] = a.beta1 * M[e] + (1.0f - a.beta1) * gr;
      V[e] = a.beta2 * V[e] + (1.0f - a.beta2) * gr * gr;
      const float denom = sqrtf(V[e]) / bc2_sqrt + a.eps;
      P[e] -= step_size * (M[e] / denom);
    }
    reinterpret_cast<float4 *>(p)[i] = pp;
    reinterpret_cast<float4 *>(m)[i] = mm;
    reinterpret_cast<float4 *>(v)[i] = vv;
    if (lp) reinterpret_cast<uint2 *>(lp)[i] = pack4_bf16(pp);
  }
  for (int64_t i = c4 * 4 + threadIdx.x; i < cnt; i += 256) {
    const float gr = g[i] * grad_scale;
    float pe = p[i] * decay;
    const float me = a.beta1 * m[i] + (1.0f - a.beta1) * gr;
    const float ve = a.beta2 * v[i] + (1.0f - a.beta2) * gr * gr;
    pe -= step_size * (me / (sqrtf(ve) / bc2_sqrt + a.eps));
    p[i] = pe; m[i] = me; v[i] = ve;
    if (lp) lp[i] = f32_to_bf16(pe);
  }
}

__global__ __launch_bounds__(256) void sumsq_chunks(const float *const *grads, const int64_t *numel, const int32_t *chunk_tensor,
                                                    const int64_t *chunk_offset, int chunk_elems, float *part) {
  __shared__ float red[16];
  const int t = chunk_tensor[blockIdx.x];
  const int64_t off = chunk_offset[blockIdx.x];
  int64_t cnt = numel[t] - off; if (cnt > chunk_elems) cnt = chunk_elems;
  const float *g = grads[t] + off;
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < cnt; i += 256) s += g[i] * g[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
__global__ __launch_bounds__(1024) void sqrt_sum(const float *part, int n, float *out) {
  __shared__ float red[16];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) s += part[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) out[0] = sqrtf(s);
}

// Sum of squares of one chunk, 16 B per lane. The split is by ADDRESS (a gradient may be a view that starts off a 16-byte
// boundary): scalar head up to the boundary, float4 body, scalar tail. Fixed summation order: the partial is reproducible.
// GUARD: every element read is also tested for finiteness (exponent bits all set = Inf or NaN); a chunk that holds such an element
// writes NaN as its partial, any other chunk its sum -- +Inf when finite values overflowed, which is not a reason to skip.
__device__ __forceinline__ int nonfinite_bits(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

template <bool GUARD>
__global__ __launch_bounds__(256) void sumsq_chunks_v4(const float *const *grads, const int64_t *numel, const int32_t *chunk_tensor,
                                                       const int64_t *chunk_offset, int chunk_elems, float *part) {
  __shared__ float red[16];
  const int t = chunk_tensor[blockIdx.x];
  const int64_t off = chunk_offset[blockIdx.x];
  int64_t cnt = numel[t] - off; if (cnt > chunk_elems) cnt = chunk_elems;
  if (cnt < 0) cnt = 0;
  const float *g = grads[t] + off;
  int64_t head = (int64_t)(((16u - (unsigned)((uintptr_t)g & 15u)) & 15u) >> 2);
  if (head > cnt) head = cnt;
  const int64_t c4 = (cnt - head) >> 2;
  const float4 *g4 = reinterpret_cast<const float4 *>(g + head);
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int bad = 0;
#pragma unroll 4
  for (int64_t i = threadIdx.x; i < c4; i += 256) {
    const float4 v = g4[i];
    s0 += v.x * v.x; s1 += v.y * v.y; s2 += v.z * v.z; s3 += v.w * v.w;
    if constexpr (GUARD) bad |= nonfinite_bits(v.x) | nonfinite_bits(v.y) | nonfinite_bits(v.z) | nonfinite_bits(v.w);
  }
  float s = (s0 + s1) + (s2 + s3);
  if ((int64_t)threadIdx.x < head) {
    s += g[threadIdx.x] * g[threadIdx.x];
    if constexpr (GUARD) bad |= nonfinite_bits(g[threadIdx.x]);
  }
  for (int64_t i = head + c4 * 4 + threadIdx.x; i < cnt; i += 256) {
    s += g[i] * g[i];
    if constexpr (GUARD) bad |= nonfinite_bits(g[i]);
  }
  s = block_sum(s, red);
  if constexpr (GUARD) {
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) part[blockIdx.x] = bad ? __uint_as_float(0x7fc00000u) : s;
  } else {
    if (threadIdx.x == 0) part[blockIdx.x] = s;
  }
}
// Final stage, one workgroup: the chunk partials are summed in double (fixed order), then the one thread that holds the sum
// evaluates clip_grad_norm_'s coefficient in double and scales hyper[2] for the adamw_kernel launch behind it.
// -> the total, valid in thread 0. `nan` (optional, shared): set when some partial is NaN.
__device__ __forceinline__ double final_sum(const float *part, int n, double *red, int *nan) {
  double s = 0.0;
  int bad = 0;
  for (int i = threadIdx.x; i < n; i += 1024) {
    const float v = part[i];
    bad |= (v != v);
    s += (double)v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  if (nan) bad = __syncthreads_or(bad); else __syncthreads();
  double tot = 0.0;
  if (threadIdx.x == 0) {
    for (int i = 0; i < 16; ++i) tot += red[i];
    if (nan) *nan = bad;
  }
  return tot;
}
// thread 0 only: norm, coefficient, hyper[2] *= coefficient (max_norm > 0), or {norm, 1} and hyper untouched (max_norm == 0)
__device__ __forceinline__ void apply_clip(double tot, double max_norm, float *hyper, float *out) {
  const float gs = hyper[2];
  const float norm = sqrtf((float)tot) * gs;            // the norm of the gradient the optimizer applies (1 / world included)
  out[0] = norm;
  if (max_norm > 0.0) {
    const double c = max_norm / ((double)norm + 1e-6);
    const double coef = c < 1.0 ? c : 1.0;              // min(1, c) as the host evaluates it
    out[1] = (float)coef;
    hyper[2] = (float)((double)gs * coef);
  } else {
    out[1] = 1.0f;
  }
}
__global__ __launch_bounds__(1024) void clip_final(const float *part, int n, double max_norm, float *hyper, float *out) {
  __shared__ double red[16];
  const double tot = final_sum(part, n, red, nullptr);
  if (threadIdx.x == 0) apply_clip(tot, max_norm, hyper, out);
}
// The guard's final stage: a NaN partial (a chunk with a non-finite element) = skip: count it, report, leave hyper alone. Otherwise
// the step is applied: Adam's t advances ON THE DEVICE and the bias corrections of that t replace the host's (which counts launches).
__global__ __launch_bounds__(1024) void guard_final(const float *part, int n, double max_norm, double beta1, double beta2,
                                                    float *hyper, float *out, int64_t *guard) {
  __shared__ double red[16];
  __shared__ int nan;
  const double tot = final_sum(part, n, red, &nan);
  if (threadIdx.x == 0) {
    const int bad = nan;
    guard[0] = bad;
    if (bad) {
      guard[1] += 1;
      out[0] = sqrtf((float)tot) * hyper[2];            // NaN, as computed
      out[1] = 0.0f;
    } else {
      const int64_t t = guard[2] + 1;
      guard[2] = t;
      hyper[0] = (float)(1.0 - pow(beta1, (double)t));
      hyper[1] = (float)sqrt(1.0 - pow(beta2, (double)t));
      apply_clip(tot, max_norm, hyper, out);
    }
  }
}

}  // namespace

static int adamw_launch(const char *name, float *const *params, const float *const *grads, float *const *exp_avg, float *const *exp_avg_sq,
                        uint16_t *const *lp_shadow, const int64_t *numel, const float *weight_decay, const float *lr_scale,
                        const int32_t *chunk_tensor, const int64_t *chunk_offset, int n_chunks, int chunk_elems, float lr,
                        float beta1, float beta2, float eps, int step, float grad_scale, const float *dev_hyper, const int64_t *guard,
                        void *stream) {
  EVP_CHECK_ARG(params && grads && exp_avg && exp_avg_sq && numel && weight_decay && lr_scale && chunk_tensor && chunk_offset,
                EVP_EINVAL, "%s: null table", name);
  EVP_CHECK_ARG(n_chunks > 0 && chunk_elems > 0 && chunk_elems % 4 == 0 && step >= 1, EVP_EINVAL, "%s: bad chunking/step", name);
  AdamArgs a;
  a.params = params; a.grads = grads; a.exp_avg = exp_avg; a.exp_avg_sq = exp_avg_sq; a.lp = lp_shadow; a.numel = numel;
  a.wd = weight_decay; a.lr_scale = lr_scale; a.chunk_tensor = chunk_tensor; a.chunk_offset = chunk_offset; a.chunk_elems = chunk_elems;
  a.dev_hyper = dev_hyper; a.guard = guard;
  a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.grad_scale = grad_scale;
  a.bc1 = (float)(1.0 - pow((double)beta1, (double)step));
  a.bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)step));
  hipLaunchKernelGGL(adamw_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, a);
  EVP_CHECK_LAUNCH(name);
  return EVP_OK;
}

extern "C" int evp_adamw_multi(float *const *params, const float *const *grads, float *const *exp_avg, float *const *exp_avg_sq,
                               uint16_t *const *lp_shadow, const int64_t *numel, const float *weight_decay, const float *lr_scale,
                               const int32_t *chunk_tensor, const int64_t *chunk_offset, int n_chunks, int chunk_elems, float lr,
                               float beta1, float beta2, float eps, int step, float grad_scale, const float *dev_hyper, void *stream) {
  return adamw_launch("evp_adamw_multi", params, grads, exp_avg, exp_avg_sq, lp_shadow, numel, weight_decay, lr_scale, chunk_tensor,
                      chunk_offset, n_chunks, chunk_elems, lr, beta1, beta2, eps, step, grad_scale, dev_hyper, nullptr, stream);
}

extern "C" int evp_adamw_guarded_multi(float *const *params, const float *const *grads, float *const *exp_avg, float *const *exp_avg_sq,
                                       uint16_t *const *lp_shadow, const int64_t *numel, const float *weight_decay,
                                       const float *lr_scale, const int32_t *chunk_tensor, const int64_t *chunk_offset, int n_chunks,
                                       int chunk_elems, float lr, float beta1, float beta2, float eps, int step, float grad_scale,
                                       const float *dev_hyper, const int64_t *guard, void *stream) {
  // the bias corrections of a guarded step are the ones evp_grad_guard_multi wrote for the applied-step count: dev_hyper is not optional
  EVP_CHECK_ARG(guard && dev_hyper, EVP_EINVAL, "evp_adamw_guarded_multi: null table (guard / dev_hyper)");
  return adamw_launch("evp_adamw_guarded_multi", params, grads, exp_avg, exp_avg_sq, lp_shadow, numel, weight_decay, lr_scale,
                      chunk_tensor, chunk_offset, n_chunks, chunk_elems, lr, beta1, beta2, eps, step, grad_scale, dev_hyper, guard, stream);
}

extern "C" int evp_grad_norm_multi(const float *const *grads, const int64_t *numel, const int32_t *chunk_tensor,
                                   const int64_t *chunk_offset, int n_chunks, int chunk_elems, float *workspace, float *out,
                                   void *stream) {
  EVP_CHECK_ARG(grads && numel && chunk_tensor && chunk_offset && workspace && out && n_chunks > 0, EVP_EINVAL, "evp_grad_norm_multi: bad argument");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sumsq_chunks, dim3(n_chunks), dim3(256), 0, s, grads, numel, chunk_tensor, chunk_offset, chunk_elems, workspace);
  EVP_CHECK_LAUNCH("evp_grad_norm_multi");
  hipLaunchKernelGGL(sqrt_sum, dim3(1), dim3(1024), 0, s, workspace, n_chunks, out);
  EVP_CHECK_LAUNCH("evp_grad_norm_multi(final)");
  return EVP_OK;
}

extern "C" int evp_grad_clip_multi(const float *const *grads, const int64_t *numel, const int32_t *chunk_tensor,
                                   const int64_t *chunk_offset, int n_chunks, int chunk_elems, float *workspace, double max_norm,
                                   float *hyper, float *out, void *stream) {
  EVP_CHECK_ARG(grads && numel && chunk_tensor && chunk_offset && workspace && hyper && out, EVP_EINVAL, "evp_grad_clip_multi: null table");
  EVP_CHECK_ARG(n_chunks > 0 && chunk_elems > 0, EVP_EINVAL, "evp_grad_clip_multi: bad chunking (n_chunks %d, chunk_elems %d)", n_chunks, chunk_elems);
  EVP_CHECK_ARG(isfinite(max_norm) && max_norm > 0.0, EVP_EINVAL, "evp_grad_clip_multi: max_norm must be finite and positive (got %g)", max_norm);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sumsq_chunks_v4<false>, dim3(n_chunks), dim3(256), 0, s, grads, numel, chunk_tensor, chunk_offset, chunk_elems, workspace);
  EVP_CHECK_LAUNCH("evp_grad_clip_multi");
  hipLaunchKernelGGL(clip_final, dim3(1), dim3(1024), 0, s, (const float *)workspace, n_chunks, max_norm, hyper, out);
  EVP_CHECK_LAUNCH("evp_grad_clip_multi(final)");
  return EVP_OK;
}

extern "C" int evp_grad_guard_multi(const float *const *grads, const int64_t *numel, const int32_t *chunk_tensor,
                                    const int64_t *chunk_offset, int n_chunks, int chunk_elems, float *workspace, double max_norm,
                                    double beta1, double beta2, float *hyper, float *out, int64_t *guard, void *stream) {
  EVP_CHECK_ARG(grads && numel && chunk_tensor && chunk_offset && workspace && hyper && out && guard, EVP_EINVAL,
                "evp_grad_guard_multi: null table");
  EVP_CHECK_ARG(n_chunks > 0 && chunk_elems > 0, EVP_EINVAL, "evp_grad_guard_multi: bad chunking (n_chunks %d, chunk_elems %d)", n_chunks, chunk_elems);
  EVP_CHECK_ARG(isfinite(max_norm) && max_norm >= 0.0, EVP_EINVAL, "evp_grad_guard_multi: max_norm must be finite and >= 0, 0 = no clip (got %g)", max_norm);
  EVP_CHECK_ARG(beta1 > 0.0 && beta1 < 1.0 && beta2 > 0.0 && beta2 < 1.0, EVP_EINVAL,
                "evp_grad_guard_multi: betas must lie in (0, 1) (got %g, %g)", beta1, beta2);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sumsq_chunks_v4<true>, dim3(n_chunks), dim3(256), 0, s, grads, numel, chunk_tensor, chunk_offset, chunk_elems, workspace);
  EVP_CHECK_LAUNCH("evp_grad_guard_multi");
  hipLaunchKernelGGL(guard_final, dim3(1), dim3(1024), 0, s, (const float *)workspace, n_chunks, max_norm, beta1, beta2, hyper, out, guard);
  EVP_CHECK_LAUNCH("evp_grad_guard_multi(final)");
  return EVP_OK;
}

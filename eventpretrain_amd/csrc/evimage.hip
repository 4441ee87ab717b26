// Event-count images for the classification fine-tuning input (the reference's dataset/dataset_utils/events_to_image.py as every
// dataset/finetune_cls/* dataset calls it with num_bins 2 and 3):
//   count      events -> int32 planes [B,3,H,W] for p == 1, p == 0, p == -1 (torch.bincount on the linear index, so x >= W wraps into the
//              next row), the clip's count of p == 0 rows, and a status count of rows whose index leaves the grid (the reference raises);
//   finish     planes -> float32 [B,C,H,W]: events_to_image_ecdp (C = 2) or events_to_image_mem, / 255, remove_hot_pixel_mem (C = 3);
//   normalize  the per-view tail the datasets apply after evg_augment / view_resize.
// The counts are integers and every sum of them is an integer sum, so a replay repeats bit for bit whatever order the atomics arrive in.
// count is a scatter of one dword per 32-byte row onto grids of up to 224 x 224 cells per plane (200 KB: three planes do not fit the LDS),
// done with global int32 atomics; finish and normalize stream the planes.
#include "evp_common.h"

#define EI_COUNT_THREADS 256
#define EI_BLOCK 1024

// lin = trunc(x * sx) + trunc(y * sy) * W in int64; the products in float64 as events_reshape leaves them, trunc as .long() converts
__global__ __launch_bounds__(EI_COUNT_THREADS) void event_image_count_kernel(const double *__restrict__ ev, const int64_t *__restrict__ off,
                                                                             int64_t n_rows, int H, int W, double sx, double sy,
                                                                             int32_t *__restrict__ planes, int32_t *__restrict__ zero_rows,
                                                                             int32_t *__restrict__ status) {
  const int c = blockIdx.y;
  int64_t b = off[c], e = off[c + 1];
  if (b < 0) b = 0;
  if (e > n_rows) e = n_rows;
  const int64_t hw = (int64_t)H * W;
  int32_t *pl = planes + (int64_t)c * 3 * hw;
  int nz = 0, bad = 0;
  for (int64_t r = b + (int64_t)blockIdx.x * EI_COUNT_THREADS + threadIdx.x; r < e; r += (int64_t)gridDim.x * EI_COUNT_THREADS) {
    const double2 xy = *reinterpret_cast<const double2 *>(ev + 4 * r);
    const double p = ev[4 * r + 3];
    const int k = p == 1.0 ? 0 : (p == 0.0 ? 1 : (p == -1.0 ? 2 : -1));
    if (k < 0) continue;
    nz += (k == 1);
    const double xs = xy.x * sx, ys = xy.y * sy;
    // (magnitudes whose index arithmetic could leave int64 are outside every grid; a NaN fails both comparisons)
    bool ok = fabs(xs) < 4.0e18 && fabs(ys) < 2.0e9;
    int64_t lin = 0;
    if (ok) {
      lin = (int64_t)xs + (int64_t)ys * (int64_t)W;
      ok = lin >= 0 && lin < hw;
    }
    if (ok) atomicAdd(pl + (int64_t)k * hw + lin, 1);
    else ++bad;
  }
  if (nz) atomicAdd(zero_rows + c, nz);
  if (bad) atomicAdd(status, bad);
}

// C = 2: {pos, neg} as floats; neg = the p == 0 plane when the clip has a p == 0 row, else the p == -1 plane
__global__ __launch_bounds__(256) void event_image_finish2_kernel(const int32_t *__restrict__ planes, const int32_t *__restrict__ zero_rows,
                                                                  int64_t hw, float *__restrict__ out) {
  const int c = blockIdx.y;
  const int32_t *pos = planes + (int64_t)c * 3 * hw;
  const int32_t *neg = pos + (zero_rows[c] > 0 ? hw : 2 * hw);
  float *o = out + (int64_t)c * 2 * hw;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (int64_t)gridDim.x * 256) {
    o[i] = (float)pos[i];
    o[hw + i] = (float)neg[i];
  }
}

// C = 3: {pos / 255, 0, neg / 255}, then remove_hot_pixel_mem: with n = 2 H W values k / 255 of planes 0 and 2, S1 = sum k, S2 = sum k^2
// (exact integers), in float64  mean = S1 / n / 255,  var = (S2 - S1 * S1 / n) / (n - 1) / 255^2,  thr = mean + 10 sqrt(max(var, 0));
// a pixel of either plane whose float32 value exceeds thr zeroes both planes at that pixel. One workgroup per clip.
__global__ __launch_bounds__(EI_BLOCK) void event_image_finish3_kernel(const int32_t *__restrict__ planes, const int32_t *__restrict__ zero_rows,
                                                                       int64_t hw, float *__restrict__ out) {
  __shared__ unsigned long long red1[EI_BLOCK], red2[EI_BLOCK];
  __shared__ double thr_s;
  const int c = blockIdx.x, tid = threadIdx.x;
  const int32_t *pos = planes + (int64_t)c * 3 * hw;
  const int32_t *neg = pos + (zero_rows[c] > 0 ? hw : 2 * hw);
  unsigned long long s1 = 0, s2 = 0;
  for (int64_t i = tid; i < hw; i += EI_BLOCK) {
    const unsigned long long a = (unsigned long long)pos[i], b = (unsigned long long)neg[i];
    s1 += a + b;
    s2 += a * a + b * b;
  }
  red1[tid] = s1;
  red2[tid] = s2;
  __syncthreads();
  for (int o = EI_BLOCK / 2; o > 0; o >>= 1) {
    if (tid < o) {
      red1[tid] += red1[tid + o];
      red2[tid] += red2[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double n = 2.0 * (double)hw, S1 = (double)red1[0], S2 = (double)red2[0];
    const double mean = S1 / n / 255.0;
    double var = (S2 - S1 * S1 / n) / (n - 1.0) / (255.0 * 255.0);
    if (!(var > 0.0)) var = 0.0;
    thr_s = mean + 10.0 * sqrt(var);
  }
  __syncthreads();
  const double thr = thr_s;
  float *o = out + (int64_t)c * 3 * hw;
  for (int64_t i = tid; i < hw; i += EI_BLOCK) {
    const float fa = (float)pos[i] / 255.0f, fb = (float)neg[i] / 255.0f;
    const bool hot = (double)fa > thr || (double)fb > thr;
    o[i] = hot ? 0.0f : fa;
    o[hw + i] = 0.0f;
    o[2 * hw + i] = hot ? 0.0f : fb;
  }
}

// the largest value of n floats at p over the workgroup (n >= 1); every thread gets it. A float max does not depend on the order.
__device__ __forceinline__ float block_max_of(const float *__restrict__ p, int64_t n, float m, float *red) {
  const int tid = threadIdx.x;
  if ((n & 3) == 0 && (((uintptr_t)p) & 15) == 0) {
    const float4 *p4 = reinterpret_cast<const float4 *>(p);
    for (int64_t i = tid; i < n / 4; i += EI_BLOCK) {
      const float4 v = p4[i];
      m = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
    }
  } else {
    for (int64_t i = tid; i < n; i += EI_BLOCK) m = fmaxf(m, p[i]);
  }
  m = wave_max(m);
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = m;
  __syncthreads();
  float t = red[0];
  for (int i = 1; i < EI_BLOCK / 64; ++i) t = fmaxf(t, red[i]);
  return t;
}

// C = 2, one workgroup per (view, channel): v = ((v / (max + 1)) - 0.5) * 2, every operation a float32 operation rounded once
__global__ __launch_bounds__(EI_BLOCK) void event_image_normalize2_kernel(float *__restrict__ views, int64_t hw) {
  __shared__ float red[EI_BLOCK / 64];
  float *p = views + (int64_t)blockIdx.x * hw;
  const float d = __fadd_rn(block_max_of(p, hw, -INFINITY, red), 1.0f);
  for (int64_t i = threadIdx.x; i < hw; i += EI_BLOCK) p[i] = __fmul_rn(__fsub_rn(p[i] / d, 0.5f), 2.0f);
}

// C = 3, one workgroup per view: planes 0 and 2 times 1.0f / max(planes 0 and 2); max == 0 is counted, and multiplies by 1000.0f under
// `guard` (the datasets with the `else: factor = 1.0 / 0.001` branch), by 1.0f / 0.0f = inf otherwise (0 * inf = NaN, as the reference)
__global__ __launch_bounds__(EI_BLOCK) void event_image_normalize3_kernel(float *__restrict__ views, int64_t hw, int guard,
                                                                          int32_t *__restrict__ status) {
  __shared__ float red[EI_BLOCK / 64];
  float *p0 = views + (int64_t)blockIdx.x * 3 * hw, *p2 = p0 + 2 * hw;
  float m = block_max_of(p0, hw, -INFINITY, red);
  m = block_max_of(p2, hw, m, red);
  if (m == 0.0f && threadIdx.x == 0) atomicAdd(status, 1);
  const float f = (m == 0.0f && guard) ? 1000.0f : 1.0f / m;
  for (int64_t i = threadIdx.x; i < hw; i += EI_BLOCK) {
    p0[i] = __fmul_rn(p0[i], f);
    p2[i] = __fmul_rn(p2[i], f);
  }
}

#define EI_SHAPE_OK(B, H, W) ((B) > 0 && (B) <= 65535 && (H) > 0 && (W) > 0 && (int64_t)(H) * (W) <= (int64_t)1 << 26)

extern "C" int evp_event_image_count(const double *events, int64_t n_rows, const int64_t *clip_offsets, int n_clips,
                                     int64_t max_rows_per_clip, int H, int W, double sx, double sy, int32_t *planes, int32_t *zero_rows,
                                     int32_t *status, void *stream) {
  EVP_CHECK_ARG(clip_offsets && planes && zero_rows && status && (events || n_rows == 0), EVP_EINVAL, "evp_event_image_count: null pointer");
  EVP_CHECK_ARG(EI_SHAPE_OK(n_clips, H, W) && n_rows >= 0 && max_rows_per_clip >= 0, EVP_ESHAPE,
                "evp_event_image_count: bad shape (n_clips=%d, %d x %d, %lld rows)", n_clips, H, W, (long long)n_rows);
  hipStream_t s = (hipStream_t)stream;
  const int64_t hw = (int64_t)H * W;
  if (evp_zero_async(planes, (size_t)n_clips * 3 * hw * 4, s) != hipSuccess || evp_zero_async(zero_rows, (size_t)n_clips * 4, s) != hipSuccess) {
    evp_set_error("evp_event_image_count: clearing the planes failed");
    return EVP_ELAUNCH;
  }
  if (n_rows == 0) return EVP_OK;
  // four rows per thread at the longest clip, at least one workgroup per clip; the loop strides, so the bound sizes the grid alone
  int64_t gx = ceil_div64(max_rows_per_clip < n_rows ? max_rows_per_clip : n_rows, 4 * EI_COUNT_THREADS);
  if (gx < 1) gx = 1;
  if (gx > 1024) gx = 1024;
  hipLaunchKernelGGL(event_image_count_kernel, dim3((unsigned)gx, (unsigned)n_clips), dim3(EI_COUNT_THREADS), 0, s, events, clip_offsets,
                     n_rows, H, W, sx, sy, planes, zero_rows, status);
  EVP_CHECK_LAUNCH("evp_event_image_count");
  return EVP_OK;
}

extern "C" int evp_event_image_finish(const int32_t *planes, const int32_t *zero_rows, int n_clips, int C, int H, int W, float *out,
                                      void *stream) {
  EVP_CHECK_ARG(planes && zero_rows && out, EVP_EINVAL, "evp_event_image_finish: null pointer");
  EVP_CHECK_ARG(C == 2 || C == 3, EVP_EINVAL, "evp_event_image_finish: C must be 2 or 3 (got %d)", C);
  EVP_CHECK_ARG(EI_SHAPE_OK(n_clips, H, W), EVP_ESHAPE, "evp_event_image_finish: bad shape (n_clips=%d, %d x %d)", n_clips, H, W);
  const int64_t hw = (int64_t)H * W;
  if (C == 2) {
    int64_t gx = ceil_div64(hw, 256);
    if (gx > 256) gx = 256;
    hipLaunchKernelGGL(event_image_finish2_kernel, dim3((unsigned)gx, (unsigned)n_clips), dim3(256), 0, (hipStream_t)stream, planes,
                       zero_rows, hw, out);
  } else {
    hipLaunchKernelGGL(event_image_finish3_kernel, dim3((unsigned)n_clips), dim3(EI_BLOCK), 0, (hipStream_t)stream, planes, zero_rows, hw,
                       out);
  }
  EVP_CHECK_LAUNCH("evp_event_image_finish");
  return EVP_OK;
}

extern "C" int evp_event_image_normalize(float *views, int n_views, int C, int H, int W, int guard, int32_t *status, void *stream) {
  EVP_CHECK_ARG(views && status, EVP_EINVAL, "evp_event_image_normalize: null pointer");
  EVP_CHECK_ARG(C == 2 || C == 3, EVP_EINVAL, "evp_event_image_normalize: C must be 2 or 3 (got %d)", C);
  EVP_CHECK_ARG(EI_SHAPE_OK(n_views, H, W), EVP_ESHAPE, "evp_event_image_normalize: bad shape (n_views=%d, %d x %d)", n_views, H, W);
  const int64_t hw = (int64_t)H * W;
  if (C == 2)
    hipLaunchKernelGGL(event_image_normalize2_kernel, dim3((unsigned)n_views * 2), dim3(EI_BLOCK), 0, (hipStream_t)stream, views, hw);
  else
    hipLaunchKernelGGL(event_image_normalize3_kernel, dim3((unsigned)n_views), dim3(EI_BLOCK), 0, (hipStream_t)stream, views, hw, guard,
                       status);
  EVP_CHECK_LAUNCH("evp_event_image_normalize");
  return EVP_OK;
}

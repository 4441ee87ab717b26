// K27: the objective and the metrics of semantic-segmentation fine-tuning from the LOW-RESOLUTION logits (include/evtpretrain.h).
// The reference resizes both heads' logits to the label size and then runs softmax, one-hot, masks, products and sums as separate
// full-size torch ops (trainer/finetune_semseg/semseg_loss.py). Here the only full-resolution operand is the label map: a pixel's
// logits are interpolated from the map's four taps into registers (tap_of / tap_combine of evp_common.h: the bits of
// evp_upsample_bilinear_fwd), used and dropped.
//   pixel pass   256 threads walk the pixels grid-stride; a thread keeps ce, A_c = sum p_c [y = c] and Q_c = sum p_c^2 in registers
//                (the class loops are unrolled over a compile-time CP in {8, 16, 32} >= C, columns >= C hold -inf and fall out of the
//                softmax by themselves, so nothing is indexed at run time and nothing spills), counts go to LDS integer counters;
//                wave shuffle -> LDS -> one row of the workspace per workgroup. The metrics form also takes the argmax and counts the
//                confusion table in LDS integers.
//   finish       one workgroup sums the rows in a fixed order in double and writes the scalars (and the table slot).
//   backward     a gather: one workgroup per map cell walks the output pixels whose taps name the cell (conservative range,
//                membership by tap_of itself), recomputes each pixel's softmax and sums wy wx dz in registers; the same reduction.
// No float atomics anywhere: two runs, and a graph replay against an eager call, give the same bits.
#include "evp_common.h"

namespace {

constexpr int SS_THREADS = 256;
constexpr int SS_MAXC = EVP_SEMSEG_MAX_CLASSES;
constexpr int SS_ROW = EVP_SEMSEG_WS_ROW;
constexpr int SS_MAX_BLOCKS = 1024;
// dwords of a workspace row: floats {ce, A_c, Q_c}, ints {n_valid, bad, T_c}
constexpr int SS_CE = 0, SS_NVALID = 1, SS_BAD = 2, SS_A = 4, SS_Q = SS_A + SS_MAXC, SS_T = SS_Q + SS_MAXC;
static_assert(SS_T + SS_MAXC == SS_ROW, "workspace row layout");
static_assert(1 + 2 * SS_MAXC + 3 <= EVP_SEMSEG_SAVED, "saved layout");
constexpr int SV_NVALID = 0, SV_N = 4, SV_D = SV_N + SS_MAXC;

struct SsGeom {
  const float *map; int64_t ld; int B, h, w, H, W, C;
  const int64_t *label; int64_t ignore; int has_ignore;
};

__device__ __forceinline__ int64_t wave_sum_i64(int64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the logits of output pixel (b, y, x): columns >= C read nothing and hold -inf
template <int CP>
__device__ __forceinline__ void pixel_logits(const SsGeom &g, int b, const Tap &ty, const Tap &tx, float (&z)[CP]) {
  const int64_t r0 = (int64_t)(b * g.h + ty.i0) * g.w, r1 = (int64_t)(b * g.h + ty.i1) * g.w;
  const float *pa = g.map + (r0 + tx.i0) * g.ld, *pb = g.map + (r0 + tx.i1) * g.ld;
  const float *pc = g.map + (r1 + tx.i0) * g.ld, *pd = g.map + (r1 + tx.i1) * g.ld;
#pragma unroll
  for (int c = 0; c < CP; ++c) z[c] = c < g.C ? tap_combine(ty, tx, pa[c], pb[c], pc[c], pd[c]) : -INFINITY;
}

// z -> p = softmax(z) in place; returns logsumexp(z)
template <int CP> __device__ __forceinline__ float softmax_inplace(float (&z)[CP]) {
  float m = z[0];
#pragma unroll
  for (int c = 1; c < CP; ++c) m = fmaxf(m, z[c]);
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < CP; ++c) { z[c] = expf(z[c] - m); s += z[c]; }
  const float inv = 1.f / s;
#pragma unroll
  for (int c = 0; c < CP; ++c) z[c] *= inv;
  return logf(s) + m;
}

template <int CP> __device__ __forceinline__ float pick(const float (&v)[CP], int k) {
  float r = 0.f;
#pragma unroll
  for (int c = 0; c < CP; ++c) r = c == k ? v[c] : r;
  return r;
}

template <int CP, bool METRICS>
__global__ __launch_bounds__(SS_THREADS) void semseg_pixel_kernel(const SsGeom g, int64_t P, uint32_t *__restrict__ ws, int32_t *__restrict__ conf_ws,
                                                                  uint8_t *__restrict__ argmax_out) {
  __shared__ float redf[SS_THREADS / 64][1 + 2 * CP];
  __shared__ int cnt[2 + CP];                              // n_valid, bad, T_c
  __shared__ int conf[METRICS ? CP * CP : 1];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, C = g.C;
  if (tid < 2 + CP) cnt[tid] = 0;
  if (METRICS)
    for (int e = tid; e < C * C; e += SS_THREADS) conf[e] = 0;
  __syncthreads();
  const float sy = (float)g.h / (float)g.H, sx = (float)g.w / (float)g.W;
  const int64_t HW = (int64_t)g.H * g.W;
  float ce = 0.f, A[CP], Q[CP];
#pragma unroll
  for (int c = 0; c < CP; ++c) { A[c] = 0.f; Q[c] = 0.f; }
  int nvalid = 0, bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * SS_THREADS + tid; i < P; i += (int64_t)gridDim.x * SS_THREADS) {
    const int64_t lab = g.label[i];
    const bool ign = g.has_ignore && lab == g.ignore;
    const bool ok = !ign && lab >= 0 && lab < (int64_t)C;
    bad += (!ign && !ok) ? 1 : 0;
    if (!ok && !(METRICS && argmax_out)) continue;
    const int b = (int)(i / HW);
    const int64_t rem = i - (int64_t)b * HW;
    const int y = (int)(rem / g.W), x = (int)(rem - (int64_t)y * g.W);
    float z[CP];
    pixel_logits<CP>(g, b, tap_of(y, g.h, sy), tap_of(x, g.w, sx), z);
    if (METRICS) {
      float best = z[0];
      int am = 0;
#pragma unroll
      for (int c = 1; c < CP; ++c)       // first maximum, a NaN counting as the largest (torch.argmax)
        if (z[c] > best || (z[c] != z[c] && best == best)) { best = z[c]; am = c; }
      if (argmax_out) argmax_out[i] = (uint8_t)am;
      if (!ok) continue;
      atomicAdd(&conf[(int)lab * C + am], 1);
    }
    const int yl = (int)lab;
    const float zy = pick<CP>(z, yl);
    const float lse = softmax_inplace<CP>(z);
    ce += lse - zy;
    ++nvalid;
    atomicAdd(&cnt[2 + yl], 1);
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      A[c] += c == yl ? z[c] : 0.f;
      Q[c] += z[c] * z[c];
    }
  }
  // wave -> LDS -> the four waves in index order -> this workgroup's row
  ce = wave_sum(ce);
  if (lane == 0) redf[wv][0] = ce;
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    if (c < C) {
      const float a = wave_sum(A[c]), q = wave_sum(Q[c]);
      if (lane == 0) { redf[wv][1 + c] = a; redf[wv][1 + CP + c] = q; }
    }
  }
  nvalid = wave_sum_i32(nvalid);
  bad = wave_sum_i32(bad);
  if (lane == 0) { atomicAdd(&cnt[0], nvalid); atomicAdd(&cnt[1], bad); }
  __syncthreads();
  uint32_t *row = ws + (int64_t)blockIdx.x * SS_ROW;
  if (tid < 1 + 2 * CP) {
    const int c = tid == 0 ? 0 : (tid - 1) % CP;
    if (tid == 0 || c < C) {
      const float v = ((redf[0][tid] + redf[1][tid]) + redf[2][tid]) + redf[3][tid];
      const int col = tid == 0 ? SS_CE : (tid - 1 < CP ? SS_A + c : SS_Q + c);
      row[col] = __float_as_uint(v);
    }
  }
  if (tid == 0) { row[SS_NVALID] = (uint32_t)cnt[0]; row[SS_BAD] = (uint32_t)cnt[1]; }
  if (tid < C) row[SS_T + tid] = (uint32_t)cnt[2 + tid];
  if (METRICS)
    for (int e = tid; e < C * C; e += SS_THREADS) conf_ws[(int64_t)blockIdx.x * C * C + e] = conf[e];
}

// One workgroup of 16 waves. Column `col` of the nblk workspace rows: lane l adds rows l, l + 64, ... in double, the 64 lane sums
// meet in a shuffle tree: one order, whatever ran first.
template <bool METRICS>
__global__ __launch_bounds__(1024) void semseg_finish_kernel(const uint32_t *__restrict__ ws, int nblk, int C, float *out, float *saved,
                                                             int32_t *status, const int32_t *__restrict__ conf_ws, int64_t *confusion,
                                                             int64_t *cursor, float *table, int64_t capacity) {
  __shared__ double tot[SS_ROW];
  __shared__ int64_t conf_s[METRICS ? SS_MAXC * SS_MAXC : 1];
  __shared__ double iou_s[SS_MAXC], acc_s[SS_MAXC];
  __shared__ int64_t slot_s;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (METRICS && tid == 0) slot_s = *cursor;
  for (int col = wv; col < SS_ROW; col += 16) {
    const bool is_int = col == SS_NVALID || col == SS_BAD || col >= SS_T;
    const bool used = col <= SS_BAD || (col >= SS_A && ((col - SS_A) % SS_MAXC) < C);
    if (!used) continue;                                   // (wave-uniform)
    double v = 0.0;
    for (int r = lane; r < nblk; r += 64) {
      const uint32_t u = ws[(int64_t)r * SS_ROW + col];
      v += is_int ? (double)(int32_t)u : (double)__uint_as_float(u);
    }
    v = wave_sum_f64(v);
    if (lane == 0) tot[col] = v;
  }
  if (METRICS) {
    const int CC = C * C;
    for (int e = wv; e < CC; e += 16) {
      int64_t v = 0;
      for (int r = lane; r < nblk; r += 64) v += (int64_t)conf_ws[(int64_t)r * CC + e];
      v = wave_sum_i64(v);
      if (lane == 0) { conf_s[e] = v; if (confusion) confusion[e] = v; }
    }
  }
  __syncthreads();
  if (METRICS && tid < C) {
    int64_t rsum = 0, csum = 0;
    for (int j = 0; j < C; ++j) { rsum += conf_s[tid * C + j]; csum += conf_s[j * C + tid]; }
    const double diag = (double)conf_s[tid * C + tid];
    iou_s[tid] = 100.0 * diag / fmax((double)(rsum + csum) - diag, 1e-12);
    acc_s[tid] = 100.0 * diag / fmax((double)rsum, 1e-12);
  }
  __syncthreads();
  if (tid != 0) return;
  const double n = tot[SS_NVALID];
  const double ce = tot[SS_CE] / n;                        // 0 / 0 = NaN when nothing is valid
  double dice = 0.0;
  for (int c = 0; c < C; ++c) {
    const double N = 2.0 * tot[SS_A + c] + 1.0, D = tot[SS_Q + c] + tot[SS_T + c] + 1.0;
    dice += 1.0 - N / D;
    if (saved) { saved[SV_N + c] = (float)N; saved[SV_D + c] = (float)D; }
  }
  dice /= (double)C;
  if (saved) saved[SV_NVALID] = (float)n;
  if (out) { out[0] = (float)ce; out[1] = (float)dice; }
  if (status) status[0] += (int32_t)tot[SS_BAD];
  if (METRICS) {
    const int64_t slot = slot_s;
    if (slot < 0 || slot >= capacity) return;              // a full table or a corrupt cursor: nothing is written
    double miou = 0.0, macc = 0.0;
    for (int c = 0; c < C; ++c) { miou += iou_s[c]; macc += acc_s[c]; }
    float *t = table + slot * 3;
    t[0] = (float)(ce + dice);
    t[1] = (float)(miou / (double)C);
    t[2] = (float)(macc / (double)C);
    *cursor = slot + 1;
  }
}

// destination indices d of n_out one of whose taps can be source index s: src(d) in [s - 1, s + 1), i.e. d + 0.5 in
// [(s - 0.5) / scale, (s + 1.5) / scale); two spare indices on either side cover the float rounding of tap_of's coordinate, and
// tap_of itself decides membership.
__device__ __forceinline__ void span_of(int s, int n_in, int n_out, int &lo, int &hi) {
  const float inv = (float)n_out / (float)n_in;
  lo = (int)floorf(((float)s - 0.5f) * inv - 0.5f) - 2;
  hi = (int)ceilf(((float)s + 1.5f) * inv - 0.5f) + 2;
  lo = max(lo, 0);
  hi = min(hi, n_out - 1);
}

template <int CP>
__global__ __launch_bounds__(SS_THREADS) void semseg_bwd_kernel(const SsGeom g, const float *__restrict__ saved, const float *__restrict__ g_ce,
                                                                const float *__restrict__ g_dice, float *__restrict__ grad, int64_t ldg) {
  __shared__ float red[SS_THREADS / 64][CP];
  __shared__ float su[CP], sv[CP];                          // a_j = p_j su_j - [j = y] sv_j
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = blockDim.x >> 6, C = g.C;
  if (tid < CP) {
    const float N = tid < C ? saved[SV_N + tid] : 0.f, D = tid < C ? saved[SV_D + tid] : 1.f;
    su[tid] = 2.f * N / (D * D);
    sv[tid] = tid < C ? 2.f / D : 0.f;
  }
  __syncthreads();
  const float kce = g_ce[0] / saved[SV_NVALID], kd = g_dice[0] / (float)C;
  const int64_t cell = blockIdx.x;
  const int b = (int)(cell / ((int64_t)g.h * g.w));
  const int ys = (int)((cell / g.w) % g.h), xs = (int)(cell % g.w);
  const float sy = (float)g.h / (float)g.H, sx = (float)g.w / (float)g.W;
  int y0, y1, x0, x1;
  span_of(ys, g.h, g.H, y0, y1);
  span_of(xs, g.w, g.W, x0, x1);
  const int nx = max(x1 - x0 + 1, 0), n = max(y1 - y0 + 1, 0) * nx;
  float acc[CP];
#pragma unroll
  for (int c = 0; c < CP; ++c) acc[c] = 0.f;
  for (int i = tid; i < n; i += blockDim.x) {
    const int y = y0 + i / nx, x = x0 + i % nx;
    const Tap ty = tap_of(y, g.h, sy), tx = tap_of(x, g.w, sx);
    if ((ty.i0 != ys && ty.i1 != ys) || (tx.i0 != xs && tx.i1 != xs)) continue;
    const int64_t lab = g.label[((int64_t)b * g.H + y) * g.W + x];
    if ((g.has_ignore && lab == g.ignore) || lab < 0 || lab >= (int64_t)C) continue;
    const float wy = (ty.i0 == ys ? ty.l0 : 0.f) + (ty.i1 == ys ? ty.l1 : 0.f);
    const float wx = (tx.i0 == xs ? tx.l0 : 0.f) + (tx.i1 == xs ? tx.l1 : 0.f);
    const float wgt = wy * wx;
    const int yl = (int)lab;
    float p[CP];
    pixel_logits<CP>(g, b, ty, tx, p);
    softmax_inplace<CP>(p);
    float s = 0.f;                                          // sum_j a_j p_j
#pragma unroll
    for (int c = 0; c < CP; ++c) s += p[c] * (p[c] * su[c] - (c == yl ? sv[c] : 0.f));
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      const float hot = c == yl ? 1.f : 0.f;
      const float a = p[c] * su[c] - hot * sv[c];
      acc[c] += wgt * (kce * (p[c] - hot) + kd * p[c] * (a - s));
    }
  }
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    if (c < C) {
      const float v = wave_sum(acc[c]);
      if (lane == 0) red[wv][c] = v;
    }
  }
  __syncthreads();
  for (int k = tid; k < (int)ldg; k += blockDim.x) {
    float v = 0.f;
    if (k < C)
      for (int i = 0; i < nw; ++i) v += red[i][k];
    grad[cell * ldg + k] = v;
  }
}

int check_geom(const char *name, const void *map, int64_t ld, int B, int h, int w, int H, int W, int C, const void *label) {
  EVP_CHECK_ARG(map && label, EVP_EINVAL, "%s: null pointer", name);
  EVP_CHECK_ARG(C >= 2 && C <= SS_MAXC, EVP_ESHAPE, "%s: %d classes (2 to %d are supported)", name, C, SS_MAXC);
  EVP_CHECK_ARG(B > 0 && h > 0 && w > 0 && H > 0 && W > 0 && ld >= C && (int64_t)B * h * w < (1ll << 31) && (int64_t)B * H * W < (1ll << 31),
                EVP_ESHAPE, "%s: bad shape (B=%d, %dx%d -> %dx%d, ld=%lld)", name, B, h, w, H, W, (long long)ld);
  return EVP_OK;
}

int nblk_of(int64_t P) {
  const int64_t n = ceil_div64(P, SS_THREADS);
  return (int)(n < 1 ? 1 : (n > SS_MAX_BLOCKS ? SS_MAX_BLOCKS : n));
}

template <bool METRICS>
int launch_pixels(const char *name, const SsGeom &g, int64_t P, int nblk, void *ws, void *conf_ws, uint8_t *argmax, hipStream_t s) {
  const dim3 grid((unsigned)nblk), block(SS_THREADS);
  if (g.C <= 8) hipLaunchKernelGGL((semseg_pixel_kernel<8, METRICS>), grid, block, 0, s, g, P, (uint32_t *)ws, (int32_t *)conf_ws, argmax);
  else if (g.C <= 16) hipLaunchKernelGGL((semseg_pixel_kernel<16, METRICS>), grid, block, 0, s, g, P, (uint32_t *)ws, (int32_t *)conf_ws, argmax);
  else hipLaunchKernelGGL((semseg_pixel_kernel<32, METRICS>), grid, block, 0, s, g, P, (uint32_t *)ws, (int32_t *)conf_ws, argmax);
  EVP_CHECK_LAUNCH(name);
  return EVP_OK;
}

}  // namespace

extern "C" int evp_semseg_nblk(int64_t pixels) { return nblk_of(pixels); }

extern "C" int evp_semseg_objective_fwd(const float *map, int64_t ld, int B, int h, int w, int H, int W, int C, const int64_t *label,
                                        int64_t ignore_label, int has_ignore, float *out, float *saved, int32_t *status, void *workspace,
                                        void *stream) {
  if (int rc = check_geom("evp_semseg_objective_fwd", map, ld, B, h, w, H, W, C, label)) return rc;
  EVP_CHECK_ARG(out && saved && workspace, EVP_EINVAL, "evp_semseg_objective_fwd: null pointer");
  const SsGeom g{map, ld, B, h, w, H, W, C, label, ignore_label, has_ignore};
  const int64_t P = (int64_t)B * H * W;
  const int nblk = nblk_of(P);
  hipStream_t s = (hipStream_t)stream;
  if (int rc = launch_pixels<false>("evp_semseg_objective_fwd", g, P, nblk, workspace, nullptr, nullptr, s)) return rc;
  hipLaunchKernelGGL(semseg_finish_kernel<false>, dim3(1), dim3(1024), 0, s, (const uint32_t *)workspace, nblk, C, out, saved, status,
                     (const int32_t *)nullptr, (int64_t *)nullptr, (int64_t *)nullptr, (float *)nullptr, (int64_t)0);
  EVP_CHECK_LAUNCH("evp_semseg_objective_fwd(finish)");
  return EVP_OK;
}

extern "C" int evp_semseg_objective_bwd(const float *map, int64_t ld, int B, int h, int w, int H, int W, int C, const int64_t *label,
                                        int64_t ignore_label, int has_ignore, const float *saved, const float *g_ce, const float *g_dice,
                                        float *grad, int64_t ldg, void *stream) {
  if (int rc = check_geom("evp_semseg_objective_bwd", map, ld, B, h, w, H, W, C, label)) return rc;
  EVP_CHECK_ARG(saved && g_ce && g_dice && grad, EVP_EINVAL, "evp_semseg_objective_bwd: null pointer");
  EVP_CHECK_ARG(ldg >= C && ldg < (1 << 20), EVP_ESHAPE, "evp_semseg_objective_bwd: bad leading dimension %lld of the gradient", (long long)ldg);
  const SsGeom g{map, ld, B, h, w, H, W, C, label, ignore_label, has_ignore};
  // pixels a cell can own: (2 H / h + 5) x (2 W / w + 5); a small footprint (same-size maps, downsampling) takes one wave per cell
  const int64_t foot = (2 * (int64_t)H / h + 5) * (2 * (int64_t)W / w + 5);
  const dim3 grid((unsigned)((int64_t)B * h * w)), block(foot > 128 ? SS_THREADS : 64);
  hipStream_t s = (hipStream_t)stream;
  if (C <= 8) hipLaunchKernelGGL(semseg_bwd_kernel<8>, grid, block, 0, s, g, saved, g_ce, g_dice, grad, ldg);
  else if (C <= 16) hipLaunchKernelGGL(semseg_bwd_kernel<16>, grid, block, 0, s, g, saved, g_ce, g_dice, grad, ldg);
  else hipLaunchKernelGGL(semseg_bwd_kernel<32>, grid, block, 0, s, g, saved, g_ce, g_dice, grad, ldg);
  EVP_CHECK_LAUNCH("evp_semseg_objective_bwd");
  return EVP_OK;
}

extern "C" int evp_semseg_metrics(const float *map, int64_t ld, int B, int h, int w, int H, int W, int C, const int64_t *label,
                                  int64_t ignore_label, int has_ignore, int64_t *cursor, float *table, int64_t capacity, int64_t *confusion,
                                  uint8_t *argmax, int32_t *status, void *workspace, void *conf_workspace, void *stream) {
  if (int rc = check_geom("evp_semseg_metrics", map, ld, B, h, w, H, W, C, label)) return rc;
  EVP_CHECK_ARG(cursor && table && workspace && conf_workspace, EVP_EINVAL, "evp_semseg_metrics: null pointer");
  EVP_CHECK_ARG(capacity > 0, EVP_ESHAPE, "evp_semseg_metrics: the table needs at least one slot");
  const SsGeom g{map, ld, B, h, w, H, W, C, label, ignore_label, has_ignore};
  const int64_t P = (int64_t)B * H * W;
  const int nblk = nblk_of(P);
  hipStream_t s = (hipStream_t)stream;
  if (int rc = launch_pixels<true>("evp_semseg_metrics", g, P, nblk, workspace, conf_workspace, argmax, s)) return rc;
  hipLaunchKernelGGL(semseg_finish_kernel<true>, dim3(1), dim3(1024), 0, s, (const uint32_t *)workspace, nblk, C, (float *)nullptr,
                     (float *)nullptr, status, (const int32_t *)conf_workspace, confusion, cursor, table, capacity);
  EVP_CHECK_LAUNCH("evp_semseg_metrics(finish)");
  return EVP_OK;
}

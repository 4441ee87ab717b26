// K28: the objective and the metrics of optical-flow fine-tuning from the LOW-RESOLUTION flow map (include/evtpretrain.h).
// The reference resizes both heads' two-channel predictions to the label size (utils/reshape.py resize_flow: bilinear, then x times
// W / w and y times H / h), and runs the masked L1 loss and, in validation, the end-point error and outlier share as separate
// full-size torch ops (trainer/finetune_flow/flow_loss.py, flow_metric.py). Here the full-resolution operands are the labels alone: a
// pixel's two components are interpolated from the map's four taps into registers (tap_of / tap_combine of evp_common.h: the bits of
// evp_upsample_bilinear_fwd), scaled, used and dropped. The structure is csrc/semseg.hip's:
//   pixel pass   256 threads walk the pixels grid-stride; a thread keeps sum(|dx| + |dy|), sum(epe) and its counts in registers;
//                wave shuffle -> LDS -> one row of the workspace per workgroup.
//   finish       one workgroup sums the rows in a fixed order in double and writes the scalars (and the table slot).
//   backward     a gather: one workgroup per map cell walks the output pixels whose taps name the cell (span_of: a conservative
//                range, membership by tap_of itself), recomputes each pixel's prediction and sums wy wx sign(p - t) in registers.
// No float atomics anywhere: two runs, and a graph replay against an eager call, give the same bits.
#include "evp_common.h"

namespace {

constexpr int FL_THREADS = 256;
constexpr int FL_ROW = EVP_FLOW_WS_ROW;
constexpr int FL_MAX_BLOCKS = 1024;
// dwords of a workspace row: floats {l1, epe}, ints {n_valid, n_sparse, n_outlier}
constexpr int FL_L1 = 0, FL_EPE = 1, FL_NVALID = 2, FL_NSPARSE = 3, FL_NOUT = 4, FL_USED = 5;
static_assert(FL_USED <= FL_ROW, "workspace row layout");
static_assert(1 <= EVP_FLOW_SAVED, "saved layout");
constexpr int SV_NVALID = 0;

struct FlGeom {
  const float *map; int64_t ld; int B, h, w, H, W;
  const float *target, *valid; float max_flow, fx, fy;      // fx, fy: the float32 roundings of W / w and H / h (resize_flow)
};

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

// the scaled prediction of output pixel (b, y, x)
__device__ __forceinline__ void pixel_flow(const FlGeom &g, int b, const Tap &ty, const Tap &tx, float &px, float &py) {
  const int64_t r0 = (int64_t)(b * g.h + ty.i0) * g.w, r1 = (int64_t)(b * g.h + ty.i1) * g.w;
  const float *pa = g.map + (r0 + tx.i0) * g.ld, *pb = g.map + (r0 + tx.i1) * g.ld;
  const float *pc = g.map + (r1 + tx.i0) * g.ld, *pd = g.map + (r1 + tx.i1) * g.ld;
  px = tap_combine(ty, tx, pa[0], pb[0], pc[0], pd[0]) * g.fx;
  py = tap_combine(ty, tx, pa[1], pb[1], pc[1], pd[1]) * g.fy;
}

// FlowLoss's mask: valid >= 0.5 and |t| < max_flow
__device__ __forceinline__ bool in_loss(const FlGeom &g, float v, float mag) { return v >= 0.5f && mag < g.max_flow; }

template <bool METRICS>
__global__ __launch_bounds__(FL_THREADS) void flow_pixel_kernel(const FlGeom g, int64_t P, const float *__restrict__ org, int org_channels,
                                                                uint32_t *__restrict__ ws) {
  __shared__ float redf[FL_THREADS / 64][2];
  __shared__ int redi[FL_THREADS / 64][3];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float sy = (float)g.h / (float)g.H, sx = (float)g.w / (float)g.W;
  const int64_t HW = (int64_t)g.H * g.W;
  float l1 = 0.f, epe_sum = 0.f;
  int nvalid = 0, nsparse = 0, nout = 0;
  for (int64_t i = (int64_t)blockIdx.x * FL_THREADS + tid; i < P; i += (int64_t)gridDim.x * FL_THREADS) {
    const int b = (int)(i / HW);
    const int64_t rem = i - (int64_t)b * HW;
    const float v = g.valid[i];
    const float tx_ = g.target[(int64_t)b * 2 * HW + rem], ty_ = g.target[((int64_t)b * 2 + 1) * HW + rem];
    const float mag = sqrtf(tx_ * tx_ + ty_ * ty_);
    const bool ok = in_loss(g, v, mag);
    bool sparse = false;
    if (METRICS && v != 0.f) {                             // the validation's mask: valid NON-ZERO and an event at the pixel
      float e2 = 0.f;
      for (int c = 0; c < org_channels; ++c) {
        const float e = org[((int64_t)b * org_channels + c) * HW + rem];
        e2 += e * e;
      }
      sparse = e2 > 0.f;
    }
    if (!ok && !sparse) continue;
    const int y = (int)(rem / g.W), x = (int)(rem - (int64_t)y * g.W);
    float px, py;
    pixel_flow(g, b, tap_of(y, g.h, sy), tap_of(x, g.w, sx), px, py);
    const float dx = px - tx_, dy = py - ty_;
    if (ok) {
      l1 += fabsf(dx) + fabsf(dy);
      ++nvalid;
    }
    if (METRICS && sparse) {
      const float epe = sqrtf(dx * dx + dy * dy);
      epe_sum += epe;
      ++nsparse;
      nout += (epe > 3.0f && epe / mag > 0.05f) ? 1 : 0;   // (mag == 0: inf, which counts)
    }
  }
  // wave -> LDS -> the four waves in index order -> this workgroup's row
  l1 = wave_sum(l1);
  nvalid = wave_sum_i32(nvalid);
  if (METRICS) {
    epe_sum = wave_sum(epe_sum);
    nsparse = wave_sum_i32(nsparse);
    nout = wave_sum_i32(nout);
  }
  if (lane == 0) {
    redf[wv][0] = l1; redf[wv][1] = epe_sum;
    redi[wv][0] = nvalid; redi[wv][1] = nsparse; redi[wv][2] = nout;
  }
  __syncthreads();
  uint32_t *row = ws + (int64_t)blockIdx.x * FL_ROW;
  if (tid < 2) row[FL_L1 + tid] = __float_as_uint(((redf[0][tid] + redf[1][tid]) + redf[2][tid]) + redf[3][tid]);
  else if (tid < FL_USED) row[tid] = (uint32_t)(redi[0][tid - 2] + redi[1][tid - 2] + redi[2][tid - 2] + redi[3][tid - 2]);
}

// One workgroup, one wave per column of the nblk workspace rows: lane l adds rows l, l + 64, ... in double, the 64 lane sums meet in a
// shuffle tree: one order, whatever ran first.
template <bool METRICS>
__global__ __launch_bounds__(FL_USED * 64) void flow_finish_kernel(const uint32_t *__restrict__ ws, int nblk, float *out, float *saved,
                                                                   int64_t *cursor, float *table, int64_t capacity) {
  __shared__ double tot[FL_USED];
  __shared__ int64_t slot_s;
  const int tid = threadIdx.x, lane = tid & 63, col = tid >> 6;
  if (METRICS && tid == 0) slot_s = *cursor;
  double v = 0.0;
  for (int r = lane; r < nblk; r += 64) {
    const uint32_t u = ws[(int64_t)r * FL_ROW + col];
    v += col >= FL_NVALID ? (double)(int32_t)u : (double)__uint_as_float(u);
  }
  v = wave_sum_f64(v);
  if (lane == 0) tot[col] = v;
  __syncthreads();
  if (tid != 0) return;
  const double n = tot[FL_NVALID];
  const double l1 = tot[FL_L1] / (2.0 * n);                // 0 / 0 = NaN when nothing is valid
  if (saved) saved[SV_NVALID] = (float)n;
  if (out) out[0] = (float)l1;
  if (METRICS) {
    const int64_t slot = slot_s;
    if (slot < 0 || slot >= capacity) return;              // a full table or a corrupt cursor: nothing is written
    const double ns = tot[FL_NSPARSE];
    float *t = table + slot * 3;
    t[0] = (float)l1;
    t[1] = (float)(tot[FL_EPE] / ns);                      // an empty mask: NaN, both
    t[2] = (float)(100.0 * tot[FL_NOUT] / ns);
    *cursor = slot + 1;
  }
}

// destination indices d of n_out one of whose taps can be source index s (csrc/semseg.hip span_of): src(d) in [s - 1, s + 1), i.e.
// d + 0.5 in [(s - 0.5) / scale, (s + 1.5) / scale); two spare indices on either side cover the float rounding of tap_of's
// coordinate, and tap_of itself decides membership.
__device__ __forceinline__ void span_of(int s, int n_in, int n_out, int &lo, int &hi) {
  const float inv = (float)n_out / (float)n_in;
  lo = (int)floorf(((float)s - 0.5f) * inv - 0.5f) - 2;
  hi = (int)ceilf(((float)s + 1.5f) * inv - 0.5f) + 2;
  lo = max(lo, 0);
  hi = min(hi, n_out - 1);
}

// d|d| / dd as autograd's abs has it: sign(0) = 0, a NaN stays one
__device__ __forceinline__ float sign_of(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : d); }

__global__ __launch_bounds__(FL_THREADS) void flow_bwd_kernel(const FlGeom g, const float *__restrict__ saved, const float *__restrict__ g_loss,
                                                              float *__restrict__ grad, int64_t ldg) {
  __shared__ float red[FL_THREADS / 64][2];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = blockDim.x >> 6;
  // g / (2 n) enters per contribution: with n == 0 no pixel contributes and the sums stay exact zeros
  const float k = g_loss[0] / (2.f * saved[SV_NVALID]);
  const float kx = g.fx * k, ky = g.fy * k;
  const int64_t cell = blockIdx.x;
  const int b = (int)(cell / ((int64_t)g.h * g.w));
  const int ys = (int)((cell / g.w) % g.h), xs = (int)(cell % g.w);
  const float sy = (float)g.h / (float)g.H, sx = (float)g.w / (float)g.W;
  const int64_t HW = (int64_t)g.H * g.W;
  int y0, y1, x0, x1;
  span_of(ys, g.h, g.H, y0, y1);
  span_of(xs, g.w, g.W, x0, x1);
  const int nx = max(x1 - x0 + 1, 0), n = max(y1 - y0 + 1, 0) * nx;
  float ax = 0.f, ay = 0.f;
  for (int i = tid; i < n; i += blockDim.x) {
    const int y = y0 + i / nx, x = x0 + i % nx;
    const Tap ty = tap_of(y, g.h, sy), tx = tap_of(x, g.w, sx);
    if ((ty.i0 != ys && ty.i1 != ys) || (tx.i0 != xs && tx.i1 != xs)) continue;
    const int64_t rem = (int64_t)y * g.W + x;
    const float tx_ = g.target[(int64_t)b * 2 * HW + rem], ty_ = g.target[((int64_t)b * 2 + 1) * HW + rem];
    if (!in_loss(g, g.valid[(int64_t)b * HW + rem], sqrtf(tx_ * tx_ + ty_ * ty_))) continue;
    const float wy = (ty.i0 == ys ? ty.l0 : 0.f) + (ty.i1 == ys ? ty.l1 : 0.f);
    const float wx = (tx.i0 == xs ? tx.l0 : 0.f) + (tx.i1 == xs ? tx.l1 : 0.f);
    const float wgt = wy * wx;
    float px, py;
    pixel_flow(g, b, ty, tx, px, py);
    ax += wgt * sign_of(px - tx_) * kx;
    ay += wgt * sign_of(py - ty_) * ky;
  }
  ax = wave_sum(ax);
  ay = wave_sum(ay);
  if (lane == 0) { red[wv][0] = ax; red[wv][1] = ay; }
  __syncthreads();
  for (int c = tid; c < (int)ldg; c += blockDim.x) {
    float v = 0.f;
    if (c < 2)
      for (int i = 0; i < nw; ++i) v += red[i][c];
    grad[cell * ldg + c] = v;
  }
}

int check_geom(const char *name, const void *map, int64_t ld, int B, int h, int w, int H, int W, const void *target, const void *valid) {
  EVP_CHECK_ARG(map && target && valid, EVP_EINVAL, "%s: null pointer", name);
  EVP_CHECK_ARG(ld >= 2, EVP_ESHAPE, "%s: leading dimension %lld of the map (two flow components need 2)", name, (long long)ld);
  EVP_CHECK_ARG(B > 0 && h > 0 && w > 0 && H > 0 && W > 0 && (int64_t)B * h * w < (1ll << 31) && (int64_t)B * H * W < (1ll << 31),
                EVP_ESHAPE, "%s: bad shape (B=%d, %dx%d -> %dx%d)", name, B, h, w, H, W);
  return EVP_OK;
}

FlGeom geom_of(const float *map, int64_t ld, int B, int h, int w, int H, int W, const float *target, const float *valid, float max_flow) {
  // the factors as resize_flow makes them: Python's double quotient stored into a float32 tensor
  return FlGeom{map, ld, B, h, w, H, W, target, valid, max_flow, (float)((double)W / (double)w), (float)((double)H / (double)h)};
}

int nblk_of(int64_t P) {
  const int64_t n = ceil_div64(P, FL_THREADS);
  return (int)(n < 1 ? 1 : (n > FL_MAX_BLOCKS ? FL_MAX_BLOCKS : n));
}

}  // namespace

extern "C" int evp_flow_nblk(int64_t pixels) { return nblk_of(pixels); }

extern "C" int evp_flow_objective_fwd(const float *map, int64_t ld, int B, int h, int w, int H, int W, const float *target, const float *valid,
                                      float max_flow, float *out, float *saved, void *workspace, void *stream) {
  if (int rc = check_geom("evp_flow_objective_fwd", map, ld, B, h, w, H, W, target, valid)) return rc;
  EVP_CHECK_ARG(out && saved && workspace, EVP_EINVAL, "evp_flow_objective_fwd: null pointer");
  const FlGeom g = geom_of(map, ld, B, h, w, H, W, target, valid, max_flow);
  const int64_t P = (int64_t)B * H * W;
  const int nblk = nblk_of(P);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(flow_pixel_kernel<false>, dim3((unsigned)nblk), dim3(FL_THREADS), 0, s, g, P, (const float *)nullptr, 0, (uint32_t *)workspace);
  EVP_CHECK_LAUNCH("evp_flow_objective_fwd");
  hipLaunchKernelGGL(flow_finish_kernel<false>, dim3(1), dim3(FL_USED * 64), 0, s, (const uint32_t *)workspace, nblk, out, saved,
                     (int64_t *)nullptr, (float *)nullptr, (int64_t)0);
  EVP_CHECK_LAUNCH("evp_flow_objective_fwd(finish)");
  return EVP_OK;
}

extern "C" int evp_flow_objective_bwd(const float *map, int64_t ld, int B, int h, int w, int H, int W, const float *target, const float *valid,
                                      float max_flow, const float *saved, const float *g_loss, float *grad, int64_t ldg, void *stream) {
  if (int rc = check_geom("evp_flow_objective_bwd", map, ld, B, h, w, H, W, target, valid)) return rc;
  EVP_CHECK_ARG(saved && g_loss && grad, EVP_EINVAL, "evp_flow_objective_bwd: null pointer");
  EVP_CHECK_ARG(ldg >= 2 && ldg < (1 << 20), EVP_ESHAPE, "evp_flow_objective_bwd: bad leading dimension %lld of the gradient", (long long)ldg);
  const FlGeom g = geom_of(map, ld, B, h, w, H, W, target, valid, max_flow);
  // pixels a cell can own: (2 H / h + 5) x (2 W / w + 5); a small footprint (same-size maps, downsampling) takes one wave per cell
  const int64_t foot = (2 * (int64_t)H / h + 5) * (2 * (int64_t)W / w + 5);
  hipLaunchKernelGGL(flow_bwd_kernel, dim3((unsigned)((int64_t)B * h * w)), dim3(foot > 128 ? FL_THREADS : 64), 0, (hipStream_t)stream, g, saved,
                     g_loss, grad, ldg);
  EVP_CHECK_LAUNCH("evp_flow_objective_bwd");
  return EVP_OK;
}

extern "C" int evp_flow_metrics(const float *map, int64_t ld, int B, int h, int w, int H, int W, const float *target, const float *valid,
                                float max_flow, const float *org, int org_channels, int64_t *cursor, float *table, int64_t capacity,
                                void *workspace, void *stream) {
  if (int rc = check_geom("evp_flow_metrics", map, ld, B, h, w, H, W, target, valid)) return rc;
  EVP_CHECK_ARG(org && cursor && table && workspace, EVP_EINVAL, "evp_flow_metrics: null pointer");
  EVP_CHECK_ARG(org_channels >= 1, EVP_ESHAPE, "evp_flow_metrics: %d channels of the event grid (at least one)", org_channels);
  EVP_CHECK_ARG(capacity > 0, EVP_ESHAPE, "evp_flow_metrics: the table needs at least one slot");
  const FlGeom g = geom_of(map, ld, B, h, w, H, W, target, valid, max_flow);
  const int64_t P = (int64_t)B * H * W;
  const int nblk = nblk_of(P);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(flow_pixel_kernel<true>, dim3((unsigned)nblk), dim3(FL_THREADS), 0, s, g, P, org, org_channels, (uint32_t *)workspace);
  EVP_CHECK_LAUNCH("evp_flow_metrics");
  hipLaunchKernelGGL(flow_finish_kernel<true>, dim3(1), dim3(FL_USED * 64), 0, s, (const uint32_t *)workspace, nblk, (float *)nullptr,
                     (float *)nullptr, cursor, table, capacity);
  EVP_CHECK_LAUNCH("evp_flow_metrics(finish)");
  return EVP_OK;
}

// GPU side of the dense fine-tuning loaders (semantic segmentation, optical flow): what the reference's dense datasets do per sample on a
// DataLoader worker besides the voxel-grid chain --
//   * the LABEL's view: semseg_label_augment / flow_label_augment / flow_label_valid_augment (dataset/augmentation/view_augment.py:91-134)
//     re-seed numpy with the sample's seed, so the label gets the grid's crop box and horizontal-flip coin: one gather per output pixel
//     under the SAME int32 [B,6] crop rows the grid's view kernel read (csrc/augment.hip), wherever they lie in device memory;
//   * DSEC's event rectification (dataset/finetune_semseg/ft_dsec_dataset.py:211-226) and DDD17's crop mask with the tail cut behind it
//     (ft_ddd17_dataset.py:116-127): a gather through the rectify map and a STABLE stream compaction per clip;
//   * MVSEC's flow label itself (dataset/finetune_flow/ft_mvsec_dataset.py:121-188): the pixel grid propagated through the resident
//     ground-truth flow frames, a handful of gathers per output pixel.
// All of it is HBM-bound: the label views write coalesced rows (8 B per pixel for the int64 label, 12 B for flow + valid) and gather 1 /
// 8 B; the compaction reads every row once per pass (32 B + 8 B of map) and writes the survivors as whole 32-byte rows, neighbouring
// survivors to neighbouring rows. No atomic orders anything: ranks come from wave ballots, an LDS exchange and a scan of chunk counts.
#include "evp_common.h"

// ---- label views --------------------------------------------------------------------------------------------------------------
// The index rule is view_augment_kernel's (csrc/augment.hip): F.interpolate(mode="nearest") on the cropped view, all in float32,
//   src = min((int)floorf((float)dst * ((float)in / (float)out)), in - 1), the flip acting on the resized view.
__device__ __forceinline__ int nearest_src(int dst, int n_in, float scale) {
  const int s = (int)floorf((float)dst * scale);
  return s < n_in - 1 ? s : n_in - 1;
}

// params[b] = {x0, y0, w, h, hflip, tflip}
__global__ __launch_bounds__(256) void semseg_label_augment_kernel(const uint8_t *__restrict__ in, const int32_t *__restrict__ params,
                                                                   int64_t *__restrict__ out, int Hin, int Win, int Hout, int Wout) {
  const int b = blockIdx.z, y = blockIdx.y;
  const int32_t *pr = params + (int64_t)b * 6;
  const int x0 = pr[0], y0 = pr[1], w = pr[2], h = pr[3], hflip = pr[4];
  const float sy = (float)h / (float)Hout, sx = (float)w / (float)Wout;
  const uint8_t *row = in + ((int64_t)b * Hin + y0 + nearest_src(y, h, sy)) * Win + x0;
  int64_t *dst = out + ((int64_t)b * Hout + y) * Wout;
  for (int x = blockIdx.x * 256 + threadIdx.x; x < Wout; x += gridDim.x * 256) {
    const int xr = hflip ? Wout - 1 - x : x;
    dst[x] = (int64_t)row[nearest_src(xr, w, sx)];
  }
}

__global__ __launch_bounds__(256) void flow_label_augment_kernel(const float *__restrict__ in, const int32_t *__restrict__ params,
                                                                 float *__restrict__ flow_out, float *__restrict__ valid_out, int Hin, int Win,
                                                                 int Hout, int Wout) {
  const int b = blockIdx.z, y = blockIdx.y;
  const int32_t *pr = params + (int64_t)b * 6;
  const int x0 = pr[0], y0 = pr[1], w = pr[2], h = pr[3], hflip = pr[4], tflip = pr[5];
  const float sy = (float)h / (float)Hout, sx = (float)w / (float)Wout;
  // flow * torch.tensor([new_w / org_w, new_h / org_h]): the quotients in double, rounded once into float32, the product in float32
  const float sxw = (float)((double)Wout / (double)w), syh = (float)((double)Hout / (double)h);
  const int64_t plane = (int64_t)Hin * Win;
  const float *rx = in + (int64_t)b * 2 * plane + (int64_t)(y0 + nearest_src(y, h, sy)) * Win + x0;
  const float *ry = rx + plane;
  const int64_t oplane = (int64_t)Hout * Wout;
  float *ox = flow_out + (int64_t)b * 2 * oplane + (int64_t)y * Wout;
  float *oy = ox + oplane;
  float *ov = valid_out + (int64_t)b * oplane + (int64_t)y * Wout;
  for (int x = blockIdx.x * 256 + threadIdx.x; x < Wout; x += gridDim.x * 256) {
    const int xr = hflip ? Wout - 1 - x : x;
    const int xs = nearest_src(xr, w, sx);
    const float fx = rx[xs], fy = ry[xs];
    float vx = fx * sxw, vy = fy * syh;
    if (hflip) vx = vx * -1.0f;
    if (tflip) {
      vx = vx * -1.0f;
      vy = vy * -1.0f;
    }
    // two roundings of the squares and one of the sum, whatever the contraction flags say
    const float sq = __fadd_rn(__fmul_rn(fx, fx), __fmul_rn(fy, fy));
    ox[x] = vx;
    oy[x] = vy;
    ov[x] = (sq > 0.0f && fabsf(fx) < 1000.0f && fabsf(fy) < 1000.0f) ? 1.0f : 0.0f;
  }
}

#define LABEL_SHAPE_OK(B, Hin, Win, Hout, Wout) \
  ((B) > 0 && (Hin) > 0 && (Win) > 0 && (Hout) > 0 && (Wout) > 0 && (B) <= 65535 && (Hout) <= 65535)

extern "C" int evp_semseg_label_augment(const uint8_t *labels, const int32_t *params, int64_t *out, int B, int Hin, int Win, int Hout,
                                        int Wout, void *stream) {
  EVP_CHECK_ARG(labels && params && out, EVP_EINVAL, "evp_semseg_label_augment: null pointer");
  EVP_CHECK_ARG(LABEL_SHAPE_OK(B, Hin, Win, Hout, Wout), EVP_ESHAPE, "evp_semseg_label_augment: bad shape (B=%d %dx%d -> %dx%d)", B, Hin,
                Win, Hout, Wout);
  const dim3 grid((unsigned)((Wout + 255) / 256), (unsigned)Hout, (unsigned)B);
  hipLaunchKernelGGL(semseg_label_augment_kernel, grid, dim3(256), 0, (hipStream_t)stream, labels, params, out, Hin, Win, Hout, Wout);
  EVP_CHECK_LAUNCH("evp_semseg_label_augment");
  return EVP_OK;
}

extern "C" int evp_flow_label_augment_f32(const float *flow, const int32_t *params, float *flow_out, float *valid_out, int B, int Hin,
                                          int Win, int Hout, int Wout, void *stream) {
  EVP_CHECK_ARG(flow && params && flow_out && valid_out, EVP_EINVAL, "evp_flow_label_augment_f32: null pointer");
  EVP_CHECK_ARG(LABEL_SHAPE_OK(B, Hin, Win, Hout, Wout), EVP_ESHAPE, "evp_flow_label_augment_f32: bad shape (B=%d %dx%d -> %dx%d)", B, Hin,
                Win, Hout, Wout);
  const dim3 grid((unsigned)((Wout + 255) / 256), (unsigned)Hout, (unsigned)B);
  hipLaunchKernelGGL(flow_label_augment_kernel, grid, dim3(256), 0, (hipStream_t)stream, flow, params, flow_out, valid_out, Hin, Win, Hout,
                     Wout);
  EVP_CHECK_LAUNCH("evp_flow_label_augment_f32");
  return EVP_OK;
}

// ---- MVSEC's ground-truth flow label: propagate a pixel grid through the flow frames ---------------------------------------------
// gen_correspond_gt_flow (dataset/finetune_flow/ft_mvsec_dataset.py:121-188) per output pixel: the frames of every sequence stay in
// device memory, a sample is a row of hops (frame index, float64 scale) the host made from two timestamps. A thread carries x, y and the
// two flags in registers; a hop is two 4- or 8-byte gathers at the rounded position (neighbouring pixels mostly read neighbouring cells),
// the two planes leave as coalesced rows. Floor: 8 B (float32 frames) gathered per hop and pixel + 8 B written.
//
// cv2.remap(..., INTER_NEAREST) picks its cell with cvRound: round half to EVEN, the border a constant 0. That rule is stated from
// OpenCV's source and has NOT been checked against a real cv2 (tests/golden/mvsec_gt_flow.npz was made with a stand-in that states the
// same rule); it lives in this one function, so a correction is one line.
__device__ __forceinline__ float remap_nearest_round(float v) { return rintf(v); }

// frame's two planes at the cell (x, y) rounds to; outside the frame, and for a NaN (which fails every comparison): 0
template <typename T>
__device__ __forceinline__ void gt_flow_fetch(const T *__restrict__ frame, int H, int W, float x, float y, double &ax, double &ay) {
  const float rx = remap_nearest_round(x), ry = remap_nearest_round(y);
  ax = ay = 0.0;
  if (rx >= 0.0f && rx < (float)W && ry >= 0.0f && ry < (float)H) {       // (-0.0 names column 0)
    const int64_t cell = (int64_t)(int)ry * W + (int)rx;
    ax = (double)frame[cell];
    ay = (double)frame[(int64_t)H * W + cell];
  }
}

template <typename T>
__global__ __launch_bounds__(256) void mvsec_flow_propagate_kernel(const T *__restrict__ frames, int64_t n_frames, int H, int W,
                                                                   const int64_t *__restrict__ hop_frame,
                                                                   const double *__restrict__ hop_scale, const int32_t *__restrict__ n_hops,
                                                                   int max_hops, float *__restrict__ out, int32_t *__restrict__ status) {
  const int b = blockIdx.y;
  const int n = n_hops[b];
  const int64_t *hf = hop_frame + (int64_t)b * max_hops;
  const double *hs = hop_scale + (int64_t)b * max_hops;
  // the sample's table, checked by every thread alike (uniform: no divergence): a row that names no frame is never followed
  bool bad = n < 0 || n > max_hops;
  if (!bad) {
    const int rows = n == 0 ? 1 : n;                                      // the direct branch reads row 0
    for (int k = 0; k < rows; ++k) bad |= hf[k] < 0 || hf[k] >= n_frames;
  }
  if (bad) {
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(status, 1);        // a counter, not an order
    return;
  }
  const int64_t plane = (int64_t)H * W;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= plane) return;
  float *ox = out + (int64_t)b * 2 * plane + p, *oy = ox + plane;
  if (n == 0) {
    // x_flow *= pre_dt / gt_dt: the product in float64, rounded once into the frame's dtype (then, a float64 frame, into the label's)
    const T *frame = frames + hf[0] * 2 * plane;
    const double s = hs[0];
    *ox = (float)(T)__dmul_rn((double)frame[p], s);
    *oy = (float)(T)__dmul_rn((double)frame[plane + p], s);
    return;
  }
  const int row = (int)(p / W), col = (int)(p - (int64_t)row * W);
  float x = (float)col, y = (float)row;
  bool x_ok = true, y_ok = true;
  for (int k = 0; k < n; ++k) {
    const double s = hs[k];
    double ax, ay;
    gt_flow_fetch(frames + hf[k] * 2 * plane, H, W, x, y, ax, ay);        // both planes at the position BEFORE the update
    x_ok &= ax != 0.0;
    y_ok &= ay != 0.0;
    // x_indices += flow_x_interp * scale_factor: product and sum each rounded to float64, then once to float32 -- never an FMA
    x = (float)__dadd_rn((double)x, __dmul_rn(ax, s));
    y = (float)__dadd_rn((double)y, __dmul_rn(ay, s));
  }
  *ox = x_ok ? __fsub_rn(x, (float)col) : 0.0f;
  *oy = y_ok ? __fsub_rn(y, (float)row) : 0.0f;
}

extern "C" int evp_mvsec_flow_propagate(const void *frames, int frames_dtype, int64_t n_frames, int H, int W, const int64_t *hop_frame,
                                        const double *hop_scale, const int32_t *n_hops, int B, int max_hops, float *label_out,
                                        int32_t *status, void *stream) {
  EVP_CHECK_ARG(frames && hop_frame && hop_scale && n_hops && label_out && status, EVP_EINVAL, "evp_mvsec_flow_propagate: null pointer");
  EVP_CHECK_ARG(frames_dtype == EVP_F32 || frames_dtype == EVP_F64, EVP_EINVAL,
                "evp_mvsec_flow_propagate: frames_dtype %d (EVP_F32 or EVP_F64)", frames_dtype);
  EVP_CHECK_ARG((((uintptr_t)frames) & (frames_dtype == EVP_F64 ? 7 : 3)) == 0 && (((uintptr_t)hop_frame | (uintptr_t)hop_scale) & 7) == 0,
                EVP_EINVAL, "evp_mvsec_flow_propagate: frames, hop_frame and hop_scale must be aligned to their elements");
  EVP_CHECK_ARG(n_frames > 0 && H > 0 && W > 0 && B > 0 && B <= 65535 && max_hops > 0 && (int64_t)H * W < (1ll << 31), EVP_ESHAPE,
                "evp_mvsec_flow_propagate: bad shape (n_frames=%lld %dx%d B=%d max_hops=%d)", (long long)n_frames, H, W, B, max_hops);
  const dim3 grid((unsigned)ceil_div64((int64_t)H * W, 256), (unsigned)B);
  if (frames_dtype == EVP_F64)
    hipLaunchKernelGGL(mvsec_flow_propagate_kernel<double>, grid, dim3(256), 0, (hipStream_t)stream, (const double *)frames, n_frames, H, W,
                       hop_frame, hop_scale, n_hops, max_hops, label_out, status);
  else
    hipLaunchKernelGGL(mvsec_flow_propagate_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float *)frames, n_frames, H, W,
                       hop_frame, hop_scale, n_hops, max_hops, label_out, status);
  EVP_CHECK_LAUNCH("evp_mvsec_flow_propagate");
  return EVP_OK;
}

// ---- rectify + mask + tail: a stable compaction per clip -----------------------------------------------------------------------
// A chunk = EVP_RECTIFY_CHUNK_ROWS rows of one clip = one workgroup of four waves; wave v owns the chunk's rows [256 v, 256 v + 256) as
// four runs of 64, lane l the row 64 j + l of run j: a run is 2 KB of contiguous input, and the survivors of a run are ranked by one
// ballot, so lanes that keep neighbouring rows store neighbouring rows.
//   counts   each chunk's survivor count -> ws[c * nchunk + k]
//   scan     ONE workgroup: exclusive scan of the n_clips * nchunk counts in place (ws[n_clips * nchunk] = the total), then the clips'
//            kept counts min(T_c, keep_last) -> offsets_out, the status words
//   scatter  row of rank r among clip c's T_c survivors -> offsets_out[c] + r - max(T_c - keep_last, 0), where that is not negative
#define RC_CHUNK EVP_RECTIFY_CHUNK_ROWS
#define RC_RUNS (RC_CHUNK / 256)
#define RC_SCAN_THREADS 1024

struct RcArgs {
  const double *in;
  const int64_t *off;
  const float *map;
  int64_t n_rows_in, max_rows;
  int map_h, map_w, H, W, nchunk;
};

struct RcRow {
  double x, y, t, p;
  bool keep;
};

// row r (absolute) of the input -> its output form and whether it stays; *outside: (int)x, (int)y names no cell of the map
__device__ __forceinline__ RcRow rc_visit(const RcArgs &a, int64_t r, bool live, bool &outside) {
  RcRow o;
  o.x = o.y = o.t = o.p = 0.0;
  o.keep = false;
  outside = false;
  if (!live) return o;
  const double2 xy = *reinterpret_cast<const double2 *>(a.in + r * 4), tp = *reinterpret_cast<const double2 *>(a.in + r * 4 + 2);
  o.t = tp.x;
  o.p = tp.y;
  double xr = xy.x, yr = xy.y;
  if (a.map) {
    // (int) truncates toward zero: every value in (-1, map_w) names a column; a NaN names none
    if (!(xr > -1.0 && xr < (double)a.map_w && yr > -1.0 && yr < (double)a.map_h)) {
      outside = true;
      return o;
    }
    const float2 m = *reinterpret_cast<const float2 *>(a.map + ((int64_t)(int)yr * a.map_w + (int)xr) * 2);
    xr = (double)m.x;
    yr = (double)m.y;
  }
  o.x = xr;
  o.y = yr;
  o.keep = xr >= 0.0 && xr < (double)a.W && yr >= 0.0 && yr < (double)a.H;      // a NaN drops, -0.0 stays, xr == W drops
  return o;
}

// the rows of clip c this kernel may read: [beg, beg + n)
__device__ __forceinline__ void rc_clip(const RcArgs &a, int c, int64_t &beg, int64_t &n) {
  beg = a.off[c];
  n = a.off[c + 1] - beg;
  if (beg < 0 || n < 0) n = 0;
  if (n > a.max_rows) n = a.max_rows;                                   // (the scan kernel counts such a clip in status[1])
  if (beg + n > a.n_rows_in) n = a.n_rows_in > beg ? a.n_rows_in - beg : 0;
}

__global__ __launch_bounds__(256) void rc_count_kernel(RcArgs a, int32_t *__restrict__ ws, int32_t *__restrict__ status) {
  __shared__ int s_cnt[4], s_out[4];
  const int c = blockIdx.y, k = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int64_t beg, n;
  rc_clip(a, c, beg, n);
  const int64_t base = (int64_t)k * RC_CHUNK + wave * 256;
  int cnt = 0, n_out = 0;
  if (base < n) {
#pragma unroll
    for (int j = 0; j < RC_RUNS; ++j) {
      const int64_t r = base + j * 64 + lane;
      bool outside;
      const RcRow row = rc_visit(a, beg + r, r < n, outside);
      cnt += __popcll(__ballot(row.keep));
      n_out += __popcll(__ballot(outside));
    }
  }
  if (lane == 0) s_cnt[wave] = cnt, s_out[wave] = n_out;
  __syncthreads();
  if (threadIdx.x == 0) {
    ws[(int64_t)c * a.nchunk + k] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    const int bad = s_out[0] + s_out[1] + s_out[2] + s_out[3];
    if (bad) atomicAdd(status + 1, bad);                                // a counter, not an order
  }
}

// exclusive scan of one int per thread over RC_SCAN_THREADS threads; red: 16 ints of LDS; -> the thread's prefix, total = the block's sum
__device__ __forceinline__ int rc_block_scan(int v, int *red, int &total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(inc, o, 64);
    if (lane >= o) inc += up;
  }
  __syncthreads();                                                      // (red may still be read from the call before)
  if (lane == 63) red[wave] = inc;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int i = 0; i < RC_SCAN_THREADS / 64; ++i) {
    const int t = red[i];
    before += i < wave ? t : 0;
    all += t;
  }
  total = all;
  return before + inc - v;
}

__global__ __launch_bounds__(RC_SCAN_THREADS) void rc_scan_kernel(RcArgs a, int n_clips, int64_t keep_last, int32_t *__restrict__ ws,
                                                                   int64_t *__restrict__ off_out, int32_t *__restrict__ status) {
  __shared__ int red[RC_SCAN_THREADS / 64];
  const int tid = threadIdx.x;
  const int64_t N = (int64_t)n_clips * a.nchunk;
  const int64_t per = (N + RC_SCAN_THREADS - 1) / RC_SCAN_THREADS;
  const int64_t i0 = tid * per < N ? tid * per : N, i1 = i0 + per < N ? i0 + per : N;
  int sum = 0;
  for (int64_t i = i0; i < i1; ++i) sum += ws[i];
  int total;
  int run = rc_block_scan(sum, red, total);
  for (int64_t i = i0; i < i1; ++i) {
    const int v = ws[i];
    ws[i] = run;
    run += v;
  }
  if (tid == 0) ws[N] = total, off_out[0] = 0;
  __syncthreads();                                                      // the prefixes other threads wrote are read below
  int carry = 0, empty = 0, bad = 0;
  for (int c0 = 0; c0 < n_clips; c0 += RC_SCAN_THREADS) {
    const int c = c0 + tid;
    int kept = 0;
    if (c < n_clips) {
      const int T = ws[(int64_t)(c + 1) * a.nchunk] - ws[(int64_t)c * a.nchunk];
      kept = (int64_t)T < keep_last ? T : (int)keep_last;
      empty += T == 0;
      const int64_t beg = a.off[c], n = a.off[c + 1] - beg;
      bad += beg < 0 || n < 0 || n > a.max_rows || beg + n > a.n_rows_in;        // rows of this clip were left unread
    }
    int tile;
    const int pre = rc_block_scan(kept, red, tile);
    if (c < n_clips) off_out[c + 1] = (int64_t)carry + pre + kept;
    carry += tile;
  }
  if (empty) atomicAdd(status, empty);
  if (bad) atomicAdd(status + 1, bad);
}

__global__ __launch_bounds__(256) void rc_scatter_kernel(RcArgs a, int64_t keep_last, const int32_t *__restrict__ ws,
                                                         const int64_t *__restrict__ off_out, double *__restrict__ out, int64_t out_rows) {
  __shared__ int s_cnt[4];
  const int c = blockIdx.y, k = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int64_t beg, n;
  rc_clip(a, c, beg, n);
  if ((int64_t)k * RC_CHUNK >= n) return;                               // (the whole workgroup: no barrier is left waiting)
  const int64_t base = (int64_t)k * RC_CHUNK + wave * 256;
  RcRow rows[RC_RUNS];
  int pre[RC_RUNS], cnt = 0;
#pragma unroll
  for (int j = 0; j < RC_RUNS; ++j) {
    const int64_t r = base + j * 64 + lane;
    bool outside;
    rows[j] = rc_visit(a, beg + r, r < n, outside);
    const unsigned long long m = __ballot(rows[j].keep);
    pre[j] = cnt + __popcll(m & ((1ull << lane) - 1ull));
    cnt += __popcll(m);
  }
  if (lane == 0) s_cnt[wave] = cnt;
  __syncthreads();
  int before = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) before += i < wave ? s_cnt[i] : 0;
  const int64_t clip0 = ws[(int64_t)c * a.nchunk];
  const int64_t T = ws[(int64_t)(c + 1) * a.nchunk] - clip0;
  const int64_t skip = T > keep_last ? T - keep_last : 0;
  const int64_t rank0 = ws[(int64_t)c * a.nchunk + k] - clip0 + before - skip;
  const int64_t dst0 = off_out[c];
#pragma unroll
  for (int j = 0; j < RC_RUNS; ++j) {
    const int64_t rank = rank0 + pre[j];
    const int64_t d = dst0 + rank;
    if (rows[j].keep && rank >= 0 && d < out_rows) {
      *reinterpret_cast<double2 *>(out + d * 4) = make_double2(rows[j].x, rows[j].y);
      *reinterpret_cast<double2 *>(out + d * 4 + 2) = make_double2(rows[j].t, rows[j].p);
    }
  }
}

static int64_t rc_nchunk(int64_t max_rows) { return max_rows > 0 ? ceil_div64(max_rows, RC_CHUNK) : 1; }

extern "C" int64_t evp_events_rectify_compact_ws_words(int n_clips, int64_t max_rows_per_clip) {
  return (int64_t)n_clips * rc_nchunk(max_rows_per_clip) + 1;
}

extern "C" int evp_events_rectify_compact_f64(const double *events_in, int64_t n_rows_in, const int64_t *offsets_in, int n_clips,
                                              int64_t max_rows_per_clip, const float *map, int map_h, int map_w, int H, int W,
                                              int64_t keep_last, double *events_out, int64_t out_rows, int64_t *offsets_out, int32_t *status,
                                              int32_t *workspace, void *stream) {
  EVP_CHECK_ARG(events_in && offsets_in && events_out && offsets_out && status && workspace, EVP_EINVAL,
                "evp_events_rectify_compact_f64: null pointer");
  EVP_CHECK_ARG((((uintptr_t)events_in | (uintptr_t)events_out) & 15) == 0 && (((uintptr_t)map) & 7) == 0, EVP_EINVAL,
                "evp_events_rectify_compact_f64: event rows must be 16-byte aligned, the map 8-byte aligned");
  EVP_CHECK_ARG(events_in != events_out, EVP_EINVAL, "evp_events_rectify_compact_f64: the compaction does not run in place");
  EVP_CHECK_ARG(n_clips > 0 && n_clips <= 65535 && max_rows_per_clip > 0 && n_rows_in >= 0 && H > 0 && W > 0 && keep_last > 0 &&
                    out_rows >= 0 && (!map || (map_h > 0 && map_w > 0)),
                EVP_ESHAPE, "evp_events_rectify_compact_f64: bad shape (n_clips=%d max_rows=%lld map %dx%d extent %dx%d keep_last=%lld)", n_clips,
                (long long)max_rows_per_clip, map_h, map_w, H, W, (long long)keep_last);
  const int64_t nchunk = rc_nchunk(max_rows_per_clip);
  EVP_CHECK_ARG((int64_t)n_clips * nchunk * RC_CHUNK < (1ll << 31) && nchunk <= 0x7fffffffll, EVP_ESHAPE,
                "evp_events_rectify_compact_f64: n_clips x max_rows_per_clip must stay below 2^31 rows (the ranks are int32)");
  RcArgs a;
  a.in = events_in, a.off = offsets_in, a.map = map, a.n_rows_in = n_rows_in, a.max_rows = max_rows_per_clip;
  a.map_h = map_h, a.map_w = map_w, a.H = H, a.W = W, a.nchunk = (int)nchunk;
  const dim3 grid((unsigned)nchunk, (unsigned)n_clips);
  hipLaunchKernelGGL(rc_count_kernel, grid, dim3(256), 0, (hipStream_t)stream, a, workspace, status);
  EVP_CHECK_LAUNCH("evp_events_rectify_compact_f64 (counts)");
  hipLaunchKernelGGL(rc_scan_kernel, dim3(1), dim3(RC_SCAN_THREADS), 0, (hipStream_t)stream, a, n_clips, keep_last, workspace, offsets_out,
                     status);
  EVP_CHECK_LAUNCH("evp_events_rectify_compact_f64 (scan)");
  hipLaunchKernelGGL(rc_scatter_kernel, grid, dim3(256), 0, (hipStream_t)stream, a, keep_last, (const int32_t *)workspace,
                     (const int64_t *)offsets_out, events_out, out_rows);
  EVP_CHECK_LAUNCH("evp_events_rectify_compact_f64 (scatter)");
  return EVP_OK;
}

// Row-wise (LayerNorm family) and column-wise (bias-gradient, BatchNorm) reductions for gfx950.
// All HBM-bound: one 64-lane wave owns one row, holds it in registers as float4 chunks (lane-strided, so every
// wave-instruction moves 1 KiB contiguous), reduces with cross-lane shuffles, writes once.
#include <cstdlib>
#include "evp_common.h"

namespace {

constexpr int ROWS_PER_BLOCK = 4;  // 4 waves / 256 threads (8 waves per block measured 10-25 % slower)
constexpr int LN_THREADS = ROWS_PER_BLOCK * 64;
constexpr int LN_MAX_BLOCKS = 512;   // backward: also the number of dgamma / dbeta / column-sum partial rows. Round 3, same-box A/B of the
                                     // ViT-Base step: 1024 blocks 10.94-11.00 ms, 768 10.86-10.88, 512 10.84-10.88, 392 10.85-10.88 -- the
                                     // partial rows (nblk x 3 D floats per launch) are written here and read again by the grouped column sum
constexpr int LN_FWD_BLOCKS = 2048;  // forward has no partials: one row per wave up to 8192 rows

// Number of float4 chunks a lane holds for a row of D floats
static inline int vpl_for(int D) {
  const int chunks = D / 4;
  const int v = (chunks + 63) / 64;
  int r = 1;
  while (r < v) r <<= 1;
  return r;
}

__device__ __forceinline__ void add4(float4 &a, float4 b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }

template <int VPL> struct Row {
  float4 v[VPL];
  __device__ __forceinline__ void load(const float *p, int D, int lane) {
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = lane + 64 * i;
      v[i] = (c * 4 < D) ? *reinterpret_cast<const float4 *>(p + c * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  __device__ __forceinline__ void add(const float *p, int D, int lane) {
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = lane + 64 * i;
      if (c * 4 < D) add4(v[i], *reinterpret_cast<const float4 *>(p + c * 4));
    }
  }
  __device__ __forceinline__ void load_any(const void *p, int dtype, int64_t off, int D, int lane) {
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = lane + 64 * i;
      if (c * 4 < D) v[i] = ld4_any(p, dtype, off + c * 4);   // (if / else: as a select, ln_bwd_kernel<2 and 4, false> wait 13 and 23
      else v[i] = make_float4(0.f, 0.f, 0.f, 0.f);            // more times for their loads, with register copies behind the waits)
    }
  }
  __device__ __forceinline__ float sum(int D, int lane) const {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i)
      if ((lane + 64 * i) * 4 < D) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    return wave_sum(s);
  }
  __device__ __forceinline__ float sumsq_centered(float mu, int D, int lane) const {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i)
      if ((lane + 64 * i) * 4 < D) {
        const float a = v[i].x - mu, b = v[i].y - mu, c = v[i].z - mu, d = v[i].w - mu;
        s += (a * a + b * b) + (c * c + d * d);
      }
    return wave_sum(s);
  }
};

// ------------------------------------------------------------------------------------------------ LN arithmetic
// Written once: the LayerNorm and the patch-embed kernels below compose these and keep only what differs.
template <int VPL>
__device__ __forceinline__ void ln_row_stats(const Row<VPL> &row, int D, int lane, float eps, float &mu, float &rs) {
  mu = row.sum(D, lane) / (float)D;
  const float var = row.sumsq_centered(mu, D, lane) / (float)D;
  rs = 1.0f / sqrtf(var + eps);
}
__device__ __forceinline__ float4 ln_xhat(float4 x, float mu, float rs) {
  return make_float4((x.x - mu) * rs, (x.y - mu) * rs, (x.z - mu) * rs, (x.w - mu) * rs);
}
// the LayerNorm output z = xhat * gamma + beta
__device__ __forceinline__ float4 ln_affine(float4 xh, float4 g, float4 b) {
  return make_float4(xh.x * g.x + b.x, xh.y * g.y + b.y, xh.z * g.z + b.z, xh.w * g.w + b.w);
}
// Backward, one chunk of one row; d = the gradient w.r.t. z. A live row adds d * xhat to dgamma and d to dbeta; every row adds its
// share of s1 = sum t and s2 = sum t * xhat, t = d * gamma (returned).
__device__ __forceinline__ float4 ln_bwd_step(float4 d, float4 xh, float4 g, bool live, float4 &dg, float4 &db, float &s1, float &s2) {
  if (live) {
    add4(dg, make_float4(d.x * xh.x, d.y * xh.y, d.z * xh.z, d.w * xh.w));
    add4(db, d);
  }
  const float4 t = make_float4(d.x * g.x, d.y * g.y, d.z * g.z, d.w * g.w);
  s1 += (t.x + t.y) + (t.z + t.w);
  s2 += (t.x * xh.x + t.y * xh.y) + (t.z * xh.z + t.w * xh.w);
  return t;
}
// dx = rstd * (t - m1 - xhat * m2) with the row means m1 = s1 / D, m2 = s2 / D
__device__ __forceinline__ float4 ln_bwd_out(float4 t, float4 xh, float rs, float m1, float m2) {
  return make_float4(rs * (t.x - m1 - xh.x * m2), rs * (t.y - m1 - xh.y * m2), rs * (t.z - m1 - xh.z * m2), rs * (t.w - m1 - xh.w * m2));
}
// combine the 4 waves' column partials (NP rows of D floats each, sh = [ROWS_PER_BLOCK][NP][D]) through LDS, then one store per
// block: part[blk][p][D] = sum over the waves of acc[p]
template <int NP, int VPL>
__device__ __forceinline__ void ln_flush_partials(const float4 (&acc)[NP][VPL], float *sh, int D, int lane, int wave, float *part) {
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int c = lane + 64 * i;
    if (c * 4 < D) {
#pragma unroll
      for (int p = 0; p < NP; ++p) *reinterpret_cast<float4 *>(sh + (wave * NP + p) * D + c * 4) = acc[p][i];
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < NP * D; e += blockDim.x) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < ROWS_PER_BLOCK; ++w) s += sh[w * NP * D + e];
    part[(int64_t)blockIdx.x * NP * D + e] = s;
  }
}

// ------------------------------------------------------------------------------------------------ LN forward
template <int VPL>
__global__ __launch_bounds__(LN_THREADS) void ln_fwd_kernel(const float *x, const float *x2, const float *x3, const float *gamma,
                                                     const float *beta, int64_t M, int D, float eps, void *y, int y_dtype,
                                                     float *mean, float *rstd) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t r = (int64_t)blockIdx.x * ROWS_PER_BLOCK + wave; r < M; r += (int64_t)gridDim.x * ROWS_PER_BLOCK) {
    Row<VPL> row;
    row.load(x + r * D, D, lane);
    if (x2) row.add(x2 + r * D, D, lane);
    if (x3) row.add(x3 + r * D, D, lane);
    float mu, rs;
    ln_row_stats(row, D, lane, eps, mu, rs);
    if (lane == 0) {
      if (mean) mean[r] = mu;
      if (rstd) rstd[r] = rs;
    }
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = lane + 64 * i;
      if (c * 4 < D) {
        const float4 g = *reinterpret_cast<const float4 *>(gamma + c * 4);
        const float4 b = *reinterpret_cast<const float4 *>(beta + c * 4);
        st4_any(y, y_dtype, r * D + c * 4, ln_affine(ln_xhat(row.v[i], mu, rs), g, b));
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ LN backward
// partial layout: part[blk][0][D] = dgamma partial, part[blk][1][D] = dbeta partial and, with CS, part[blk][2][D] = column sums
// of the OUTPUT dx (= the residual-stream gradient: its column sum is the bias gradient of the Linear that fed the stream,
// so the grouped column-sum launch reduces these few rows instead of re-reading the whole f32 gradient)
template <int VPL, bool CS>
__global__ __launch_bounds__(LN_THREADS) void ln_bwd_kernel(const void *dy, int dy_dtype, const float *x, const float *x2,
                                                     const float *x3, const float *gamma, const float *mean,
                                                     const float *rstd, const float *gres, int64_t M, int D, float *dx,
                                                     void *dx_lp, float *part) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float *sh = reinterpret_cast<float *>(smem_raw);  // [ROWS_PER_BLOCK][NP][D]
  constexpr int NP = CS ? 3 : 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float4 acc[NP][VPL];                              // dgamma, dbeta and, with CS, the column sums of dx
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int i = 0; i < VPL; ++i) acc[p][i] = make_float4(0.f, 0.f, 0.f, 0.f);

  // TWO rows per wave and iteration, every load of both rows (x, dy, the residual-stream gradient, the row statistics) requested
  // before anything is reduced: the one-row form issued x and dy, ran two shuffle reductions, and only then asked for gres -- 6-9
  // loads in flight per wave and a dependent HBM round trip in the middle of every row (42 launches at 3.8-4.4 TB/s).
  // Same-box A/B against the one-row form (tools/ab_step.py, round 3): 11.366 against 11.387 ms per ViT-Base step -- inside the noise;
  // the kernel is not bound by its loads in flight.
  // (rows wider than 1024 floats per 64 lanes -- VPL > 4 -- keep one row per iteration: two would spill)
  constexpr int NR = VPL <= 4 ? 2 : 1;
  const int64_t stride = (int64_t)gridDim.x * ROWS_PER_BLOCK;
  for (int64_t r0 = (int64_t)blockIdx.x * ROWS_PER_BLOCK + wave; r0 < M; r0 += NR * stride) {
    const int64_t rr[2] = {r0, r0 + stride};
    const bool live[2] = {true, r0 + stride < M};
    Row<VPL> xr[NR], gr[NR], qr[NR];
    float mu[NR], rs[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) {
      const int64_t r = live[k] ? rr[k] : r0;          // a dead second row re-reads the first (never stored, never summed)
      xr[k].load(x + r * D, D, lane);
      gr[k].load_any(dy, dy_dtype, r * D, D, lane);
      if (gres) qr[k].load(gres + r * D, D, lane);
      mu[k] = mean[r];
      rs[k] = rstd[r];
    }
#pragma unroll
    for (int k = 0; k < NR; ++k) {
      const int64_t r = live[k] ? rr[k] : r0;
      if (x2) xr[k].add(x2 + r * D, D, lane);
      if (x3) xr[k].add(x3 + r * D, D, lane);
    }
    float s1[2] = {0.f, 0.f}, s2[2] = {0.f, 0.f};      // (entries >= NR stay 0)
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = lane + 64 * i;
      if (c * 4 < D) {
        const float4 g = *reinterpret_cast<const float4 *>(gamma + c * 4);
#pragma unroll
        for (int k = 0; k < NR; ++k) {                 // x -> xhat and dy -> dy * gamma, in place
          const float4 xh = ln_xhat(xr[k].v[i], mu[k], rs[k]);
          gr[k].v[i] = ln_bwd_step(gr[k].v[i], xh, g, live[k], acc[0][i], acc[1][i], s1[k], s2[k]);
          xr[k].v[i] = xh;
        }
      }
    }
    // four reductions interleaved: the shuffles of one hide under the others' latency
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float a0 = __shfl_xor(s1[0], o, 64), a1 = __shfl_xor(s2[0], o, 64), a2 = __shfl_xor(s1[1], o, 64), a3 = __shfl_xor(s2[1], o, 64);
      s1[0] += a0; s2[0] += a1; s1[1] += a2; s2[1] += a3;
    }
#pragma unroll
    for (int k = 0; k < NR; ++k) {
      if (!live[k]) continue;
      const int64_t r = rr[k];
      const float m1 = s1[k] / (float)D, m2 = s2[k] / (float)D;
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        const int c = lane + 64 * i;
        if (c * 4 < D) {
          float4 o = ln_bwd_out(gr[k].v[i], xr[k].v[i], rs[k], m1, m2);
          if (gres) add4(o, qr[k].v[i]);
          if (dx) *reinterpret_cast<float4 *>(dx + r * D + c * 4) = o;
          if (dx_lp) st4_any(dx_lp, EVP_BF16, r * D + c * 4, o);
          if constexpr (CS) add4(acc[2][i], o);
        }
      }
    }
  }
  ln_flush_partials(acc, sh, D, lane, wave, part);
}

// out0[d] = sum_blk part[blk][0][d], out1[d] = sum_blk part[blk][1][d].
// 1024 threads = 64 columns x 16 partial-row groups: coalesced 256-byte reads, 16-way parallel over the partials.
__global__ __launch_bounds__(1024) void ln_bwd_finalize(const float *part, int nblk, int D, float *out0, float *out1) {
  __shared__ float sh[16][65];
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + c;
  float s = 0.f;
  if (e < 2 * D)
    for (int b = g; b < nblk; b += 16) s += part[(int64_t)b * 2 * D + e];
  sh[g][c] = s;
  __syncthreads();
  if (g == 0 && e < 2 * D) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) t += sh[i][c];
    if (e < D) { if (out0) out0[e] = t; }
    else { if (out1) out1[e - D] = t; }
  }
}

// backward grid cap; EVP_LN_BWD_BLOCKS overrides it for A/B runs (read once)
static inline int ln_bwd_cap() {
  static const int v = [] {
    const char *e = getenv("EVP_LN_BWD_BLOCKS");
    const int n = e ? atoi(e) : 0;
    return n >= 64 && n <= 8192 ? n : LN_MAX_BLOCKS;
  }();
  return v;
}
static inline int ln_grid(int64_t M, int cap = 0) {
  if (cap <= 0) cap = ln_bwd_cap();
  int64_t g = (M + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

// ------------------------------------------------------------------------------------------------ column sums
// out[n] += sum_m x[m,n]. Block = 16 column chunks (8 columns each, one 16/32-byte load per thread) x 16 row lanes
// over a slab of CS_ROWS rows; the 16 row lanes meet in LDS, then ONE f32 atomic per column and block.
constexpr int CS_ROWS = 256;
template <typename T>
__device__ __forceinline__ void colsum_body(const T *x, int64_t M, int N, int64_t ld, float *out, int col_block, int row_slab, float (*sh)[129]) {
  const int cc = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int n = col_block * 128 + cc * 8;
  const int64_t r0 = (int64_t)row_slab * CS_ROWS, r1 = r0 + CS_ROWS < M ? r0 + CS_ROWS : M;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (n < N) {
    const bool full = n + 7 < N;
    for (int64_t r = r0 + rl; r < r1; r += 16) {
      const T *p = x + r * ld + n;
      if (full) {
        float4 a, b;
        if constexpr (sizeof(T) == 2) {
          const uint4 u = *reinterpret_cast<const uint4 *>(p);
          a = unpack4_bf16(make_uint2(u.x, u.y)), b = unpack4_bf16(make_uint2(u.z, u.w));
        } else {
          a = *reinterpret_cast<const float4 *>(p), b = *reinterpret_cast<const float4 *>(p + 4);
        }
        acc[0] += a.x; acc[1] += a.y; acc[2] += a.z; acc[3] += a.w;
        acc[4] += b.x; acc[5] += b.y; acc[6] += b.z; acc[7] += b.w;
      } else {
        for (int e = 0; e < 8 && n + e < N; ++e) acc[e] += ElemIO<T>::ld(p + e);
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) sh[rl][cc * 8 + e] = acc[e];
  __syncthreads();
  if (threadIdx.x < 128) {
    const int c = threadIdx.x;
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) t += sh[i][c];
    if (col_block * 128 + c < N) atomicAdd(out + col_block * 128 + c, t);
  }
}
template <typename T>
__global__ __launch_bounds__(256) void colsum_kernel(const T *x, int64_t M, int N, int64_t ld, float *out) {
  __shared__ float sh[16][129];
  colsum_body(x, M, N, ld, out, blockIdx.x, blockIdx.y, sh);
}

// grouped form: many independent column sums in one launch (the deferred bias gradients of a whole step).
struct ColsumProblem { const void *x; float *out; long long M; int N, ld, dtype, pad; };
struct ColsumItem { int prob, col_block, row_slab, pad; };
__global__ __launch_bounds__(256) void colsum_grouped_kernel(const ColsumProblem *__restrict__ probs, const ColsumItem *__restrict__ items) {
  __shared__ float sh[16][129];
  const ColsumItem it = items[blockIdx.x];
  const ColsumProblem g = probs[it.prob];
  if (g.dtype == EVP_BF16) colsum_body((const bf16_t *)g.x, g.M, g.N, g.ld, g.out, it.col_block, it.row_slab, sh);
  else colsum_body((const float *)g.x, g.M, g.N, g.ld, g.out, it.col_block, it.row_slab, sh);
}

// ------------------------------------------------------------------------------------------------ patch-embed post-op
// out = GELU(LayerNorm(y)) + pos[token]: the LayerNorm kernels above, one row per iteration, plus the GELU and the position add
template <int VPL>
__global__ __launch_bounds__(LN_THREADS) void embed_post_fwd_kernel(const float *y, const float *gamma, const float *beta,
                                                             const float *pos, const int64_t *ids_keep, int64_t M,
                                                             int n_keep, int L, int D, float eps, float *out, float *mean,
                                                             float *rstd) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t r = (int64_t)blockIdx.x * ROWS_PER_BLOCK + wave; r < M; r += (int64_t)gridDim.x * ROWS_PER_BLOCK) {
    Row<VPL> row;
    row.load(y + r * D, D, lane);
    float mu, rs;
    ln_row_stats(row, D, lane, eps, mu, rs);
    if (lane == 0) { mean[r] = mu; rstd[r] = rs; }
    const int64_t tok = ids_keep ? ids_keep[r] : (r % L);
    const float *pr = pos ? pos + tok * D : nullptr;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = lane + 64 * i;
      if (c * 4 < D) {
        const float4 g = *reinterpret_cast<const float4 *>(gamma + c * 4);
        const float4 b = *reinterpret_cast<const float4 *>(beta + c * 4);
        const float4 pe = pr ? *reinterpret_cast<const float4 *>(pr + c * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 z = ln_affine(ln_xhat(row.v[i], mu, rs), g, b);
        *reinterpret_cast<float4 *>(out + r * D + c * 4) = make_float4(gelu_f(z.x) + pe.x, gelu_f(z.y) + pe.y, gelu_f(z.z) + pe.z, gelu_f(z.w) + pe.w);
      }
    }
  }
}

template <int VPL>
__global__ __launch_bounds__(LN_THREADS) void embed_post_bwd_kernel(const float *g_in, const float *y, const float *gamma,
                                                             const float *beta, const float *mean, const float *rstd,
                                                             int64_t M, int D, void *dy, int dy_dtype, float *part) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float *sh = reinterpret_cast<float *>(smem_raw);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float4 acc[2][VPL];                               // dgamma, dbeta
#pragma unroll
  for (int i = 0; i < VPL; ++i) acc[0][i] = acc[1][i] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t r = (int64_t)blockIdx.x * ROWS_PER_BLOCK + wave; r < M; r += (int64_t)gridDim.x * ROWS_PER_BLOCK) {
    Row<VPL> xr, gr;
    xr.load(y + r * D, D, lane);
    gr.load(g_in + r * D, D, lane);
    const float mu = mean[r], rs = rstd[r];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = lane + 64 * i;
      if (c * 4 < D) {
        const float4 g = *reinterpret_cast<const float4 *>(gamma + c * 4);
        const float4 b = *reinterpret_cast<const float4 *>(beta + c * 4);
        const float4 xh = ln_xhat(xr.v[i], mu, rs), z = ln_affine(xh, g, b), gi = gr.v[i];
        // gradient w.r.t. the LayerNorm output z = xh*gamma+beta
        const float4 d = make_float4(gi.x * dgelu_f(z.x), gi.y * dgelu_f(z.y), gi.z * dgelu_f(z.z), gi.w * dgelu_f(z.w));
        gr.v[i] = ln_bwd_step(d, xh, g, true, acc[0][i], acc[1][i], s1, s2);
        xr.v[i] = xh;
      }
    }
    s1 = wave_sum(s1) / (float)D;
    s2 = wave_sum(s2) / (float)D;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = lane + 64 * i;
      if (c * 4 < D) st4_any(dy, dy_dtype, r * D + c * 4, ln_bwd_out(gr.v[i], xr.v[i], rs, s1, s2));
    }
  }
  ln_flush_partials(acc, sh, D, lane, wave, part);
}

// ------------------------------------------------------------------------------------------------ BatchNorm over rows
// Every pass in two widths W: 1, one element per lane, and 4 (C % 4 == 0 and 16-byte aligned tensors), 16-byte (f32) / 8-byte (bf16)
// accesses. The per-slab passes run 256 / W column groups x W row lanes over one slab of BN_ROWS rows; at W = 4 the row lanes meet
// in LDS.
constexpr int BN_ROWS = 64;
template <int W> __device__ __forceinline__ void ldw_any(const void *p, int dtype, int64_t i, float (&v)[W]) {
  static_assert(W == 1 || W == 4, "BatchNorm widths");
  if constexpr (W == 4) {
    const float4 t = ld4_any(p, dtype, i);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else v[0] = ld_any(p, dtype, i);
}
template <int W> __device__ __forceinline__ void stw_any(void *p, int dtype, int64_t i, const float (&v)[W]) {
  if constexpr (W == 4) st4_any(p, dtype, i, make_float4(v[0], v[1], v[2], v[3]));
  else st_any(p, dtype, i, v[0]);
}
// dy' = the upstream gradient behind the ReLU (zero where the output y is not positive)
template <int W> __device__ __forceinline__ void bn_load_dy(const void *dy, const void *y, int dtype, int64_t i, int relu, float (&d)[W]) {
  ldw_any<W>(dy, dtype, i, d);
  if (relu) {
    float yv[W];
    ldw_any<W>(y, dtype, i, yv);
#pragma unroll
    for (int j = 0; j < W; ++j)
      if (!(yv[j] > 0.f)) d[j] = 0.f;
  }
}

// Welford per (slab, column): part[slab][0][C] = mean, part[slab][1][C] = M2, count = rows in slab
template <int W>
__global__ __launch_bounds__(256) void bn_stats_partial(const void *x, int dtype, int64_t R, int C, float *part) {
  constexpr int NG = 256 / W;
  const int cg = threadIdx.x % NG, rl = threadIdx.x / NG;
  const int c = blockIdx.x * 256 + cg * W;
  const int64_t r0 = (int64_t)blockIdx.y * BN_ROWS;
  const int64_t r1 = r0 + BN_ROWS < R ? r0 + BN_ROWS : R;
  float mean[W], m2[W];
#pragma unroll
  for (int j = 0; j < W; ++j) mean[j] = m2[j] = 0.f;
  int n = 0;
  if (c < C)
    for (int64_t r = r0 + rl; r < r1; r += W) {
      float v[W];
      ldw_any<W>(x, dtype, r * C + c, v);
      ++n;
#pragma unroll
      for (int j = 0; j < W; ++j) {
        const float d = v[j] - mean[j];
        if constexpr (W == 1) mean[j] += d / (float)n;   // pins the parent's rounding: width 1 divides, width 4 multiplies by 1 / n
        else mean[j] += d * (1.0f / (float)n);
        m2[j] += d * (v[j] - mean[j]);
      }
    }
  if constexpr (W == 1) {
    if (c < C) {
      part[((int64_t)blockIdx.y * 2 + 0) * C + c] = mean[0];
      part[((int64_t)blockIdx.y * 2 + 1) * C + c] = m2[0];
    }
  } else {
    __shared__ float sh[3][W][260];
#pragma unroll
    for (int j = 0; j < W; ++j) { sh[0][rl][cg * W + j] = (float)n; sh[1][rl][cg * W + j] = mean[j]; sh[2][rl][cg * W + j] = m2[j]; }
    __syncthreads();
    const int cc = threadIdx.x;                      // one column per thread for the combine
    if (blockIdx.x * 256 + cc < C) {
      float nn = sh[0][0][cc], mu = sh[1][0][cc], q = sh[2][0][cc];
      for (int i = 1; i < W; ++i) {
        const float nb = sh[0][i][cc];
        if (nb > 0.f) {
          const float delta = sh[1][i][cc] - mu, tot = nn + nb;
          mu += delta * nb / tot;
          q += sh[2][i][cc] + delta * delta * nn * nb / tot;
          nn = tot;
        }
      }
      part[((int64_t)blockIdx.y * 2 + 0) * C + blockIdx.x * 256 + cc] = mu;
      part[((int64_t)blockIdx.y * 2 + 1) * C + blockIdx.x * 256 + cc] = q;
    }
  }
}
// 1024 threads = 64 columns x 16 slab groups: each thread folds every 16th slab (Chan's pairwise update, in double), the 16 partial
// (n, mean, M2) triples of a column then meet in LDS. (One thread per column walking all R / 64 slabs serially took 68 us at
// R = 12 608, C = 4096: 16 workgroups, a dependent chain of 197 double-precision divisions each.)
__global__ __launch_bounds__(1024) void bn_stats_finalize(const float *part, int nslab, int64_t R, int C, float eps, float momentum, float *mean_out,
                                                          float *invstd_out, float *running_mean, float *running_var) {
  __shared__ double sh[3][16][65];
  const int cl = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  double mean = 0.0, m2 = 0.0, n = 0.0;
  if (c < C)
    for (int s = g; s < nslab; s += 16) {
      const int64_t r0 = (int64_t)s * BN_ROWS;
      const double nb = (double)((r0 + BN_ROWS < R ? r0 + BN_ROWS : R) - r0);
      const double mb = part[((int64_t)s * 2 + 0) * C + c], m2b = part[((int64_t)s * 2 + 1) * C + c];
      const double delta = mb - mean, tot = n + nb;
      mean += delta * nb / tot;
      m2 += m2b + delta * delta * n * nb / tot;
      n = tot;
    }
  sh[0][g][cl] = n; sh[1][g][cl] = mean; sh[2][g][cl] = m2;
  __syncthreads();
  if (g == 0 && c < C) {
    for (int i = 1; i < 16; ++i) {
      const double nb = sh[0][i][cl];
      if (nb > 0.0) {
        const double delta = sh[1][i][cl] - mean, tot = n + nb;
        mean += delta * nb / tot;
        m2 += sh[2][i][cl] + delta * delta * n * nb / tot;
        n = tot;
      }
    }
    const float var_b = (float)(m2 / n);
    mean_out[c] = (float)mean;
    invstd_out[c] = 1.0f / sqrtf(var_b + eps);
    if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * (float)mean;
    if (running_var) running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)(m2 / (n > 1.0 ? n - 1.0 : 1.0));
  }
}
template <int W>
__global__ __launch_bounds__(256) void bn_apply(const void *x, int dtype, int64_t total, int C, const float *gamma,
                                                const float *beta, const float *mean, const float *invstd, int relu, void *y) {
  for (int64_t iw = (int64_t)blockIdx.x * 256 + threadIdx.x; iw < total / W; iw += (int64_t)gridDim.x * 256) {
    const int64_t i = iw * W;
    const int c = (int)(i % C);
    float o[W], mu[W], is[W];
    ldw_any<W>(x, dtype, i, o);
    ldw_any<W>(mean, EVP_F32, c, mu);
    ldw_any<W>(invstd, EVP_F32, c, is);
#pragma unroll
    for (int j = 0; j < W; ++j) o[j] = (o[j] - mu[j]) * is[j];
    if (gamma) {
      float g[W], b[W];
      ldw_any<W>(gamma, EVP_F32, c, g);
      ldw_any<W>(beta, EVP_F32, c, b);
#pragma unroll
      for (int j = 0; j < W; ++j) o[j] = o[j] * g[j] + b[j];
    }
    if (relu) {
#pragma unroll
      for (int j = 0; j < W; ++j) o[j] = fmaxf(o[j], 0.f);
    }
    stw_any<W>(y, dtype, i, o);
  }
}
// part[slab][0][C] = sum dy', part[slab][1][C] = sum dy' * xhat
template <int W>
__global__ __launch_bounds__(256) void bn_bwd_partial(const void *dy, const void *x, const void *y, int dtype, int64_t R, int C,
                                                      const float *mean, const float *invstd, int relu, float *part) {
  constexpr int NG = 256 / W;
  const int cg = threadIdx.x % NG, rl = threadIdx.x / NG;
  const int c = blockIdx.x * 256 + cg * W;
  const int64_t r0 = (int64_t)blockIdx.y * BN_ROWS;
  const int64_t r1 = r0 + BN_ROWS < R ? r0 + BN_ROWS : R;
  float s0[W], s1[W];
#pragma unroll
  for (int j = 0; j < W; ++j) s0[j] = s1[j] = 0.f;
  if (c < C) {
    float mu[W], is[W];
    ldw_any<W>(mean, EVP_F32, c, mu);
    ldw_any<W>(invstd, EVP_F32, c, is);
    for (int64_t r = r0 + rl; r < r1; r += W) {
      float d[W], xv[W];
      bn_load_dy<W>(dy, y, dtype, r * C + c, relu, d);
      ldw_any<W>(x, dtype, r * C + c, xv);
#pragma unroll
      for (int j = 0; j < W; ++j) {
        s0[j] += d[j];
        s1[j] += d[j] * (xv[j] - mu[j]) * is[j];
      }
    }
  }
  if constexpr (W == 1) {
    if (c < C) {
      part[((int64_t)blockIdx.y * 2 + 0) * C + c] = s0[0];
      part[((int64_t)blockIdx.y * 2 + 1) * C + c] = s1[0];
    }
  } else {                                           // pins the parent's rounding: the four row lanes add pairwise
    __shared__ float sh[2][W][260];
#pragma unroll
    for (int j = 0; j < W; ++j) { sh[0][rl][cg * W + j] = s0[j]; sh[1][rl][cg * W + j] = s1[j]; }
    __syncthreads();
    const int cc = threadIdx.x;
    if (blockIdx.x * 256 + cc < C) {
      part[((int64_t)blockIdx.y * 2 + 0) * C + blockIdx.x * 256 + cc] = (sh[0][0][cc] + sh[0][1][cc]) + (sh[0][2][cc] + sh[0][3][cc]);
      part[((int64_t)blockIdx.y * 2 + 1) * C + blockIdx.x * 256 + cc] = (sh[1][0][cc] + sh[1][1][cc]) + (sh[1][2][cc] + sh[1][3][cc]);
    }
  }
}
__global__ __launch_bounds__(1024) void bn_bwd_finalize(const float *part, int nslab, int C, float *sum_dy, float *sum_dy_xhat) {
  __shared__ float sh[2][16][65];
  const int cl = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  float a = 0.f, b = 0.f;
  if (c < C)
    for (int s = g; s < nslab; s += 16) {
      a += part[((int64_t)s * 2 + 0) * C + c];
      b += part[((int64_t)s * 2 + 1) * C + c];
    }
  sh[0][g][cl] = a; sh[1][g][cl] = b;
  __syncthreads();
  if (g == 0 && c < C) {
    for (int i = 1; i < 16; ++i) { a += sh[0][i][cl]; b += sh[1][i][cl]; }
    sum_dy[c] = a;
    sum_dy_xhat[c] = b;
  }
}
template <int W>
__global__ __launch_bounds__(256) void bn_bwd_apply(const void *dy, const void *x, const void *y, int dtype, int64_t R, int C,
                                                    const float *gamma, const float *mean, const float *invstd, int relu,
                                                    const float *sum_dy, const float *sum_dy_xhat, void *dx) {
  const int64_t total = R * C;
  const float invR = 1.0f / (float)R;
  for (int64_t iw = (int64_t)blockIdx.x * 256 + threadIdx.x; iw < total / W; iw += (int64_t)gridDim.x * 256) {
    const int64_t i = iw * W;
    const int c = (int)(i % C);
    float d[W], xv[W], mu[W], is[W], s0[W], s1[W], g[W], o[W];
    bn_load_dy<W>(dy, y, dtype, i, relu, d);
    ldw_any<W>(x, dtype, i, xv);
    ldw_any<W>(mean, EVP_F32, c, mu);
    ldw_any<W>(invstd, EVP_F32, c, is);
    ldw_any<W>(sum_dy, EVP_F32, c, s0);
    ldw_any<W>(sum_dy_xhat, EVP_F32, c, s1);
    if (gamma) ldw_any<W>(gamma, EVP_F32, c, g);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const float xh = (xv[j] - mu[j]) * is[j];
      o[j] = (gamma ? g[j] : 1.f) * is[j] * (d[j] - s0[j] * invR - xh * s1[j] * invR);
    }
    stw_any<W>(dx, dtype, i, o);
  }
}

}  // namespace

#define DISPATCH_VPL(D, CALL)                                   \
  switch (vpl_for(D)) {                                         \
    case 1: { constexpr int V = 1; CALL; } break;               \
    case 2: { constexpr int V = 2; CALL; } break;               \
    case 4: { constexpr int V = 4; CALL; } break;               \
    case 8: { constexpr int V = 8; CALL; } break;               \
    default: { constexpr int V = 16; CALL; } break;             \
  }

// what every row kernel needs of its shape
static inline bool ln_shape_ok(int64_t M, int D) { return M > 0 && D > 0 && D % 4 == 0 && D <= 4096; }

// A backward launch: `lds` bytes of dynamic LDS (above 48 KiB the kernel's limit has to be raised first), then, with dgamma or dbeta
// given, the reduction of the per-block partial rows workspace[grid][2][D]. Both NULL: the caller reduces them itself (deferred, grouped).
template <typename... P, typename... A>
static int ln_bwd_launch(const char *entry, void (*kernel)(P...), int grid, size_t lds, hipStream_t s, float *workspace, int D, float *dgamma,
                         float *dbeta, A... args) {
  if (lds > 48 * 1024) {
    hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    EVP_CHECK_ARG(ea == hipSuccess, EVP_ELAUNCH, "%s: hipFuncSetAttribute(%zu) failed: %s", entry, lds, hipGetErrorString(ea));
  }
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(LN_THREADS), lds, s, args...);
  EVP_CHECK_LAUNCH(entry);
  if (dgamma || dbeta) {
    hipLaunchKernelGGL(ln_bwd_finalize, dim3((2 * D + 63) / 64), dim3(1024), 0, s, workspace, grid, D, dgamma, dbeta);
    hipError_t ef = hipGetLastError();
    EVP_CHECK_ARG(ef == hipSuccess, EVP_ELAUNCH, "%s(finalize): launch failed: %s", entry, hipGetErrorString(ef));
  }
  return EVP_OK;
}

extern "C" int evp_layernorm_fwd(const float *x, const float *x2, const float *x3, const float *gamma, const float *beta,
                                 int64_t M, int D, float eps, void *y, int y_dtype, float *mean, float *rstd, void *stream) {
  EVP_CHECK_ARG(x && gamma && beta && y, EVP_EINVAL, "evp_layernorm_fwd: null pointer");
  EVP_CHECK_ARG(ln_shape_ok(M, D), EVP_ESHAPE, "evp_layernorm_fwd: need M>0, D%%4==0, D<=4096 (M=%lld D=%d)", (long long)M, D);
  hipStream_t s = (hipStream_t)stream;
  DISPATCH_VPL(D, hipLaunchKernelGGL(ln_fwd_kernel<V>, dim3(ln_grid(M, LN_FWD_BLOCKS)), dim3(LN_THREADS), 0, s, x, x2, x3, gamma, beta, M, D, eps, y, y_dtype, mean, rstd));
  EVP_CHECK_LAUNCH("evp_layernorm_fwd");
  return EVP_OK;
}

extern "C" int evp_layernorm_bwd_nblk(int64_t M) { return ln_grid(M); }

extern "C" int evp_layernorm_bwd(const void *dy, int dy_dtype, const float *x, const float *x2, const float *x3,
                                 const float *gamma, const float *mean, const float *rstd, const float *gres, int64_t M, int D,
                                 float *dx, void *dx_lp, float *dgamma, float *dbeta, float *workspace, void *stream) {
  EVP_CHECK_ARG(dy && x && gamma && mean && rstd && workspace, EVP_EINVAL, "evp_layernorm_bwd: null pointer");
  EVP_CHECK_ARG(dx || dx_lp, EVP_EINVAL, "evp_layernorm_bwd: no output requested");
  EVP_CHECK_ARG(ln_shape_ok(M, D), EVP_ESHAPE, "evp_layernorm_bwd: need D%%4==0, D<=4096 (D=%d)", D);
  const size_t sh = (size_t)ROWS_PER_BLOCK * 2 * D * sizeof(float);
  int rc;
  DISPATCH_VPL(D, rc = ln_bwd_launch("evp_layernorm_bwd", ln_bwd_kernel<V, false>, ln_grid(M), sh, (hipStream_t)stream, workspace, D, dgamma, dbeta,
                                     dy, dy_dtype, x, x2, x3, gamma, mean, rstd, gres, M, D, dx, dx_lp, workspace));
  return rc;
}

extern "C" int evp_layernorm_bwd_cs(const void *dy, int dy_dtype, const float *x, const float *x2, const float *x3,
                                    const float *gamma, const float *mean, const float *rstd, const float *gres, int64_t M, int D,
                                    float *dx, void *dx_lp, float *workspace, void *stream) {
  EVP_CHECK_ARG(dy && x && gamma && mean && rstd && workspace, EVP_EINVAL, "evp_layernorm_bwd_cs: null pointer");
  EVP_CHECK_ARG(dx || dx_lp, EVP_EINVAL, "evp_layernorm_bwd_cs: no output requested");
  EVP_CHECK_ARG(ln_shape_ok(M, D), EVP_ESHAPE, "evp_layernorm_bwd_cs: need D%%4==0, D<=4096 (D=%d)", D);
  const size_t sh = (size_t)ROWS_PER_BLOCK * 3 * D * sizeof(float);
  // three partial rows per wave live in LDS: 160 KiB per workgroup is the limit (D <= 3412 at 4 rows per block); wider rows take
  // evp_layernorm_bwd (two partial rows) plus a column sum of dx (ops.layernorm_bwd does that by itself)
  EVP_CHECK_ARG(sh <= 160 * 1024, EVP_ESHAPE, "evp_layernorm_bwd_cs: D=%d needs %zu bytes of LDS (> 160 KiB); use evp_layernorm_bwd", D, sh);
  int rc;
  DISPATCH_VPL(D, rc = ln_bwd_launch("evp_layernorm_bwd_cs", ln_bwd_kernel<V, true>, ln_grid(M), sh, (hipStream_t)stream, workspace, D, nullptr, nullptr,
                                     dy, dy_dtype, x, x2, x3, gamma, mean, rstd, gres, M, D, dx, dx_lp, workspace));
  return rc;
}

extern "C" int evp_colsum_nblk(int64_t M) { return (int)((M + CS_ROWS - 1) / CS_ROWS); }

extern "C" int evp_colsum(const void *x, int x_dtype, int64_t M, int N, int64_t ld, float *out, float *workspace, void *stream) {
  (void)workspace;  // kept in the signature for ABI stability; the reduction now meets in LDS + one atomic per column
  EVP_CHECK_ARG(x && out, EVP_EINVAL, "evp_colsum: null pointer");
  EVP_CHECK_ARG(M > 0 && N > 0 && ld >= N && ld % 8 == 0, EVP_ESHAPE, "evp_colsum: bad shape (ld must be a multiple of 8)");
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = evp_zero_async(out, sizeof(float) * N, s);
  EVP_CHECK_ARG(e == hipSuccess, EVP_ELAUNCH, "evp_colsum: memset failed: %s", hipGetErrorString(e));
  dim3 grid((N + 127) / 128, evp_colsum_nblk(M));
  if (x_dtype == EVP_BF16) hipLaunchKernelGGL(colsum_kernel<bf16_t>, grid, dim3(256), 0, s, (const bf16_t *)x, M, N, ld, out);
  else hipLaunchKernelGGL(colsum_kernel<float>, grid, dim3(256), 0, s, (const float *)x, M, N, ld, out);
  EVP_CHECK_LAUNCH("evp_colsum");
  return EVP_OK;
}

extern "C" int evp_colsum_grouped(const void *problems, const void *items, int n_items, void *stream) {
  EVP_CHECK_ARG(problems && items && n_items > 0, EVP_EINVAL, "evp_colsum_grouped: bad argument");
  hipLaunchKernelGGL(colsum_grouped_kernel, dim3((unsigned)n_items), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const ColsumProblem *>(problems), reinterpret_cast<const ColsumItem *>(items));
  EVP_CHECK_LAUNCH("evp_colsum_grouped");
  return EVP_OK;
}

extern "C" int evp_embed_post_fwd(const float *y, const float *gamma, const float *beta, const float *pos,
                                  const int64_t *ids_keep, int B, int n_keep, int L, int D, float eps, float *out, float *mean,
                                  float *rstd, void *stream) {
  EVP_CHECK_ARG(y && gamma && beta && out && mean && rstd, EVP_EINVAL, "evp_embed_post_fwd: null pointer");
  EVP_CHECK_ARG(B > 0 && n_keep > 0 && n_keep <= L && ln_shape_ok((int64_t)B * n_keep, D), EVP_ESHAPE, "evp_embed_post_fwd: bad shape");
  hipStream_t s = (hipStream_t)stream;
  const int64_t M = (int64_t)B * n_keep;
  DISPATCH_VPL(D, hipLaunchKernelGGL(embed_post_fwd_kernel<V>, dim3(ln_grid(M)), dim3(LN_THREADS), 0, s, y, gamma, beta, pos, ids_keep, M, n_keep, L, D, eps, out, mean, rstd));
  EVP_CHECK_LAUNCH("evp_embed_post_fwd");
  return EVP_OK;
}

extern "C" int evp_embed_post_bwd(const float *g, const float *y, const float *gamma, const float *beta, const float *mean,
                                  const float *rstd, int64_t M, int D, void *dy, int dy_dtype, float *dgamma, float *dbeta,
                                  float *workspace, void *stream) {
  EVP_CHECK_ARG(g && y && gamma && beta && mean && rstd && dy && workspace, EVP_EINVAL, "evp_embed_post_bwd: null pointer");
  EVP_CHECK_ARG(ln_shape_ok(M, D), EVP_ESHAPE, "evp_embed_post_bwd: bad shape");
  const size_t sh = (size_t)ROWS_PER_BLOCK * 2 * D * sizeof(float);
  int rc;
  DISPATCH_VPL(D, rc = ln_bwd_launch("evp_embed_post_bwd", embed_post_bwd_kernel<V>, ln_grid(M), sh, (hipStream_t)stream, workspace, D, dgamma, dbeta,
                                     g, y, gamma, beta, mean, rstd, M, D, dy, dy_dtype, workspace));
  return rc;
}

extern "C" int evp_batchnorm_nblk(int64_t R) { return (int)((R + BN_ROWS - 1) / BN_ROWS); }

// the three launches of a BatchNorm direction at one width; grids: (256-column block, slab), 64 columns, 256 x W elements (capped)
static inline int bn_apply_grid(int64_t total, int W) {
  const int64_t g = (total / W + 255) / 256;
  return (int)(g > 4096 ? 4096 : g);
}
template <int W>
static int bn_fwd_launch(const void *x, int dtype, int64_t R, int C, const float *gamma, const float *beta, float eps, float momentum, int relu,
                         void *y, float *mean, float *invstd, float *running_mean, float *running_var, float *workspace, hipStream_t s) {
  const int ns = evp_batchnorm_nblk(R);
  hipLaunchKernelGGL(bn_stats_partial<W>, dim3((C + 255) / 256, ns), dim3(256), 0, s, x, dtype, R, C, workspace);
  EVP_CHECK_LAUNCH("evp_batchnorm_fwd(stats)");
  hipLaunchKernelGGL(bn_stats_finalize, dim3((C + 63) / 64), dim3(1024), 0, s, workspace, ns, R, C, eps, momentum, mean, invstd, running_mean, running_var);
  EVP_CHECK_LAUNCH("evp_batchnorm_fwd(finalize)");
  hipLaunchKernelGGL(bn_apply<W>, dim3(bn_apply_grid(R * C, W)), dim3(256), 0, s, x, dtype, R * C, C, gamma, beta, mean, invstd, relu, y);
  EVP_CHECK_LAUNCH("evp_batchnorm_fwd(apply)");
  return EVP_OK;
}
template <int W>
static int bn_bwd_launch(const void *dy, const void *x, const void *y, int dtype, int64_t R, int C, const float *gamma, const float *mean,
                         const float *invstd, int relu, void *dx, float *sum_dy, float *sum_dy_xhat, float *workspace, hipStream_t s) {
  const int ns = evp_batchnorm_nblk(R);
  hipLaunchKernelGGL(bn_bwd_partial<W>, dim3((C + 255) / 256, ns), dim3(256), 0, s, dy, x, y, dtype, R, C, mean, invstd, relu, workspace);
  EVP_CHECK_LAUNCH("evp_batchnorm_bwd(partial)");
  hipLaunchKernelGGL(bn_bwd_finalize, dim3((C + 63) / 64), dim3(1024), 0, s, workspace, ns, C, sum_dy, sum_dy_xhat);
  EVP_CHECK_LAUNCH("evp_batchnorm_bwd(finalize)");
  hipLaunchKernelGGL(bn_bwd_apply<W>, dim3(bn_apply_grid(R * C, W)), dim3(256), 0, s, dy, x, y, dtype, R, C, gamma, mean, invstd, relu, sum_dy, sum_dy_xhat, dx);
  EVP_CHECK_LAUNCH("evp_batchnorm_bwd(apply)");
  return EVP_OK;
}

extern "C" int evp_batchnorm_fwd(const void *x, int dtype, int64_t R, int C, const float *gamma, const float *beta, float eps,
                                 float momentum, int relu, void *y, float *mean, float *invstd, float *running_mean,
                                 float *running_var, float *workspace, void *stream) {
  EVP_CHECK_ARG(x && y && mean && invstd && workspace, EVP_EINVAL, "evp_batchnorm_fwd: null pointer");
  EVP_CHECK_ARG(R > 1 && C > 0, EVP_ESHAPE, "evp_batchnorm_fwd: need R>1 rows");
  EVP_CHECK_ARG((gamma == nullptr) == (beta == nullptr), EVP_EINVAL, "evp_batchnorm_fwd: gamma and beta go together");
  const bool v4 = (C % 4 == 0) && (((uintptr_t)x | (uintptr_t)y) & 15) == 0;
  return (v4 ? bn_fwd_launch<4> : bn_fwd_launch<1>)(x, dtype, R, C, gamma, beta, eps, momentum, relu, y, mean, invstd, running_mean, running_var,
                                                    workspace, (hipStream_t)stream);
}

extern "C" int evp_batchnorm_bwd(const void *dy, const void *x, const void *y, int dtype, int64_t R, int C, const float *gamma,
                                 const float *mean, const float *invstd, int relu, void *dx, float *dgamma, float *dbeta,
                                 float *workspace, void *stream) {
  EVP_CHECK_ARG(dy && x && mean && invstd && dx && workspace, EVP_EINVAL, "evp_batchnorm_bwd: null pointer");
  EVP_CHECK_ARG(!relu || y, EVP_EINVAL, "evp_batchnorm_bwd: relu needs y");
  hipStream_t s = (hipStream_t)stream;
  float *sum_dy = workspace + (int64_t)evp_batchnorm_nblk(R) * 2 * C, *sum_dy_xhat = sum_dy + C;
  const bool v4 = (C % 4 == 0) && (((uintptr_t)dy | (uintptr_t)x | (uintptr_t)y | (uintptr_t)dx) & 15) == 0;
  const int rc = (v4 ? bn_bwd_launch<4> : bn_bwd_launch<1>)(dy, x, y, dtype, R, C, gamma, mean, invstd, relu, dx, sum_dy, sum_dy_xhat, workspace, s);
  if (rc != EVP_OK) return rc;
  hipError_t e = hipSuccess;
  if (dgamma) e = hipMemcpyAsync(dgamma, sum_dy_xhat, sizeof(float) * C, hipMemcpyDeviceToDevice, s);
  if (dbeta && e == hipSuccess) e = hipMemcpyAsync(dbeta, sum_dy, sizeof(float) * C, hipMemcpyDeviceToDevice, s);
  EVP_CHECK_ARG(e == hipSuccess, EVP_ELAUNCH, "evp_batchnorm_bwd: copying the affine gradients failed: %s", hipGetErrorString(e));
  return EVP_OK;
}

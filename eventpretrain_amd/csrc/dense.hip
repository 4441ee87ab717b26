// Dense-prediction heads (UPerNet / FCN decoders on ViT token maps; reference model/finetune_dense/ft_dense_decoder.py): everything that
// makes a token map two-dimensional. All maps are token-major: row (b, y, x) = (b * H + y) * W + x of a [B*H*W, C] matrix with a leading
// dimension in ELEMENTS, so a channel slice of a wider buffer is a map (every torch.cat(dim=1) of the reference is "write into your slice":
// outputs take ld and a column offset). Element types EVP_F32 | EVP_BF16 per operand; the arithmetic is float32.
//   evp_im2col3x3 / evp_col2im3x3      patch rows of a 3x3, stride 1, zero-padding 1 convolution and the adjoint (the convolution itself is
//                                      evp_gemm on the patch rows: inner order (c, ky, kx) = conv.weight.view(O, I * 9))
//   evp_adaptive_avgpool_fwd / _bwd    nn.AdaptiveAvgPool2d(s): bin i = [floor(i H / s), ceil((i + 1) H / s)), bins may overlap
//   evp_upsample_bilinear_fwd / _bwd   F.interpolate(mode="bilinear", align_corners=False)
//   evp_channel_scale                  nn.Dropout2d for a given [B, C] scale table (and, without one, a strided cast-copy)
//   evp_batchnorm_eval                 BatchNorm on running statistics (+ ReLU)
//   evp_colsum_ordered                 column sums in a fixed order (the bias gradient of a convolution in front of BatchNorm)
// No atomics: every adjoint is a gather, every sum has a fixed order, so two launches on the same inputs give the same bits.
#include "evp_common.h"

namespace {

inline unsigned grid_for(int64_t work) {
  int64_t g = (work + 255) / 256;
  return (unsigned)(g > 16384 ? 16384 : (g < 1 ? 1 : g));
}
inline bool dtype_ok(int d) { return d == EVP_F32 || d == EVP_BF16; }

// ---- im2col -------------------------------------------------------------------------------------------------------------------------
// One workgroup = one output row (b, y) x one chunk of CC channels (CC % 8 == 0). The halo in[b, y-1..y+1, -1..W, c0..c0+CC) is staged in
// LDS as float32 [3][W + 2][CC] (coalesced over the channels, zeros outside the map); then every token x of the row owns the CC * 9
// CONTIGUOUS elements cols[(b,y,x), c0 * 9 ...) and the threads write them in whole pieces of 8 elements (16 bytes of bf16, 2 x 16 of f32):
// the (c, ky, kx) order makes a thread-per-input-element write strided by 9, this one is not.
template <typename TO>
__global__ __launch_bounds__(256) void im2col3x3_kernel(const void *__restrict__ in, int in_dtype, int64_t ldi, int H, int W, int C, int CC,
                                                        TO *__restrict__ cols, int64_t ldc) {
  extern __shared__ float halo[];      // [3][W + 2][CC]
  const int by = blockIdx.x, b = by / H, y = by - b * H;
  const int c0 = blockIdx.y * CC, cc_n = min(CC, C - c0);      // cc_n % 8 == 0 (C % 8 == 0)
  const int W2 = W + 2;
  for (int e = threadIdx.x; e < 3 * W2 * cc_n; e += 256) {
    const int cc = e % cc_n, t = e / cc_n, xx = t % W2, r = t / W2;
    const int yy = y + r - 1, xs = xx - 1;
    float v = 0.f;
    if (yy >= 0 && yy < H && xs >= 0 && xs < W) v = ld_any(in, in_dtype, ((int64_t)(b * H + yy) * W + xs) * ldi + c0 + cc);
    halo[(r * W2 + xx) * CC + cc] = v;
  }
  __syncthreads();
  const int seg8 = cc_n * 9 / 8;      // 8-element pieces per token
  for (int e = threadIdx.x; e < W * seg8; e += 256) {
    const int x = e / seg8, j0 = (e - x * seg8) * 8;
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int j = j0 + i, cc = j / 9, k = j - cc * 9, ky = k / 3, kx = k - ky * 3;
      v[i] = halo[(ky * W2 + x + kx) * CC + cc];
    }
    TO *dst = cols + ((int64_t)by * W + x) * ldc + (int64_t)c0 * 9 + j0;
    if constexpr (sizeof(TO) == 4) {
      reinterpret_cast<float4 *>(dst)[0] = make_float4(v[0], v[1], v[2], v[3]);
      reinterpret_cast<float4 *>(dst)[1] = make_float4(v[4], v[5], v[6], v[7]);
    } else {
      const uint2 lo = pack4_bf16(make_float4(v[0], v[1], v[2], v[3])), hi = pack4_bf16(make_float4(v[4], v[5], v[6], v[7]));
      *reinterpret_cast<uint4 *>(dst) = make_uint4(lo.x, lo.y, hi.x, hi.y);
    }
  }
}

// ---- the element kernels: one map form ------------------------------------------------------------------------------------------------
// out[row, off + c] = op(row, c) over an [rows, C] map: the grid-stride loop, the (c, row) decode and the strided store, once. An Op
// holds its operands and returns the float of one element; its sums keep their order (rows outer), so the result has one set of bits.
template <typename Op>
__global__ __launch_bounds__(256) void map_kernel(const Op op, int64_t rows, int C, void *__restrict__ out, int out_dtype, int64_t ldo, int64_t ooff) {
  const int64_t total = rows * C;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int c = (int)(e % C);
    const int64_t row = e / C;
    st_any(out, out_dtype, row * ldo + ooff + c, op(row, c));
  }
}

// row = (b * H + y) * W + x
struct Pix { int b, y, x; };
__device__ __forceinline__ Pix pix_of(int64_t row, int H, int W) {
  return Pix{(int)(row / ((int64_t)H * W)), (int)((row / W) % H), (int)(row % W)};
}

// dx[b,y,x,c] = sum over (ky, kx), ky outer, of dcols[(b, y-ky+1, x-kx+1), c*9 + ky*3 + kx] where that token exists: <= 9 terms, fixed order
struct Col2im3x3 {
  const void *dcols; int dtype; int64_t ldc; int H, W;
  __device__ float operator()(int64_t row, int c) const {
    const Pix p = pix_of(row, H, W);
    float acc = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int yo = p.y - ky + 1;
      if (yo < 0 || yo >= H) continue;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int xo = p.x - kx + 1;
        if (xo < 0 || xo >= W) continue;
        acc += ld_any(dcols, dtype, (row + (int64_t)(yo - p.y) * W + (xo - p.x)) * ldc + (int64_t)c * 9 + ky * 3 + kx);
      }
    }
    return acc;
  }
};

// ---- adaptive average pooling -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int bin_lo(int i, int n, int s) { return (i * n) / s; }
__device__ __forceinline__ int bin_hi(int i, int n, int s) { return ((i + 1) * n + s - 1) / s; }

struct AvgPoolFwd {      // row = (b, i, j) of the [B*s*s, C] output
  const void *in; int in_dtype; int64_t ldi; int H, W, s;
  __device__ float operator()(int64_t row, int c) const {
    const Pix p = pix_of(row, s, s);
    const int y0 = bin_lo(p.y, H, s), y1 = bin_hi(p.y, H, s), x0 = bin_lo(p.x, W, s), x1 = bin_hi(p.x, W, s);
    float acc = 0.f;
    for (int y = y0; y < y1; ++y)
      for (int x = x0; x < x1; ++x) acc += ld_any(in, in_dtype, ((int64_t)(p.b * H + y) * W + x) * ldi + c);
    return acc / (float)((y1 - y0) * (x1 - x0));
  }
};

// dx[b,y,x,c] = sum over the bins (i, j) that contain (y, x), i outer, of g[b,i,j,c] / area(i, j)
struct AvgPoolBwd {
  const void *g; int g_dtype; int64_t ldg; int H, W, s;
  __device__ float operator()(int64_t row, int c) const {
    const Pix p = pix_of(row, H, W);
    float acc = 0.f;
    for (int i = 0; i < s; ++i) {
      const int y0 = bin_lo(i, H, s), y1 = bin_hi(i, H, s);
      if (p.y < y0 || p.y >= y1) continue;
      for (int j = 0; j < s; ++j) {
        const int x0 = bin_lo(j, W, s), x1 = bin_hi(j, W, s);
        if (p.x < x0 || p.x >= x1) continue;
        acc += ld_any(g, g_dtype, ((int64_t)(p.b * s + i) * s + j) * ldg + c) / (float)((y1 - y0) * (x1 - x0));
      }
    }
    return acc;
  }
};

// ---- bilinear resize (Tap / tap_of: evp_common.h) ---------------------------------------------------------------------------------------
struct UpsampleFwd {      // [B*h*w, C] -> row (b, y, x) of [B*H*W, C]
  const void *in; int in_dtype; int64_t ldi; int h, w, H, W;
  __device__ float operator()(int64_t row, int c) const {
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    const Pix p = pix_of(row, H, W);
    const Tap ty = tap_of(p.y, h, sy), tx = tap_of(p.x, w, sx);
    const int64_t r0 = (int64_t)(p.b * h + ty.i0) * w, r1 = (int64_t)(p.b * h + ty.i1) * w;
    const float a = ld_any(in, in_dtype, (r0 + tx.i0) * ldi + c), bb = ld_any(in, in_dtype, (r0 + tx.i1) * ldi + c);
    const float cc = ld_any(in, in_dtype, (r1 + tx.i0) * ldi + c), d = ld_any(in, in_dtype, (r1 + tx.i1) * ldi + c);
    return tap_combine(ty, tx, a, bb, cc, d);
  }
};

// gather form of the adjoint: source pixel (ys, xs) sums, rows outer, over the destination pixels one of whose taps is (ys, xs)
struct UpsampleBwd {
  const void *g; int g_dtype; int64_t ldg; int h, w, H, W;
  __device__ float operator()(int64_t row, int c) const {
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    const Pix p = pix_of(row, h, w);      // the source pixel
    float acc = 0.f;
    for (int y = 0; y < H; ++y) {
      const Tap ty = tap_of(y, h, sy);
      const float wy = (ty.i0 == p.y ? ty.l0 : 0.f) + (ty.i1 == p.y ? ty.l1 : 0.f);
      if (ty.i0 != p.y && ty.i1 != p.y) continue;
      for (int x = 0; x < W; ++x) {
        const Tap tx = tap_of(x, w, sx);
        if (tx.i0 != p.x && tx.i1 != p.x) continue;
        const float wx = (tx.i0 == p.x ? tx.l0 : 0.f) + (tx.i1 == p.x ? tx.l1 : 0.f);
        acc += wy * wx * ld_any(g, g_dtype, ((int64_t)(p.b * H + y) * W + x) * ldg + c);
      }
    }
    return acc;
  }
};

// ---- channel scale / strided cast-copy ----------------------------------------------------------------------------------------------
struct ChannelScale {
  const void *in; int in_dtype; int64_t ldi; const float *m; int P, C;
  __device__ float operator()(int64_t row, int c) const {
    float v = ld_any(in, in_dtype, row * ldi + c);
    if (m) v *= m[(row / P) * C + c];
    return v;
  }
};

// ---- BatchNorm on running statistics ------------------------------------------------------------------------------------------------
struct BatchNormEval {
  const void *x; int x_dtype; int64_t ldx; const float *gamma, *beta, *rmean, *rvar; float eps; int relu;
  __device__ float operator()(int64_t row, int c) const {
    const float invstd = 1.f / sqrtf(rvar[c] + eps);
    float v = (ld_any(x, x_dtype, row * ldx + c) - rmean[c]) * invstd;
    if (gamma) v = v * gamma[c] + beta[c];
    if (relu) v = fmaxf(v, 0.f);
    return v;
  }
};

// data gradient of the above: dx = g * gamma / sqrt(running_var + eps), zero where the ReLU output y is not positive
struct BatchNormEvalBwd {
  const void *g; int g_dtype; int64_t ldg; const void *y; int y_dtype; int64_t ldy; const float *gamma, *rvar; float eps; int relu;
  __device__ float operator()(int64_t row, int c) const {
    float v = ld_any(g, g_dtype, row * ldg + c) * (1.f / sqrtf(rvar[c] + eps));
    if (gamma) v *= gamma[c];
    if (relu && !(ld_any(y, y_dtype, row * ldy + c) > 0.f)) v = 0.f;
    return v;
  }
};

// ---- ordered column sums ------------------------------------------------------------------------------------------------------------
// out[c] = sum_r x[r, c]: 64 columns per workgroup, 4 row lanes per column (rows r = lane, lane + 4, ...), the four partials added in
// lane order. The same order every launch, whatever R.
__global__ __launch_bounds__(256) void colsum_ordered_kernel(const void *__restrict__ x, int dtype, int64_t R, int C, int64_t ld, float *__restrict__ out) {
  __shared__ float part[4][64];
  const int cl = threadIdx.x & 63, lane = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
  float acc = 0.f;
  if (c < C)
    for (int64_t r = lane; r < R; r += 4) acc += ld_any(x, dtype, r * ld + c);
  part[lane][cl] = acc;
  __syncthreads();
  if (lane == 0 && c < C) out[c] = ((part[0][cl] + part[1][cl]) + part[2][cl]) + part[3][cl];
}

// The host side of a map entry point, once: `in` is the map the Op reads first (its rows are in_width elements wide, ldi apart), the
// output is the slice [rows, ooff : ooff + C] of rows ldo apart. `dims_ok`: the entry point's own shape rules.
template <typename Op>
int map_launch(const char *name, const Op &op, const void *in, int in_dtype, int64_t ldi, int64_t in_width, bool dims_ok, int64_t rows, int C,
               void *out, int out_dtype, int64_t ldo, int64_t ooff, void *stream) {
  EVP_CHECK_ARG(in && out, EVP_EINVAL, "%s: null pointer", name);
  EVP_CHECK_ARG(dtype_ok(in_dtype) && dtype_ok(out_dtype), EVP_EINVAL, "%s: bad dtype", name);
  EVP_CHECK_ARG(dims_ok && ldi >= in_width && ooff >= 0 && ldo >= ooff + C, EVP_ESHAPE, "%s: bad shape", name);
  hipLaunchKernelGGL(map_kernel<Op>, dim3(grid_for(rows * C)), dim3(256), 0, (hipStream_t)stream, op, rows, C, out, out_dtype, ldo, ooff);
  EVP_CHECK_LAUNCH(name);
  return EVP_OK;
}

}  // namespace

#define DENSE_MAP_ARGS_OK(B, H, W, C) ((B) > 0 && (H) > 0 && (W) > 0 && (C) > 0 && (int64_t)(B) * (H) * (W) < (1ll << 31))

extern "C" int evp_im2col3x3(const void *in, int in_dtype, int64_t ldi, int B, int H, int W, int C, void *cols, int cols_dtype, int64_t ldc,
                             void *stream) {
  EVP_CHECK_ARG(in && cols, EVP_EINVAL, "evp_im2col3x3: null pointer");
  EVP_CHECK_ARG(dtype_ok(in_dtype) && dtype_ok(cols_dtype), EVP_EINVAL, "evp_im2col3x3: bad dtype");
  EVP_CHECK_ARG(DENSE_MAP_ARGS_OK(B, H, W, C) && C % 8 == 0 && ldi >= C && ldc >= (int64_t)C * 9 && ldc % 8 == 0 && W <= 510, EVP_ESHAPE,
                "evp_im2col3x3: bad shape (C %% 8 == 0, ldc %% 8 == 0, W <= 510; B=%d H=%d W=%d C=%d)", B, H, W, C);
  EVP_CHECK_ARG(((uintptr_t)cols & 15) == 0, EVP_EINVAL, "evp_im2col3x3: cols must be 16-byte aligned");
  // channel chunk: the largest multiple of 8 up to 64 whose halo fits 48 KiB of LDS
  int CC = C < 64 ? C : 64;
  while (CC > 8 && (size_t)3 * (W + 2) * CC * sizeof(float) > 48 * 1024) CC -= 8;
  const size_t lds = (size_t)3 * (W + 2) * CC * sizeof(float);
  const dim3 grid((unsigned)(B * H), (unsigned)((C + CC - 1) / CC));
  if (cols_dtype == EVP_F32)
    hipLaunchKernelGGL(im2col3x3_kernel<float>, grid, dim3(256), lds, (hipStream_t)stream, in, in_dtype, ldi, H, W, C, CC, (float *)cols, ldc);
  else
    hipLaunchKernelGGL(im2col3x3_kernel<bf16_t>, grid, dim3(256), lds, (hipStream_t)stream, in, in_dtype, ldi, H, W, C, CC, (bf16_t *)cols, ldc);
  EVP_CHECK_LAUNCH("evp_im2col3x3");
  return EVP_OK;
}

extern "C" int evp_col2im3x3(const void *dcols, int dtype, int64_t ldc, int B, int H, int W, int C, void *dx, int dx_dtype, int64_t ldx, int64_t xoff,
                             void *stream) {
  return map_launch("evp_col2im3x3", Col2im3x3{dcols, dtype, ldc, H, W}, dcols, dtype, ldc, (int64_t)C * 9, DENSE_MAP_ARGS_OK(B, H, W, C),
                    (int64_t)B * H * W, C, dx, dx_dtype, ldx, xoff, stream);
}

extern "C" int evp_adaptive_avgpool_fwd(const void *in, int in_dtype, int64_t ldi, int B, int H, int W, int C, int s, void *out, int out_dtype,
                                        int64_t ldo, int64_t ooff, void *stream) {
  return map_launch("evp_adaptive_avgpool_fwd", AvgPoolFwd{in, in_dtype, ldi, H, W, s}, in, in_dtype, ldi, C,
                    DENSE_MAP_ARGS_OK(B, H, W, C) && s > 0 && s <= 4096, (int64_t)B * s * s, C, out, out_dtype, ldo, ooff, stream);
}

extern "C" int evp_adaptive_avgpool_bwd(const void *g, int g_dtype, int64_t ldg, int B, int H, int W, int C, int s, void *dx, int dx_dtype,
                                        int64_t ldx, int64_t xoff, void *stream) {
  return map_launch("evp_adaptive_avgpool_bwd", AvgPoolBwd{g, g_dtype, ldg, H, W, s}, g, g_dtype, ldg, C,
                    DENSE_MAP_ARGS_OK(B, H, W, C) && s > 0 && s <= 4096, (int64_t)B * H * W, C, dx, dx_dtype, ldx, xoff, stream);
}

extern "C" int evp_upsample_bilinear_fwd(const void *in, int in_dtype, int64_t ldi, int B, int h, int w, int H, int W, int C, void *out,
                                         int out_dtype, int64_t ldo, int64_t ooff, void *stream) {
  return map_launch("evp_upsample_bilinear_fwd", UpsampleFwd{in, in_dtype, ldi, h, w, H, W}, in, in_dtype, ldi, C,
                    DENSE_MAP_ARGS_OK(B, H, W, C) && DENSE_MAP_ARGS_OK(B, h, w, C), (int64_t)B * H * W, C, out, out_dtype, ldo, ooff, stream);
}

extern "C" int evp_upsample_bilinear_bwd(const void *g, int g_dtype, int64_t ldg, int B, int h, int w, int H, int W, int C, void *dx, int dx_dtype,
                                         int64_t ldx, int64_t xoff, void *stream) {
  return map_launch("evp_upsample_bilinear_bwd", UpsampleBwd{g, g_dtype, ldg, h, w, H, W}, g, g_dtype, ldg, C,
                    DENSE_MAP_ARGS_OK(B, H, W, C) && DENSE_MAP_ARGS_OK(B, h, w, C), (int64_t)B * h * w, C, dx, dx_dtype, ldx, xoff, stream);
}

extern "C" int evp_channel_scale(const void *in, int in_dtype, int64_t ldi, const float *m, int B, int P, int C, void *out, int out_dtype, int64_t ldo,
                                 int64_t ooff, void *stream) {
  return map_launch("evp_channel_scale", ChannelScale{in, in_dtype, ldi, m, P, C}, in, in_dtype, ldi, C, DENSE_MAP_ARGS_OK(B, P, 1, C),
                    (int64_t)B * P, C, out, out_dtype, ldo, ooff, stream);
}

extern "C" int evp_batchnorm_eval(const void *x, int x_dtype, int64_t ldx, int64_t R, int C, const float *gamma, const float *beta,
                                  const float *running_mean, const float *running_var, float eps, int relu, void *y, int y_dtype, int64_t ldo,
                                  int64_t ooff, void *stream) {
  EVP_CHECK_ARG(running_mean && running_var, EVP_EINVAL, "evp_batchnorm_eval: null pointer");
  EVP_CHECK_ARG((gamma == nullptr) == (beta == nullptr), EVP_EINVAL, "evp_batchnorm_eval: gamma and beta go together");
  return map_launch("evp_batchnorm_eval", BatchNormEval{x, x_dtype, ldx, gamma, beta, running_mean, running_var, eps, relu}, x, x_dtype, ldx, C,
                    DENSE_MAP_ARGS_OK(R, 1, 1, C), R, C, y, y_dtype, ldo, ooff, stream);
}

extern "C" int evp_batchnorm_eval_bwd(const void *g, int g_dtype, int64_t ldg, const void *y, int y_dtype, int64_t ldy, int64_t R, int C,
                                      const float *gamma, const float *running_var, float eps, int relu, void *dx, int dx_dtype, int64_t ldx,
                                      void *stream) {
  EVP_CHECK_ARG(running_var, EVP_EINVAL, "evp_batchnorm_eval_bwd: null pointer");
  EVP_CHECK_ARG(!relu || (y && dtype_ok(y_dtype) && ldy >= C), EVP_EINVAL, "evp_batchnorm_eval_bwd: relu needs y");
  return map_launch("evp_batchnorm_eval_bwd", BatchNormEvalBwd{g, g_dtype, ldg, y, y_dtype, ldy, gamma, running_var, eps, relu}, g, g_dtype, ldg, C,
                    DENSE_MAP_ARGS_OK(R, 1, 1, C), R, C, dx, dx_dtype, ldx, 0, stream);
}

extern "C" int evp_colsum_ordered(const void *x, int dtype, int64_t R, int C, int64_t ld, float *out, void *stream) {
  EVP_CHECK_ARG(x && out && dtype_ok(dtype), EVP_EINVAL, "evp_colsum_ordered: bad argument");
  EVP_CHECK_ARG(R > 0 && C > 0 && ld >= C, EVP_ESHAPE, "evp_colsum_ordered: bad shape");
  hipLaunchKernelGGL(colsum_ordered_kernel, dim3((unsigned)((C + 63) / 64)), dim3(256), 0, (hipStream_t)stream, x, dtype, R, C, ld, out);
  EVP_CHECK_LAUNCH("evp_colsum_ordered");
  return EVP_OK;
}

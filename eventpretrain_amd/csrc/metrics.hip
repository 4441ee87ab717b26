// K25: classification metrics of one evaluation batch -- mean cross entropy, top-1 and top-5 accuracy -- written into the next
// slot of a device-resident table (ft_cls_trainer.py:152-164 of the reference with timm's `accuracy`, restated in
// include/evtpretrain.h). One 64-lane wave owns one row of logits: a row of up to 1024 classes is read once into registers
// (float4 per lane where the leading dimension and the address allow, so a wave instruction moves 1 KiB), and max, sum-exp,
// label logit and rank all come from that one read; longer rows walk 1024-column chunks with a running (max, sum). Reductions
// go wave shuffle -> LDS -> a sum in fixed order; no float atomics, so a replay is bit-identical. The slot index lives in device
// memory (`cursor`), is read once when the finishing kernel starts and is advanced by the one thread that ends the reduction:
// a captured HIP graph fills slot after slot by itself.
#include "evp_common.h"

namespace {

constexpr int CM_CHUNK = 1024;                     // columns a wave holds in registers: 16 per lane
constexpr int CM_SINGLE_ROWS = EVP_CLS_METRICS_SINGLE_ROWS;   // up to here one workgroup walks all rows and finishes the batch itself
constexpr int CM_MAX_BLOCKS = EVP_CLS_METRICS_WS / 3;          // two-launch form: block partials {loss, hits1, hits5}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// column of register slot i of this lane in the chunk that starts at c0
template <bool VEC> __device__ __forceinline__ int col_of(int c0, int lane, int i) {
  return VEC ? c0 + 4 * (lane + 64 * (i >> 2)) + (i & 3) : c0 + lane + 64 * i;
}

template <bool VEC> __device__ __forceinline__ void load_chunk(const float *lr, int c0, int n_cls, int lane, float (&v)[16]) {
  if (VEC) {      // ld % 4 == 0 and a 16-byte-aligned base: c < n_cls <= ld implies c + 3 < ld, the whole float4 is inside the row
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = c0 + 4 * (lane + 64 * i);
      const float4 q = c < n_cls ? *reinterpret_cast<const float4 *>(lr + c) : make_float4(0.f, 0.f, 0.f, 0.f);
      v[4 * i] = q.x; v[4 * i + 1] = q.y; v[4 * i + 2] = q.z; v[4 * i + 3] = q.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int c = c0 + lane + 64 * i;
      v[i] = c < n_cls ? lr[c] : 0.f;
    }
  }
}

// does column j (value a) come before the label's column `lab` (value x) in the order torch.topk(largest=True) uses: a larger
// value first, NaN larger than every number, equal values (NaN against NaN included) lower index first. Comparisons only.
__device__ __forceinline__ bool comes_before(float a, int j, float x, int lab) {
  const bool an = a != a, xn = x != x;
  if (an || xn) return an && (!xn || j < lab);
  return a > x || (a == x && j < lab);
}

// One row, by one wave; every lane returns the same values. loss = logsumexp(row) - row[label]; rank = columns before the label's.
// A label outside [0, n_cls) reads nothing: the loss is NaN and the rank n_cls (a miss for every k).
template <bool VEC>
__device__ __forceinline__ void row_metrics(const float *lr, int64_t label, int n_cls, int lane, float &loss, int &rank) {
  const bool ok = label >= 0 && label < (int64_t)n_cls;
  const int lab = ok ? (int)label : -1;
  const bool single = n_cls <= CM_CHUNK;
  float x = 0.f;
  if (ok && !single) x = lr[lab];        // a long row needs the label's logit before its first chunk is ranked
  // running maximum m of this lane's columns and s = sum exp(v - ref(m)), ref(m) = m, or 0 while m is still -inf
  float m = -INFINITY, s = 0.f;
  int cnt = 0;
  for (int c0 = 0; c0 < n_cls; c0 += CM_CHUNK) {
    float v[16];
    load_chunk<VEC>(lr, c0, n_cls, lane, v);
    if (single && ok) {                  // the label's logit out of the registers: exactly one lane holds it
      float xc = 0.f;
      bool has = false;
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (col_of<VEC>(c0, lane, i) == lab) { xc = v[i]; has = true; }
      const unsigned long long owners = __ballot(has);
      x = __shfl(xc, __ffsll(owners) - 1, 64);
    }
    float mc = -INFINITY;
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (col_of<VEC>(c0, lane, i) < n_cls) mc = fmaxf(mc, v[i]);       // (fmaxf drops a NaN: it reaches the loss through the sum)
    const float mn = fmaxf(m, mc);
    const float ref = mn == -INFINITY ? 0.f : mn;
    if (m != -INFINITY) s *= expf(m - ref);                             // (m <= mn: the factor is <= 1; while m is -inf, s is 0 or NaN and stays)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int j = col_of<VEC>(c0, lane, i);
      if (j < n_cls) {
        s += expf(v[i] - ref);
        if (ok && j != lab && comes_before(v[i], j, x, lab)) ++cnt;
      }
    }
    m = mn;
  }
  const float M = wave_max(m);
  const float ref = M == -INFINITY ? 0.f : M;
  const float S = wave_sum(m == -INFINITY ? s : s * expf(m - ref));
  loss = ok ? (logf(S) + ref) - x : __builtin_nanf("");
  rank = ok ? wave_sum_i(cnt) : n_cls;
}

// The rows r = first, first + stride, ... of this wave, in that order: sum of the row losses and the two hit counts.
template <bool VEC>
__device__ __forceinline__ void walk_rows(const float *logits, const int64_t *labels, int64_t R, int n_cls, int64_t ld, int64_t first,
                                          int64_t stride, int lane, float &loss, int &h1, int &h5) {
  const int k5 = n_cls < 5 ? n_cls : 5;       // timm: maxk = min(max(topk), n_cls)
  loss = 0.f; h1 = 0; h5 = 0;
  for (int64_t r = first; r < R; r += stride) {
    float l; int rank;
    row_metrics<VEC>(logits + r * ld, labels[r], n_cls, lane, l, rank);
    loss += l;
    h1 += rank < 1;
    h5 += rank < k5;
  }
}

// wave values -> LDS -> thread 0 sums the waves in index order; valid in thread 0 only
__device__ __forceinline__ void block_totals(float &loss, int &h1, int &h5, float *redf, int *redi) {
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if ((threadIdx.x & 63) == 0) { redf[w] = loss; redi[2 * w] = h1; redi[2 * w + 1] = h5; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float l = 0.f; int a = 0, b = 0;
    for (int i = 0; i < nw; ++i) { l += redf[i]; a += redi[2 * i]; b += redi[2 * i + 1]; }
    loss = l; h1 = a; h5 = b;
  }
}

__device__ __forceinline__ void write_slot(int64_t *cursor, float *table, int64_t slot, float loss_sum, int h1, int h5, int64_t R, float pct) {
  float *t = table + slot * 3;
  t[0] = loss_sum / (float)R;
  t[1] = (float)h1 * pct;         // pct = (float)(100.0 / R): the hit count times 100 / R, as the eager meters compute it
  t[2] = (float)h5 * pct;
  *cursor = slot + 1;
}

// R <= CM_SINGLE_ROWS: one workgroup of 16 waves walks all rows and finishes the batch itself
template <bool VEC>
__global__ __launch_bounds__(1024) void cls_metrics_single_kernel(const float *logits, const int64_t *labels, int64_t R, int n_cls, int64_t ld,
                                                                  int64_t *cursor, float *table, int64_t capacity, float pct) {
  __shared__ float redf[16];
  __shared__ int redi[32];
  __shared__ int64_t slot_s;
  if (threadIdx.x == 0) slot_s = *cursor;
  __syncthreads();
  const int64_t slot = slot_s;
  if (slot < 0 || slot >= capacity) return;      // (uniform) a full table or a corrupt cursor: nothing is written
  float loss; int h1, h5;
  walk_rows<VEC>(logits, labels, R, n_cls, ld, threadIdx.x >> 6, blockDim.x >> 6, threadIdx.x & 63, loss, h1, h5);
  block_totals(loss, h1, h5, redf, redi);
  if (threadIdx.x == 0) write_slot(cursor, table, slot, loss, h1, h5, R, pct);
}

// larger R: 4 waves per block over the rows, block partials into the workspace ...
template <bool VEC>
__global__ __launch_bounds__(256) void cls_metrics_rows_kernel(const float *logits, const int64_t *labels, int64_t R, int n_cls, int64_t ld,
                                                               float *ws) {
  __shared__ float redf[4];
  __shared__ int redi[8];
  float loss; int h1, h5;
  walk_rows<VEC>(logits, labels, R, n_cls, ld, (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), (int64_t)gridDim.x * 4, threadIdx.x & 63, loss, h1, h5);
  block_totals(loss, h1, h5, redf, redi);
  if (threadIdx.x == 0) {
    ws[3 * blockIdx.x] = loss;
    ws[3 * blockIdx.x + 1] = __int_as_float(h1);
    ws[3 * blockIdx.x + 2] = __int_as_float(h5);
  }
}
// ... and one workgroup sums them (thread t holds block t's partial; nblk <= 1024) and writes the slot
__global__ __launch_bounds__(1024) void cls_metrics_finish_kernel(const float *ws, int nblk, int64_t R, int64_t *cursor, float *table,
                                                                  int64_t capacity, float pct) {
  __shared__ float redf[16];
  __shared__ int redi[32];
  __shared__ int64_t slot_s;
  if (threadIdx.x == 0) slot_s = *cursor;
  __syncthreads();
  const int64_t slot = slot_s;
  if (slot < 0 || slot >= capacity) return;
  const bool have = (int)threadIdx.x < nblk;
  float loss = have ? ws[3 * threadIdx.x] : 0.f;
  int h1 = have ? __float_as_int(ws[3 * threadIdx.x + 1]) : 0;
  int h5 = have ? __float_as_int(ws[3 * threadIdx.x + 2]) : 0;
  loss = wave_sum(loss); h1 = wave_sum_i(h1); h5 = wave_sum_i(h5);
  block_totals(loss, h1, h5, redf, redi);
  if (threadIdx.x == 0) write_slot(cursor, table, slot, loss, h1, h5, R, pct);
}

}  // namespace

extern "C" int evp_cls_metrics(const float *logits, const int64_t *labels, int64_t R, int n_cls, int64_t ld, int64_t *cursor, float *table,
                               int64_t capacity, float *workspace, void *stream) {
  EVP_CHECK_ARG(logits && labels && cursor && table, EVP_EINVAL, "evp_cls_metrics: null pointer");
  EVP_CHECK_ARG(R > 0 && n_cls > 0 && ld >= n_cls && R < 2147483647LL, EVP_ESHAPE, "evp_cls_metrics: bad shape (R=%lld, n_cls=%d, ld=%lld)",
                (long long)R, n_cls, (long long)ld);
  EVP_CHECK_ARG(capacity > 0, EVP_ESHAPE, "evp_cls_metrics: the table needs at least one slot");
  EVP_CHECK_ARG(R <= CM_SINGLE_ROWS || workspace, EVP_EINVAL, "evp_cls_metrics: more than %d rows need the workspace (null pointer)", CM_SINGLE_ROWS);
  hipStream_t s = (hipStream_t)stream;
  const bool vec = ld % 4 == 0 && ((uintptr_t)logits & 15) == 0;
  const float pct = (float)(100.0 / (double)R);
  if (R <= CM_SINGLE_ROWS) {
    if (vec) hipLaunchKernelGGL(cls_metrics_single_kernel<true>, dim3(1), dim3(1024), 0, s, logits, labels, R, n_cls, ld, cursor, table, capacity, pct);
    else hipLaunchKernelGGL(cls_metrics_single_kernel<false>, dim3(1), dim3(1024), 0, s, logits, labels, R, n_cls, ld, cursor, table, capacity, pct);
    EVP_CHECK_LAUNCH("evp_cls_metrics");
    return EVP_OK;
  }
  int64_t nblk = (R + 3) / 4;
  if (nblk > CM_MAX_BLOCKS) nblk = CM_MAX_BLOCKS;
  if (vec) hipLaunchKernelGGL(cls_metrics_rows_kernel<true>, dim3((unsigned)nblk), dim3(256), 0, s, logits, labels, R, n_cls, ld, workspace);
  else hipLaunchKernelGGL(cls_metrics_rows_kernel<false>, dim3((unsigned)nblk), dim3(256), 0, s, logits, labels, R, n_cls, ld, workspace);
  EVP_CHECK_LAUNCH("evp_cls_metrics(rows)");
  hipLaunchKernelGGL(cls_metrics_finish_kernel, dim3(1), dim3(1024), 0, s, workspace, (int)nblk, R, cursor, table, capacity, pct);
  EVP_CHECK_LAUNCH("evp_cls_metrics(finish)");
  return EVP_OK;
}

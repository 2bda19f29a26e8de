// Segmented summary statistics of float32 tensors (what one TensorBoard summary step needs of every summarised tensor): TensorFlow's
// 1551-bucket histogram, num / n_zero / n_nonfinite, min / max / sum / sum of squares -- frcnn_hip/summary.py turns a record into a
// HistogramProto.  The bucket rule and the limit table are csrc/summary_math.h.
//
// One call takes a device table of (pointer, element count) -- trainable filters, their biases, activations and score tensors are
// scattered over the session's buffers -- and makes three enqueues whatever the number of tensors: a memset of the records, k_summary_stats
// on a (SUMMARY_BLOCKS, count) grid, k_summary_finish.
//
//   k_summary_stats   workgroup (b, s) takes the float4 vectors b*256+t, +nblk*256, ... of segment s (nblk = summary_nblk(n): a short
//                     tensor uses one workgroup, the others leave at once, before touching the LDS).  The segment pointer is 4-byte aligned
//                     only (gradients and weights are views at arbitrary float offsets), so the <= 3 floats before the first 16-byte
//                     boundary and the <= 3 after the last whole vector are read as scalars by workgroup 0.  Limits (12.4 KB) and the
//                     workgroup's counts (6.2 KB, u32) live in the LDS; a non-zero finite value is one binary search + one LDS atomic;
//                     the x == 0 lanes of a wave (half of a post-ReLU map, all on one address otherwise) are counted with a ballot and
//                     added once per workgroup.  Non-zero counts go to the record with 64-bit INTEGER atomics: exact in any order.
//   k_summary_finish  one thread per segment folds the workgroups' (min, max, sum, sum of squares) partials in workgroup order.  Every
//                     lane's share, the wave tree, the order of the four waves and this fold are functions of (pointer alignment, n)
//                     alone: no float atomics, the same bits on every run.
//
// Compiled with -ffp-contract=off like the rest of the library: the square and the add round separately.
#include "common.h"
#include "summary_math.h"

#define SUMMARY_THREADS 256
#define SUMMARY_BLOCKS 64                      // workgroups per segment at most (gridDim.x)
#define SUMMARY_MIN_PER_BLOCK 4096             // elements below which a segment does not get another workgroup
#define SUMMARY_MAX_SEGMENTS 65535             // gridDim.y

static_assert(FRCNN_SUMMARY_BUCKETS == SUMMARY_BUCKETS, "include/frcnn_hip.h and csrc/summary_math.h disagree on the bucket count");
static_assert(FRCNN_SUMMARY_RECORD >= SUMMARY_BUCKETS + 7, "record too short");

__device__ const SummaryLimits d_summary_limits = summary_make_limits();

struct SummarySeg {                            // one row of the caller's table
  const float* p;
  long long n;
};
struct SummaryPartial {
  double mn, mx, sum, sumsq;
};

__host__ __device__ __forceinline__ int summary_nblk(long long n) {
  const long long b = (n + SUMMARY_MIN_PER_BLOCK - 1) / SUMMARY_MIN_PER_BLOCK;
  return (int)(b < SUMMARY_BLOCKS ? b : SUMMARY_BLOCKS);
}

struct SummaryAcc {                            // one lane's running state
  double sum, sumsq;
  float mn, mx;
  u32 nonfinite, zeros;                        // zeros: the wave's count, the same in every lane (ballot)
};

// Called by all 64 lanes of a wave together (the ballot counts the wave's zero lanes); `valid` = this lane holds an element.
__device__ __forceinline__ void summary_add(float x, bool valid, const double* lim, u32* cnt, SummaryAcc& a) {
  const bool fin = valid && summary_finite_bits(__float_as_uint(x));
  const bool zero = fin && x == 0.0f;
  a.zeros += (u32)__popcll(__ballot(zero));
  a.nonfinite += (valid && !fin) ? 1u : 0u;
  if (fin) {
    const double d = (double)x;
    a.sum += d;
    a.sumsq += d * d;
    a.mn = x < a.mn ? x : a.mn;
    a.mx = x > a.mx ? x : a.mx;
    if (!zero) atomicAdd(&cnt[summary_bucket(lim, d)], 1u);
  }
}

__global__ void __launch_bounds__(SUMMARY_THREADS) k_summary_stats(const SummarySeg* __restrict__ segs, long long* __restrict__ out,
                                                                   SummaryPartial* __restrict__ partial) {
  __shared__ double lim[SUMMARY_BUCKETS];
  __shared__ u32 cnt[SUMMARY_BUCKETS];
  __shared__ SummaryPartial wpart[SUMMARY_THREADS / 64];
  __shared__ u32 wcount[SUMMARY_THREADS / 64][2];
  const int s = blockIdx.y, b = blockIdx.x, t = threadIdx.x;
  const SummarySeg seg = segs[s];
  const long long n = seg.n;
  const int nblk = summary_nblk(n);
  if (b >= nblk) return;                       // (uniform over the workgroup; also n <= 0)
  for (int i = t; i < SUMMARY_BUCKETS; i += SUMMARY_THREADS) {
    lim[i] = d_summary_limits.v[i];
    cnt[i] = 0;
  }
  __syncthreads();

  const float* p = seg.p;
  long long head = (long long)(((16 - ((uintptr_t)p & 15)) & 15) >> 2);      // floats before the first 16-byte boundary
  if (head > n) head = n;
  const long long nv = (n - head) >> 2;        // whole float4 vectors
  const long long tail0 = head + 4 * nv;       // first element after them; n - tail0 <= 3
  const float4* pv = (const float4*)(p + head);

  SummaryAcc a = {0.0, 0.0, FLT_MAX, -FLT_MAX, 0u, 0u};
  const long long stride = (long long)nblk * SUMMARY_THREADS;
  // every lane of a wave makes the same number of trips (the bound is rounded up to the wave), lanes past the end carry valid = false
  for (long long base = (long long)b * SUMMARY_THREADS + (t & ~63); base < nv; base += stride) {
    const long long v = base + (t & 63);
    const bool valid = v < nv;
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
    if (valid) x = pv[v];
    summary_add(x.x, valid, lim, cnt, a);
    summary_add(x.y, valid, lim, cnt, a);
    summary_add(x.z, valid, lim, cnt, a);
    summary_add(x.w, valid, lim, cnt, a);
  }
  if (b == 0 && t < 64) {                      // the scalar head and tail: at most 6 elements, wave 0 of workgroup 0
    const long long edge = head + (n - tail0);
    const bool valid = t < edge;
    float x = 0.f;
    if (valid) x = t < head ? p[t] : p[tail0 + (t - head)];
    summary_add(x, valid, lim, cnt, a);
  }

  // wave: (min, max, sum, sum of squares, non-finite count) by a fixed butterfly; the zero count is already the wave's
  for (int o = 32; o; o >>= 1) {
    a.sum += __shfl_xor(a.sum, o, 64);
    a.sumsq += __shfl_xor(a.sumsq, o, 64);
    const float mn = __shfl_xor(a.mn, o, 64), mx = __shfl_xor(a.mx, o, 64);
    a.mn = mn < a.mn ? mn : a.mn;
    a.mx = mx > a.mx ? mx : a.mx;
    a.nonfinite += __shfl_xor(a.nonfinite, o, 64);
  }
  if ((t & 63) == 0) {
    wpart[t >> 6] = SummaryPartial{(double)a.mn, (double)a.mx, a.sum, a.sumsq};
    wcount[t >> 6][0] = a.zeros;
    wcount[t >> 6][1] = a.nonfinite;
  }
  __syncthreads();                             // also: every LDS atomic of the workgroup has landed
  long long* rec = out + (size_t)s * FRCNN_SUMMARY_RECORD;
  unsigned long long* urec = (unsigned long long*)rec;
  if (t == 0) {
    SummaryPartial r = wpart[0];
    u32 zeros = wcount[0][0], nonfinite = wcount[0][1];
    for (int w = 1; w < SUMMARY_THREADS / 64; ++w) {
      r.mn = wpart[w].mn < r.mn ? wpart[w].mn : r.mn;
      r.mx = wpart[w].mx > r.mx ? wpart[w].mx : r.mx;
      r.sum += wpart[w].sum;
      r.sumsq += wpart[w].sumsq;
      zeros += wcount[w][0];
      nonfinite += wcount[w][1];
    }
    partial[(size_t)s * SUMMARY_BLOCKS + b] = r;
    if (zeros) {
      atomicAdd(&urec[SUMMARY_ZERO_BUCKET], (unsigned long long)zeros);
      atomicAdd(&urec[FRCNN_SUMMARY_NZERO], (unsigned long long)zeros);
    }
    if (nonfinite) atomicAdd(&urec[FRCNN_SUMMARY_NNONFINITE], (unsigned long long)nonfinite);
  }
  for (int i = t; i < SUMMARY_BUCKETS; i += SUMMARY_THREADS) {
    const u32 c = cnt[i];
    if (c) atomicAdd(&urec[i], (unsigned long long)c);
  }
}

__global__ void __launch_bounds__(SUMMARY_THREADS) k_summary_finish(const SummarySeg* __restrict__ segs, int count, long long* __restrict__ out,
                                                                    const SummaryPartial* __restrict__ partial) {
  const int s = blockIdx.x * SUMMARY_THREADS + threadIdx.x;
  if (s >= count) return;
  const long long n = segs[s].n;
  const int nblk = summary_nblk(n);
  SummaryPartial r = {DBL_MAX, -DBL_MAX, 0.0, 0.0};      // Histogram::Clear()'s min / max: what an empty (or all non-finite) tensor reports
  for (int b = 0; b < nblk; ++b) {
    const SummaryPartial q = partial[(size_t)s * SUMMARY_BLOCKS + b];
    r.mn = q.mn < r.mn ? q.mn : r.mn;
    r.mx = q.mx > r.mx ? q.mx : r.mx;
    r.sum += q.sum;
    r.sumsq += q.sumsq;
  }
  long long* rec = out + (size_t)s * FRCNN_SUMMARY_RECORD;
  // a workgroup that saw no finite value reports (FLT_MAX, -FLT_MAX): keep Clear()'s values unless some value was counted
  const bool any = n > 0 && n > rec[FRCNN_SUMMARY_NNONFINITE];
  double* drec = (double*)rec;
  rec[FRCNN_SUMMARY_NUM] = n > 0 ? n : 0;
  drec[FRCNN_SUMMARY_MIN] = any ? r.mn : DBL_MAX;
  drec[FRCNN_SUMMARY_MAX] = any ? r.mx : -DBL_MAX;
  drec[FRCNN_SUMMARY_SUM] = r.sum;
  drec[FRCNN_SUMMARY_SUMSQ] = r.sumsq;
}

extern "C" int frcnn_summary_limits(double* out1551) {
  if (!out1551) return FRCNN_E_ARG;
  const SummaryLimits L = summary_make_limits();          // evaluated here, at run time, by the host
  for (int i = 0; i < SUMMARY_BUCKETS; ++i) out1551[i] = L.v[i];
  return FRCNN_OK;
}

extern "C" size_t frcnn_summary_stats_workspace_bytes(int count) {
  if (count < 0 || count > SUMMARY_MAX_SEGMENTS) return 0;
  return align_up((size_t)count * SUMMARY_BLOCKS * sizeof(SummaryPartial), 256) + 256;
}

extern "C" int frcnn_summary_stats(const void* seg_table_d, int count, void* out_d, void* ws, size_t ws_bytes, void* stream) {
  if (count < 0 || count > SUMMARY_MAX_SEGMENTS) return FRCNN_E_ARG;
  if (count == 0) return FRCNN_OK;
  if (!seg_table_d || !out_d || !ws) return FRCNN_E_ARG;
  if (ws_bytes < frcnn_summary_stats_workspace_bytes(count)) return FRCNN_E_WS;
  hipStream_t s = (hipStream_t)stream;
  SummaryPartial* partial = (SummaryPartial*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
  HIP_TRY(hipMemsetAsync(out_d, 0, (size_t)count * FRCNN_SUMMARY_RECORD * sizeof(long long), s));
  hipLaunchKernelGGL(k_summary_stats, dim3(SUMMARY_BLOCKS, count), dim3(SUMMARY_THREADS), 0, s, (const SummarySeg*)seg_table_d, (long long*)out_d,
                     partial);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_summary_finish, dim3(cdiv(count, SUMMARY_THREADS)), dim3(SUMMARY_THREADS), 0, s, (const SummarySeg*)seg_table_d, count,
                     (long long*)out_d, partial);
  LAUNCH_CHECK();
  return FRCNN_OK;
}

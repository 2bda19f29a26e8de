// COCO bbox evaluation, the per-(image, category) half: IoU of every (detection, gt) pair in float64 and the crowd-aware greedy
// matching at T IoU thresholds x A area ranges (lib/datasets/coco_eval.py states the protocol; evaluate -> accumulate -> summarize, the
// last two stay host numpy).  Compiled with -ffp-contract=off: one rounding per operation, so the IoU equals the host's bit for bit.
//
// One workgroup of one wave per group.  The wave first fills the group's D x G IoU tile, then lane a*T+t runs the sequential greedy scan
// of (area range a, threshold t) over the <= max_det detections; its "gt already matched" flags are bytes at [g*64 + lane].  Tile and
// flags live in LDS when D*G*8 + 68*G <= COCO_LDS_BYTES (16 KiB: ten groups per CU), else in the group's slice of the workspace.
#include "common.h"

#define COCO_LANES 64
#define COCO_LDS_BYTES 16384
#define COCO_SCAN_THREADS 1024

// pair_off[g] = sum over groups before g of D*G (the pair-CSR of iou_out and of the workspace tiles); one workgroup, chunked scan
__global__ void __launch_bounds__(COCO_SCAN_THREADS) k_coco_pair_offsets(const long long* __restrict__ det_off, const long long* __restrict__ gt_off,
                                                                          int n_groups, long long* __restrict__ pair_off) {
  __shared__ long long part[COCO_SCAN_THREADS];
  const int tid = threadIdx.x;
  const int chunk = (n_groups + COCO_SCAN_THREADS - 1) / COCO_SCAN_THREADS;
  const int lo = min(tid * chunk, n_groups), hi = min(lo + chunk, n_groups);
  long long s = 0;
  for (int g = lo; g < hi; ++g) s += (det_off[g + 1] - det_off[g]) * (gt_off[g + 1] - gt_off[g]);
  part[tid] = s;
  __syncthreads();
  for (int step = 1; step < COCO_SCAN_THREADS; step <<= 1) {      // inclusive Hillis-Steele scan of the chunk sums
    const long long v = tid >= step ? part[tid - step] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  long long run = part[tid] - s;
  for (int g = lo; g < hi; ++g) {
    pair_off[g] = run;
    run += (det_off[g + 1] - det_off[g]) * (gt_off[g + 1] - gt_off[g]);
  }
  if (tid == COCO_SCAN_THREADS - 1) pair_off[n_groups] = part[tid];
}

// xywh boxes, float64, no "+1": 0 unless both overlaps are positive, else i / (crowd ? det area : det area + gt area - i)
__device__ __forceinline__ double coco_iou(const double* d, const double* g, bool crowd) {
  const double dx2 = d[0] + d[2], dy2 = d[1] + d[3], gx2 = g[0] + g[2], gy2 = g[1] + g[3];
  const double iw = (dx2 < gx2 ? dx2 : gx2) - (d[0] > g[0] ? d[0] : g[0]);
  const double ih = (dy2 < gy2 ? dy2 : gy2) - (d[1] > g[1] ? d[1] : g[1]);
  if (iw <= 0.0 || ih <= 0.0) return 0.0;
  const double inter = iw * ih, da = d[2] * d[3];
  const double uni = crowd ? da : (da + g[2] * g[3]) - inter;
  return inter / uni;
}

__global__ void __launch_bounds__(COCO_LANES) k_coco_match(
    const double* __restrict__ det_xywh, const long long* __restrict__ det_off, const double* __restrict__ gt_xywh,
    const double* __restrict__ gt_area, const unsigned char* __restrict__ gt_crowd, const long long* __restrict__ gt_off,
    const double* __restrict__ iou_thrs, int T, const double* __restrict__ area_rng, int A, int n_groups,
    unsigned char* __restrict__ det_matched, unsigned char* __restrict__ det_ignored, unsigned char* __restrict__ gt_ignored,
    double* __restrict__ iou_out, const long long* __restrict__ pair_off, unsigned char* ws_tiles, size_t ws_tile_bytes) {
  extern __shared__ double lds[];
  const int grp = blockIdx.x, lane = threadIdx.x;
  const long long d0 = det_off[grp], g0 = gt_off[grp];
  const long long D = det_off[grp + 1] - d0, G = gt_off[grp + 1] - g0;
  const long long n_det = det_off[n_groups], n_gt = gt_off[n_groups];
  if (D < 0 || G < 0 || (D == 0 && G == 0)) return;

  // gt_ignored[a][g] = crowd or annotation area outside [lo, hi]; written for every group, read back below by this workgroup
  for (long long i = lane; i < (long long)A * G; i += COCO_LANES) {
    const int a = (int)(i / G);
    const long long g = i - (long long)a * G;
    const double ar = gt_area[g0 + g];
    gt_ignored[(size_t)a * n_gt + g0 + g] = (gt_crowd[g0 + g] != 0 || ar < area_rng[2 * a] || ar > area_rng[2 * a + 1]) ? 1 : 0;
  }
  if (D == 0) return;                         // gts only: their flags are all there is to write

  const size_t need = (size_t)D * G * 8 + (size_t)G * COCO_LANES;
  const bool in_lds = need + (size_t)G * 4 <= COCO_LDS_BYTES;
  double* tile;
  unsigned char* taken;                       // [g*64 + lane]: gt g matched by an earlier detection of this lane's (a, t)
  if (in_lds) {
    tile = lds;
    taken = (unsigned char*)(lds + D * G);
  } else {
    const size_t off = (size_t)pair_off[grp] * 8 + (size_t)g0 * COCO_LANES;
    if (off + need > ws_tile_bytes) return;   // a workspace sized for other totals: never write past it
    tile = (double*)(ws_tiles + off);
    taken = (unsigned char*)(tile + D * G);
  }
  for (long long i = lane; i < D * G; i += COCO_LANES) {
    const long long d = i / G, g = i - d * G;
    const double v = coco_iou(det_xywh + 4 * (d0 + d), gt_xywh + 4 * (g0 + g), gt_crowd[g0 + g] != 0);
    tile[i] = v;
    if (iou_out) iou_out[pair_off[grp] + i] = v;
  }
  for (long long i = lane; i < G * COCO_LANES; i += COCO_LANES) taken[i] = 0;
  __threadfence_block();
  __syncthreads();
  if (lane >= A * T) return;

  const int a = lane / T, t = lane - a * T;
  const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
  const double thr = iou_thrs[t] < 1.0 - 1e-10 ? iou_thrs[t] : 1.0 - 1e-10;
  const unsigned char* ign = gt_ignored + (size_t)a * n_gt + g0;
  const unsigned char* crowd = gt_crowd + g0;
  unsigned char* dm = det_matched + ((size_t)a * T + t) * n_det + d0;
  unsigned char* di = det_ignored + ((size_t)a * T + t) * n_det + d0;
  for (long long d = 0; d < D; ++d) {
    const double* row = tile + d * G;
    double best = thr;
    long long m = -1;
    // gts are visited non-ignored first, each class in original order: two passes, the second only if the first found nothing
    for (long long g = 0; g < G; ++g) {
      if (ign[g] || taken[g * COCO_LANES + lane]) continue;          // (a non-ignored gt is never a crowd)
      const double v = row[g];
      if (v < best) continue;
      best = v;
      m = g;
    }
    if (m < 0) {
      for (long long g = 0; g < G; ++g) {
        if (!ign[g] || (taken[g * COCO_LANES + lane] && !crowd[g])) continue;
        const double v = row[g];
        if (v < best) continue;
        best = v;
        m = g;
      }
    }
    unsigned char ig;
    if (m >= 0) {
      ig = ign[m];
      taken[m * COCO_LANES + lane] = 1;
    } else {
      const double ar = det_xywh[4 * (d0 + d) + 2] * det_xywh[4 * (d0 + d) + 3];
      ig = (ar < lo || ar > hi) ? 1 : 0;
    }
    dm[d] = m >= 0 ? 1 : 0;
    di[d] = ig;
  }
}

static inline size_t coco_header_bytes(int n_groups) { return align_up(((size_t)n_groups + 1) * sizeof(long long), 256); }

extern "C" size_t frcnn_coco_match_workspace_bytes(int n_groups, long long n_det, long long n_gt, long long n_pairs) {
  if (n_groups < 0 || n_det < 0 || n_gt < 0 || n_pairs < 0) return 0;
  return coco_header_bytes(n_groups) + align_up((size_t)n_pairs * 8 + (size_t)n_gt * COCO_LANES, 256) + 256;
}

extern "C" int frcnn_coco_match(const double* det_xywh_d, const long long* det_off_d, const double* gt_xywh_d, const double* gt_area_d,
                                const unsigned char* gt_crowd_d, const long long* gt_off_d, int n_groups, const double* iou_thrs_d, int T,
                                const double* area_rng_d, int A, unsigned char* det_matched_d, unsigned char* det_ignored_d,
                                unsigned char* gt_ignored_d, double* iou_out_d, void* ws, size_t ws_bytes, void* stream) {
  if (n_groups < 0 || T < 1 || A < 1 || !det_off_d || !gt_off_d || !iou_thrs_d || !area_rng_d) return FRCNN_E_ARG;
  if ((long long)A * T > COCO_LANES) return FRCNN_E_UNSUPPORTED;
  if (n_groups == 0) return FRCNN_OK;
  if (!ws) return FRCNN_E_ARG;              // (the box / flag arrays may be NULL when the offsets say they are empty: never dereferenced)
  const size_t header = coco_header_bytes(n_groups);
  if (ws_bytes < header) return FRCNN_E_WS;
  hipStream_t s = (hipStream_t)stream;
  long long* pair_off = (long long*)ws;
  hipLaunchKernelGGL(k_coco_pair_offsets, dim3(1), dim3(COCO_SCAN_THREADS), 0, s, det_off_d, gt_off_d, n_groups, pair_off);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_coco_match, dim3(n_groups), dim3(COCO_LANES), COCO_LDS_BYTES, s, det_xywh_d, det_off_d, gt_xywh_d, gt_area_d, gt_crowd_d,
                     gt_off_d, iou_thrs_d, T, area_rng_d, A, n_groups, det_matched_d, det_ignored_d, gt_ignored_d, iou_out_d, pair_off,
                     (unsigned char*)ws + header, ws_bytes - header);
  LAUNCH_CHECK();
  return FRCNN_OK;
}

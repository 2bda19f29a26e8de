// Test-time post-processing of libfrcnn_hip.so (gfx950, wave64): im_detect's box stage, per-class hard NMS and Soft-NMS, bounding-box
// voting, the merge of two flip views and the final max_per_image cut (model/test.py:95-105 and :162-180), batched over B images.
// The proposal side lives in detect_kernels.hip; what the two share is in nms_shared.h.  Compiled with -ffp-contract=off like it: every
// f32 op keeps its own rounding, as in the reference's numpy / Cython code (citations relative to the reference's lib/).
#include "common.h"
#include "nms_shared.h"
#include "softnms_math.h"
#include "boxvote_math.h"

// ------------------------------------------------------------------------------------------------
// THE STAGING RULE, stated once.  Row r of an image is a candidate of foreground class j iff r < num_rois and cls_prob[r, j] >
// score_thresh (test.py:163).  Its box is rois[r, 1:5] / im_scale, each division in double and rounded to f32 (test.py:95); with
// bbox_pred that box is decoded with the class's deltas (decode_box, test.py:101) and clipped to the image ONE-SIDED -- x1, y1 from below
// at 0, x2, y2 from above at dim - 1 (test.py:67-77); without it (cfg.TEST.BBOX_REG False, test.py:103-105) it is the scaled roi itself,
// neither regressed nor clipped.  Every kernel that needs a candidate -- hard NMS, Soft-NMS, and the vote stage, which must see exactly
// the boxes the NMS stage saw -- gets it from stage_candidate; k_im_detect_boxes applies the same two helpers to every row and class.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 scaled_roi(const float* ro, double im_scale) {
  return make_float4((float)((double)ro[1] / im_scale), (float)((double)ro[2] / im_scale), (float)((double)ro[3] / im_scale),
                     (float)((double)ro[4] / im_scale));
}
__device__ __forceinline__ float4 decode_clip(const float4 box, const float4 d, float hi_x, float hi_y) {
  float4 b = decode_box(box, d);
  b.x = rmax(b.x, 0.0f); b.y = rmax(b.y, 0.0f);
  b.z = rmin(b.z, hi_x); b.w = rmin(b.w, hi_y);
  return b;
}

// A ROW LOADER is load(r, box, score) -> is row r a candidate.  The caller hands it a zero box and a zero score; the loader overwrites
// what its source holds for the row, so a row that is no candidate keeps the zero box, and a row past the end the zero score too.

// the rows of workgroup (class blockIdx.x + 1, image blockIdx.y) of a per-class kernel
struct ClassRows {
  const float *prob, *bbox_pred, *rois;     // the image's slices; bbox_pred is meaningful only if `regress`
  bool regress;
  int R, C, j, nr;                          // j: the class, 0 is background (test.py:162); nr = min(num_rois, R)
  double im_scale;
  float hi_x, hi_y, score_thresh;
};
__device__ __forceinline__ ClassRows class_rows(const float* prob_all, const float* bbox_pred_all, const float* rois_all,
                                                const int* num_rois, int R, int C, double im_scale, float hi_x, float hi_y,
                                                float score_thresh) {
  const int img = blockIdx.y;
  return ClassRows{prob_all + (size_t)img * R * C, bbox_pred_all + (size_t)img * R * 4 * C, rois_all + (size_t)img * R * 5,
                   bbox_pred_all != nullptr, R, C, (int)blockIdx.x + 1, num_rois ? min(num_rois[img], R) : R, im_scale, hi_x, hi_y,
                   score_thresh};
}
// the workgroup's (image, foreground class) as an index into cls_dets [.., R, 5] / cls_count
__device__ __forceinline__ size_t class_slot(int C) { return (size_t)(int)blockIdx.y * (C - 1) + blockIdx.x; }
// row r < R of the class, as a row loader: the score is read for every such row, a candidate or not; the box only for a candidate.
// on_candidate() runs inside the candidate's branch: the hard stage counts its candidates there, which at R = 1000 measures 1 % faster
// than counting on the returned flag (profiles/detect_post_refactor.txt).
template <typename OnCandidate>
__device__ __forceinline__ bool stage_candidate(const ClassRows& v, int r, float4& box, float& score, OnCandidate on_candidate) {
  score = v.prob[(size_t)r * v.C + v.j];
  const bool valid = (r < v.nr) && (score > v.score_thresh);
  if (valid) {
    box = scaled_roi(v.rois + 5 * (size_t)r, v.im_scale);
    if (v.regress) box = decode_clip(box, *(const float4*)(v.bbox_pred + (size_t)r * 4 * v.C + 4 * v.j), v.hi_x, v.hi_y);
    on_candidate();
  }
  return valid;
}
__device__ __forceinline__ bool stage_candidate(const ClassRows& v, int r, float4& box, float& score) {
  return stage_candidate(v, r, box, score, [] {});
}
// row r of one class given as dets [n,5] = x1,y1,x2,y2,score (frcnn_soft_nms, frcnn_box_vote): every row below n is a candidate
__device__ __forceinline__ bool dets_candidate(const float* dets, int n, int r, float4& box, float& score) {
  if (r >= n) return false;
  const float* d = dets + 5 * (size_t)r;
  box = make_float4(d[0], d[1], d[2], d[3]);
  score = d[4];
  return true;
}

// im_detect's box stage alone (model/test.py:95-102): the staging rule's box for EVERY row and class, no filter
__global__ void k_im_detect_boxes(const float* __restrict__ rois, const float* __restrict__ bbox_pred, int R, int C,
                                  double im_scale, float hi_x, float hi_y, float4* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= R * C) return;
  float4 b = scaled_roi(rois + 5 * (size_t)(t / C), im_scale);
  if (bbox_pred) b = decode_clip(b, ((const float4*)bbox_pred)[t], hi_x, hi_y);
  out[t] = b;
}

extern "C" int frcnn_im_detect_boxes(const float* rois_d, const float* bbox_pred_d, int R, int C, double im_scale, int im_h,
                                     int im_w, float* boxes_d, void* stream) {
  if (R < 0 || C <= 0 || !(im_scale > 0)) return FRCNN_E_ARG;
  if (R == 0) return FRCNN_OK;
  if (!rois_d || !boxes_d) return FRCNN_E_ARG;          // bbox_pred_d NULL: cfg.TEST.BBOX_REG False
  hipLaunchKernelGGL(k_im_detect_boxes, dim3(cdiv(R * C, 256)), dim3(256), 0, (hipStream_t)stream, rois_d, bbox_pred_d, R, C,
                     im_scale, (float)(im_w - 1), (float)(im_h - 1), (float4*)boxes_d);
  LAUNCH_CHECK();
  return FRCNN_OK;
}

// ------------------------------------------------------------------------------------------------
// kernel A (hard NMS): one workgroup per (foreground class, image): staging, rank sort, suppression bitmask and greedy reduce -- all in
//           LDS (the mask of 1024 x 16 words reuses the sort scratch).
// kernel B: one workgroup per image: exact max_per_image-th score by 4-pass radix select, then an
//           order-preserving compaction (wave ballot + popcount prefix) into the record list.
// ------------------------------------------------------------------------------------------------
#define PC_MAXR 1024
#define PC_THREADS 1024          // the 64x64-IoU mask rows of a class are the bulk of the work: spread them over 16 waves

// dynamic LDS: sboxes float4[Rp] | sscores float[Rp] | union { keys u64[Rp] + boxes float4[Rp] ; mask u64[Rp * Rp/64] }
static size_t perclass_lds_bytes(int R) {
  const size_t Rp = (size_t)align_up((size_t)R, 64);
  const size_t sort_b = Rp * (sizeof(u64) + sizeof(float4)), mask_b = Rp * (Rp / 64) * sizeof(u64);
  return Rp * (sizeof(float4) + sizeof(float)) + (sort_b > mask_b ? sort_b : mask_b);
}

template <int RULE>
__global__ __launch_bounds__(PC_THREADS) void k_perclass_nms(const float* __restrict__ prob_all, const float* __restrict__ bbox_pred_all,
                                                      const float* __restrict__ rois_all, const int* __restrict__ num_rois,
                                                      int R, int C, double im_scale, float hi_x, float hi_y, float thr,
                                                      float score_thresh, float* __restrict__ cls_dets_all,
                                                      int* __restrict__ cls_count_all) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pc_smem[];
  __shared__ int nvalid_s;
  const int Rp = (R + 63) & ~63;
  float4* sboxes = (float4*)pc_smem;
  float* sscores = (float*)(sboxes + Rp);
  unsigned char* un = (unsigned char*)(sscores + Rp);
  u64* keys = (u64*)un;
  float4* boxes = (float4*)(keys + Rp);
  u64* mask = (u64*)un;                                 // valid after the sort: keys / boxes are dead by then
  const ClassRows v = class_rows(prob_all, bbox_pred_all, rois_all, num_rois, R, C, im_scale, hi_x, hi_y, score_thresh);
  float* out = cls_dets_all + class_slot(C) * (size_t)R * 5;
  const int tid = threadIdx.x;
  if (tid == 0) nvalid_s = 0;
  __syncthreads();
  for (int r = tid; r < R; r += PC_THREADS) {
    float4 b = make_float4(0, 0, 0, 0);
    float s;
    const bool valid = stage_candidate(v, r, b, s, [&] { atomicAdd(&nvalid_s, 1); });
    boxes[r] = b;
    keys[r] = valid ? make_key(s, (u32)r) : (u64)(0xffffffffu - (u32)r);        // invalid rows sort last
  }
  __syncthreads();
  const int nv = nvalid_s;
  for (int r = tid; r < R; r += PC_THREADS) {
    const u64 mine = keys[r];
    int rk = 0;
    for (int q = 0; q < R; ++q) rk += (keys[q] > mine) ? 1 : 0;
    if (rk < nv) {
      sboxes[rk] = boxes[r];
      sscores[rk] = key_score(mine);
    }
  }
  __syncthreads();                                      // keys / boxes dead from here: the mask takes their place
  const int words = (nv + 63) / 64;
  for (int t = tid; t < nv * words; t += PC_THREADS) {
    const int i = t / words, w = t % words;
    u64 bits = 0;
    if (w >= (i >> 6)) {
      const float4 bi = sboxes[i];
      const float ai = box_area(bi);
      const int nj = min(64, nv - w * 64);
      for (int q = 0; q < nj; ++q) {
        const int gj = w * 64 + q;
        if (gj > i) {
          const float4 bj = sboxes[gj];
          if (rule_suppresses<RULE>(bi, ai, bj, box_area(bj), thr)) bits |= (1ull << q);
        }
      }
    }
    mask[(size_t)i * words + w] = bits;
  }
  __syncthreads();
  if (tid < 64) {
    const int n = (nv > 0) ? greedy_reduce_lds(mask, nv, words, [&](int pos, int i) {
      const float4 b = sboxes[i];
      float* o = out + 5 * (size_t)pos;
      o[0] = b.x; o[1] = b.y; o[2] = b.z; o[3] = b.w; o[4] = sscores[i];
    }) : 0;
    if (tid == 0) cls_count_all[class_slot(C)] = n;
  }
}

__global__ __launch_bounds__(1024) void k_final_select(const float* __restrict__ cls_dets_all, const int* __restrict__ cls_count_all,
                                                       int nfg, int R, int max_per_image, float* __restrict__ out_dets_all,
                                                       int* __restrict__ out_count, int max_out, long long out_stride) {
  __shared__ int hist[256];
  __shared__ int wave_off[16];
  __shared__ u32 sel_prefix, sel_mask;
  __shared__ int sel_k, total_s, running_s, pick_b, pick_a;
  __shared__ int wtot[4];
  const int img = blockIdx.x;
  const float* cls_dets = cls_dets_all + (size_t)img * nfg * R * 5;
  const int* cls_count = cls_count_all + (size_t)img * nfg;
  float* out_dets = out_dets_all + (size_t)img * (size_t)out_stride;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int span = nfg * R;
  if (tid == 0) { total_s = 0; running_s = 0; }
  __syncthreads();
  for (int t = tid; t < nfg; t += 1024) atomicAdd(&total_s, cls_count[t]);
  __syncthreads();
  const int total = total_s;
  u32 cut = 0;                                              // keep everything (test.py:175: only if len > max)
  if (max_per_image > 0 && total > max_per_image) {
    if (tid == 0) { sel_prefix = 0; sel_mask = 0; sel_k = max_per_image; }
    for (int shift = 24; shift >= 0; shift -= 8) {
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      const u32 pf = sel_prefix, mk = sel_mask;
      for (int t = tid; t < span; t += 1024) {
        const int c = t / R, p = t % R;
        if (p < cls_count[c]) {
          const u32 key = sortable_u32(cls_dets[(size_t)t * 5 + 4]);
          if ((key & mk) == pf) atomicAdd(&hist[(key >> shift) & 255], 1);
        }
      }
      __syncthreads();
      pick_bin(hist, sel_k, wtot, &pick_b, &pick_a);
      if (tid == 0) {
        sel_k -= pick_a;
        sel_prefix |= ((u32)pick_b << shift);
        sel_mask |= (255u << shift);
      }
      __syncthreads();
    }
    cut = sel_prefix;                                       // key of np.sort(scores)[-max_per_image]
  }
  // order-preserving compaction, class-major
  for (int base = 0; base < span; base += 1024) {
    const int t = base + tid;
    bool f = false;
    if (t < span) {
      const int c = t / R, p = t % R;
      f = (p < cls_count[c]) && (sortable_u32(cls_dets[(size_t)t * 5 + 4]) >= cut);     // test.py:178 `>=`
    }
    const u64 bal = __ballot(f);
    if (lane == 0) wave_off[wave] = __popcll(bal);
    __syncthreads();
    int off = running_s;
    for (int w = 0; w < wave; ++w) off += wave_off[w];
    if (f) {
      const int pos = off + __popcll(bal & ((1ull << lane) - 1ull));
      if (pos < max_out) {
        const float* d = cls_dets + (size_t)t * 5;
        float* o = out_dets + (size_t)pos * 6;
        o[0] = d[0]; o[1] = d[1]; o[2] = d[2]; o[3] = d[3]; o[4] = d[4];
        o[5] = (float)(t / R + 1);
      }
    }
    __syncthreads();
    if (tid == 0) {
      int s = 0;
      for (int w = 0; w < 16; ++w) s += wave_off[w];
      running_s += s;
    }
    __syncthreads();
  }
  if (tid == 0) out_count[img] = running_s;
  for (int p = running_s + tid; p < max_out; p += 1024) {
    float* o = out_dets + (size_t)p * 6;
    o[0] = o[1] = o[2] = o[3] = o[4] = o[5] = 0.0f;
  }
}

// ------------------------------------------------------------------------------------------------
// Soft-NMS (csrc/softnms_math.h states the rule): per-class suppression that decays a neighbour's score instead of deleting it.
// There is no bitmask to precompute: a class is a chain of up to R dependent select-then-decay steps, so ONE wave runs it with the
// class resident in registers -- candidate r sits in lane r % 64, slot r / 64 (PL slots a lane, PL * 64 >= R, PL <= 16): box, area and
// current score, 6 VGPRs a slot, plus one bit of a per-lane `live` word.  A step: the lane-local best key was already found while the
// previous step decayed; the wave maximum of its score half and then of its index half (DPP all-reduce inside each row of 16, four
// readlanes) names the winner, whose lane is r % 64, so its box comes by readlane; lane 0 stores the row; every lane decays its live
// slots and finds its next local best in the same pass.  No LDS and no barrier anywhere.  Sixteen waves with a barrier per step would
// spend the step on the barrier pair; the price of one wave is that the Gaussian weight's float64 polynomial (about 40 FP64
// operations and one FP64 division a candidate) is paid PL times in sequence.  Assumed, not measured, when this was written: about
// 150 cycles for the two reductions and the broadcast plus about 40 cycles a slot for the linear weight (IoU with its division), i.e.
// "a few hundred cycles" a step at R = 300.  MEASURED (profiles/soft_nms.txt, 2.4 GHz assumed): 1 400 cycles a step at 2 slots, 2 700
// (linear) / 4 500 (Gaussian) at the 5 slots of R = 300, 7 000 / 12 500 at 16 -- ten times the estimate.  Presumably a lone wave pays the
// whole latency of every dependent VALU operation (the IEEE division alone is a chain of ten of them a slot) with nothing else to issue
// meanwhile.  At 300 rois that is +0.10 ms (linear) / +0.21 ms (Gaussian) on the 0.055 ms of the hard stage for 8 images -- under 2 % of
// the 8-image step -- but 0.25 ms of the 3.2 ms a one-by-one test_net image takes (309 -> 287 images/s, ResNet-50).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ u32 wave_max_u32(u32 v) {       // all 64 lanes active
  v = max(v, (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false));    // quad_perm [1,0,3,2]
  v = max(v, (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false));    // quad_perm [2,3,0,1]
  v = max(v, (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, false));   // row_half_mirror
  v = max(v, (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, false));   // row_mirror: every lane holds its row's maximum
  const u32 a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16);
  const u32 c = __builtin_amdgcn_readlane(v, 32), d = __builtin_amdgcn_readlane(v, 48);
  return max(max(a, b), max(c, d));
}
__device__ __forceinline__ float readlane_f32(float v, int lane_uniform) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane_uniform));
}

// the loop of softnms_math.h on one wave; emit(pos, box, score, r) is called by every lane with uniform arguments -> the count
template <int PL, int METHOD, typename Emit>
__device__ __forceinline__ int soft_nms_wave(float4 (&box)[PL], float (&sc)[PL], u32 live, float thr, int rule, double sigma,
                                             float min_score, Emit emit) {
  const u32 lane = threadIdx.x;
  float ar[PL];
  u32 bhi = 0, blo = 0;                                 // the lane's best live key; 0 = none (no finite score maps to 0)
  float4 bb = make_float4(0, 0, 0, 0);
  float ba = 0.0f, bs = 0.0f;                           // bs: the best slot's score itself (the key does not hold a zero's sign)
#pragma unroll
  for (int i = 0; i < PL; ++i) {
    ar[i] = softnms_area(box[i].x, box[i].y, box[i].z, box[i].w);
    const u32 hi = softnms_sortable(sc[i]);
    if (((live >> i) & 1u) && hi > bhi) {               // slots ascend in r: `>` keeps the lower r of equal scores
      bhi = hi, blo = ~(lane + 64u * i), bb = box[i], ba = ar[i], bs = sc[i];
    }
  }
  int m = 0;
  for (;;) {
    const u32 whi = wave_max_u32(bhi);
    if (whi == 0) break;                                // nothing left
    const u32 wr = ~wave_max_u32(bhi == whi ? blo : 0u);
    const int wl = __builtin_amdgcn_readfirstlane((int)(wr & 63u));
    const float wscore = readlane_f32(bs, wl);
    if (wscore < min_score) break;
    const float4 wb = make_float4(readlane_f32(bb.x, wl), readlane_f32(bb.y, wl), readlane_f32(bb.z, wl), readlane_f32(bb.w, wl));
    const float wa = readlane_f32(ba, wl);
    emit(m, wb, wscore, wr);
    ++m;
    bhi = 0, blo = 0;
#pragma unroll
    for (int i = 0; i < PL; ++i) {
      const u32 r = lane + 64u * i, bit = 1u << i;
      if (r == wr) live &= ~bit;
      if (live & bit) {
        const float ov = softnms_iou(wb.x, wb.y, wb.z, wb.w, wa, box[i].x, box[i].y, box[i].z, box[i].w, ar[i]);
        const float w = METHOD == SOFTNMS_LINEAR ? softnms_weight_linear(ov, thr, rule) : softnms_weight_gaussian(ov, sigma);
        sc[i] = sc[i] * w;
        const u32 hi = softnms_sortable(sc[i]);
        if (hi > bhi) bhi = hi, blo = ~r, bb = box[i], ba = ar[i], bs = sc[i];
      }
    }
  }
  return m;
}

// the wave's register slots from a row loader, asked for every r in [0, 64 * PL) -> the lane's `live` word
template <int PL, typename Load>
__device__ __forceinline__ u32 soft_fill(float4 (&box)[PL], float (&sc)[PL], Load load) {
  u32 live = 0;
#pragma unroll
  for (int i = 0; i < PL; ++i) {
    float4 b = make_float4(0, 0, 0, 0);
    float s = 0.0f;
    if (load((int)threadIdx.x + 64 * i, b, s)) live |= 1u << i;
    box[i] = b;
    sc[i] = s;
  }
  return live;
}

template <int PL, int METHOD>
__global__ __launch_bounds__(64) void k_perclass_soft_nms(const float* __restrict__ prob_all, const float* __restrict__ bbox_pred_all,
                                                          const float* __restrict__ rois_all, const int* __restrict__ num_rois,
                                                          int R, int C, double im_scale, float hi_x, float hi_y, float thr, int rule,
                                                          double sigma, float min_score, float score_thresh,
                                                          float* __restrict__ cls_dets_all, int* __restrict__ cls_count_all) {
  const ClassRows v = class_rows(prob_all, bbox_pred_all, rois_all, num_rois, R, C, im_scale, hi_x, hi_y, score_thresh);
  float* out = cls_dets_all + class_slot(C) * (size_t)R * 5;
  const int lane = threadIdx.x;
  float4 box[PL];
  float sc[PL];
  const u32 live = soft_fill<PL>(box, sc, [&](int r, float4& b, float& s) { return r < R && stage_candidate(v, r, b, s); });
  const int n = soft_nms_wave<PL, METHOD>(box, sc, live, thr, rule, sigma, min_score, [&](int pos, float4 b, float s, u32) {
    if (lane == 0) {                                    // pos < the class's candidates <= R
      float* o = out + 5 * (size_t)pos;
      o[0] = b.x; o[1] = b.y; o[2] = b.z; o[3] = b.w; o[4] = s;
    }
  });
  if (lane == 0) cls_count_all[class_slot(C)] = n;
}

// one class given as dets [k,5]: the emitted rows and their input rows in order, the rest 0 / -1, and the count
template <int PL, int METHOD>
__global__ __launch_bounds__(64) void k_soft_nms(const float* __restrict__ dets, int k, float thr, int rule, double sigma, float min_score,
                                                 float* __restrict__ out_dets, int* __restrict__ out_index, int* __restrict__ out_count) {
  const int lane = threadIdx.x;
  float4 box[PL];
  float sc[PL];
  const u32 live = soft_fill<PL>(box, sc, [&](int r, float4& b, float& s) { return dets_candidate(dets, k, r, b, s); });
  const int n = soft_nms_wave<PL, METHOD>(box, sc, live, thr, rule, sigma, min_score, [&](int pos, float4 b, float s, u32 r) {
    if (lane == 0) {                                    // pos < k
      float* o = out_dets + 5 * (size_t)pos;
      o[0] = b.x; o[1] = b.y; o[2] = b.z; o[3] = b.w; o[4] = s;
      out_index[pos] = (int)r;
    }
  });
  for (int p = n + lane; p < k; p += 64) {
    float* o = out_dets + 5 * (size_t)p;
    o[0] = o[1] = o[2] = o[3] = o[4] = 0.0f;
    out_index[p] = -1;
  }
  if (lane == 0) *out_count = n;
}

// slots a lane: 2 (n <= 128), 5 (<= 320: the 300 rois of test time), 8 (<= 512), 16 (<= 1024)
static int soft_slots(int n) { return n <= 128 ? 2 : n <= 320 ? 5 : n <= 512 ? 8 : 16; }
#define SOFT_PICK(KERN, pl, method)                                                                                        \
  ((method) == SOFTNMS_LINEAR ? ((pl) == 2 ? KERN<2, 1> : (pl) == 5 ? KERN<5, 1> : (pl) == 8 ? KERN<8, 1> : KERN<16, 1>)    \
                              : ((pl) == 2 ? KERN<2, 2> : (pl) == 5 ? KERN<5, 2> : (pl) == 8 ? KERN<8, 2> : KERN<16, 2>))

extern "C" int frcnn_soft_nms(const float* dets_d, int k, double nms_thresh, int rule, int method, double sigma, float min_score,
                              float* out_dets_d, int* out_index_d, int* out_count_d, void* stream) {
  if (k < 0 || !dets_d || !out_dets_d || !out_index_d || !out_count_d || !softnms_args_ok(rule, method, sigma, min_score))
    return FRCNN_E_ARG;
  if (k > SOFTNMS_MAX) return FRCNN_E_UNSUPPORTED;
  auto kern = SOFT_PICK(k_soft_nms, soft_slots(k), method);
  hipLaunchKernelGGL(kern, dim3(1), dim3(64), 0, (hipStream_t)stream, dets_d, k, softnms_thresh_f32(nms_thresh, rule), rule, sigma,
                     min_score, out_dets_d, out_index_d, out_count_d);
  LAUNCH_CHECK();
  return FRCNN_OK;
}

extern "C" int frcnn_soft_nms_host(const float* dets, int k, double nms_thresh, int rule, int method, double sigma, float min_score,
                                   float* out_dets, int* out_index, int* out_count) {
  if (k < 0 || !dets || !out_dets || !out_index || !out_count || !softnms_args_ok(rule, method, sigma, min_score)) return FRCNN_E_ARG;
  if (k > SOFTNMS_MAX) return FRCNN_E_UNSUPPORTED;
  float cur[SOFTNMS_MAX];
  uint64_t key[SOFTNMS_MAX];
  *out_count = softnms_host(dets, k, softnms_thresh_f32(nms_thresh, rule), rule, method, sigma, min_score, cur, key, out_dets, out_index);
  return FRCNN_OK;
}

// ------------------------------------------------------------------------------------------------
// Bounding-box voting and the merge of two flip views (csrc/boxvote_math.h states both rules).
// k_perclass_vote runs between the per-class stage (hard or Soft-NMS) and k_final_select: one workgroup per (foreground class, image)
// stages the class's candidates into LDS BY ROW -- box 16 B + original score 4 B a row, 20 KB at 1024 rows, plus one validity bit a row
// from a wave ballot -- and then thread t owns the kept detections t, t + 256, ... of cls_dets: it walks the rows in ascending order,
// every lane of a wave reading the SAME LDS address (a broadcast, no bank conflict), skips the rows that are no candidates (their bit is
// wave-uniform: no divergence), accumulates the voters in double and overwrites its four coordinates in place.  The trip count is R for every thread.  256 threads: the hard stage keeps a few
// dozen rows a class, Soft-NMS at min_score 0 up to R -- four waves, one a SIMD, cover 1024 kept rows in four rounds, and the double
// sums are five additions and four products a VOTER against some thirty float32 operations and a division a CANDIDATE, so the float64
// rate of the VALU is not what bounds it.  No global atomics, nothing allocated: legal on a capturing stream like its neighbours.
// ------------------------------------------------------------------------------------------------
#define VOTE_THREADS 256

struct VoteLds {
  float4 box[BOXVOTE_MAX];
  float score[BOXVOTE_MAX];
  u64 valid[BOXVOTE_MAX / 64];
};

// rows [0, nrows) of `c` from a row loader; nrows <= BOXVOTE_MAX = 1024 and base a multiple of 256 below it: r <= 1023
template <typename Load>
__device__ __forceinline__ void vote_fill(VoteLds& c, int nrows, Load load) {
  const int tid = threadIdx.x;
  for (int base = 0; base < nrows; base += VOTE_THREADS) {
    const int r = base + tid;
    float4 b = make_float4(0, 0, 0, 0);
    float s = 0.0f;
    const u64 bal = __ballot(load(r, b, s));            // the wave's 64 rows are one word: r >> 6 is uniform in the wave
    c.box[r] = b;
    c.score[r] = s;
    if ((tid & 63) == 0) c.valid[r >> 6] = bal;
  }
  __syncthreads();
}

// rows [0, nrows) of `c` are staged (nrows <= BOXVOTE_MAX); kept [m,5] -> out [m,5] (may be the same rows: a thread reads its row first)
__device__ __forceinline__ void vote_rows(const VoteLds& c, int nrows, const float* kept, int m, double vote_thresh, float* out) {
  const int words = (nrows + 63) >> 6;
  for (int base = 0; base < m; base += VOTE_THREADS) {
    const int d = base + (int)threadIdx.x;
    const bool mine = d < m;
    float a[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (mine)
      for (int k = 0; k < 5; ++k) a[k] = kept[5 * (size_t)d + k];
    const float aa = boxvote_area(a[0], a[1], a[2], a[3]);
    BoxVoteAcc acc;
    boxvote_clear(acc);
    for (int w = 0; w < words; ++w) {
      u64 bits = c.valid[w];
      while (bits) {
        const int r = w * 64 + (int)__builtin_ctzll(bits);
        bits &= bits - 1;
        const float4 b = c.box[r];
        boxvote_see(acc, a[0], a[1], a[2], a[3], aa, b.x, b.y, b.z, b.w, c.score[r], vote_thresh);
      }
    }
    if (mine) {
      boxvote_finish(acc, a);
      for (int k = 0; k < 5; ++k) out[5 * (size_t)d + k] = a[k];
    }
  }
}

__global__ __launch_bounds__(VOTE_THREADS) void k_perclass_vote(const float* __restrict__ prob_all, const float* __restrict__ bbox_pred_all,
                                                                const float* __restrict__ rois_all, const int* __restrict__ num_rois,
                                                                int R, int C, double im_scale, float hi_x, float hi_y, float score_thresh,
                                                                double vote_thresh, float* __restrict__ cls_dets_all,
                                                                const int* __restrict__ cls_count_all) {
  __shared__ VoteLds c;
  const ClassRows v = class_rows(prob_all, bbox_pred_all, rois_all, num_rois, R, C, im_scale, hi_x, hi_y, score_thresh);
  float* dets = cls_dets_all + class_slot(C) * (size_t)R * 5;
  vote_fill(c, R, [&](int r, float4& b, float& s) { return r < R && stage_candidate(v, r, b, s); });
  const int m = min(cls_count_all[class_slot(C)], R);
  vote_rows(c, R, dets, m, vote_thresh, dets);
}

// one class: kept [m,5] and cands [n,5] in global memory -> out [m,5]
__global__ __launch_bounds__(VOTE_THREADS) void k_box_vote(const float* __restrict__ kept, int m, const float* __restrict__ cands, int n,
                                                           double vote_thresh, float* __restrict__ out) {
  __shared__ VoteLds c;
  vote_fill(c, n, [&](int r, float4& b, float& s) { return dets_candidate(cands, n, r, b, s); });
  vote_rows(c, n, kept, m, vote_thresh, out);
}

extern "C" int frcnn_box_vote(const float* kept_d, int m, const float* cands_d, int n, double vote_thresh, float* out_d, void* stream) {
  if (m < 0 || n < 0 || !kept_d || !cands_d || !out_d || !boxvote_thresh_ok(vote_thresh)) return FRCNN_E_ARG;
  if (m > BOXVOTE_MAX || n > BOXVOTE_MAX) return FRCNN_E_UNSUPPORTED;
  if (m == 0) return FRCNN_OK;
  hipLaunchKernelGGL(k_box_vote, dim3(1), dim3(VOTE_THREADS), 0, (hipStream_t)stream, kept_d, m, cands_d, n, vote_thresh, out_d);
  LAUNCH_CHECK();
  return FRCNN_OK;
}

extern "C" int frcnn_box_vote_host(const float* kept, int m, const float* cands, int n, double vote_thresh, float* out) {
  if (m < 0 || n < 0 || !kept || !cands || !out || !boxvote_thresh_ok(vote_thresh)) return FRCNN_E_ARG;
  if (m > BOXVOTE_MAX || n > BOXVOTE_MAX) return FRCNN_E_UNSUPPORTED;
  boxvote_host(kept, m, cands, n, vote_thresh, out);
  return FRCNN_OK;
}

// ------------------------------------------------------------------------------------------------
// The launch plan of detect_post, stated once: per-class stage (hard NMS or Soft-NMS) -> optional vote -> k_final_select, all on one
// stream over a workspace of cls_dets f32 [B, C-1, R, 5] | cls_count int [B, C-1].  The three entries below validate what is their own
// (all of it FRCNN_E_ARG) and call it; after that a bad shape or stride is FRCNN_E_ARG, then R > PC_MAXR is FRCNN_E_UNSUPPORTED, then a
// short workspace is FRCNN_E_WS.
// ------------------------------------------------------------------------------------------------
struct PostArgs {
  const float *cls_prob, *bbox_pred, *rois;             // bbox_pred NULL: TEST.BBOX_REG False
  const int* num_rois;
  int B, R, C;
  double im_scale;
  int im_h, im_w;
  double nms_thresh;
  int rule;
  float score_thresh;
  int max_per_image;
  double sigma;                                         // sigma, min_score: Soft-NMS only
  float min_score;
  float* out_dets;
  int* out_count;
  int max_out;
  long long out_stride;                                 // floats between images; 0 = max_out * 6
  void* ws;
  size_t ws_bytes;
  void* stream;
};

extern "C" size_t frcnn_detect_post_batched_workspace_bytes(int B, int R, int C) {
  const size_t nfg = (size_t)(C > 1 ? C - 1 : 1), b = (size_t)(B > 0 ? B : 1), r = (size_t)(R > 0 ? R : 1);
  return align_up(b * nfg * r * 5 * sizeof(float), 256) + align_up(b * nfg * sizeof(int), 256);
}
extern "C" size_t frcnn_detect_post_workspace_bytes(int R, int C) { return frcnn_detect_post_batched_workspace_bytes(1, R, C); }
extern "C" size_t frcnn_detect_post_soft_batched_workspace_bytes(int B, int R, int C) {
  return frcnn_detect_post_batched_workspace_bytes(B, R, C);
}
extern "C" size_t frcnn_detect_post_vote_batched_workspace_bytes(int B, int R, int C) {
  return frcnn_detect_post_batched_workspace_bytes(B, R, C);
}

// method: 0 hard NMS, SOFTNMS_LINEAR, SOFTNMS_GAUSSIAN (validated by the caller); vote_thresh 0: no vote stage
static int detect_post_run(const PostArgs& a, int method, double vote_thresh) {
  if (!a.cls_prob || !a.rois || !a.out_dets || !a.out_count || !a.ws) return FRCNN_E_ARG;
  if (a.B <= 0 || a.R <= 0 || a.C < 2 || a.max_out <= 0 || !(a.im_scale > 0)) return FRCNN_E_ARG;
  const long long out_stride = a.out_stride == 0 ? (long long)a.max_out * 6 : a.out_stride;
  if (out_stride < (long long)a.max_out * 6) return FRCNN_E_ARG;
  if (a.R > PC_MAXR) return FRCNN_E_UNSUPPORTED;
  if (frcnn_detect_post_batched_workspace_bytes(a.B, a.R, a.C) > a.ws_bytes) return FRCNN_E_WS;
  const int B = a.B, R = a.R, C = a.C, nfg = C - 1;
  float* cls_dets = (float*)a.ws;
  int* cls_count = (int*)((char*)a.ws + align_up((size_t)B * nfg * R * 5 * sizeof(float), 256));
  hipStream_t st = (hipStream_t)a.stream;
  const float hi_x = (float)(a.im_w - 1), hi_y = (float)(a.im_h - 1);
  if (method == 0) {
    const size_t lds = perclass_lds_bytes(R);
    auto kern = a.rule == NMS_RULE_GPU ? k_perclass_nms<NMS_RULE_GPU> : k_perclass_nms<NMS_RULE_CPU>;
    if (lds > 48 * 1024)      // beyond the default dynamic-LDS limit (R > ~512); not a stream operation, legal during capture
      HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3(nfg, B), dim3(PC_THREADS), lds, st, a.cls_prob, a.bbox_pred, a.rois, a.num_rois, R, C, a.im_scale, hi_x,
                       hi_y, rule_threshold(a.nms_thresh, a.rule), a.score_thresh, cls_dets, cls_count);
  } else {
    auto kern = SOFT_PICK(k_perclass_soft_nms, soft_slots(R), method);
    hipLaunchKernelGGL(kern, dim3(nfg, B), dim3(64), 0, st, a.cls_prob, a.bbox_pred, a.rois, a.num_rois, R, C, a.im_scale, hi_x, hi_y,
                       softnms_thresh_f32(a.nms_thresh, a.rule), a.rule, a.sigma, a.min_score, a.score_thresh, cls_dets, cls_count);
  }
  LAUNCH_CHECK();
  if (vote_thresh != 0) {
    hipLaunchKernelGGL(k_perclass_vote, dim3(nfg, B), dim3(VOTE_THREADS), 0, st, a.cls_prob, a.bbox_pred, a.rois, a.num_rois, R, C,
                       a.im_scale, hi_x, hi_y, a.score_thresh, vote_thresh, cls_dets, (const int*)cls_count);
    LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_final_select, dim3(B), dim3(1024), 0, st, cls_dets, cls_count, nfg, R, a.max_per_image, a.out_dets,
                     a.out_count, a.max_out, out_stride);
  LAUNCH_CHECK();
  return FRCNN_OK;
}

extern "C" int frcnn_detect_post_batched(const float* cls_prob_d, const float* bbox_pred_d, const float* rois_d,
                                         const int* num_rois_d, int B, int R, int C, double im_scale, int im_h, int im_w,
                                         double nms_thresh, int rule, float score_thresh, int max_per_image, float* out_dets_d,
                                         int* out_count_d, int max_out, long long out_stride, void* ws, size_t ws_bytes,
                                         void* stream) {
  if (!rule_ok(rule)) return FRCNN_E_ARG;
  return detect_post_run(PostArgs{cls_prob_d, bbox_pred_d, rois_d, num_rois_d, B, R, C, im_scale, im_h, im_w, nms_thresh, rule,
                                  score_thresh, max_per_image, 0.0, 0.0f, out_dets_d, out_count_d, max_out, out_stride, ws, ws_bytes,
                                  stream}, 0, 0.0);
}

extern "C" int frcnn_detect_post(const float* cls_prob_d, const float* bbox_pred_d, const float* rois_d,
                                 const int* num_rois_d, int R, int C, double im_scale, int im_h, int im_w,
                                 double nms_thresh, float score_thresh, int max_per_image, float* out_dets_d,
                                 int* out_count_d, int max_out, void* ws, size_t ws_bytes, void* stream) {
  return frcnn_detect_post_batched(cls_prob_d, bbox_pred_d, rois_d, num_rois_d, 1, R, C, im_scale, im_h, im_w, nms_thresh,
                                   FRCNN_NMS_RULE_CPU, score_thresh, max_per_image, out_dets_d, out_count_d, max_out, 0, ws, ws_bytes,
                                   stream);
}

extern "C" int frcnn_detect_post_soft_batched(const float* cls_prob_d, const float* bbox_pred_d, const float* rois_d,
                                              const int* num_rois_d, int B, int R, int C, double im_scale, int im_h, int im_w,
                                              double nms_thresh, int rule, float score_thresh, int max_per_image, int method,
                                              double sigma, float min_score, float* out_dets_d, int* out_count_d, int max_out,
                                              long long out_stride, void* ws, size_t ws_bytes, void* stream) {
  if (!softnms_args_ok(rule, method, sigma, min_score)) return FRCNN_E_ARG;
  return detect_post_run(PostArgs{cls_prob_d, bbox_pred_d, rois_d, num_rois_d, B, R, C, im_scale, im_h, im_w, nms_thresh, rule,
                                  score_thresh, max_per_image, sigma, min_score, out_dets_d, out_count_d, max_out, out_stride, ws,
                                  ws_bytes, stream}, method, 0.0);
}

extern "C" int frcnn_detect_post_vote_batched(const float* cls_prob_d, const float* bbox_pred_d, const float* rois_d,
                                              const int* num_rois_d, int B, int R, int C, double im_scale, int im_h, int im_w,
                                              double nms_thresh, int rule, float score_thresh, int max_per_image, int method,
                                              double sigma, float min_score, double vote_thresh, float* out_dets_d, int* out_count_d,
                                              int max_out, long long out_stride, void* ws, size_t ws_bytes, void* stream) {
  if (!boxvote_thresh_ok(vote_thresh)) return FRCNN_E_ARG;
  if (method != 0 && method != SOFTNMS_LINEAR && method != SOFTNMS_GAUSSIAN) return FRCNN_E_ARG;
  if (method == 0 ? !rule_ok(rule) : !softnms_args_ok(rule, method, sigma, min_score)) return FRCNN_E_ARG;
  return detect_post_run(PostArgs{cls_prob_d, bbox_pred_d, rois_d, num_rois_d, B, R, C, im_scale, im_h, im_w, nms_thresh, rule,
                                  score_thresh, max_per_image, sigma, min_score, out_dets_d, out_count_d, max_out, out_stride, ws,
                                  ws_bytes, stream}, method, vote_thresh);
}

#define MERGE_THREADS 128
// one workgroup per output row (2R rows an image): the row's 5C + 5 values, see boxvote_math.h; the counts are read on the device
__global__ __launch_bounds__(MERGE_THREADS) void k_merge_flip_views(const float* __restrict__ cls_prob, const float* __restrict__ bbox_pred,
                                                                    const float* __restrict__ rois, const int* __restrict__ num_rois,
                                                                    int R, int C, float wm1, float* __restrict__ out_prob,
                                                                    float* __restrict__ out_pred, float* __restrict__ out_rois,
                                                                    int* __restrict__ out_num) {
  const int rp = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int n0 = num_rois ? boxvote_clamp_count(num_rois[2 * b], R) : R, n1 = num_rois ? boxvote_clamp_count(num_rois[2 * b + 1], R) : R;
  int view, row;
  boxvote_merge_source(rp, n0, n1, &view, &row);
  const size_t src = (size_t)(2 * b + (view > 0 ? 1 : 0)) * R + row, dst = (size_t)b * 2 * R + rp;
  for (int j = tid; j < C; j += MERGE_THREADS) out_prob[dst * C + j] = boxvote_merge_prob(cls_prob + src * C, view, j);
  if (bbox_pred)
    for (int k = tid; k < 4 * C; k += MERGE_THREADS) out_pred[dst * 4 * C + k] = boxvote_merge_delta(bbox_pred + src * 4 * C, view, k);
  if (tid < 5) out_rois[dst * 5 + tid] = boxvote_merge_roi(rois + src * 5, view, tid, wm1);
  if (rp == 0 && tid == 0) out_num[b] = n0 + n1;
}

static bool merge_args_ok(const void* cls_prob, const void* rois, int B, int R, int C, float im_w_scaled, const void* out_prob,
                          const void* bbox_pred, const void* out_pred, const void* out_rois, const void* out_num) {
  return cls_prob && rois && out_prob && out_rois && out_num && (!bbox_pred || out_pred) && B > 0 && R > 0 && C >= 2 && im_w_scaled > 0;
}

extern "C" int frcnn_merge_flip_views(const float* cls_prob_d, const float* bbox_pred_d, const float* rois_d, const int* num_rois_d,
                                      int B, int R, int C, float im_w_scaled, float* out_prob_d, float* out_pred_d, float* out_rois_d,
                                      int* out_num_d, void* stream) {
  if (!merge_args_ok(cls_prob_d, rois_d, B, R, C, im_w_scaled, out_prob_d, bbox_pred_d, out_pred_d, out_rois_d, out_num_d)) return FRCNN_E_ARG;
  if (B > 65535) return FRCNN_E_ARG;
  hipLaunchKernelGGL(k_merge_flip_views, dim3(2 * R, B), dim3(MERGE_THREADS), 0, (hipStream_t)stream, cls_prob_d, bbox_pred_d, rois_d,
                     num_rois_d, R, C, im_w_scaled - 1.0f, out_prob_d, out_pred_d, out_rois_d, out_num_d);
  LAUNCH_CHECK();
  return FRCNN_OK;
}

extern "C" int frcnn_merge_flip_views_host(const float* cls_prob, const float* bbox_pred, const float* rois, const int* num_rois, int B,
                                           int R, int C, float im_w_scaled, float* out_prob, float* out_pred, float* out_rois,
                                           int* out_num) {
  if (!merge_args_ok(cls_prob, rois, B, R, C, im_w_scaled, out_prob, bbox_pred, out_pred, out_rois, out_num)) return FRCNN_E_ARG;
  boxvote_merge_host(cls_prob, bbox_pred, rois, num_rois, B, R, C, im_w_scaled, out_prob, out_pred, out_rois, out_num);
  return FRCNN_OK;
}

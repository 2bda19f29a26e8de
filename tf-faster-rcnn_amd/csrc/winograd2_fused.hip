// Winograd F(2x2,3x3) convolution, 64 -> 64 channels (block1's conv2), in ONE launch: input transform, the 16 products on the exactly
// split bf16 pipe and the output transform.  The three launches it replaces (k_wino_input -> k_gemm_x3 x 16 -> k_wino_output) move
// 1 229 MB of V and M per 300 000 pixels that exist only between them; the result needs 154 MB.
//
// One workgroup (4 waves) owns RUN = 64 consecutive tiles, in the flattened (img, ty, tx) order of k_wino_input, and all 64 output
// channels; wave w multiplies the 32 tiles (w >> 1) by the 32 channels (w & 1).  It walks the 16 transform points g = (xi, nu), nu outer:
//   * V[g] of its tiles is formed from x by the expressions of k_wino_input (row pass, then column pass; single-rounded adds and
//     subtracts, out-of-image taps 0) and written to LDS as f32, 16-byte chunk c of row t at c ^ (t & 15);
//   * the three bf16 planes of U[g] (frcnn_gemm_x3_pack, 24 KB) come in by direct-to-LDS loads, chunk c of row n at c ^ ((n >> 1) & 7);
//   * the block product runs as in k_gemm_x3: x3_split8 on the A fragments, the x3_mma16 group per 16 k in ascending k, the two
//     accumulators combined as k_gemm_x3 does for a null bias;
//   * k_wino_output's sums are left-to-right chains -- s0 = (m0 + m1) + m2, s1 = (m1 - m2) - m3 over xi, then
//     o0 = ((s.0 + s.1) + s.2) + b, o1 = ((s.1 - s.2) - s.3) + b over nu -- so M[g] is folded into them as it arrives and never stored.
// Every value is produced by the same operations in the same order as in the three launches: the result is bit for bit theirs
// (tests/test_wino2_fused_gpu.py).  x is read ONCE: a thread keeps the 4 x 4 taps of its four (tile, 4 channels) pairs in registers
// for all 16 points (192 registers: column 3 takes over column 0's when nu = 0 is done), so forming V is register arithmetic.  While
// point g is multiplied, V[g + 1] is formed into the other V buffer, a quarter under each k group, and U[g + 1] travels to the other
// U buffer; one barrier per point.  256 VGPRs + 128 AGPRs, no scratch, one workgroup per CU; LDS 2 x 16 KB V + 2 x 24 KB U = 80 KB.
#include "common.h"
#include "x3_mma.h"

namespace {

constexpr int W2_RUN = 64, W2_C = 64, W2_NT = 256;
constexpr int W2_V_BYTES = W2_RUN * W2_C * 4;            // 16 KB: one point's V block, 256-byte rows
constexpr int W2_P_BYTES = W2_C * W2_C * 2;              // 8 KB: one bf16 plane of one point's filter, 128-byte rows
constexpr int W2_U_BYTES = 3 * W2_P_BYTES;
constexpr int W2_LDS = 2 * W2_V_BYTES + 2 * W2_U_BYTES;
constexpr int W2_ITEMS = W2_RUN * (W2_C / 4) / W2_NT;    // (tile, 4 channels) pairs per thread and point
constexpr unsigned W2_OOB = 0x80000000u;                 // a byte offset past every supported tensor: the buffer load returns 0

// B^T's rows / B's columns as (first, second, subtract): (d0 - d2, d1 + d2, d2 - d1, d1 - d3)
__device__ __forceinline__ int w2_first(int p) { return p == 0 ? 0 : (p == 2 ? 2 : 1); }
__device__ __forceinline__ int w2_second(int p) { return p == 0 ? 2 : (p == 1 ? 2 : (p == 2 ? 1 : 3)); }

__device__ __forceinline__ float4 w2_pm(const float4 a, const float4 b, bool sub) {      // a - b is a + (-b) to the bit
  const float4 c = sub ? make_float4(-b.x, -b.y, -b.z, -b.w) : b;
  return make_float4(a.x + c.x, a.y + c.y, a.z + c.z, a.w + c.w);
}

struct Wino2Params {
  const float* x; const unsigned short* up; const float* bias; float* y;
  int N, H, W, TH, TW, T, act;
};

__global__ __launch_bounds__(W2_NT) void k_wino2_conv_x3(const Wino2Params p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];      // V[2] | U[2]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int run0 = blockIdx.x * W2_RUN;
  const int H = p.H, W = p.W;

  // ---- the thread's share of the input transform: tiles (tid >> 4) + 16 r, channels 4 (tid & 15) .. + 3
  const int c4 = tid & 15;
  int off0[W2_ITEMS];                   // byte offset of tap (0, 0)
  unsigned ok[W2_ITEMS];                // bit r: tap row r inside the image, bit 4 + j: tap column j
#pragma unroll
  for (int r = 0; r < W2_ITEMS; ++r) {
    const int t = run0 + (tid >> 4) + 16 * r, tc = min(t, p.T - 1);       // tiles past T: every tap masked
    const int tx = tc % p.TW, ty = (tc / p.TW) % p.TH, img = tc / (p.TW * p.TH);
    const int ih0 = 2 * ty - 1, iw0 = 2 * tx - 1;
    unsigned m = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      m |= ((unsigned)(ih0 + i) < (unsigned)H ? 1u : 0u) << i;
      m |= ((unsigned)(iw0 + i) < (unsigned)W ? 1u : 0u) << (4 + i);
    }
    ok[r] = t < p.T ? m : 0u;
    off0[r] = (((img * H + ih0) * W + iw0) * W2_C + c4 * 4) * 4;
  }
  const auto xr = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, p.N * H * W * W2_C * 4, 0x00020000);
  auto tap = [&](int r, int i, int j) {
    const bool in = ((ok[r] >> i) & (ok[r] >> (4 + j)) & 1u) != 0;
    const unsigned o = in ? (unsigned)(off0[r] + (i * W + j) * (W2_C * 4)) : W2_OOB;
    return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(xr, (int)o, 0, 0));
  };
  // the thread's 4 x 16 taps stay in registers: x is read once.  Column 0 is read by the points of nu = 0 only and column 3 by those
  // of nu = 3 only, so column 3 is loaded when column 0 has been used up and takes over its registers.
  float4 d[W2_ITEMS][4][4];
  auto load_column = [&](int j) {
#pragma unroll
    for (int r = 0; r < W2_ITEMS; ++r)
#pragma unroll
      for (int i = 0; i < 4; ++i) d[r][i][j] = tap(r, i, j);
  };
  load_column(0); load_column(2); load_column(1);
  auto form_v = [&](int xi, int nu, int r, int buf) {
    const int ia = w2_first(xi), ib = w2_second(xi), ja = w2_first(nu), jb = w2_second(nu);
    const bool rsub = xi != 1, csub = nu != 1;
    const float4 ba = w2_pm(d[r][ia][ja], d[r][ib][ja], rsub), bb = w2_pm(d[r][ia][jb], d[r][ib][jb], rsub);
    const int row = (tid >> 4) + 16 * r;
    *(float4*)(smem + buf * W2_V_BYTES + row * (W2_C * 4) + ((c4 ^ (row & 15)) * 16)) = w2_pm(ba, bb, csub);
  };

  // ---- the filter planes of a point: 24 direct-to-LDS instructions of 8 rows x 128 B, 6 per wave
  const unsigned lds0 = (unsigned)(size_t)(LDS_AS char*)smem;
  // instruction u = 6 wave + t fills plane u >> 3, rows 8 (u & 7) + (lane >> 3): byte u * 1024 + (lane >> 3) * 128 of the point's planes,
  // and the row's swizzle (row >> 1) & 7 = (4 (u & 1) + (lane >> 4)) & 7 depends on the parity of t only
  int u_lane[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) u_lane[t] = (lane >> 3) * (W2_C * 2) + (((lane & 7) ^ ((4 * t + (lane >> 4)) & 7)) * 16);
  auto load_u = [&](int g, int buf) {
    const char* src = (const char*)p.up + g * W2_U_BYTES + wave * 6 * 1024;
#pragma unroll
    for (int t = 0; t < 6; ++t)
      glds16(src + t * 1024 + u_lane[t & 1], __builtin_amdgcn_readfirstlane(lds0 + 2 * W2_V_BYTES + buf * W2_U_BYTES + (wave * 6 + t) * 1024));
  };

  // ---- the wave's block: tiles tb * 32 + .., channels cb * 32 + ..
  const int tb = wave >> 1, cb = wave & 1;
  const int frow = lane & 31, khalf = lane >> 5;
  const int a_row = (tb * 32 + frow) * (W2_C * 4), a_sw = frow & 15;
  const int b_row = (cb * 32 + frow) * (W2_C * 2), b_sw = (frow >> 1) & 7;
  f32x16 s0, s1, o[2][2];

  load_u(0, 0);
#pragma unroll
  for (int r = 0; r < W2_ITEMS; ++r) form_v(0, 0, r, 0);
  wait_vmcnt<0>();
  __syncthreads();

#pragma unroll
  for (int nu = 0; nu < 4; ++nu) {
#pragma unroll
    for (int xi = 0; xi < 4; ++xi) {
      const int buf = xi & 1;
      const int nxi = (xi + 1) & 3, nnu = xi == 3 ? nu + 1 : nu;
      const bool more = xi < 3 || nu < 3;
      if (more) load_u(nxi * 4 + nnu, buf ^ 1);
      if (nu == 0 && xi == 3) load_column(3);            // V of every point of nu = 0 has been formed
      f32x16 acc, acs;
#pragma unroll
      for (int r = 0; r < 16; ++r) { acc[r] = 0.f; acs[r] = 0.f; }
      const char* va = smem + buf * W2_V_BYTES + a_row;
      const char* ub = smem + 2 * W2_V_BYTES + buf * W2_U_BYTES + b_row;
#pragma unroll
      for (int q = 0; q < 4; ++q) {                      // four groups of 16 k, ascending
        bf16x8 ah, am, al;
        const float4 f0 = *(const float4*)(va + (((4 * q + 2 * khalf) ^ a_sw) * 16));
        const float4 f1 = *(const float4*)(va + (((4 * q + 2 * khalf + 1) ^ a_sw) * 16));
        const char* qb = ub + (((2 * q + khalf) ^ b_sw) * 16);
        const bf16x8 bh = __builtin_bit_cast(bf16x8, *(const uint4*)(qb));
        const bf16x8 bm = __builtin_bit_cast(bf16x8, *(const uint4*)(qb + W2_P_BYTES));
        const bf16x8 bl = __builtin_bit_cast(bf16x8, *(const uint4*)(qb + 2 * W2_P_BYTES));
        x3_split8(f0, f1, ah, am, al);
        x3_mma16<6>(ah, am, al, bh, bm, bl, acc, acs);
        if (more) form_v(nxi, nnu, q, buf ^ 1);          // a quarter of the next point's V under each k group
      }
      // A^T over xi, as the products arrive
      f32x16 m;
#pragma unroll
      for (int r = 0; r < 16; ++r) m[r] = x3_combine_plain(acc[r], acs[r]);
      if (xi == 0) s0 = m;
      if (xi == 1) { s0 = s0 + m; s1 = m; }
      if (xi == 2) { s0 = s0 + m; s1 = s1 - m; }
      if (xi == 3) {                                     // ... and over nu
        s1 = s1 - m;
        if (nu == 0) { o[0][0] = s0; o[1][0] = s1; }
        if (nu == 1) { o[0][0] = o[0][0] + s0; o[1][0] = o[1][0] + s1; o[0][1] = s0; o[1][1] = s1; }
        if (nu == 2) { o[0][0] = o[0][0] + s0; o[1][0] = o[1][0] + s1; o[0][1] = o[0][1] - s0; o[1][1] = o[1][1] - s1; }
        if (nu == 3) { o[0][1] = o[0][1] - s0; o[1][1] = o[1][1] - s1; }
      }
      // the sums are only read after the last point: pin them here, or the compiler sinks every fold down there and keeps all 16
      // products alive (in scratch) until then
      asm volatile("" : "+v"(s0));
      if (xi >= 1) asm volatile("" : "+v"(s1));
      if (xi == 3) {
        if (nu < 3) asm volatile("" : "+v"(o[0][0]), "+v"(o[1][0]));
        if (nu > 0) asm volatile("" : "+v"(o[0][1]), "+v"(o[1][1]));
      }
      wait_vmcnt<0>();
      __syncthreads();
    }
  }

  // ---- bias, activation, the tile's 2 x 2 pixels: lane = channel, register r = tile (r & 3) + 8 (r >> 2) + 4 khalf of the block
  const int ch = cb * 32 + frow;
  const float bv = p.bias ? p.bias[ch] : 0.f;
  const bool relu = p.act == FRCNN_ACT_RELU;
  // the block's first tile, then one tile at a time ((img, ty, tx) order): no division per register
  int t = run0 + tb * 32 + 4 * khalf;
  int tx = t % p.TW, ty = (t / p.TW) % p.TH, img = t / (p.TW * p.TH);
  auto next_tile = [&]() {
    ++t; ++tx;
    const bool wx = tx == p.TW;
    tx = wx ? 0 : tx; ty += wx ? 1 : 0;
    const bool wy = ty == p.TH;
    ty = wy ? 0 : ty; img += wy ? 1 : 0;
  };
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    if (r) {
#pragma unroll
      for (int k = 0; k < ((r & 3) ? 1 : 5); ++k) next_tile();
    }
    if (t < p.T) {
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const int oh = 2 * ty + a, ow = 2 * tx + b;
          if (oh >= H || ow >= W) continue;
          float v = o[a][b][r] + bv;
          if (relu) v = act_relu(v);
          p.y[((img * H + oh) * W + ow) * W2_C + ch] = v;
        }
    }
  }
}

}  // namespace

// y = act(conv3x3(x, stride 1, SAME) + bias) for x [N][H][W][64] -> y [N][H][W][64] as Winograd F(2x2,3x3) in one launch;
// u_planes_d = frcnn_gemm_x3_pack(U [16][64][64]) of frcnn_winograd_filter_transform(m = 2).  Bit for bit
// frcnn_winograd_input_transform -> frcnn_gemm_x3 (G = 16, terms = 6) -> frcnn_winograd_output_transform.  No workspace, no state.
extern "C" int frcnn_winograd2_conv_x3(const float* x_d, int N, int H, int W, const void* u_planes_d, const float* bias_d, int act,
                                       float* y_d, void* stream) {
  if (!x_d || !u_planes_d || !y_d || N <= 0 || H <= 0 || W <= 0) return FRCNN_E_ARG;
  if (act != FRCNN_ACT_NONE && act != FRCNN_ACT_RELU) return FRCNN_E_UNSUPPORTED;
  if ((long long)N * H * W * W2_C * 4 >= (1ll << 31)) return FRCNN_E_UNSUPPORTED;        // 32-bit byte offsets
  Wino2Params p;
  p.x = x_d; p.up = (const unsigned short*)u_planes_d; p.bias = bias_d; p.y = y_d;
  p.N = N; p.H = H; p.W = W; p.TH = (H + 1) / 2; p.TW = (W + 1) / 2; p.T = N * p.TH * p.TW; p.act = act;
  static KernelOnce once;
  HIP_TRY(kernel_once(once, (const void*)k_wino2_conv_x3, W2_NT, W2_LDS));
  hipLaunchKernelGGL(k_wino2_conv_x3, dim3((unsigned)cdiv(p.T, W2_RUN)), dim3(W2_NT), W2_LDS, (hipStream_t)stream, p);
  LAUNCH_CHECK();
  return FRCNN_OK;
}

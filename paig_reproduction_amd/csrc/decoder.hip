// Spatial-transformer decoder + compositing + per-frame SSE, forward and
// backward, batched over every decoded frame of a step in one launch.
//
// Reference: PhysicsNet.conv_st_decoder, nn/network/physics_models.py:151-199
// and stn(), nn/network/stn.py:5-16 (aten affine_grid + grid_sample, bilinear,
// zeros padding, align_corners=False), compositing softmax :192-198, loss
// :119-135.  The reference calls the decoder once per rollout step and
// rebuilds every warp grid; here one launch covers all B*T frames.
//
// Per object k the warp is a pure translation: theta = [[1,0,t2],[0,1,t5]],
// t2 = (H/2 - x_k)/h (fp32, as the reference), the grid is formed in fp64 as
// affine_grid does (Q9) and cast to fp32 before grid_sample's unnormalize.
// Sources (template+5, sigmoid(content): [K][.][h][h]) are staged in LDS once
// per block; the background (already sigmoid'ed) is read from global.
//
// Backward recomputes the forward per pixel, forms dL/dout = 2*dsse[f]*(out -
// target) (+ an optional dense dL/dout), and produces
//   * dpos[f][2k+{0,1}] = -(sum_p dix_p * h/2) / h   (grid_sample grid-grad
//     -> affine_grid -> theta -> loc chain), reduced in fp64 per frame;
//   * per-block partial source gradients (template, content, background),
//     gathered (not scattered) from a per-frame pixel-gradient image, so the
//     sum is deterministic; paig_slab_reduce finishes it.
#include "common.h"

#include <stdlib.h>

#include <type_traits>

namespace {

#include "rollout_cells.h"

struct Src {
  const float* tmpl;  // [K][h*h] raw template logits (VariableFromNetwork)
  const float* cont;  // [K][3][h*h] raw content logits
  const float* bg;    // [3][H*W] background, already sigmoid'ed
};

struct PosView {
  const float* p;
  long long outer, inner;
  int grp;
  // the attention-window scale sigma (physics_models.py:160-162): theta0 =
  // theta4 = sg in fp64, and sgf = fl32(sigma), the scalar of the fp32
  // products theta2, theta5 (:166-167)
  double sg;
  float sgf;
  // a device-resident sigma (the learnable scale: the host does not know it),
  // or null: sg / sgf above hold.  Kernels call load() once at entry.
  const double* sgp = nullptr;
  __device__ __forceinline__ void load() {
    if (sgp) {   // uniform: one scalar load
      sg = *sgp;
      sgf = (float)sg;
    }
  }
  // theta2 / theta5 of an object at l on one axis: fp32 as the reference
  // forms it, widened for the fp64 grid (Q9)
  __device__ __forceinline__ double theta_t(float l, int H, int h) const {
    return (double)((((float)H / 2.f - l) / (float)h) * sgf);
  }
  __device__ __forceinline__ const float* at(int f) const {
    return grp > 0 ? p + (long long)(f / grp) * outer + (long long)(f % grp) * inner : p + (long long)f * inner;
  }
};

// affine_grid base coordinate: linspace(-1, 1, n)[j] * (n - 1) / n  in fp64
__device__ __forceinline__ double base_coord(int j, int n) {
  const double step = 2.0 / (double)(n - 1);
  const double v = (j < n / 2) ? -1.0 + step * (double)j : 1.0 - step * (double)(n - 1 - j);
  return v * (double)(n - 1) / (double)n;
}

// grid_sample unnormalized source coordinate for output index j, from the
// block's table of base coordinates bc[j] = base_coord(j, n)
__device__ __forceinline__ float src_coord(double bcj, double t, int h, double sg) {
  const float g = (float)(sg * bcj + t);
  return ((g + 1.f) * (float)h - 1.f) / 2.f;
}

struct Bil {
  int x0, y0;
  float fx, fy;  // ix - x0, iy - y0
};

__device__ __forceinline__ Bil bil(float ix, float iy) {
  Bil b;
  const float fx0 = floorf(ix), fy0 = floorf(iy);
  b.x0 = (int)fx0;
  b.y0 = (int)fy0;
  b.fx = ix - fx0;
  b.fy = iy - fy0;
  return b;
}

__device__ __forceinline__ float tap(const float* s, int h, int y, int x) {
  return (x >= 0 && x < h && y >= 0 && y < h) ? s[y * h + x] : 0.f;
}

// value and d/dix, d/diy of the bilinear sample of source s (h x h, zero padded)
__device__ __forceinline__ void sample(const float* s, int h, const Bil& b, float& v, float& dx, float& dy) {
  const float nw = tap(s, h, b.y0, b.x0), ne = tap(s, h, b.y0, b.x0 + 1);
  const float sw = tap(s, h, b.y0 + 1, b.x0), se = tap(s, h, b.y0 + 1, b.x0 + 1);
  const float ex = 1.f - b.fx, ey = 1.f - b.fy;
  v = nw * ex * ey + ne * b.fx * ey + sw * ex * b.fy + se * b.fx * b.fy;
  dx = (ne - nw) * ey + (se - sw) * b.fy;
  dy = (sw - nw) * ex + (se - ne) * b.fx;
}

// Per-frame sampling coordinate tables: cx[k][j] = ix of output column j,
// cy[k][i] = iy of output row i (the warp is separable).  fp64 grid math once
// per (frame, object, row/col) instead of per pixel.  Caller syncs.
constexpr int MAXH = 64;
template <int K>
__device__ __forceinline__ void coord_tables(const PosView& pos, int f, int H, int h, float (*cx)[MAXH],
                                             float (*cy)[MAXH], const double* bc) {
  const float* pf = pos.at(f);
  for (int t = threadIdx.x; t < K * 2 * H; t += blockDim.x) {
    const int k = t / (2 * H), r = t % (2 * H);
    const float l = r < H ? pf[2 * k] : pf[2 * k + 1];
    const double tt = pos.theta_t(l, H, h);
    if (r < H) cx[k][r] = src_coord(bc[r], tt, h, pos.sg);
    else cy[k][r - H] = src_coord(bc[r - H], tt, h, pos.sg);
  }
}

// the fp64 affine_grid base coordinates (frame-invariant): computed once per
// block; the kernels' first in-loop barrier orders them before use
__device__ __forceinline__ void init_base(double* bc, int H) {
  for (int j = threadIdx.x; j < H; j += blockDim.x) bc[j] = base_coord(j, H);
}

template <int K>
__device__ __forceinline__ void stage_sources(const Src& S, int h, float* T, float* Cn) {
  const int hh = h * h;
  for (int i = threadIdx.x; i < K * hh; i += blockDim.x) T[i] = S.tmpl[i] + 5.f;
  for (int i = threadIdx.x; i < K * 3 * hh; i += blockDim.x) Cn[i] = 1.f / (1.f + expf(-S.cont[i]));
}

// forward composite of one pixel; returns out[3], masks m[K+1], samples
template <int K>
__device__ __forceinline__ void composite(const float* T, const float* Cn, const float* bg, int HW, int p, int h,
                                          const Bil* bl, float* out, float* m, float (*cs)[3]) {
  const int hh = h * h;
  float lg[K + 1];
  float mx = 1.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    float v, dx, dy;
    sample(T + k * hh, h, bl[k], v, dx, dy);
    lg[k] = v - 5.f;
    mx = fmaxf(mx, lg[k]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      sample(Cn + (k * 3 + c) * hh, h, bl[k], v, dx, dy);
      cs[k][c] = v;
    }
  }
  lg[K] = 1.f;
  float s = 0.f;
#pragma unroll
  for (int k = 0; k <= K; ++k) {
    m[k] = __expf(lg[k] - mx);   // v_exp_f32: ~1e-7 relative, far inside the 1e-4 bar
    s += m[k];
  }
  const float rs = __builtin_amdgcn_rcpf(s);
#pragma unroll
  for (int k = 0; k <= K; ++k) m[k] = m[k] * rs;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float o = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) o += m[k] * cs[k][c];
    out[c] = o + m[K] * bg[c * HW + p];
  }
}

template <int K>
__global__ void __launch_bounds__(256)
dec_fwd_k(PosView pos, Src S, FViewW out, FView tgt, float* __restrict__ sse, int F, int h, int H) {
  pos.load();
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int hh = h * h, HW = H * H;
  float* T = lds;
  float* Cn = T + K * hh;
  __shared__ float red[4];
  __shared__ float cx[K][MAXH], cy[K][MAXH];
  __shared__ double bc[MAXH];
  init_base(bc, H);
  stage_sources<K>(S, h, T, Cn);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int f = blockIdx.x; f < F; f += gridDim.x) {
    __syncthreads();   // previous frame done with the tables
    coord_tables<K>(pos, f, H, h, cx, cy, bc);
    __syncthreads();
    float* of = out.frame(f);
    const float* tf = sse ? tgt.frame(f) : nullptr;
    float acc = 0.f;
    for (int p = threadIdx.x; p < HW; p += blockDim.x) {
      const int i = p / H, j = p % H;
      Bil bl[K];
#pragma unroll
      for (int k = 0; k < K; ++k) bl[k] = bil(cx[k][j], cy[k][i]);
      float o[3], m[K + 1], cs[K][3];
      composite<K>(T, Cn, S.bg, HW, p, h, bl, o, m, cs);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        of[c * HW + p] = o[c];
        if (tf) {
          const float d = tf[c * HW + p] - o[c];
          acc = fmaf(d, d, acc);
        }
      }
    }
    if (sse) {
      acc = wave_sum(acc);
      if (lane == 0) red[wv] = acc;
      __syncthreads();
      if (threadIdx.x == 0) {
        float s = 0.f;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w];
        sse[f] = s;
      }
      __syncthreads();
    }
  }
}

// (the generic backward, dec_bwd_k, follows the target / loss-weight views below)

// ---------------------------------------------------------------------------
// Register-resident forward for the small frames of the headline workloads
// ((K, H) = (2, 32) spring/bouncing, (3, 36) 3bp).  Every
// thread owns the same PPT pixels and SPT source texels in every frame, so
//   * the background values it composites are loaded once per block,
//   * its background / template / content gradients accumulate in registers
//     and are written to the slab row once at the end (no per-frame global
//     read-modify-write),
//   * the next frame's target pixels are prefetched behind the current frame,
//   * the bilinear tap weights (and their d/dix, d/diy) are formed once per
//     (pixel, object) and shared by the template and the 3 content planes,
// The backward of these shapes is dec_bwd_cu_k below; the generic kernels
// above remain for the large (mnist 64x64) frames.
struct Taps {
  int o[4];      // offsets of nw, ne, sw, se in an h x h plane (0 when out of range)
  float w[4];    // bilinear weights (0 for out-of-range taps: zero padding)
  float wx[4];   // d weight / d ix
  float wy[4];   // d weight / d iy
};

__device__ __forceinline__ Taps make_taps(const Bil& b, int h) {
  Taps t;
  const bool x0 = b.x0 >= 0 && b.x0 < h, x1 = b.x0 + 1 >= 0 && b.x0 + 1 < h;
  const bool y0 = b.y0 >= 0 && b.y0 < h, y1 = b.y0 + 1 >= 0 && b.y0 + 1 < h;
  const bool v[4] = {x0 && y0, x1 && y0, x0 && y1, x1 && y1};
  const int xs[4] = {b.x0, b.x0 + 1, b.x0, b.x0 + 1}, ys[4] = {b.y0, b.y0, b.y0 + 1, b.y0 + 1};
  const float ex = 1.f - b.fx, ey = 1.f - b.fy;
  const float w[4] = {ex * ey, b.fx * ey, ex * b.fy, b.fx * b.fy};
  const float wx[4] = {-ey, ey, -b.fy, b.fy};
  const float wy[4] = {-ex, -b.fx, ex, b.fx};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    t.o[q] = v[q] ? ys[q] * h + xs[q] : 0;
    t.w[q] = v[q] ? w[q] : 0.f;
    t.wx[q] = v[q] ? wx[q] : 0.f;
    t.wy[q] = v[q] ? wy[q] : 0.f;
  }
  return t;
}

// template (plane 0) and content (planes 1..3) of object k at one pixel:
// values, and (BWD) their d/dix, d/diy
template <bool BWD>
__device__ __forceinline__ void sample4(const float* Tk, const float* Ck, int hh, const Taps& t, float* v, float* dx,
                                        float* dy) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float* s = c == 0 ? Tk : Ck + (c - 1) * hh;
    float a = 0.f, gx = 0.f, gy = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float x = s[t.o[q]];
      a = fmaf(x, t.w[q], a);
      if (BWD) {
        gx = fmaf(x, t.wx[q], gx);
        gy = fmaf(x, t.wy[q], gy);
      }
    }
    v[c] = a;
    if (BWD) {
      dx[c] = gx;
      dy[c] = gy;
    }
  }
}

// softmax compositing of K objects + background from sampled planes sv[k][0..3]
template <int K>
__device__ __forceinline__ void blend(const float (*sv)[4], const float* bgv, float* out, float* m) {
  float lg[K + 1];
  float mx = 1.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    lg[k] = sv[k][0] - 5.f;
    mx = fmaxf(mx, lg[k]);
  }
  lg[K] = 1.f;
  float s = 0.f;
#pragma unroll
  for (int k = 0; k <= K; ++k) {
    m[k] = __expf(lg[k] - mx);   // v_exp_f32: ~1e-7 relative, far inside the 1e-4 bar
    s += m[k];
  }
  const float rs = __builtin_amdgcn_rcpf(s);
#pragma unroll
  for (int k = 0; k <= K; ++k) m[k] = m[k] * rs;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float o = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) o += m[k] * sv[k][1 + c];
    out[c] = o + m[K] * bgv[c];
  }
}

template <int K, int H>
__global__ void __launch_bounds__(256)
dec_fwd_reg_k(PosView pos, Src S, FViewW out, FView tgt, float* __restrict__ sse, int F) {
  pos.load();
  constexpr int h = H / 2, hh = h * h, HW = H * H, PPT = (HW + 255) / 256;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* T = lds;
  float* Cn = T + K * hh;
  __shared__ float red[4];
  __shared__ float cx[K][MAXH], cy[K][MAXH];
  __shared__ double bc[MAXH];
  init_base(bc, H);
  stage_sources<K>(S, h, T, Cn);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float bgv[PPT][3], tn[PPT][3];
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int p = tid + 256 * j;
#pragma unroll
    for (int c = 0; c < 3; ++c) bgv[j][c] = (p < HW) ? S.bg[c * HW + p] : 0.f;
  }
  auto fetch = [&](int f) {
    const float* tf = tgt.frame(f);
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      const int p = tid + 256 * j;
#pragma unroll
      for (int c = 0; c < 3; ++c) tn[j][c] = (p < HW) ? tf[c * HW + p] : 0.f;
    }
  };
  if (sse && (int)blockIdx.x < F) fetch(blockIdx.x);
  for (int f = blockIdx.x; f < F; f += gridDim.x) {
    __syncthreads();   // previous frame done with the tables
    coord_tables<K>(pos, f, H, h, cx, cy, bc);
    __syncthreads();
    float tc[PPT][3];
#pragma unroll
    for (int j = 0; j < PPT; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) tc[j][c] = tn[j][c];
    if (sse && f + (int)gridDim.x < F) fetch(f + gridDim.x);
    float* of = out.frame(f);
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      const int p = tid + 256 * j;
      if (p >= HW) break;
      const int i = p / H, jj = p % H;
      float sv[K][4], o[3], m[K + 1];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const Taps t = make_taps(bil(cx[k][jj], cy[k][i]), h);
        sample4<false>(T + k * hh, Cn + k * 3 * hh, hh, t, sv[k], nullptr, nullptr);
      }
      blend<K>(sv, bgv[j], o, m);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        of[c * HW + p] = o[c];
        const float d = tc[j][c] - o[c];
        acc = fmaf(d, d, acc);
      }
    }
    if (sse) {
      acc = wave_sum(acc);
      if (lane == 0) red[wv] = acc;
      __syncthreads();
      if (tid == 0) sse[f] = (red[0] + red[1]) + (red[2] + red[3]);
    }
  }
}

// Per-frame gather table entry of the backward: for source column (row) s of
// an object at position l on that axis, the first output index j0 of a
// 5-wide window of output columns (rows) and their bilinear weights on s
// (nonzero where floor(c[j]) == s: 1 - frac, or floor(c[j]) + 1 == s: frac;
// c[j] = the sample coordinate of output index j, as coord_tables() forms
// it from the fp64 base coordinates bc[]).  The warp's slope is sigma / 2
// source texels per output index, so at most 4 / sigma output indices
// contribute (one more with rounding at both ends): 5 for sigma >= 1, the
// range these tables serve (sigma < 1 takes the generic backward, whose
// window is sized per launch).  The coordinates are evaluated directly (no
// scan over a coordinate table): c is j sigma/2 + c[0] up to fp32 rounding
// (~1e-6), so the first j with floor(c[j]) >= s-1 is one of three candidates
// around that estimate.
constexpr int GW = 5;
__device__ __forceinline__ void gather_entry(const PosView& pos, float l, const double* bc, int H, int h, int s,
                                             int* j0, float* wt) {
  const double tt = pos.theta_t(l, H, h), sg = pos.sg;
  const float c0 = src_coord(bc[0], tt, h, sg);
  // the coordinate slope is sigma / 2 per output index
  const int je = (int)ceilf((2.f / pos.sgf) * ((float)s - 1.f - c0)) - 1;
  int j = je;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int jj = je + i;
    const float c = jj < 0 ? -1e30f : (jj >= H ? 1e30f : src_coord(bc[jj], tt, h, sg));
    if (floorf(c) < (float)(s - 1)) j = jj + 1;
  }
  // the window stays inside [0, H): indices before the first contributor get
  // their (zero) weights like any other, so no gather needs an index clamp
  if (j < 0) j = 0;
  if (j > H - GW) j = H - GW;
  *j0 = j;
#pragma unroll
  for (int b = 0; b < GW; ++b) {
    const float v = src_coord(bc[j + b], tt, h, sg), f0 = floorf(v);
    const int x0 = (int)f0;
    const float fr = v - f0;
    wt[b] = (x0 == s ? 1.f - fr : 0.f) + (x0 + 1 == s ? fr : 0.f);
  }
}

// ---------------------------------------------------------------------------
// Decoder backward, one CU per block (1024 / 768 threads), the headline
// shapes ((K, H) = (2, 32) spring/bouncing, (3, 36) 3bp).
//
// Work list: the LIVE frames only.  Frames are grouped in sequences of R
// (= pos.grp; the rollout decode) of which the first Rl carry a loss weight
// (the reference trains on loss[:, :pred_steps] only, physics_models.py:
// 129-139): compact frame n -> f = (n / Rl) * R + n % Rl.  The dead frames'
// position gradients are zeroed by a grid-stride pass; nothing else of theirs
// is read.  Each block walks a contiguous run of >= DEC_FPB_MIN live frames,
// so the partial source-gradient slab (one row per block) stays a fraction
// of the target bytes.
//
// Per frame, one thread per output pixel (H = 36: a second pixel slot for
// 528 of the 768):
//   pass 1: sample the K objects' template + 3 content planes (value and
//     d/dix, d/diy from one padded float4 texel image: 4 ds_read_b128 per
//     object), composite, dL/dout = 2 dsse[f] (out - target) (+ dense dout);
//     background grads accumulate in registers (the thread's pixels are
//     fixed), the per-object pixel gradients (dT, dC0..2) go to an LDS image
//     G, the position-gradient sums to a per-wave fp64 reduction (Q9);
//   pass 2: every source texel gathers its <= 5 x 5 contributing pixels from
//     G through per-frame separable weight tables (no atomics: a fixed
//     order); for K = 2 an item is a texel's plane pair, so all 1024 threads
//     take one.
// Frames are software-pipelined over ONE barrier each: iteration it forms
// the axis and gather tables of frame it+1, runs pass 2 of frame it-1 and
// pass 1 of frame it (double / triple buffers for G, the fp64 partials and
// the tables).  The position gradients reduce as fp64 DPP row
// sums per wave, finished by one wave each in the next iteration.  Every global load of frame it+1 (its
// positions, its loss weight, its targets) is issued one iteration ahead,
// so no wave waits on memory inside the loop.
constexpr int DEC_FPB_MIN = 3, DEC_CU_MAX_BLOCKS = 256;   // 3: 200 blocks for the 600 live rollout frames (16.5 -> 13.4 us; 4: 150)

template <int K, int H>
struct DecCu {
  // threads per block: 16 waves (4 per SIMD, <= 128 VGPRs); 12 for K = 3,
  // whose per-pixel state needs more registers (<= 168 VGPRs) and whose
  // 1296 pixels then fall into 768 + 528 slots
  static constexpr int NT = K >= 3 ? 768 : 1024, NW = NT / 64;
  static constexpr int h = H / 2, hp = h + 2, hh = h * h, HW = H * H;
  static constexpr int PS = (HW + NT - 1) / NT;          // pixel slots per thread
  static constexpr int PL = K == 2 ? 2 : 4;              // planes per pass-2 item
  static constexpr int NI = K * hh * (4 / PL);           // pass-2 items
  static constexpr int NIT = (NI + NT - 1) / NT;         // pass-2 items per thread
  // G (per-pixel dT, dC0 | dC1, dC2) as two float2 images, each row laid out
  // even columns first, then odd ones: a pass-2 half-wave reads 16 texels'
  // pixels 2 apart = 16 consecutive float2s; the row pitch (float2s, = 8
  // mod 16 where LDS allows) puts the next texel row's reads on the other
  // 128 B of the banks
  static constexpr int GPITCH = K == 2 ? H + 8 : H;
  static constexpr int NC = K * 2 * H, NG = K * 2 * h;   // axis / gather table entries
  // their threads: the waves right after the 2K that finish the position
  // gradients (old waves: the scheduler favours them, so the extra work
  // does not become the barrier's tail)
  static constexpr int TC0 = 64 * 2 * K, TG0 = TC0 + NC;
  static_assert(TG0 + NG <= NT, "tables need more threads");
  // fp64 partials per position gradient: the 4 row sums of every wave, or
  // (K = 3, LDS budget) the 2 half-wave sums
  static constexpr int RPW = K >= 3 ? 2 : 4, NR = NW * RPW;
  // the two passes in alternating order by wave half (the K = 3 state does
  // not fit the registers twice)
  static constexpr bool ALT = K == 2;
  static_assert(NR <= 64, "one wave finishes a position gradient");
};

// slot of output column j in a G row (even columns first)
template <int H>
__device__ __forceinline__ int gslot(int j) { return (j & 1) * (H / 2) + (j >> 1); }

// Compact live frame -> real frame and its position / target addresses,
// advanced incrementally (no per-frame integer divisions).  Grouped mode
// (the rollout decode): positions and targets are both grouped by R, the
// first Rl steps of each sequence live.  Otherwise frame n = n, each view
// keeping its own (group, step) counter.
struct DecCursor {
  int f, pq, pr, tq, tr;
};
// The decoders' targets: fp32 frames (p), or the uint8 dataset rows the batch
// was gathered from (p8: the device-resident dataset's NHWC bytes, in the flat
// order Q5's reshape keeps, so element offsets are the fp32 view's; ix: the
// batch's dataset row per sequence, as paig_gather_u8_f32_ex saved it, or null
// for sequence q at q * fs).  A byte target is byte / 255 exactly as the
// gather forms it (div255): bit-identical losses and gradients from a quarter
// of the bytes, and the gather need not write the frames only the decoders
// read.  Uniform per launch.
struct TView {
  const float* p;
  const unsigned char* p8;
  const long long* ix;
  long long fs, gs;
  int grp;
  // T8 (a template parameter of the kernels that read targets): p8, else p.
  // raw*: the value as loaded (T8: the byte / the 4-byte word in the float's
  // bits), no arithmetic on it, so a prefetched target's load stays in flight
  // until val* converts it where it is used
  template <bool T8>
  __device__ __forceinline__ float raw1(long long o) const {
    if constexpr (T8) return __int_as_float((int)p8[o]);
    else return p[o];
  }
  template <bool T8>
  __device__ __forceinline__ static float val1(float r) {
    if constexpr (T8) return div255((float)__float_as_int(r));
    else return r;
  }
  template <bool T8>
  __device__ __forceinline__ float4 raw4(long long o) const {
    if constexpr (T8) return make_float4(__int_as_float(*reinterpret_cast<const int*>(p8 + o)), 0.f, 0.f, 0.f);
    else return *reinterpret_cast<const float4*>(p + o);
  }
  template <bool T8>
  __device__ __forceinline__ static void val4(float4 r, float* v) {
    if constexpr (T8) {
      const unsigned w = (unsigned)__float_as_int(r.x);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = div255((float)((w >> (8 * e)) & 255u));
    } else {
      v[0] = r.x, v[1] = r.y, v[2] = r.z, v[3] = r.w;
    }
  }
};
// A backward's per-frame loss weights: the array dsse (a), or (mode 1 / 2)
// formed in-kernel from the loss adjoints (loss_weight, common.h), so the
// step needs no paig_loss_bwd launch.  Uniform per launch.
struct WSrc {
  const float* a;
  const float* dt;
  const float* de;
  const float* dr;
  float ae;
  int B, Te, R, pred, mode;
  float w0, w1;   // (prep) the two weights a mode-1 / 2 launch can have
  // LW (a template parameter of the kernels: mode != 0) -- one form per
  // instantiation, so the array form keeps its registers
  __host__ __device__ __forceinline__ bool on() const { return a != nullptr || mode != 0; }
  // once per block: the pred-step (or reconstruction) weight and the
  // extrapolation-step one, as loss_weight forms them per frame
  template <bool LW>
  __device__ __forceinline__ void prep() {
    if constexpr (LW) {
      w0 = loss_weight(mode, 0, dt, de, dr, ae, B, Te, R, pred);
      w1 = mode == 2 && pred < R ? loss_weight(2, pred, dt, de, dr, ae, B, Te, R, pred) : w0;
    }
  }
  template <bool LW>
  __device__ __forceinline__ bool has() const {
    if constexpr (LW) return true;
    else return a != nullptr;
  }
  // frame c: a[c.f], or by its step c.pr (mode 2: frames grouped by R)
  template <bool LW>
  __device__ __forceinline__ float at(const DecCursor& c) const {
    if constexpr (LW) return mode == 2 && c.pr >= pred ? w1 : w0;
    else return a[c.f];
  }
};
struct DecFrames {
  PosView pos;
  TView tgt;
  int R, Rl;
  bool grouped;
  __device__ DecFrames(PosView p, TView t, int rl) : pos(p), tgt(t), R(p.grp), Rl(rl) {
    grouped = R > 0 && Rl > 0 && Rl < R;
  }
  __device__ int live(int F) const { return grouped ? (F / R) * Rl : F; }
  __device__ DecCursor at(int n) const {
    DecCursor c;
    if (grouped) {
      c.pq = c.tq = n / Rl;
      c.pr = c.tr = n % Rl;
      c.f = c.pq * R + c.pr;
    } else {
      c.f = n;
      c.pq = pos.grp > 0 ? n / pos.grp : 0;
      c.pr = pos.grp > 0 ? n % pos.grp : 0;
      c.tq = tgt.grp > 0 ? n / tgt.grp : 0;
      c.tr = tgt.grp > 0 ? n % tgt.grp : 0;
    }
    return c;
  }
  __device__ DecCursor next(DecCursor c) const {
    if (grouped) {
      if (++c.pr == Rl) {
        c.pr = 0;
        ++c.pq;
      }
      c.tq = c.pq;
      c.tr = c.pr;
      c.f = c.pq * R + c.pr;
    } else {
      ++c.f;
      if (pos.grp > 0 && ++c.pr == pos.grp) {
        c.pr = 0;
        ++c.pq;
      }
      if (tgt.grp > 0 && ++c.tr == tgt.grp) {
        c.tr = 0;
        ++c.tq;
      }
    }
    return c;
  }
  __device__ const float* pos_of(const DecCursor& c) const {
    return pos.grp > 0 ? pos.p + (long long)c.pq * pos.outer + (long long)c.pr * pos.inner
                       : pos.p + (long long)c.f * pos.inner;
  }
  // Row indices of the block's target sequences (T8 with tgt.ix): frames
  // first .. first+nf-1 span sequences q0 .. (the first IXN of them staged).
  // ix_load at the top of a kernel puts this thread's entry and the first
  // frame's row in flight across the prologue; ix_store, before the
  // prologue's barrier, publishes the entries in LDS, where tgt_off reads
  // them: no frame's target loads wait on a dependent global load.
  static constexpr int IXN = 32;
  struct IxStage {
    int q0 = 0, span = 0;
    long long mine = 0, row0 = 0;
  };
  template <bool T8>
  __device__ IxStage ix_load(int first, int nf, int tid) const {
    IxStage st;
    if (!T8 || !tgt.ix || nf <= 0 || tgt.grp <= 0) return st;
    st.q0 = at(first).tq;
    st.span = at(first + nf - 1).tq - st.q0 + 1;
    if (tid < st.span && tid < IXN) st.mine = tgt.ix[st.q0 + tid];
    st.row0 = tgt.ix[st.q0];
    return st;
  }
  __device__ void ix_store(const IxStage& st, long long* ixs, int tid) const {
    if (tid < st.span && tid < IXN) ixs[tid] = st.mine;
  }
  // the first frame's target offset from the row ix_load fetched
  template <bool T8>
  __device__ long long tgt_off0(const DecCursor& c, const IxStage& st) const {
    if (T8 && tgt.ix && tgt.grp > 0) return st.row0 * tgt.fs + (long long)c.tr * tgt.gs;
    return tgt_off<T8>(c);
  }
  // element offset of the target frame (of p or p8); ixs: the staged row
  // indices (null before the barrier that publishes them)
  template <bool T8>
  __device__ long long tgt_off(const DecCursor& c, const long long* ixs = nullptr, int q0 = 0) const {
    if (tgt.grp <= 0) return (long long)c.f * tgt.fs;
    long long q = c.tq;
    if (T8 && tgt.ix) q = ixs && c.tq - q0 < IXN ? ixs[c.tq - q0] : tgt.ix[c.tq];
    return q * tgt.fs + (long long)c.tr * tgt.gs;
  }
};

// The generic backward (any H = 2h <= MAXH; the gather window of pass 2 is
// sized from the launch's sigma, so it also serves the one-CU shapes at
// sigma < 1, whose window is wider than the one-CU kernels' 5-wide tables).
// Every frame is walked: the dead ones (step >= live of a group, or a zero
// weight and no dense gradient) get zero position gradients and are not read.
// Targets (T8) and loss weights (LW) as in the one-CU kernels.
// slab row layout per block: [K*h*h template | K*3*h*h content | 3*H*W bg]
//
// dsig (nullable; the learnable scale, physics_models.py:155-161): dL/dsigma
// of every frame.  ix_j = ((g_j + 1) h - 1) / 2 with g_j = sigma bc[j] + t_x,
// t_x = fl32(((H/2 - x_k) / h) fl32(sigma)), so d ix_j / d sigma = (h / 2)
// (bc[j] + (H/2 - x_k) / h): the pixel gradients gx, gy that feed sx, sy,
// weighted by the base coordinate, in two more fp64 sums per object, reduced
// with them; skipped frames get 0.
template <int K, bool T8, bool LW>
__global__ void __launch_bounds__(256)
dec_bwd_k(PosView pos, Src S, TView tgt, WSrc dsse, FView dout, float* __restrict__ dpos,
          float* __restrict__ slab, float* __restrict__ gscratch, double* __restrict__ dsig, int F, int live, int h,
          int H) {
  pos.load();
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int hh = h * h, HW = H * H;
  float* T = lds;
  float* Cn = T + K * hh;
  float* G = gscratch ? gscratch + (long long)blockIdx.x * K * 4 * HW : Cn + K * 3 * hh;  // [K][4][HW]
  __shared__ double redd[4][4 * K];   // sx, sy per object | (dsig) their bc-weighted sums
  __shared__ int skip_s;
  __shared__ float cx[K][MAXH], cy[K][MAXH];
  __shared__ double bc[MAXH];
  init_base(bc, H);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nw = blockDim.x >> 6;
  const long long slab_len = (long long)K * hh + (long long)K * 3 * hh + 3LL * HW;
  float* srow = slab + (long long)blockIdx.x * slab_len;
  float* s_tm = srow;
  float* s_ct = srow + K * hh;
  float* s_bg = s_ct + K * 3 * hh;
  // zero this block's slab row (each element is owned by exactly one thread below)
  for (int s = threadIdx.x; s < K * hh; s += blockDim.x) {
    s_tm[s] = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) s_ct[(s / hh * 3 + c) * hh + s % hh] = 0.f;
  }
  for (int p = threadIdx.x; p < HW; p += blockDim.x)
#pragma unroll
    for (int c = 0; c < 3; ++c) s_bg[c * HW + p] = 0.f;
  stage_sources<K>(S, h, T, Cn);
  const DecFrames FR(pos, tgt, 0);
  const bool has_w = dsse.template has<LW>();
  dsse.template prep<LW>();
  __syncthreads();

  for (int f = blockIdx.x; f < F; f += gridDim.x) {
    const DecCursor cur = FR.at(f);
    const bool dead = live > 0 && cur.pr >= live;
    const float w_f = has_w && !dead ? 2.f * dsse.template at<LW>(cur) : 0.f;
    const float* dof = dout.p ? dout.frame(f) : nullptr;
    if (threadIdx.x == 0) skip_s = (w_f == 0.f && dof == nullptr);
    __syncthreads();
    if (skip_s) {
      if (threadIdx.x < 2 * K) dpos[(long long)f * 2 * K + threadIdx.x] = 0.f;
      if (dsig && threadIdx.x == 64) dsig[f] = 0.0;
      __syncthreads();
      continue;
    }
    coord_tables<K>(pos, f, H, h, cx, cy, bc);
    __syncthreads();
    const long long to = has_w ? FR.template tgt_off<T8>(cur) : 0;
    double sx[K], sy[K], bx[K], by[K];
#pragma unroll
    for (int k = 0; k < K; ++k) sx[k] = sy[k] = bx[k] = by[k] = 0.0;

    // ---- pass 1: per-pixel gradients
    for (int p = threadIdx.x; p < HW; p += blockDim.x) {
      const int i = p / H, j = p % H;
      Bil bl[K];
#pragma unroll
      for (int k = 0; k < K; ++k) bl[k] = bil(cx[k][j], cy[k][i]);
      float o[3], m[K + 1], cs[K][3];
      composite<K>(T, Cn, S.bg, HW, p, h, bl, o, m, cs);
      float g[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float tv = has_w ? TView::val1<T8>(tgt.template raw1<T8>(to + c * HW + p)) : 0.f;
        g[c] = w_f * (o[c] - tv);
        if (dof) g[c] += dof[c * HW + p];
        s_bg[c * HW + p] += m[K] * g[c];
      }
#pragma unroll
      for (int k = 0; k < K; ++k) {
        float dT = 0.f;
        float dC[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          dC[c] = m[k] * g[c];
          dT = fmaf(g[c], cs[k][c] - o[c], dT);
        }
        dT *= m[k];
        G[(k * 4 + 0) * HW + p] = dT;
        float v, dx, dy;
        sample(T + k * hh, h, bl[k], v, dx, dy);
        float gx = dT * dx, gy = dT * dy;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          G[(k * 4 + 1 + c) * HW + p] = dC[c];
          sample(Cn + (k * 3 + c) * hh, h, bl[k], v, dx, dy);
          gx = fmaf(dC[c], dx, gx);
          gy = fmaf(dC[c], dy, gy);
        }
        sx[k] += (double)gx;
        sy[k] += (double)gy;
        if (dsig) {
          bx[k] += (double)gx * bc[j];
          by[k] += (double)gy * bc[i];
        }
      }
    }
    // ---- per-frame dpos (and dsigma) reduction (fp64)
#pragma unroll
    for (int k = 0; k < K; ++k) {
      double a = wave_sum_d(sx[k]), b = wave_sum_d(sy[k]);
      if (lane == 0) {
        redd[wv][2 * k] = a;
        redd[wv][2 * k + 1] = b;
      }
      if (dsig) {
        a = wave_sum_d(bx[k]), b = wave_sum_d(by[k]);
        if (lane == 0) {
          redd[wv][2 * K + 2 * k] = a;
          redd[wv][2 * K + 2 * k + 1] = b;
        }
      }
    }
    __syncthreads();
    if (threadIdx.x < 2 * K) {
      double s = 0.0;
      for (int w = 0; w < nw; ++w) s += redd[w][threadIdx.x];
      // d theta = sum_p dgrid = sum_p dix * h/2 ; dloc = -(dtheta * sigma) / h
      const float dth = (float)(s * (double)h * 0.5);
      dpos[(long long)f * 2 * K + threadIdx.x] = -(dth * pos.sgf) / (float)h;
    }
    if (dsig && threadIdx.x == 64) {   // (a wave of its own: beside the position gradients')
      const float* pf = pos.at(f);
      double tot = 0.0;
      for (int k = 0; k < K; ++k) {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        for (int w = 0; w < nw; ++w) {
          s[0] += redd[w][2 * k];
          s[1] += redd[w][2 * k + 1];
          s[2] += redd[w][2 * K + 2 * k];
          s[3] += redd[w][2 * K + 2 * k + 1];
        }
        // d t / d sigma of the two axes: theta_t's fp32 quotient, widened
        const double ax = (double)(((float)H / 2.f - pf[2 * k]) / (float)h);
        const double ay = (double)(((float)H / 2.f - pf[2 * k + 1]) / (float)h);
        tot += (s[2] + s[3]) + (ax * s[0] + ay * s[1]);
      }
      dsig[f] = tot * ((double)h * 0.5);
    }
    // ---- pass 2: gather source gradients from the pixel-gradient image
    for (int s = threadIdx.x; s < K * hh; s += blockDim.x) {
      const int k = s / hh, q = s % hh, ys = q / h, xs = q % h;
      // output index j has ix(j) ~= a + j*sigma*h/H; candidates with floor(ix) in {xs-1, xs}
      const float a0x = cx[k][0], a0y = cy[k][0];
      const float slope = (float)h / (float)H * pos.sgf;
      int jlo = (int)floorf(((float)xs - 1.f - a0x) / slope) - 1, jhi = (int)ceilf(((float)xs + 1.f - a0x) / slope) + 1;
      int ilo = (int)floorf(((float)ys - 1.f - a0y) / slope) - 1, ihi = (int)ceilf(((float)ys + 1.f - a0y) / slope) + 1;
      if (jlo < 0) jlo = 0;
      if (ilo < 0) ilo = 0;
      if (jhi > H - 1) jhi = H - 1;
      if (ihi > H - 1) ihi = H - 1;
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      for (int i = ilo; i <= ihi; ++i) {
        const float iy = cy[k][i];
        const float fy0 = floorf(iy);
        const int y0 = (int)fy0;
        const float fy = iy - fy0;
        const float wy = (y0 == ys ? 1.f - fy : 0.f) + (y0 + 1 == ys ? fy : 0.f);
        if (wy == 0.f) continue;
        float row[4] = {0.f, 0.f, 0.f, 0.f};
        for (int j = jlo; j <= jhi; ++j) {
          const float ix = cx[k][j];
          const float fx0 = floorf(ix);
          const int x0 = (int)fx0;
          const float fx = ix - fx0;
          const float wx = (x0 == xs ? 1.f - fx : 0.f) + (x0 + 1 == xs ? fx : 0.f);
          if (wx == 0.f) continue;
#pragma unroll
          for (int c = 0; c < 4; ++c) row[c] = fmaf(wx, G[(k * 4 + c) * HW + i * H + j], row[c]);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = fmaf(wy, row[c], acc[c]);
      }
      s_tm[s] += acc[0];
#pragma unroll
      for (int c = 0; c < 3; ++c) s_ct[(k * 3 + c) * hh + q] += acc[1 + c];
    }
    __syncthreads();
  }
}

// separable bilinear setup of one axis: tap index (padded source), masked
// weights of the two taps and their d/dcoord (0 for out-of-range taps)
struct Ax {
  int c;            // padded index of the first tap, in [0, h]
  float w0, w1;     // interpolation weights
  float d0, d1;     // d w / d coord: -1 / +1, or 0 when the tap is padding
};
__device__ __forceinline__ Ax axis(float ic, int h) {
  const float f0 = floorf(ic);
  const int i0 = (int)f0;
  const float fr = ic - f0;
  const bool v0 = (unsigned)i0 < (unsigned)h, v1 = (unsigned)(i0 + 1) < (unsigned)h;
  Ax a;
  a.c = (i0 < -1 ? -1 : (i0 > h - 1 ? h - 1 : i0)) + 1;
  a.w0 = v0 ? 1.f - fr : 0.f;
  a.w1 = v1 ? fr : 0.f;
  a.d0 = v0 ? -1.f : 0.f;
  a.d1 = v1 ? 1.f : 0.f;
  return a;
}

// bilinear sample of two source planes at once (packed fp32 math: the two
// planes of a texel's float4 half), from the separable tap weights
// ax / ay = (w0, w1, dw0, dw1) of the column / row: value and (DRV) d/dix,
// d/diy
template <bool DRV>
__device__ __forceinline__ void samp_pair(pf32x2 A, pf32x2 B, pf32x2 Cc, pf32x2 D, float4 ax, float4 ay, pf32x2& v,
                                          pf32x2& dx, pf32x2& dy) {
  const pf32x2 top = ax.x * A + ax.y * B, bot = ax.x * Cc + ax.y * D;
  v = ay.x * top + ay.y * bot;
  if constexpr (DRV) {
    const pf32x2 dtop = ax.z * A + ax.w * B, dbot = ax.z * Cc + ax.w * D;
    dx = ay.x * dtop + ay.y * dbot;
    dy = ay.z * top + ay.w * bot;
  }
}

// One 8-byte LDS read that the compiler cannot pair with a neighbour into a
// ds_read2_b64 (8 LDS cycles for 2 x 8 B per lane, half the bandwidth of
// two single reads).  Its completion is tracked by lds_wait below, not by
// the compiler.
template <int OFF>
__device__ __forceinline__ pf32x2 lds_read_b64(unsigned addr) {
  pf32x2 v;
  asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(OFF));
  return v;
}
// wait until at most N LDS operations are outstanding, then hand out the
// NV values read by lds_read_b64 (tied as in/out operands, so no use of them
// can be scheduled above the wait)
template <int N, int NV>
__device__ __forceinline__ void lds_wait(pf32x2* v) {
  static_assert(NV == 5 || NV == 10, "batch size");
  if constexpr (NV == 5) {
    asm volatile("s_waitcnt lgkmcnt(%5)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]) : "i"(N));
  } else {
    asm volatile("s_waitcnt lgkmcnt(%10)"
                 : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]),
                   "+v"(v[8]), "+v"(v[9])
                 : "i"(N));
  }
}

// Diagnostic build only (-DPAIG_DEC_STAMPS, tools/dec_stamps.sh): s_memtime
// at the phase boundaries of blocks 0-3, every wave, the first 32
// iterations, stored by lane 0 (vector stores) for tools/dec_stamps.py.
#ifdef PAIG_DEC_STAMPS
__device__ unsigned long long paig_dec_stamps[4][16][33][6];
#define DEC_STAMP(it, ph)                                                                     \
  do {                                                                                        \
    if (blockIdx.x < 4 && (threadIdx.x & 63) == 0 && (it) < 33)                               \
      paig_dec_stamps[blockIdx.x][threadIdx.x >> 6][(it)][(ph)] = __builtin_amdgcn_s_memtime(); \
  } while (0)
#else
#define DEC_STAMP(it, ph) \
  do {                    \
  } while (0)
#endif

template <int K, int H, bool T8, bool LW>
__global__ void __launch_bounds__((DecCu<K, H>::NT))
dec_bwd_cu_k(PosView pos, Src S, TView tgt, WSrc dsse, FView dout, float* __restrict__ dpos,
             float* __restrict__ slab, int F, int Rl, int FPB) {
  using C = DecCu<K, H>;
  constexpr int h = C::h, hp = C::hp, hh = C::hh, HW = C::HW, PS = C::PS, NIT = C::NIT, GPITCH = C::GPITCH;
  constexpr int NT = C::NT, PL = C::PL, NI = C::NI, NC = C::NC, NG = C::NG, TC0 = C::TC0, TG0 = C::TG0, NR = C::NR;
  __shared__ float4 SRC[K][hp * hp];              // (template + 5, sigmoid(content) x 3), zero border
  __shared__ float2 G[2][2][K][H * GPITCH];       // [frame parity][plane pair][object][row][slot]
  __shared__ float4 AXW[2][K][2][H];              // per output column (0) / row (1): tap weights w0, w1 and
  __shared__ int AXC[2][K][2][H];                 //   their d/dcoord d0, d1; padded index of the first tap
  __shared__ int J0[3][K][2][h];                  // gather tables (3 frames in flight): first index
  __shared__ float WT[3][K][2][h][GW];            //   of the 5-wide window and its weights
  __shared__ double RED[2][2 * K][NR];            // fp64 position-gradient partials (RPW per wave)
  __shared__ double BC[H];                        // affine_grid base coordinates (fp64, frame-invariant)
  __shared__ long long IXS[DecFrames::IXN];       // byte targets' dataset rows (ix_load / ix_store)

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int R = pos.grp;
  const bool grouped = R > 0 && Rl > 0 && Rl < R;
  const int NL = grouped ? (F / R) * Rl : F;
  const int first = blockIdx.x * FPB;
  const int nf = first < NL ? (NL - first < FPB ? NL - first : FPB) : 0;

  // ---- frame cursors (wave-uniform)
  const DecFrames FR(pos, tgt, Rl);
  const auto ixst = FR.template ix_load<T8>(first, nf, tid);
  const int q0 = ixst.q0;
  dsse.template prep<LW>();
  auto cur_at = [&](int n) { return FR.at(n); };
  auto advance = [&](DecCursor c) { return FR.next(c); };
  auto pos_of = [&](const DecCursor& c) { return FR.pos_of(c); };

  // ---- prologue: frame 0's loads first (their latency overlaps the staging below)
  float bgv[PS][3], gbg[PS][3], tn[PS][3];
  float gsrc[NIT][PL];
  // this thread's table entry: an axis entry (tid in [TC0, TC0 + NC)) or a
  // gather entry (tid in [TG0, TG0 + NG)); (ck, cax) = the object / axis
  // whose position it reads
  const int tc = tid - TC0, tg = tid - TG0;
  const bool is_c = tc >= 0 && tc < NC, is_g = tg >= 0 && tg < NG;
  const int ck = is_c ? tc / (2 * H) : (is_g ? tg / (2 * h) : 0);
  const int cax = is_c ? (tc / H) & 1 : (is_g ? (tg / h) & 1 : 0);
  const int cj = is_c ? tc % H : (is_g ? tg % h : 0);
  // the tables of a frame from this thread's position value l (BC complete)
  auto tables = [&](float l, int aslot, int gslot_) {
    if (is_c) {
      const Ax x = axis(src_coord(BC[cj], pos.theta_t(l, H, h), h, pos.sg), h);
      AXW[aslot][ck][cax][cj] = make_float4(x.w0, x.w1, x.d0, x.d1);
      AXC[aslot][ck][cax][cj] = x.c;
    } else if (is_g) {
      gather_entry(pos, l, BC, H, h, cj, &J0[gslot_][ck][cax][cj], WT[gslot_][ck][cax][cj]);
    }
  };
  // targets -> tn (no SSE weight: none read); staged: the row from IXS, else
  // (the block's first frame) from ix_load
  auto fetch = [&](const DecCursor& c, bool staged) {
    if (!dsse.template has<LW>()) return;
    const long long to = staged ? FR.template tgt_off<T8>(c, IXS, q0) : FR.template tgt_off0<T8>(c, ixst);
#pragma unroll
    for (int s = 0; s < PS; ++s) {
      const int p = tid + NT * s;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) tn[s][ch] = p < HW ? FR.tgt.template raw1<T8>(to + ch * HW + p) : 0.f;
    }
  };
  auto is_active = [&](float w) { return w != 0.f || dout.p != nullptr; };
  // cursors: ccur = frame it, c1 = frame it+1, c2 = frame it+2 (clamped to the block's last)
  DecCursor cprev{}, ccur = cur_at(first < NL ? first : 0);
  DecCursor c1 = nf > 1 ? advance(ccur) : ccur;
  DecCursor c2 = nf > 2 ? advance(c1) : c1;
  float w_cur = 0.f, p0 = 0.f, ppos = 0.f;
  bool act_cur = false, act_prev = false;
#pragma unroll
  for (int s2 = 0; s2 < PS; ++s2)
#pragma unroll
    for (int c = 0; c < 3; ++c) tn[s2][c] = 0.f;
  if (nf > 0) {
    if constexpr (!T8) fetch(ccur, false);
    p0 = pos_of(ccur)[2 * ck + cax];
    ppos = pos_of(c1)[2 * ck + cax];
    w_cur = dsse.template has<LW>() ? uniform_f(dsse.template at<LW>(ccur)) : 0.f;
    act_cur = is_active(w_cur);
  }
  // sources, background, base coordinates, dead frames' position gradients
  for (int t = tid; t < K * hp * hp; t += NT) {
    const int k = t / (hp * hp), q = t % (hp * hp), y = q / hp - 1, x = q % hp - 1;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((unsigned)y < (unsigned)h && (unsigned)x < (unsigned)h) {
      const int o = y * h + x;
      v.x = S.tmpl[k * hh + o] + 5.f;
      v.y = 1.f / (1.f + expf(-S.cont[(k * 3 + 0) * hh + o]));
      v.z = 1.f / (1.f + expf(-S.cont[(k * 3 + 1) * hh + o]));
      v.w = 1.f / (1.f + expf(-S.cont[(k * 3 + 2) * hh + o]));
    }
    SRC[k][q] = v;
  }
#pragma unroll
  for (int s = 0; s < PS; ++s) {
    const int p = tid + NT * s;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      bgv[s][c] = p < HW ? S.bg[c * HW + p] : 0.f;
      gbg[s][c] = 0.f;
    }
  }
#pragma unroll
  for (int u = 0; u < NIT; ++u)
#pragma unroll
    for (int q = 0; q < PL; ++q) gsrc[u][q] = 0.f;
  for (int j = tid; j < H; j += NT) BC[j] = base_coord(j, H);
  // dead frames (steps Rl..R-1 of every sequence): zero position gradients
  if (grouped) {
    const int per = (R - Rl) * 2 * K, nd = (F / R) * per;
    for (int e = blockIdx.x * NT + tid; e < nd; e += gridDim.x * NT) {
      const int b = e / per, rem = e - b * per;
      dpos[((long long)b * R + Rl + rem / (2 * K)) * 2 * K + rem % (2 * K)] = 0.f;
    }
  }
  if constexpr (T8) {   // (byte targets: the row load was in flight across the staging above)
    FR.ix_store(ixst, IXS, tid);
    if (nf > 0) fetch(ccur, false);
  }
  __syncthreads();   // SRC, BC
  if (nf > 0) tables(p0, 0, 0);
  __syncthreads();
  DEC_STAMP(0, 0);

  for (int it = 0; it <= nf; ++it) {
    // tables of frame it+1 (its positions arrived during the last iteration),
    // then the loads of frame it+2's positions and frame it+1's weight
    // (clamped to a valid frame on the last iterations: issued
    // unconditionally, so the memory-counter waits stay exact)
    if (it + 1 < nf) tables(ppos, (it + 1) & 1, (it + 1) % 3);
    ppos = pos_of(c2)[2 * ck + cax];
    const float wnext = dsse.template has<LW>() ? dsse.template at<LW>(c1) : 0.f;
    DEC_STAMP(it, 1);
    // The two passes of an iteration, in an order that alternates between the
    // wave halves (each SIMD holds waves w, w+4, w+8, w+12): half the waves
    // gather (LDS-read heavy) while the other half sample (VALU heavy).
    auto pass2 = [&]() {
    // ---- pass 2 of frame it-1: source texels gather from G; its position gradients
  #ifdef PAIG_DEC_SKIP_P2   // diagnostic builds only (tools/dec_stamps.sh): phase cost by elimination
      if (false) {
  #else
      if (it >= 1 && act_prev) {
  #endif
        const int sl = (it - 1) & 1, gs = (it - 1) % 3;
        if (wv < 2 * K) {   // wave e finishes position gradient e from the NR row partials
          const double v = lane < NR ? RED[sl][wv][lane] : 0.0;
          const double tot = wave_sum_dpp_d(v);
          const float dth = (float)(tot * (double)h * 0.5);
          if (lane == 0) dpos[(long long)cprev.f * 2 * K + wv] = -(dth * pos.sgf) / (float)h;
        }
  #pragma unroll
        for (int u = 0; u < NIT; ++u) {
          const int t = tid + NT * u;
          if (NIT == 1 || t < NI) {
            // item t: texel tx = t % (K hh), plane pair hf (PL = 2) or all 4 planes
            const int tx = t % (K * hh), hf = PL == 2 ? t / (K * hh) : 0;
            const int k = tx / hh, q = tx % hh, ys = q / h, xs = q % h;
            const int i0 = J0[gs][k][1][ys], c0 = J0[gs][k][0][xs];
            float wy[GW], wx[GW];
  #pragma unroll
            for (int a2 = 0; a2 < GW; ++a2) {
              wy[a2] = WT[gs][k][1][ys][a2];
              wx[a2] = WT[gs][k][0][xs][a2];
            }
            // columns c0 + b: the even b share c0's parity (consecutive slots
            // from gslot(c0)), the odd b the other one: every read below is an
            // immediate offset from one of two bases.  The reads are issued as
            // single ds_read_b64 (inline asm: the compiler would pair them into
            // ds_read2_b64, which moves half the bytes per LDS cycle), one
            // column (5 rows x the plane pairs) per batch, two batches ahead.
            const int be = i0 * GPITCH + gslot<H>(c0), bo = i0 * GPITCH + gslot<H>(c0 + 1);
            unsigned ae[2], ao[2];
#pragma unroll
            for (int q2 = 0; q2 < 2; ++q2) {
              ae[q2] = (unsigned)(uintptr_t)&G[sl][q2 == 0 ? hf : 1][k][be];
              ao[q2] = (unsigned)(uintptr_t)&G[sl][q2 == 0 ? hf : 1][k][bo];
            }
            // packed fp32 accumulators: one plane pair per pf32x2
            pf32x2 acc[PL / 2];
#pragma unroll
            for (int q2 = 0; q2 < PL / 2; ++q2) acc[q2] = pf32x2{0.f, 0.f};
            pf32x2 vb[3][GW][PL / 2];   // batches in flight (ring of 3 columns)
            auto issue = [&](auto bc) {
              constexpr int b = decltype(bc)::value;
#pragma unroll
              for (int a2 = 0; a2 < GW; ++a2)
#pragma unroll
                for (int q2 = 0; q2 < PL / 2; ++q2)
                  vb[b % 3][a2][q2] = lds_read_b64<(b >> 1) * 8>((b & 1 ? ao[q2] : ae[q2]) + a2 * GPITCH * 8);
            };
            auto consume = [&](auto bc) {
              constexpr int b = decltype(bc)::value;
              // the reads issued after this column's: columns b+1 and b+2 (if any)
              constexpr int younger = ((b + 2 < GW ? 2 : (b + 1 < GW ? 1 : 0))) * GW * (PL / 2);
              lds_wait<(younger < 15 ? younger : 15), GW * (PL / 2)>(&vb[b % 3][0][0]);
              pf32x2 r[PL / 2];
#pragma unroll
              for (int q2 = 0; q2 < PL / 2; ++q2) r[q2] = pf32x2{0.f, 0.f};
#pragma unroll
              for (int a2 = 0; a2 < GW; ++a2)
#pragma unroll
                for (int q2 = 0; q2 < PL / 2; ++q2) r[q2] += wy[a2] * vb[b % 3][a2][q2];
#pragma unroll
              for (int q2 = 0; q2 < PL / 2; ++q2) acc[q2] += wx[b] * r[q2];
            };
            issue(std::integral_constant<int, 0>{});
            issue(std::integral_constant<int, 1>{});
            issue(std::integral_constant<int, 2>{});
            consume(std::integral_constant<int, 0>{});
            issue(std::integral_constant<int, 3>{});
            consume(std::integral_constant<int, 1>{});
            issue(std::integral_constant<int, 4>{});
            consume(std::integral_constant<int, 2>{});
            consume(std::integral_constant<int, 3>{});
            consume(std::integral_constant<int, 4>{});
  #pragma unroll
            for (int q2 = 0; q2 < PL / 2; ++q2) {
              gsrc[u][2 * q2] += acc[q2].x;
              gsrc[u][2 * q2 + 1] += acc[q2].y;
            }
          }
        }
      } else if (it >= 1 && tid < 2 * K) {
        dpos[(long long)cprev.f * 2 * K + tid] = 0.f;
      }
    };
    auto pass1 = [&]() {
    // ---- pass 1 of frame it
  #ifdef PAIG_DEC_SKIP_P1
      if (false) {
  #else
      if (it < nf && act_cur) {
  #endif
        const int sl = it & 1;
        const float w_f = 2.f * w_cur;
        const float* dof = dout.p ? dout.p + (long long)ccur.f * dout.fs : nullptr;
        double sx[K], sy[K];
  #pragma unroll
        for (int k = 0; k < K; ++k) sx[k] = sy[k] = 0.0;
  #pragma unroll
        for (int s = 0; s < PS; ++s) {
          const int p = tid + NT * s;
          if (PS > 1 && p >= HW) break;
          const int i = p / H, j = p % H;
          // K >= 3: the derivative planes are re-formed from the texels after
          // the blend instead of being held across it (register budget)
          constexpr bool HOLD = K < 3;
          float sv[K][4], sdx[HOLD ? K : 1][4], sdy[HOLD ? K : 1][4];
          float4 wxa[K], wya[K];
          int base[K];
  #pragma unroll
          for (int k = 0; k < K; ++k) {
            wxa[k] = AXW[sl][k][0][j];
            wya[k] = AXW[sl][k][1][i];
            base[k] = AXC[sl][k][1][i] * hp + AXC[sl][k][0][j];
          }
  #pragma unroll
          for (int k = 0; k < K; ++k) {
            const float4 ax = wxa[k], ay = wya[k];
            const int bs = base[k];
            const float4 a = SRC[k][bs], b = SRC[k][bs + 1], c = SRC[k][bs + hp], d = SRC[k][bs + hp + 1];
            const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
            const float cv[4] = {c.x, c.y, c.z, c.w}, dv[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const float top = fmaf(ax.y, bv[q], ax.x * av[q]), bot = fmaf(ax.y, dv[q], ax.x * cv[q]);
              sv[k][q] = fmaf(ay.y, bot, ay.x * top);
              if constexpr (HOLD) {
                const float dtop = fmaf(ax.w, bv[q], ax.z * av[q]), dbot = fmaf(ax.w, dv[q], ax.z * cv[q]);
                sdx[k][q] = fmaf(ay.y, dbot, ay.x * dtop);
                sdy[k][q] = fmaf(ay.w, bot, ay.z * top);
              }
            }
          }
          float o[3], m[K + 1];
          blend<K>(sv, bgv[s], o, m);
          float g[3];
  #pragma unroll
          for (int c = 0; c < 3; ++c) {
            g[c] = w_f * (o[c] - TView::val1<T8>(tn[s][c]));
            if (dof) g[c] += dof[c * HW + p];
            gbg[s][c] = fmaf(m[K], g[c], gbg[s][c]);
          }
          const int gof = i * GPITCH + gslot<H>(j);
  #pragma unroll
          for (int k = 0; k < K; ++k) {
            float dT = 0.f;
            float dC[3];
  #pragma unroll
            for (int c = 0; c < 3; ++c) {
              dC[c] = m[k] * g[c];
              dT = fmaf(g[c], sv[k][1 + c] - o[c], dT);
            }
            dT *= m[k];
            G[sl][0][k][gof] = make_float2(dT, dC[0]);
            G[sl][1][k][gof] = make_float2(dC[1], dC[2]);
            const float gq[4] = {dT, dC[0], dC[1], dC[2]};
            float gx = 0.f, gy = 0.f;
            if constexpr (HOLD) {
  #pragma unroll
              for (int q = 0; q < 4; ++q) {
                gx = fmaf(gq[q], sdx[k][q], gx);
                gy = fmaf(gq[q], sdy[k][q], gy);
              }
            } else {
              const int bs = base[k];
              const float4 a = SRC[k][bs], b = SRC[k][bs + 1], c = SRC[k][bs + hp], d = SRC[k][bs + hp + 1];
              pf32x2 gxy = {0.f, 0.f}, gyy = {0.f, 0.f};
  #pragma unroll
              for (int q = 0; q < 4; q += 2) {
                pf32x2 v, dx, dy;
                samp_pair<true>(q ? pf32x2{a.z, a.w} : pf32x2{a.x, a.y}, q ? pf32x2{b.z, b.w} : pf32x2{b.x, b.y},
                                q ? pf32x2{c.z, c.w} : pf32x2{c.x, c.y}, q ? pf32x2{d.z, d.w} : pf32x2{d.x, d.y}, wxa[k],
                                wya[k], v, dx, dy);
                const pf32x2 gp = {gq[q], gq[q + 1]};
                gxy += gp * dx;
                gyy += gp * dy;
              }
              gx = gxy.x + gxy.y;
              gy = gyy.x + gyy.y;
            }
            sx[k] += (double)gx;
            sy[k] += (double)gy;
          }
        }
        double sv2[2 * K];
  #pragma unroll
        for (int k = 0; k < K; ++k) {
          sv2[2 * k] = sx[k];
          sv2[2 * k + 1] = sy[k];
        }
        row_sums_dpp_d<2 * K>(sv2);
        if constexpr (C::RPW == 2) {
  #pragma unroll
          for (int e = 0; e < 2 * K; ++e) sv2[e] += __shfl_xor(sv2[e], 16, 64);   // rows 0+1, 2+3
          if ((lane & 31) == 0)
  #pragma unroll
            for (int e = 0; e < 2 * K; ++e) RED[sl][e][wv * 2 + (lane >> 5)] = sv2[e];
        } else {
          if ((lane & 15) == 0)
  #pragma unroll
            for (int e = 0; e < 2 * K; ++e) RED[sl][e][wv * 4 + (lane >> 4)] = sv2[e];
        }
      }
    };
    if (!C::ALT || wv < C::NW / 2) {
      pass2();
      DEC_STAMP(it, 2);
      pass1();
    } else {
      pass1();
      DEC_STAMP(it, 2);
      pass2();
    }
    DEC_STAMP(it, 3);
    // ---- frame it+1: targets (in flight across the barrier and pass 2) and loss weight
    cprev = ccur;
    act_prev = act_cur;
    if (it + 1 < nf) {
      ccur = c1;
      c1 = c2;
      if (it + 3 < nf) c2 = advance(c2);
      fetch(ccur, true);
      w_cur = uniform_f(wnext);
      act_cur = is_active(w_cur);
    } else {
      act_cur = false;
    }
    DEC_STAMP(it, 4);
    __syncthreads();
    DEC_STAMP(it, 5);
  }
  // ---- this block's partial source gradients -> its slab row (each element
  // owned by exactly one thread, written once)
  float* srow = slab + (long long)blockIdx.x * ((long long)K * hh * 4 + 3LL * HW);
  float* s_tm = srow;
  float* s_ct = srow + K * hh;
  float* s_bg = s_ct + K * 3 * hh;
#pragma unroll
  for (int u = 0; u < NIT; ++u) {
    const int t = tid + NT * u;
    if (t < NI) {
      const int tx = t % (K * hh), pq = PL == 2 ? (t / (K * hh)) * 2 : 0;
      const int k = tx / hh, q = tx % hh;
#pragma unroll
      for (int q2 = 0; q2 < PL; ++q2) {
        const int pl = pq + q2;   // 0: template, 1..3: content channel pl-1
        if (pl == 0) s_tm[tx] = gsrc[u][q2];
        else s_ct[(k * 3 + pl - 1) * hh + q] = gsrc[u][q2];
      }
    }
  }
#pragma unroll
  for (int s = 0; s < PS; ++s) {
    const int p = tid + NT * s;
    if (p < HW)
#pragma unroll
      for (int c = 0; c < 3; ++c) s_bg[c * HW + p] = gbg[s][c];
  }
}

// ---------------------------------------------------------------------------
// Decoder backward for 64 x 64 frames (mnist: (K, H) = (2, 64)), one CU per
// block.  One frame's pixel-gradient image G (K objects x 4 planes x 4096
// pixels = 128 KB) does not fit the LDS beside the sources, so a frame is
// processed in two bands of H/2 output rows:
//   pass 1 (band b): sample / composite / dL/dout for the band's rows and the
//     GW-1 rows below it (the halo: their G only; their background and
//     position-gradient sums are taken in their own band, once per pixel);
//   pass 2 (band b): every (source texel, plane pair) whose 5-row gather
//     window starts in the band gathers its <= 5 x 5 pixels from G (the
//     window lies inside band + halo), accumulating in registers over frames.
// Each thread owns pixels tid + NT s, s = 0..3: slots 0, 1 form band 0 and
// 2, 3 band 1; slot 2 of the first NHALO threads is also band 0's halo, so
// targets, background values and background gradients stay in registers.
// The source gradients are the same gather as dec_bwd_cu_k's (a fixed order,
// no atomics); the position gradients the same fp64 sums.
template <int K, int H>
struct DecBand {
  static constexpr int NT = 1024, NW = NT / 64;
  static constexpr int h = H / 2, hp = h + 2, hh = h * h, HW = H * H;
  static constexpr int BR = H / 2;          // output rows per band
  static constexpr int GR = BR + GW - 1;    // G rows: band + halo
  static constexpr int GPITCH = H + 8;      // float2 slots per G row (even columns first; 8 mod 16)
  static constexpr int PS = HW / NT;        // pixel slots per thread
  static constexpr int NHALO = (GW - 1) * H;
  static constexpr int NI = K * hh * 2;     // pass-2 items: (texel, plane pair)
  static constexpr int NIT = NI / NT;
  static constexpr int NC = K * 2 * H, NG = K * 2 * h, TG0 = NC;   // axis / gather table threads
  static constexpr int NR = NW * 4;         // fp64 position-gradient partials (4 row sums per wave)
  static_assert(HW % NT == 0 && PS == 4 && K * hh == 2 * NT && NHALO <= NT && TG0 + NG <= NT && NR <= 64,
                "decoder band geometry");
};

template <int K, int H, bool T8, bool LW>
__global__ void __launch_bounds__(1024)
dec_bwd_band_k(PosView pos, Src S, TView tgt, WSrc dsse, FView dout, float* __restrict__ dpos,
               float* __restrict__ slab, int F, int Rl, int FPB) {
  using C = DecBand<K, H>;
  constexpr int h = C::h, hp = C::hp, hh = C::hh, HW = C::HW, NT = C::NT, PS = C::PS, BR = C::BR;
  constexpr int GPITCH = C::GPITCH, NIT = C::NIT, NC = C::NC, NG = C::NG, TG0 = C::TG0, NR = C::NR;
  __shared__ float4 SRC[K][hp * hp];           // (template + 5, sigmoid(content) x 3), zero border
  __shared__ float2 G[2][K][C::GR * GPITCH];   // [plane pair][object][band row][slot]
  __shared__ float4 AXW[K][2][H];              // per output column (0) / row (1): w0, w1, d0, d1
  __shared__ int AXC[K][2][H];                 //   and the padded index of the first tap
  __shared__ int J0[K][2][h];                  // gather tables: first index of the 5-wide window
  __shared__ float WT[K][2][h][GW];            //   and its weights
  __shared__ double RED[2 * K][NR];
  __shared__ double BC[H];
  __shared__ long long IXS[DecFrames::IXN];    // byte targets' dataset rows (ix_load / ix_store)

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int R = pos.grp;
  const bool grouped = R > 0 && Rl > 0 && Rl < R;
  const int NL = grouped ? (F / R) * Rl : F;
  const int first = blockIdx.x * FPB;
  const int nf = first < NL ? (NL - first < FPB ? NL - first : FPB) : 0;
  const DecFrames FR(pos, tgt, Rl);
  const auto ixst = FR.template ix_load<T8>(first < NL ? first : 0, nf, tid);
  const int q0 = ixst.q0;
  dsse.template prep<LW>();

  const int tg = tid - TG0;
  const bool is_c = tid < NC, is_g = tg >= 0 && tg < NG;
  const int ck = is_c ? tid / (2 * H) : (is_g ? tg / (2 * h) : 0);
  const int cax = is_c ? (tid / H) & 1 : (is_g ? (tg / h) & 1 : 0);
  const int cj = is_c ? tid % H : (is_g ? tg % h : 0);

  float gbg[PS][3];
  float gsrc[NIT][2];
#pragma unroll
  for (int s = 0; s < PS; ++s)
#pragma unroll
    for (int c = 0; c < 3; ++c) gbg[s][c] = 0.f;
#pragma unroll
  for (int u = 0; u < NIT; ++u) gsrc[u][0] = gsrc[u][1] = 0.f;
  DecCursor cur = FR.at(first < NL ? first : 0);
  for (int t = tid; t < K * hp * hp; t += NT) {
    const int k = t / (hp * hp), q = t % (hp * hp), y = q / hp - 1, x = q % hp - 1;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((unsigned)y < (unsigned)h && (unsigned)x < (unsigned)h) {
      const int o = y * h + x;
      v.x = S.tmpl[k * hh + o] + 5.f;
      v.y = 1.f / (1.f + expf(-S.cont[(k * 3 + 0) * hh + o]));
      v.z = 1.f / (1.f + expf(-S.cont[(k * 3 + 1) * hh + o]));
      v.w = 1.f / (1.f + expf(-S.cont[(k * 3 + 2) * hh + o]));
    }
    SRC[k][q] = v;
  }
  for (int j = tid; j < H; j += NT) BC[j] = base_coord(j, H);
  if (grouped) {   // dead frames (steps Rl..R-1 of every sequence): zero position gradients
    const int per = (R - Rl) * 2 * K, nd = (F / R) * per;
    for (int e = blockIdx.x * NT + tid; e < nd; e += gridDim.x * NT) {
      const int b = e / per, rem = e - b * per;
      dpos[((long long)b * R + Rl + rem / (2 * K)) * 2 * K + rem % (2 * K)] = 0.f;
    }
  }
  if constexpr (T8) FR.ix_store(ixst, IXS, tid);
  __syncthreads();   // SRC, BC

  for (int it = 0; it < nf; ++it) {
    const float w = dsse.template has<LW>() ? uniform_f(dsse.template at<LW>(cur)) : 0.f;
    const float* dof = dout.p ? dout.p + (long long)cur.f * dout.fs : nullptr;
    const DecCursor nxt = it + 1 < nf ? FR.next(cur) : cur;
    if (w == 0.f && dof == nullptr) {   // block-uniform: no gradient flows through this frame
      if (tid < 2 * K) dpos[(long long)cur.f * 2 * K + tid] = 0.f;
      cur = nxt;
      continue;
    }
    const long long to = FR.template tgt_off<T8>(cur, IXS, q0);
    // ---- the frame's axis and gather tables (the previous frame's last
    // barrier ordered every read of the old ones)
    if (is_c || is_g) {
      const float l = FR.pos_of(cur)[2 * ck + cax];
      if (is_c) {
        const Ax x = axis(src_coord(BC[cj], pos.theta_t(l, H, h), h, pos.sg), h);
        AXW[ck][cax][cj] = make_float4(x.w0, x.w1, x.d0, x.d1);
        AXC[ck][cax][cj] = x.c;
      } else {
        gather_entry(pos, l, BC, H, h, cj, &J0[ck][cax][cj], WT[ck][cax][cj]);
      }
    }
    __syncthreads();
    const float w_f = 2.f * w;
    double sx[K], sy[K];
#pragma unroll
    for (int k = 0; k < K; ++k) sx[k] = sy[k] = 0.0;

    // one pixel of pass 1 (slot s, band b); own: the band owns the pixel
    // (background / position-gradient sums), else it is band 0's halo
    auto pixel = [&](int s, int b, bool own) __attribute__((always_inline)) {
      asm volatile("" ::: "memory");   // tables re-read per pixel (registers)
      const int p = tid + NT * s, i = p / H, j = p % H;
      // background and target from memory, issued before the sampling
      // (registers hold the background gradients)
      const float bq3[3] = {S.bg[p], S.bg[HW + p], S.bg[2 * HW + p]};
      float tq[3] = {0.f, 0.f, 0.f};
      if (dsse.template has<LW>())
#pragma unroll
        for (int c = 0; c < 3; ++c) tq[c] = TView::val1<T8>(FR.tgt.template raw1<T8>(to + c * HW + p));
      float sv[K][4];
      // the texels of object k and their bilinear (derivative) weights
      auto texels = [&](int k, float4& ax, float4& ay, float (*tv)[4]) __attribute__((always_inline)) {
        ax = AXW[k][0][j];
        ay = AXW[k][1][i];
        const int bs = AXC[k][1][i] * hp + AXC[k][0][j];
        const float4 a = SRC[k][bs], bq = SRC[k][bs + 1], c = SRC[k][bs + hp], d = SRC[k][bs + hp + 1];
        const float4 t4[4] = {a, bq, c, d};
#pragma unroll
        for (int n = 0; n < 4; ++n) {
          tv[n][0] = t4[n].x;
          tv[n][1] = t4[n].y;
          tv[n][2] = t4[n].z;
          tv[n][3] = t4[n].w;
        }
      };
#pragma unroll
      for (int k = 0; k < K; ++k) {
        float4 ax, ay;
        float tv[4][4];
        texels(k, ax, ay, tv);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float top = fmaf(ax.y, tv[1][q], ax.x * tv[0][q]), bot = fmaf(ax.y, tv[3][q], ax.x * tv[2][q]);
          sv[k][q] = fmaf(ay.y, bot, ay.x * top);
        }
      }
      float o[3], m[K + 1];
      blend<K>(sv, bq3, o, m);
      float g[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        g[c] = w_f * (o[c] - tq[c]);
        if (dof) g[c] += dof[c * HW + p];
        if (own) gbg[s][c] = fmaf(m[K], g[c], gbg[s][c]);
      }
      const int gof = (i - b * BR) * GPITCH + gslot<H>(j);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        float dT = 0.f;
        float dC[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          dC[c] = m[k] * g[c];
          dT = fmaf(g[c], sv[k][1 + c] - o[c], dT);
        }
        dT *= m[k];
        G[0][k][gof] = make_float2(dT, dC[0]);
        G[1][k][gof] = make_float2(dC[1], dC[2]);
        if (own) {   // d/dix, d/diy of the 4 planes re-formed from the texels (registers)
          const float gq[4] = {dT, dC[0], dC[1], dC[2]};
          float4 ax, ay;
          float tv[4][4];
          asm volatile("" ::: "memory");   // re-read, not CSE'd with the sampling reads (held across the blend)
          texels(k, ax, ay, tv);
          float gx = 0.f, gy = 0.f;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float top = fmaf(ax.y, tv[1][q], ax.x * tv[0][q]), bot = fmaf(ax.y, tv[3][q], ax.x * tv[2][q]);
            const float dtop = fmaf(ax.w, tv[1][q], ax.z * tv[0][q]), dbot = fmaf(ax.w, tv[3][q], ax.z * tv[2][q]);
            gx = fmaf(gq[q], fmaf(ay.y, dbot, ay.x * dtop), gx);
            gy = fmaf(gq[q], fmaf(ay.w, bot, ay.z * top), gy);
          }
          sx[k] += (double)gx;
          sy[k] += (double)gy;
          // pinned here: left free, the compiler sinks every pixel's fp64
          // adds to the end of the band and holds their operands (spills)
          asm volatile("" : "+v"(sx[k]), "+v"(sy[k]));
        }
      }
    };
    // pass 2 of band b: the items whose window starts in the band
    auto gather = [&](int b) __attribute__((always_inline)) {
      // the tables are re-read per band (not CSE'd across band 1's pass 1:
      // holding them would spill)
      asm volatile("" ::: "memory");
#pragma unroll
      for (int u = 0; u < NIT; ++u) {
        const int hf = u >> 1, tx = tid + NT * (u & 1);   // K hh = 2 NT: items u, u+1 share a plane pair
        const int k = tx / hh, q = tx % hh, ys = q / h, xs = q % h;
        const int i0 = J0[k][1][ys] - b * BR;
        if ((unsigned)i0 < (unsigned)BR) {
        const int c0 = J0[k][0][xs];
        float wy[GW], wx[GW];
#pragma unroll
        for (int a2 = 0; a2 < GW; ++a2) {
          wy[a2] = WT[k][1][ys][a2];
          wx[a2] = WT[k][0][xs][a2];
        }
        int so[GW];
#pragma unroll
        for (int bb = 0; bb < GW; ++bb) so[bb] = gslot<H>(c0 + bb);
        const float2* gk = &G[hf][k][i0 * GPITCH];
        float ax = 0.f, ay = 0.f;
#pragma unroll
        for (int a2 = 0; a2 < GW; ++a2) {
          float rx = 0.f, ry = 0.f;
#pragma unroll
          for (int bb = 0; bb < GW; ++bb) {
            const float2 v = gk[a2 * GPITCH + so[bb]];
            rx = fmaf(wx[bb], v.x, rx);
            ry = fmaf(wx[bb], v.y, ry);
          }
          ax = fmaf(wy[a2], rx, ax);
          ay = fmaf(wy[a2], ry, ay);
        }
        gsrc[u][0] += ax;
        gsrc[u][1] += ay;
        }
        __builtin_amdgcn_sched_barrier(0);   // one item's 25 reads in flight at a time (registers)
      }
    };

    // ---- band 0: slots 0, 1 (+ the halo: slot 2 of the first NHALO threads)
    pixel(0, 0, true);
    __builtin_amdgcn_sched_barrier(0);
    pixel(1, 0, true);
    __builtin_amdgcn_sched_barrier(0);
    if (tid < C::NHALO) pixel(2, 0, false);
    __syncthreads();
    gather(0);
    __syncthreads();
    // ---- band 1: slots 2, 3; then the position gradients
    pixel(2, 1, true);
    __builtin_amdgcn_sched_barrier(0);
    pixel(3, 1, true);
    {
      double sv2[2 * K];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        sv2[2 * k] = sx[k];
        sv2[2 * k + 1] = sy[k];
      }
      row_sums_dpp_d<2 * K>(sv2);
      if ((lane & 15) == 0)
#pragma unroll
        for (int e = 0; e < 2 * K; ++e) RED[e][wv * 4 + (lane >> 4)] = sv2[e];
    }
    __syncthreads();
    if (wv < 2 * K) {   // wave e finishes position gradient e
      const double tot = wave_sum_dpp_d(lane < NR ? RED[wv][lane] : 0.0);
      const float dth = (float)(tot * (double)h * 0.5);
      if (lane == 0) dpos[(long long)cur.f * 2 * K + wv] = -(dth * pos.sgf) / (float)h;
    }
    gather(1);
    cur = nxt;
    __syncthreads();
  }
  // ---- this block's partial source gradients -> its slab row
  float* srow = slab + (long long)blockIdx.x * ((long long)K * hh * 4 + 3LL * HW);
  float* s_tm = srow;
  float* s_ct = srow + K * hh;
  float* s_bg = s_ct + K * 3 * hh;
#pragma unroll
  for (int u = 0; u < NIT; ++u) {
    const int hf = u >> 1, tx = tid + NT * (u & 1);
    const int k = tx / hh, q = tx % hh;
#pragma unroll
    for (int q2 = 0; q2 < 2; ++q2) {
      const int pl = 2 * hf + q2;   // 0: template, 1..3: content channel pl-1
      if (pl == 0) s_tm[tx] = gsrc[u][q2];
      else s_ct[(k * 3 + pl - 1) * hh + q] = gsrc[u][q2];
    }
  }
#pragma unroll
  for (int s = 0; s < PS; ++s)
#pragma unroll
    for (int c = 0; c < 3; ++c) s_bg[c * HW + tid + NT * s] = gbg[s][c];
}

// ---------------------------------------------------------------------------
// Decoder forward for the headline shapes ((K, H) = (2, 32), (3, 36)).
// HBM-bound: per frame the target is read and the decoded frame written
// (2 x 3 H W floats); everything else (sources, axis tables) lives in LDS.
//   * each thread owns 4 consecutive pixels of one row: the row's axis table
//     entry is shared by the 4, and targets / outputs / background move as one
//     16-byte access per channel;
//   * a block walks a contiguous run of frames, software-pipelined over ONE
//     barrier per frame: iteration it forms the axis tables of frame it+1 (from
//     positions loaded an iteration earlier), issues frame it+1's target loads
//     and frame it+2's position loads, samples / composites frame it and writes
//     it, and sums its SSE per wave (finished by thread 0 next iteration);
//   * sources are sampled as in the backward (padded float4 texel image,
//     separable tap weights), two planes per packed fp32 op.
template <int K, int H>
struct DecFw {
  static constexpr int h = H / 2, hp = h + 2, HW = H * H;
  static constexpr int GPR = H / 4, NGRP = H * GPR;        // 4-pixel groups per row / frame
  static constexpr int NT = (NGRP + 63) / 64 * 64, NW = NT / 64;
  static constexpr int NC = K * 2 * H;                      // axis table entries
  // texel image rows: even padded columns first, then odd ones (the 4 pixels
  // of a quad span 2 source columns, so neighbouring quads read texels 2
  // apart: split by parity they are consecutive); row pitch in texels chosen
  // by a bank model of the ds_read_b128 lane groups (1.04 / 1.10 LDS cycles
  // per group against 1.41 / 1.36 for the plain image)
  static constexpr int P = H == 32 ? 24 : (H == 36 ? 25 : hp + 1);
  static_assert(H % 4 == 0 && NC <= NT && hp % 2 == 0 && P >= hp, "decoder forward geometry");
};
__device__ __forceinline__ int texel_slot(int hp, int x) { return (x & 1) * (hp / 2) + (x >> 1); }

// Rank of lane l in the order of ds_read_b128's four 16-lane bank groups
// ({0-3,12-15,20-27}, {4-11,16-19,28-31}, the same + 32): the pixel quads of
// one group are then 16 consecutive quads (two output rows at H = 32), whose
// texels are consecutive in the split image.
__device__ __forceinline__ int b128_rank(int l) {
  const int m = l & 31;
  int g, r;
  if (m < 4) g = 0, r = m;
  else if (m < 12) g = 1, r = m - 4;
  else if (m < 16) g = 0, r = m - 8;
  else if (m < 20) g = 1, r = m - 8;
  else if (m < 28) g = 0, r = m - 12;
  else g = 1, r = m - 16;
  return (l & 32) + g * 16 + r;
}

template <int K, int H, bool T8>
__device__ __forceinline__ void dec_fwd_cu_body(PosView pos, Src S, FViewW out, TView tgt, float* __restrict__ sse, int F,
                                                int FPB, int bid) {
  pos.load();
  using C = DecFw<K, H>;
  constexpr int h = C::h, hp = C::hp, HW = C::HW, GPR = C::GPR, NC = C::NC, NW = C::NW, P = C::P;
  __shared__ float4 SRC[K][hp * P];     // (template + 5, sigmoid(content) x 3), zero border, split rows
  __shared__ float4 AXC[2][K][4][GPR];  // column 4g+q: w0, w1, texel slots of the two taps (bits)
  __shared__ float4 AXR[2][K][H];       // row: w0, w1, texel-row offset (bits), -
  __shared__ float RED[2][NW];          // per-wave SSE partials
  __shared__ double BC[H];
  __shared__ long long IXS[DecFrames::IXN];   // byte targets' dataset rows (ix_load / ix_store)

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int first = bid * FPB;
  const int nf = first < F ? (F - first < FPB ? F - first : FPB) : 0;
  if (nf == 0) return;   // block-uniform
  const DecFrames FR(pos, tgt, 0);
  const auto ixst = FR.template ix_load<T8>(first, nf, tid);
  const int q0 = ixst.q0;
  const int n = wv * 64 + b128_rank(lane);   // this thread's pixel quad
  const bool px = n < C::NGRP;
  const int i = px ? n / GPR : 0, g = px ? n % GPR : 0, p = i * H + 4 * g;
  const bool is_c = tid < NC;
  const int ck = is_c ? tid / (2 * H) : 0, cax = is_c ? (tid / H) & 1 : 0, cj = is_c ? tid % H : 0;
  const bool has_t = sse != nullptr;

  auto ld4 = [&](const float* b) { return *reinterpret_cast<const float4*>(b); };
  float4 tn[3], bgv[3];
  auto fetch = [&](const DecCursor& c, float4* t, bool staged) {
    if (!has_t || !px) return;
    const long long to = (staged ? FR.template tgt_off<T8>(c, IXS, q0) : FR.template tgt_off0<T8>(c, ixst)) + p;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) t[ch] = FR.tgt.template raw4<T8>(to + ch * HW);
  };
  DecCursor ccur = FR.at(first);
  DecCursor c1 = nf > 1 ? FR.next(ccur) : ccur;
  DecCursor c2 = nf > 2 ? FR.next(c1) : c1;
  if constexpr (!T8) fetch(ccur, tn, false);
  float p0 = 0.f, ppos = 0.f;
  if (is_c) {
    p0 = FR.pos_of(ccur)[2 * ck + cax];
    ppos = FR.pos_of(c1)[2 * ck + cax];
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) bgv[ch] = px ? ld4(S.bg + ch * HW + p) : make_float4(0.f, 0.f, 0.f, 0.f);
  for (int t = tid; t < K * hp * hp; t += C::NT) {
    const int k = t / (hp * hp), q = t % (hp * hp), yp = q / hp, xp = q % hp, y = yp - 1, x = xp - 1;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((unsigned)y < (unsigned)h && (unsigned)x < (unsigned)h) {
      const int o = y * h + x, hh = h * h;
      v.x = S.tmpl[k * hh + o] + 5.f;
      v.y = 1.f / (1.f + expf(-S.cont[(k * 3 + 0) * hh + o]));
      v.z = 1.f / (1.f + expf(-S.cont[(k * 3 + 1) * hh + o]));
      v.w = 1.f / (1.f + expf(-S.cont[(k * 3 + 2) * hh + o]));
    }
    SRC[k][yp * P + texel_slot(hp, xp)] = v;
  }
  for (int j = tid; j < H; j += C::NT) BC[j] = base_coord(j, H);
  auto tables = [&](float l, int slot) {
    if (is_c) {
      const Ax x = axis(src_coord(BC[cj], pos.theta_t(l, H, h), h, pos.sg), h);
      if (cax == 0)
        AXC[slot][ck][cj & 3][cj >> 2] =
            make_float4(x.w0, x.w1, __int_as_float(texel_slot(hp, x.c)), __int_as_float(texel_slot(hp, x.c + 1)));
      else
        AXR[slot][ck][cj] = make_float4(x.w0, x.w1, __int_as_float(x.c * P), 0.f);
    }
  };
  if constexpr (T8) {   // (byte targets: the row load was in flight across the staging above)
    FR.ix_store(ixst, IXS, tid);
    fetch(ccur, tn, false);
  }
  __syncthreads();   // SRC, BC
  tables(p0, 0);
  __syncthreads();

  DecCursor cprev = ccur;
  for (int it = 0; it < nf; ++it) {
    if (it + 1 < nf) tables(ppos, (it + 1) & 1);
    if (is_c) ppos = FR.pos_of(c2)[2 * ck + cax];
    float4 tq[3];
    if (it + 1 < nf) fetch(c1, tq, true);
    if (has_t && it >= 1 && tid == 0) {   // SSE of frame it-1 (partials before the last barrier)
      float a = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) a += RED[(it - 1) & 1][w];
      sse[cprev.f] = a;
    }
    const int sl = it & 1;
    float acc = 0.f;
    if (px) {
      float o[4][3];
      float4 ay[K];
      int rb[K];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        ay[k] = AXR[sl][k][i];
        rb[k] = __float_as_int(ay[k].z);
      }
      const float bq[3][4] = {{bgv[0].x, bgv[0].y, bgv[0].z, bgv[0].w},
                              {bgv[1].x, bgv[1].y, bgv[1].z, bgv[1].w},
                              {bgv[2].x, bgv[2].y, bgv[2].z, bgv[2].w}};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float sv[K][4];
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float4 ax = AXC[sl][k][q][g];
          const int sa = rb[k] + __float_as_int(ax.z), sb = rb[k] + __float_as_int(ax.w);
          const float4 a = SRC[k][sa], b = SRC[k][sb], c = SRC[k][sa + P], d = SRC[k][sb + P];
          pf32x2 v0, v1, dx, dy;
          samp_pair<false>(pf32x2{a.x, a.y}, pf32x2{b.x, b.y}, pf32x2{c.x, c.y}, pf32x2{d.x, d.y}, ax, ay[k], v0, dx, dy);
          samp_pair<false>(pf32x2{a.z, a.w}, pf32x2{b.z, b.w}, pf32x2{c.z, c.w}, pf32x2{d.z, d.w}, ax, ay[k], v1, dx, dy);
          sv[k][0] = v0.x;
          sv[k][1] = v0.y;
          sv[k][2] = v1.x;
          sv[k][3] = v1.y;
        }
        const float bg3[3] = {bq[0][q], bq[1][q], bq[2][q]};
        float m[K + 1];
        blend<K>(sv, bg3, o[q], m);
      }
      float* of = out.frame(ccur.f) + p;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        *reinterpret_cast<float4*>(of + ch * HW) = make_float4(o[0][ch], o[1][ch], o[2][ch], o[3][ch]);
        if (has_t) {
          float tv[4];
          TView::val4<T8>(tn[ch], tv);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float d = tv[q] - o[q][ch];
            acc = fmaf(d, d, acc);
          }
        }
      }
    }
    if (has_t) {
      acc = wave_sum_dpp(acc);
      if (lane == 0) RED[sl][wv] = acc;
    }
    cprev = ccur;
    ccur = c1;
    c1 = c2;
    if (it + 3 < nf) c2 = FR.next(c2);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) tn[ch] = tq[ch];
    __syncthreads();
  }
  if (has_t && tid == 0) {
    float a = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) a += RED[(nf - 1) & 1][w];
    sse[cprev.f] = a;
  }
}

template <int K, int H, bool T8>
__global__ void __launch_bounds__((DecFw<K, H>::NT))
dec_fwd_cu_k(PosView pos, Src S, FViewW out, TView tgt, float* __restrict__ sse, int F, int FPB) {
  dec_fwd_cu_body<K, H, T8>(pos, S, out, tgt, sse, F, FPB, blockIdx.x);
}

// The physics rollout (rollout.hip's forward, one thread per sequence) and
// the reconstruction decode in ONE launch: the two are independent (both
// follow the position head and the velocity MLP), and the rollout's few
// latency-bound threads would otherwise hold the whole GPU for its 46 x 5
// serial substeps.  Blocks 0 .. nr-1 roll out NT sequences each; the others
// run the decode exactly as dec_fwd_cu_k (block bid - nr).
struct RollArgs {
  const float* pos0;
  long long ld;
  const float* vel0;
  PhysPtr Q;
  float* pvs;
  int B, R;
};
template <int K, int H, int D, int CELL>
__global__ void __launch_bounds__((DecFw<K, H>::NT))
dec_fwd_roll_k(RollArgs ra, int nr, PosView pos, Src S, FViewW out, TView tgt, float* __restrict__ sse, int F, int FPB) {
  if ((int)blockIdx.x < nr) {   // block-uniform
    // the rollout's serial chain shares its SIMD with decode waves: it issues
    // first, so the launch's length stays the decode's, not a slowed rollout's
    __builtin_amdgcn_s_setprio(3);
    const int b = (int)blockIdx.x * DecFw<K, H>::NT + (int)threadIdx.x;
    if (b < ra.B) rollout_fwd_seq<D, CELL>(ra.pos0, ra.ld, ra.vel0, ra.Q, ra.pvs, ra.B, ra.R, b);
    return;
  }
  dec_fwd_cu_body<K, H, false>(pos, S, out, tgt, sse, F, FPB, (int)blockIdx.x - nr);
}

template <int K>
static int dec_launch_fwd(PosView pv, Src S, FViewW out, TView tgt, float* sse, int F, int h, int H, hipStream_t st) {
  const int lds = (K * h * h * 4) * 4;
  int g = (F + 1) / 2 < 1024 ? (F + 1) / 2 : 1024;   // >= 2 frames per block: source staging amortised
  // the one-barrier-per-frame kernel: 16-byte accesses need 16-byte aligned
  // frames (4-byte aligned ones for byte targets)
  const uintptr_t tb = tgt.p8 ? (uintptr_t)tgt.p8 : (uintptr_t)tgt.p;
  const int ta = tgt.p8 ? 4 : 16;
  const bool al = ((uintptr_t)out.p | (uintptr_t)S.bg) % 16 == 0 && out.fs % 4 == 0 &&
                  (sse == nullptr || (tb % ta == 0 && tgt.fs % 4 == 0 && tgt.gs % 4 == 0));
  const bool cu = al && H == 2 * h && ((K == 2 && (H == 32 || H == 64)) || (K == 3 && H == 36));
  PAIG_REQUIRE(cu || !tgt.p8 || sse == nullptr,
               "decoder_fwd: byte targets need the one-CU kernel (K=%d H=%d, 4-byte aligned frames)", K, H);
  const FView tf{tgt.p, tgt.fs, tgt.gs, tgt.grp};   // (the fp32 fallbacks)
  if (cu) {
    const int fpb = cdiv(F, g);
    g = cdiv(F, fpb);
    auto launch = [&](auto t8) {
      constexpr bool T8 = decltype(t8)::value;
      if constexpr (K == 2) {
        if (H == 64)
          hipLaunchKernelGGL((dec_fwd_cu_k<2, 64, T8>), dim3(g), dim3(DecFw<2, 64>::NT), 0, st, pv, S, out, tgt, sse, F,
                             fpb);
        else
          hipLaunchKernelGGL((dec_fwd_cu_k<2, 32, T8>), dim3(g), dim3(DecFw<2, 32>::NT), 0, st, pv, S, out, tgt, sse, F,
                             fpb);
      } else
        hipLaunchKernelGGL((dec_fwd_cu_k<3, 36, T8>), dim3(g), dim3(DecFw<3, 36>::NT), 0, st, pv, S, out, tgt, sse, F,
                           fpb);
    };
    if (tgt.p8 && sse) launch(std::true_type{});
    else launch(std::false_type{});
    PAIG_CHECK_LAUNCH();
    return 0;
  }
  if constexpr (K == 2) {
    if (H == 32) {
      hipLaunchKernelGGL((dec_fwd_reg_k<2, 32>), dim3(g), dim3(256), lds, st, pv, S, out, tf, sse, F);
      PAIG_CHECK_LAUNCH();
      return 0;
    }
  }
  if constexpr (K == 3) {
    if (H == 36) {
      hipLaunchKernelGGL((dec_fwd_reg_k<3, 36>), dim3(g), dim3(256), lds, st, pv, S, out, tf, sse, F);
      PAIG_CHECK_LAUNCH();
      return 0;
    }
  }
    hipLaunchKernelGGL((dec_fwd_k<K>), dim3(g), dim3(256), lds, st, pv, S, out, tf, sse, F, h, H);
  PAIG_CHECK_LAUNCH();
  return 0;
}

// The reference decoder's intermediate per-object tensors (attributes
// transf_contents / transf_masks, physics_models.py:186-196): for every frame
// the K warped contents sigmoid(content_k) o warp_k, the tiled background, and
// the K+1 compositing masks (softmax over [template_k o warp_k, 1]), each
// [F][3][H][W] (the mask is the same on the 3 channels, as the reference's
// 3-channel template makes it).  Off the hot path: computed on request.
template <int K>
__global__ void __launch_bounds__(256)
dec_parts_k(PosView pos, Src S, float* __restrict__ contents, float* __restrict__ masks, int F, int h, int H) {
  pos.load();
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int hh = h * h, HW = H * H;
  float* T = lds;
  float* Cn = T + K * hh;
  __shared__ float cx[K][MAXH], cy[K][MAXH];
  __shared__ double bc[MAXH];
  init_base(bc, H);
  stage_sources<K>(S, h, T, Cn);
  const long long plane = (long long)F * 3 * HW;   // one [F][3][H][W] tensor
  for (int f = blockIdx.x; f < F; f += gridDim.x) {
    __syncthreads();
    coord_tables<K>(pos, f, H, h, cx, cy, bc);
    __syncthreads();
    for (int p = threadIdx.x; p < HW; p += blockDim.x) {
      const int i = p / H, j = p % H;
      Bil bl[K];
#pragma unroll
      for (int k = 0; k < K; ++k) bl[k] = bil(cx[k][j], cy[k][i]);
      float o[3], m[K + 1], cs[K][3];
      composite<K>(T, Cn, S.bg, HW, p, h, bl, o, m, cs);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const long long at = ((long long)f * 3 + c) * HW + p;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          contents[k * plane + at] = cs[k][c];
          masks[k * plane + at] = m[k];
        }
        contents[K * plane + at] = S.bg[c * HW + p];
        masks[K * plane + at] = m[K];
      }
    }
  }
}

// General affine spatial transformer (stn(), nn/network/stn.py:5-16: aten
// affine_grid + grid_sample, bilinear, zeros padding, align_corners=False)
// for any theta [N][2][3]: U [N][C][Hi][Wi] -> O [N][C][Ho][Wo].  The grid is
// formed in theta's precision T, as affine_grid does (fp64 for the fp64
// physics-derived thetas, Q9), and cast to fp32 before sampling (the
// reference's grid.float()); the theta gradient sums in T (affine_grid's
// backward), from fp32 grid gradients.
template <typename T>
__device__ __forceinline__ T ag_base(int j, int n) {   // affine_grid linspace * (n-1)/n
  const T step = T(2) / (T)(n - 1 > 0 ? n - 1 : 1);
  const T v = n == 1 ? T(0) : ((j < n / 2) ? T(-1) + step * (T)j : T(1) - step * (T)(n - 1 - j));
  return v * (T)(n - 1) / (T)n;
}

template <typename T>
__global__ void __launch_bounds__(256)
stn_fwd_k(const float* __restrict__ U, const T* __restrict__ th, float* __restrict__ O, int N, int C, int Hi, int Wi,
          int Ho, int Wo) {
  const long long total = (long long)N * Ho * Wo;
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const int n = (int)(t / (Ho * Wo)), p = (int)(t % (Ho * Wo)), i = p / Wo, j = p % Wo;
    const T* a = th + n * 6;
    const T xb = ag_base<T>(j, Wo), yb = ag_base<T>(i, Ho);
    const float gx = (float)(a[0] * xb + a[1] * yb + a[2]), gy = (float)(a[3] * xb + a[4] * yb + a[5]);
    const float ix = ((gx + 1.f) * (float)Wi - 1.f) * 0.5f, iy = ((gy + 1.f) * (float)Hi - 1.f) * 0.5f;
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    const int x0 = (int)fx0, y0 = (int)fy0;
    const float fx = ix - fx0, fy = iy - fy0;
    const float w[4] = {(1.f - fx) * (1.f - fy), fx * (1.f - fy), (1.f - fx) * fy, fx * fy};
    const int xs[4] = {x0, x0 + 1, x0, x0 + 1}, ys[4] = {y0, y0, y0 + 1, y0 + 1};
    for (int c = 0; c < C; ++c) {
      const float* u = U + ((long long)n * C + c) * Hi * Wi;
      float v = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (xs[q] >= 0 && xs[q] < Wi && ys[q] >= 0 && ys[q] < Hi) v += w[q] * u[ys[q] * Wi + xs[q]];
      O[((long long)n * C + c) * Ho * Wo + p] = v;
    }
  }
}

// backward: dU by atomics (scatter of the bilinear weights; this general
// helper is off the training path), dtheta per sample by a block reduction
// (one block per sample, deterministic)
template <typename T>
__global__ void __launch_bounds__(256)
stn_bwd_k(const float* __restrict__ U, const T* __restrict__ th, const float* __restrict__ dO, float* __restrict__ dU,
          T* __restrict__ dth, int N, int C, int Hi, int Wi, int Ho, int Wo) {
  const int n = blockIdx.x;
  const T* a = th + n * 6;
  T acc[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
  for (int p = threadIdx.x; p < Ho * Wo; p += blockDim.x) {
    const int i = p / Wo, j = p % Wo;
    const T xb = ag_base<T>(j, Wo), yb = ag_base<T>(i, Ho);
    const float gx = (float)(a[0] * xb + a[1] * yb + a[2]), gy = (float)(a[3] * xb + a[4] * yb + a[5]);
    const float ix = ((gx + 1.f) * (float)Wi - 1.f) * 0.5f, iy = ((gy + 1.f) * (float)Hi - 1.f) * 0.5f;
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    const int x0 = (int)fx0, y0 = (int)fy0;
    const float fx = ix - fx0, fy = iy - fy0;
    float dix = 0.f, diy = 0.f;
    for (int c = 0; c < C; ++c) {
      const float* u = U + ((long long)n * C + c) * Hi * Wi;
      float* du = dU ? dU + ((long long)n * C + c) * Hi * Wi : nullptr;
      const float g = dO[((long long)n * C + c) * Ho * Wo + p];
      auto tapv = [&](int y, int x) { return (x >= 0 && x < Wi && y >= 0 && y < Hi) ? u[y * Wi + x] : 0.f; };
      const float nw = tapv(y0, x0), ne = tapv(y0, x0 + 1), sw = tapv(y0 + 1, x0), se = tapv(y0 + 1, x0 + 1);
      dix += g * ((ne - nw) * (1.f - fy) + (se - sw) * fy);
      diy += g * ((sw - nw) * (1.f - fx) + (se - ne) * fx);
      if (du) {
        const float w[4] = {(1.f - fx) * (1.f - fy), fx * (1.f - fy), (1.f - fx) * fy, fx * fy};
        const int xs[4] = {x0, x0 + 1, x0, x0 + 1}, ys[4] = {y0, y0, y0 + 1, y0 + 1};
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (xs[q] >= 0 && xs[q] < Wi && ys[q] >= 0 && ys[q] < Hi) atomicAdd(du + ys[q] * Wi + xs[q], g * w[q]);
      }
    }
    // ix = ((gx + 1) Wi - 1) / 2 -> dgx = dix * Wi / 2 (fp32, grid_sample's
    // grid gradient); gx = a0 xb + a1 yb + a2 in T
    const T dgx = (T)(dix * (float)Wi * 0.5f), dgy = (T)(diy * (float)Hi * 0.5f);
    acc[0] += dgx * xb;
    acc[1] += dgx * yb;
    acc[2] += dgx;
    acc[3] += dgy * xb;
    acc[4] += dgy * yb;
    acc[5] += dgy;
  }
  __shared__ T red[4][6];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    T v = acc[q];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) red[wv][q] = v;
  }
  __syncthreads();
  if (threadIdx.x < 6 && dth) {
    T v = T(0);
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) v += red[w][threadIdx.x];
    dth[n * 6 + threadIdx.x] = v;
  }
}

// The learnable attention-window scale (the reference's commented-out
// trainable logsigma, physics_models.py:155-161): sigma = exp(ln 2 tanh(u))
// from the fp32 parameter u, in fp64 -- strictly inside (0.5, 2), 1 at u = 0.
constexpr double LN2 = 0.6931471805599453;   // np.log(2.0)

__global__ void sigma_from_u_k(const float* __restrict__ u, double* __restrict__ sg) {
  if (threadIdx.x == 0) *sg = exp(LN2 * tanh((double)*u));
}

// dL/du = (sum of both decoders' per-frame dL/dsigma, fixed order, fp64) *
// d sigma / du = ln 2 sigma (1 - tanh(u)^2), rounded to fp32 into u's
// gradient slot (accumulate: added to it)
__global__ void __launch_bounds__(256)
sigma_grad_k(const double* __restrict__ a, int na, const double* __restrict__ b, int nb, const float* __restrict__ u,
             float* __restrict__ gu, int accumulate) {
  __shared__ double red[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < na; i += 256) s += a[i];
  for (int i = threadIdx.x; i < nb; i += 256) s += b[i];
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double tot = (red[0] + red[1]) + (red[2] + red[3]);
    const double t = tanh((double)*u), sg = exp(LN2 * t);
    const float g = (float)(tot * (LN2 * sg * (1.0 - t * t)));
    *gu = accumulate ? *gu + g : g;
  }
}

}  // namespace

// ---- host side: every decision of a decoder call is made once here.  The
// sigma operand (DecSigma), the target and loss-weight operands (dec_tview /
// dec_wsrc, which own their preconditions), the kernels' <T8, LW> choice
// (dec_t8_lw) and the backward's launch geometry (dec_bwd_plan: what the size
// queries report is what the launch writes).  The exported variants are thin
// forwards onto dec_fwd / dec_fwd_rollout / dec_bwd / dec_parts.

#define DEC_TRY(call)           \
  do {                          \
    if (int rc_ = (call)) return rc_; \
  } while (0)

// The attention-window scale of one call (physics_models.py:155-162): a host
// value in [0.5, 2] (no clamping outside), or -- the *_sigma_dev entry points:
// the learnable scale, which the host never sees -- one double the kernels
// read from device memory (host is then an unused 1.0).
struct DecSigma {
  double host;
  const double* dev;
  bool on_dev;
  static DecSigma of(double sigma) { return {sigma, nullptr, false}; }
  static DecSigma at(const double* sigma_dev) { return {1.0, sigma_dev, true}; }
};

static int dec_sigma_check(const char* who, const DecSigma& sg) {
  PAIG_REQUIRE(!sg.on_dev || sg.dev, "%s: a device sigma is required", who);
  PAIG_REQUIRE(sg.on_dev || (sg.host >= 0.5 && sg.host <= 2.0), "%s: sigma=%g outside [0.5, 2]", who, sg.host);
  return 0;
}

static PosView dec_pos(const float* pos, long long outer, long long inner, int grp, const DecSigma& sg) {
  return PosView{pos, outer, inner, grp, sg.host, (float)sg.host, sg.dev};
}

// The target forms an entry point takes; dec_tview finishes the view an
// export filled with its raw arguments.  sse_ok: no forward without an SSE
// output (the backward passes true).
enum DecTgtForm { DEC_TGT_F32, DEC_TGT_U8, DEC_TGT_EITHER };

static int dec_tview(const char* who, DecTgtForm form, TView& t, bool sse_ok) {
  PAIG_REQUIRE(form != DEC_TGT_EITHER || !t.p != !t.p8, "%s: exactly one of the fp32 / byte targets", who);
  PAIG_REQUIRE(form != DEC_TGT_U8 || t.p8, "%s: byte targets are required", who);
  PAIG_REQUIRE(!t.ix || t.grp > 0, "%s: a row index needs grouped targets", who);
  PAIG_REQUIRE(!t.p8 || sse_ok, "%s: byte targets need an SSE output", who);
  if (!t.p8) t.ix = nullptr;
  return 0;
}

// The backward's loss weights: the array (mode 0) or the loss adjoints
// (mode 1: reconstruction frames, 2: rollout frames, grouped by R).
static int dec_wsrc(const char* who, WSrc& w, int pos_grp, int F) {
  PAIG_REQUIRE(w.mode >= 0 && w.mode <= 2 && (w.mode == 0 || (w.B > 0 && w.Te > 0 && w.R > 0)),
               "%s: loss-weight mode %d", who, w.mode);
  PAIG_REQUIRE(w.mode != 0 || !w.dt, "%s: loss adjoints given with lw_mode 0", who);
  PAIG_REQUIRE(w.mode != 2 || (pos_grp == w.R && F % w.R == 0), "%s: rollout weights need frames grouped by R=%d", who,
               w.R);
  if (w.mode != 0) w.a = nullptr;
  return 0;
}

// fn(T8, LW) with the runtime (byte targets, in-kernel weights) pair as the
// kernels' template arguments
template <typename Fn>
static void dec_t8_lw(bool t8, bool lw, Fn&& fn) {
  auto with = [&](auto LW) {
    if (t8) fn(std::true_type{}, LW);
    else fn(std::false_type{}, LW);
  };
  if (lw) with(std::true_type{});
  else with(std::false_type{});
}

// The one-CU-per-block kernels' shapes (the generic kernels otherwise).
static bool dec_cu_shape(int K, int h, int H) {
  return H == 2 * h && ((K == 2 && (H == 32 || H == 64)) || (K == 3 && H == 36));
}

// frames per block of the one-CU kernel: >= DEC_FPB_MIN (the slab row of a
// block is ~1.7 frames of targets), at most DEC_CU_MAX_BLOCKS blocks
static int dec_cu_fpb(int NL) {
  static int fmin = -1;
  if (fmin < 0) {   // A/B: PAIG_DEC_FPB_MIN
    const char* e = getenv("PAIG_DEC_FPB_MIN");
    fmin = e ? atoi(e) : DEC_FPB_MIN;
    if (fmin < 1) fmin = 1;
  }
  int fpb = cdiv(NL, DEC_CU_MAX_BLOCKS);
  return fpb < fmin ? fmin : fpb;
}

// The backward's launch over F frames grouped by grp (0: ungrouped) of which
// the first `live` per group carry a loss weight (0: all).  The only place
// this arithmetic exists: the paig_decoder_bwd_blocks* / _bwd_scratch* queries
// report it and dec_bwd launches it.
struct DecBwdPlan {
  bool cu;          // the one-CU kernels, else the generic ones
  int rows;         // blocks = slab rows
  int fpb;          // (one-CU) frames per block
  int live;         // the kernels' live argument
  size_t scratch;   // (generic) floats of global scratch: the per-frame pixel-gradient image when it does not fit LDS
  int lds;          // (generic) dynamic LDS bytes
};

static DecBwdPlan dec_bwd_plan(int F, int grp, int live, int K, int h, int H, const DecSigma& sg) {
  // The one-CU kernels' 5-wide gather tables bound the window for sigma >= 1
  // (<= 4 / sigma + 1 output indices per source texel and axis); below that
  // (up to 9) the generic kernels take the one-CU shapes too, as they do for
  // a device sigma, which the host cannot choose a kernel by.
  if (!sg.on_dev && sg.host >= 1.0 && dec_cu_shape(K, h, H)) {
    // the live frames only; the dead ones of every group are skipped
    const int NL = (grp > 0 && live > 0 && live < grp) ? (F / grp) * live : F;
    const int n = NL > 0 ? NL : 1, fpb = dec_cu_fpb(n);
    return {true, cdiv(n, fpb), fpb, NL == F ? 0 : live, 0, 0};
  }
  // generic: every frame is walked (dead ones skipped by their step or zero
  // weight), two per block up to ~3 blocks per CU (latency hiding for the
  // per-frame passes)
  const int g = F <= 0 ? 1 : (F + 1) / 2 < 768 ? (F + 1) / 2 : 768;
  const size_t src = (size_t)K * h * h * 4, img = (size_t)K * 4 * H * H;
  if ((src + img) * 4 <= 120 * 1024) return {false, g, 0, live, 0, (int)((src + img) * 4)};
  return {false, g, 0, live, g * img, (int)(src * 4)};
}

static int dec_fwd(const float* pos, long long pos_outer, long long pos_inner, int pos_grp, const float* tmpl,
                   const float* cont, const float* bg, float* out, long long out_fs, DecTgtForm form, TView t,
                   float* sse, int F, int K, int h, int H, const DecSigma& sg, void* stream) {
  DEC_TRY(dec_sigma_check("decoder_fwd", sg));
  DEC_TRY(dec_tview("decoder_fwd", form, t, sse != nullptr));
  if (F <= 0) return 0;
  PAIG_REQUIRE(H == 2 * h, "decoder: H=%d must be 2*tmpl=%d", H, 2 * h);
  const PosView pv = dec_pos(pos, pos_outer, pos_inner, pos_grp, sg);
  Src S{tmpl, cont, bg};
  FViewW o{out, out_fs};
  hipStream_t st = (hipStream_t)stream;
  if (K == 2) return dec_launch_fwd<2>(pv, S, o, t, sse, F, h, H, st);
  if (K == 3) return dec_launch_fwd<3>(pv, S, o, t, sse, F, h, H, st);
  paig_set_error("decoder: unsupported n_objs %d", K);
  return PAIG_E_UNSUPPORTED;
}

// dsig (with a device sigma only): dL/dsigma [F]
static int dec_bwd(const float* pos, long long pos_outer, long long pos_inner, int pos_grp, const float* tmpl,
                   const float* cont, const float* bg, DecTgtForm form, TView t, WSrc dsse, const float* dout,
                   long long dout_fs, float* dpos, float* slab, float* scratch, int F, int live, int K, int h, int H,
                   const DecSigma& sg, double* dsig, void* stream) {
  DEC_TRY(dec_sigma_check("decoder_bwd", sg));
  PAIG_REQUIRE(sg.on_dev || !dsig, "decoder_bwd: dL/dsigma needs a device-resident sigma");
  DEC_TRY(dec_tview("decoder_bwd", form, t, true));
  DEC_TRY(dec_wsrc("decoder_bwd", dsse, pos_grp, F));
  if (F <= 0) return 0;
  PAIG_REQUIRE(H == 2 * h, "decoder: H=%d must be 2*tmpl=%d", H, 2 * h);
  PAIG_REQUIRE(live >= 0 && (live == 0 || pos_grp > 0), "decoder_bwd: live=%d needs grouped frames (pos_grp=%d)", live,
               pos_grp);
  PAIG_REQUIRE(pos_grp <= 0 || F % pos_grp == 0, "decoder_bwd: F=%d is not a multiple of the group %d", F, pos_grp);
  PAIG_REQUIRE(pos_grp <= 0 || t.grp == pos_grp || live == 0,
               "decoder_bwd: target group %d must equal the position group %d", t.grp, pos_grp);
  // live > 0 promises that the frames past `live` in every group carry a zero
  // SSE weight and no dense gradient: the one-CU kernels skip them, the
  // generic ones walk them (zero contribution), so both give the same result
  PAIG_REQUIRE(live == 0 || dout == nullptr, "decoder_bwd: live=%d with a dense dL/dout (dead frames would be skipped)",
               live);
  const PosView pv = dec_pos(pos, pos_outer, pos_inner, pos_grp, sg);
  Src S{tmpl, cont, bg};
  FView d{dout, dout_fs, 0, 0};
  hipStream_t st = (hipStream_t)stream;
  const DecBwdPlan pl = dec_bwd_plan(F, pos_grp, live, K, h, H, sg);
  const bool t8 = t.p8 && dsse.on(), lw = dsse.mode != 0;
  if (pl.cu) {
    dec_t8_lw(t8, lw, [&](auto t8c, auto lwc) {
      constexpr bool T8 = decltype(t8c)::value, LW = decltype(lwc)::value;
      if (K == 2 && H == 64)
        hipLaunchKernelGGL((dec_bwd_band_k<2, 64, T8, LW>), dim3(pl.rows), dim3(DecBand<2, 64>::NT), 0, st, pv, S, t,
                           dsse, d, dpos, slab, F, pl.live, pl.fpb);
      else if (K == 2)
        hipLaunchKernelGGL((dec_bwd_cu_k<2, 32, T8, LW>), dim3(pl.rows), dim3(DecCu<2, 32>::NT), 0, st, pv, S, t, dsse, d,
                           dpos, slab, F, pl.live, pl.fpb);
      else
        hipLaunchKernelGGL((dec_bwd_cu_k<3, 36, T8, LW>), dim3(pl.rows), dim3(DecCu<3, 36>::NT), 0, st, pv, S, t, dsse, d,
                           dpos, slab, F, pl.live, pl.fpb);
    });
    PAIG_CHECK_LAUNCH();
    return 0;
  }
  // byte targets and in-kernel loss weights: the one-CU shapes (at sigma < 1
  // through the generic kernels)
  PAIG_REQUIRE(!t.p8 || dec_cu_shape(K, h, H), "decoder_bwd: byte targets need the one-CU kernels (K=%d H=%d)", K, H);
  PAIG_REQUIRE(!lw || dec_cu_shape(K, h, H), "decoder_bwd: in-kernel loss weights need the one-CU kernels (K=%d H=%d)",
               K, H);
  PAIG_REQUIRE(!pl.scratch || scratch, "decoder_bwd: scratch required");
  float* gs = pl.scratch ? scratch : nullptr;
  if (K != 2 && K != 3) {
    paig_set_error("decoder: unsupported n_objs %d", K);
    return PAIG_E_UNSUPPORTED;
  }
  dec_t8_lw(t8, lw, [&](auto t8c, auto lwc) {
    constexpr bool T8 = decltype(t8c)::value, LW = decltype(lwc)::value;
    auto go = [&](auto kern) {
      if (pl.lds > 64 * 1024)
        (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, pl.lds);
      hipLaunchKernelGGL(kern, dim3(pl.rows), dim3(256), pl.lds, st, pv, S, t, dsse, d, dpos, slab, gs, dsig, F, pl.live,
                         h, H);
    };
    if (K == 2) go(dec_bwd_k<2, T8, LW>);
    else go(dec_bwd_k<3, T8, LW>);
  });
  PAIG_CHECK_LAUNCH();
  return 0;
}

// The rollout (paig_rollout_fwd's arguments) and the reconstruction decode
// (paig_decoder_fwd's, fp32 targets and an SSE output) in one launch, where
// the one-CU decoder serves the shape: (K, H) in {(2, 32), (3, 36), (2, 64)}
// with 16-byte aligned frames; the cell / D pairs of paig_rollout_fwd.
static int dec_fwd_rollout(int cell, const float* pos0, long long pos0_ld, const float* vel0, const float* dt,
                           const double* p0, const double* p1, float* pvs, int B, int D, int R, const float* pos,
                           long long pos_outer, long long pos_inner, int pos_grp, const float* tmpl, const float* cont,
                           const float* bg, float* out, long long out_fs, const float* tgt, long long tgt_fs,
                           int tgt_grp, long long tgt_gs, float* sse, int F, int K, int h, int H, const DecSigma& sg,
                           void* stream) {
  DEC_TRY(dec_sigma_check("decoder_fwd_rollout", sg));
  PAIG_REQUIRE(B > 0 && F > 0 && R > 0, "decoder_fwd_rollout: B=%d F=%d R=%d", B, F, R);
  PAIG_REQUIRE(cell == 1 || (p0 && p1), "decoder_fwd_rollout: physics params required");
  PAIG_REQUIRE(H == 2 * h && sse && tgt, "decoder_fwd_rollout: H=%d tmpl=%d, targets and an SSE output required", H, h);
  const bool al = ((uintptr_t)out | (uintptr_t)bg | (uintptr_t)tgt) % 16 == 0 && out_fs % 4 == 0 && tgt_fs % 4 == 0 &&
                  tgt_gs % 4 == 0;
  PAIG_REQUIRE(al, "decoder_fwd_rollout: 16-byte aligned frames required");
  const PosView pv = dec_pos(pos, pos_outer, pos_inner, pos_grp, sg);
  Src S{tmpl, cont, bg};
  FViewW o{out, out_fs};
  TView t{tgt, nullptr, nullptr, tgt_fs, tgt_gs, tgt_grp};
  RollArgs ra{pos0, pos0_ld, vel0, PhysPtr{dt, p0, p1}, pvs, B, R};
  hipStream_t st = (hipStream_t)stream;
  auto launch = [&](auto kern, int nt) {
    // the decode's blocks exactly as paig_decoder_fwd (<= 1024: four per CU,
    // one round).  Where they fill that round the rollout's blocks push
    // decode blocks into a second one: callers merge only while
    // min((F + 1) / 2, 1024) + ceil(B / NT) <= 1024 (measured: B = 512 and
    // 1024 lose 0.4-0.6% merged, with the decode's grid capped or not)
    const int nr = cdiv(B, nt);
    int g = (F + 1) / 2 < 1024 ? (F + 1) / 2 : 1024;
    const int fpb = cdiv(F, g);
    g = cdiv(F, fpb);
    hipLaunchKernelGGL(kern, dim3(nr + g), dim3(nt), 0, st, ra, nr, pv, S, o, t, sse, F, fpb);
    return 0;
  };
  int rc = -1;
  if (K == 2 && H == 32 && D == 4 && cell == 0) rc = launch(dec_fwd_roll_k<2, 32, 4, CELL_SPRING>, DecFw<2, 32>::NT);
  else if (K == 2 && H == 32 && D == 4 && cell == 1) rc = launch(dec_fwd_roll_k<2, 32, 4, CELL_BOUNCE>, DecFw<2, 32>::NT);
  else if (K == 3 && H == 36 && D == 6 && cell == 2) rc = launch(dec_fwd_roll_k<3, 36, 6, CELL_GRAVITY>, DecFw<3, 36>::NT);
  else if (K == 2 && H == 64 && D == 4 && cell == 0) rc = launch(dec_fwd_roll_k<2, 64, 4, CELL_SPRING>, DecFw<2, 64>::NT);
  if (rc < 0) {
    paig_set_error("decoder_fwd_rollout: unsupported (K=%d, H=%d, cell %d, D=%d)", K, H, cell, D);
    return PAIG_E_UNSUPPORTED;
  }
  PAIG_CHECK_LAUNCH();
  return 0;
}

static int dec_parts(const float* pos, long long pos_inner, const float* tmpl, const float* cont, const float* bg,
                     float* contents, float* masks, int F, int K, int h, int H, const DecSigma& sg, void* stream) {
  DEC_TRY(dec_sigma_check("decoder_parts", sg));
  if (F <= 0) return 0;
  PAIG_REQUIRE(H == 2 * h && H <= MAXH, "decoder_parts: H=%d must be 2*tmpl=%d (<= %d)", H, 2 * h, MAXH);
  const PosView pv = dec_pos(pos, 0, pos_inner, 0, sg);
  Src S{tmpl, cont, bg};
  hipStream_t st = (hipStream_t)stream;
  const int g = F < 2048 ? F : 2048;
  const int lds = (K * h * h * 4) * 4;
  if (K == 2) hipLaunchKernelGGL((dec_parts_k<2>), dim3(g), dim3(256), lds, st, pv, S, contents, masks, F, h, H);
  else if (K == 3) hipLaunchKernelGGL((dec_parts_k<3>), dim3(g), dim3(256), lds, st, pv, S, contents, masks, F, h, H);
  else {
    paig_set_error("decoder_parts: unsupported n_objs %d", K);
    return PAIG_E_UNSUPPORTED;
  }
  PAIG_CHECK_LAUNCH();
  return 0;
}

// ---- the C ABI.  Per operation: the *_sigma entry point takes the window
// scale (double sigma, in [0.5, 2]: theta0 = theta4 = sigma in fp64, theta2 /
// theta5 scaled by fl32(sigma) in fp32, physics_models.py:160-167), the
// *_sigma_dev one reads it from device memory (const double* sigma_dev, one
// element), and the one without a suffix means sigma = 1.
#define DEC_POS_P const float *pos, long long pos_outer, long long pos_inner, int pos_grp
#define DEC_POS pos, pos_outer, pos_inner, pos_grp
#define DEC_SRC_P const float *tmpl, const float *cont, const float *bg
#define DEC_SRC tmpl, cont, bg
#define DEC_TGT_P long long tgt_fs, int tgt_grp, long long tgt_gs
#define DEC_F32 DEC_TGT_F32, TView{tgt, nullptr, nullptr, tgt_fs, tgt_gs, tgt_grp}
#define DEC_U8 DEC_TGT_U8, TView{nullptr, tgt, tgt_idx, tgt_fs, tgt_gs, tgt_grp}
#define DEC_DIMS_P int F, int K, int h, int H
#define DEC_DIMS F, K, h, H

extern "C" {

// Slab rows (= blocks) and global scratch (floats; 0 when the per-frame
// pixel-gradient image fits LDS) of the backward: dec_bwd_plan.  A device
// sigma: always the generic backward (every frame walked).
int paig_decoder_bwd_blocks_sigma(int F, int grp, int live, int K, int h, int H, double sigma) {
  return dec_bwd_plan(F, grp, live, K, h, H, DecSigma::of(sigma)).rows;
}
int paig_decoder_bwd_blocks_sigma_dev(DEC_DIMS_P) { return dec_bwd_plan(F, 0, 0, K, h, H, DecSigma::at(nullptr)).rows; }
int paig_decoder_bwd_blocks(int F, int grp, int live, int K, int h, int H) {
  return paig_decoder_bwd_blocks_sigma(F, grp, live, K, h, H, 1.0);
}
size_t paig_decoder_bwd_scratch_sigma(DEC_DIMS_P, double sigma) {
  return dec_bwd_plan(F, 0, 0, K, h, H, DecSigma::of(sigma)).scratch;
}
size_t paig_decoder_bwd_scratch_sigma_dev(DEC_DIMS_P) {
  return dec_bwd_plan(F, 0, 0, K, h, H, DecSigma::at(nullptr)).scratch;
}
size_t paig_decoder_bwd_scratch(DEC_DIMS_P) { return paig_decoder_bwd_scratch_sigma(DEC_DIMS, 1.0); }
size_t paig_decoder_slab_len(int K, int h, int H) { return (size_t)K * h * h * 4 + 3 * (size_t)H * H; }

int paig_decoder_fwd_sigma(DEC_POS_P, DEC_SRC_P, float* out, long long out_fs, const float* tgt, DEC_TGT_P, float* sse,
                           DEC_DIMS_P, double sigma, void* stream) {
  return dec_fwd(DEC_POS, DEC_SRC, out, out_fs, DEC_F32, sse, DEC_DIMS, DecSigma::of(sigma), stream);
}
int paig_decoder_fwd_sigma_dev(DEC_POS_P, DEC_SRC_P, float* out, long long out_fs, const float* tgt, DEC_TGT_P,
                               float* sse, DEC_DIMS_P, const double* sigma_dev, void* stream) {
  return dec_fwd(DEC_POS, DEC_SRC, out, out_fs, DEC_F32, sse, DEC_DIMS, DecSigma::at(sigma_dev), stream);
}
int paig_decoder_fwd(DEC_POS_P, DEC_SRC_P, float* out, long long out_fs, const float* tgt, DEC_TGT_P, float* sse,
                     DEC_DIMS_P, void* stream) {
  return dec_fwd(DEC_POS, DEC_SRC, out, out_fs, DEC_F32, sse, DEC_DIMS, DecSigma::of(1.0), stream);
}

// byte targets (the dataset's rows behind tgt_idx) and an SSE output
int paig_decoder_fwd_t8_sigma(DEC_POS_P, DEC_SRC_P, float* out, long long out_fs, const unsigned char* tgt,
                              const long long* tgt_idx, DEC_TGT_P, float* sse, DEC_DIMS_P, double sigma, void* stream) {
  return dec_fwd(DEC_POS, DEC_SRC, out, out_fs, DEC_U8, sse, DEC_DIMS, DecSigma::of(sigma), stream);
}
int paig_decoder_fwd_t8_sigma_dev(DEC_POS_P, DEC_SRC_P, float* out, long long out_fs, const unsigned char* tgt,
                                  const long long* tgt_idx, DEC_TGT_P, float* sse, DEC_DIMS_P, const double* sigma_dev,
                                  void* stream) {
  return dec_fwd(DEC_POS, DEC_SRC, out, out_fs, DEC_U8, sse, DEC_DIMS, DecSigma::at(sigma_dev), stream);
}
int paig_decoder_fwd_t8(DEC_POS_P, DEC_SRC_P, float* out, long long out_fs, const unsigned char* tgt,
                        const long long* tgt_idx, DEC_TGT_P, float* sse, DEC_DIMS_P, void* stream) {
  return dec_fwd(DEC_POS, DEC_SRC, out, out_fs, DEC_U8, sse, DEC_DIMS, DecSigma::of(1.0), stream);
}

#define DEC_ROLL_P                                                                                                  \
  int cell, const float *pos0, long long pos0_ld, const float *vel0, const float *dt, const double *p0,             \
      const double *p1, float *pvs, int B, int D, int R, DEC_POS_P, DEC_SRC_P, float *out, long long out_fs,        \
      const float *tgt, DEC_TGT_P, float *sse, DEC_DIMS_P
#define DEC_ROLL                                                                                                     \
  cell, pos0, pos0_ld, vel0, dt, p0, p1, pvs, B, D, R, DEC_POS, DEC_SRC, out, out_fs, tgt, tgt_fs, tgt_grp, tgt_gs, \
      sse, DEC_DIMS

int paig_decoder_fwd_rollout_sigma(DEC_ROLL_P, double sigma, void* stream) {
  return dec_fwd_rollout(DEC_ROLL, DecSigma::of(sigma), stream);
}
int paig_decoder_fwd_rollout_sigma_dev(DEC_ROLL_P, const double* sigma_dev, void* stream) {
  return dec_fwd_rollout(DEC_ROLL, DecSigma::at(sigma_dev), stream);
}
int paig_decoder_fwd_rollout(DEC_ROLL_P, void* stream) { return dec_fwd_rollout(DEC_ROLL, DecSigma::of(1.0), stream); }

// The backward with the weight array dsse: fp32 targets, or (_t8) bytes
#define DEC_BWD_OUT_P const float *dout, long long dout_fs, float *dpos, float *slab, float *scratch
#define DEC_BWD_OUT dout, dout_fs, dpos, slab, scratch
#define DEC_NO_LW WSrc{dsse, nullptr, nullptr, nullptr, 0.f, 0, 0, 0, 0, 0}

int paig_decoder_bwd(DEC_POS_P, DEC_SRC_P, const float* tgt, DEC_TGT_P, const float* dsse, DEC_BWD_OUT_P, int F,
                     int live, int K, int h, int H, void* stream) {
  return dec_bwd(DEC_POS, DEC_SRC, DEC_F32, DEC_NO_LW, DEC_BWD_OUT, F, live, K, h, H, DecSigma::of(1.0), nullptr, stream);
}
int paig_decoder_bwd_t8(DEC_POS_P, DEC_SRC_P, const unsigned char* tgt, const long long* tgt_idx, DEC_TGT_P,
                        const float* dsse, DEC_BWD_OUT_P, int F, int live, int K, int h, int H, void* stream) {
  return dec_bwd(DEC_POS, DEC_SRC, DEC_U8, DEC_NO_LW, DEC_BWD_OUT, F, live, K, h, H, DecSigma::of(1.0), nullptr, stream);
}

// The backward with either target form (tgt fp32, or tgt8 + tgt_idx bytes:
// exactly one non-null) and the loss weights read from dsse (lw_mode 0) or
// formed in-kernel from the loss adjoints dt / de / dr (lw_mode 1:
// reconstruction frames, 2: rollout frames; paig_loss_bwd's values, so no
// weight arrays and no paig_loss_bwd launch).  lw_mode != 0: the one-CU shapes.
// _sigma_dev: always the generic kernels, and dsig (nullable) [F]: every
// frame's dL/dsigma in fp64, 0.0 for the frames the launch skips (dead or
// weightless).  Slab rows / scratch: the matching _bwd_blocks* / _bwd_scratch*.
#define DEC_EX_P                                                                                                   \
  DEC_POS_P, DEC_SRC_P, const float *tgt, const unsigned char *tgt8, const long long *tgt_idx, DEC_TGT_P,          \
      const float *dsse, int lw_mode, const float *dt, const float *de, const float *dr, float ae, int lB, int lTe, \
      int lR, int lpred, DEC_BWD_OUT_P, int F, int live, int K, int h, int H
#define DEC_EX                                                                                                  \
  DEC_POS, DEC_SRC, DEC_TGT_EITHER, TView{tgt, tgt8, tgt_idx, tgt_fs, tgt_gs, tgt_grp},                         \
      WSrc{dsse, dt, de, dr, ae, lB, lTe, lR, lpred, lw_mode}, DEC_BWD_OUT, F, live, K, h, H

int paig_decoder_bwd_ex_sigma(DEC_EX_P, double sigma, void* stream) {
  return dec_bwd(DEC_EX, DecSigma::of(sigma), nullptr, stream);
}
int paig_decoder_bwd_ex_sigma_dev(DEC_EX_P, const double* sigma_dev, double* dsig, void* stream) {
  return dec_bwd(DEC_EX, DecSigma::at(sigma_dev), dsig, stream);
}
int paig_decoder_bwd_ex(DEC_EX_P, void* stream) { return dec_bwd(DEC_EX, DecSigma::of(1.0), nullptr, stream); }

int paig_decoder_parts_sigma(const float* pos, long long pos_inner, DEC_SRC_P, float* contents, float* masks, DEC_DIMS_P,
                             double sigma, void* stream) {
  return dec_parts(pos, pos_inner, DEC_SRC, contents, masks, DEC_DIMS, DecSigma::of(sigma), stream);
}
int paig_decoder_parts_sigma_dev(const float* pos, long long pos_inner, DEC_SRC_P, float* contents, float* masks,
                                 DEC_DIMS_P, const double* sigma_dev, void* stream) {
  return dec_parts(pos, pos_inner, DEC_SRC, contents, masks, DEC_DIMS, DecSigma::at(sigma_dev), stream);
}
int paig_decoder_parts(const float* pos, long long pos_inner, DEC_SRC_P, float* contents, float* masks, DEC_DIMS_P,
                       void* stream) {
  return dec_parts(pos, pos_inner, DEC_SRC, contents, masks, DEC_DIMS, DecSigma::of(1.0), stream);
}

int paig_sigma_from_u(const float* u, double* sigma_dev, void* stream) {
  PAIG_REQUIRE(u && sigma_dev, "sigma_from_u: null argument");
  hipLaunchKernelGGL(sigma_from_u_k, dim3(1), dim3(64), 0, (hipStream_t)stream, u, sigma_dev);
  PAIG_CHECK_LAUNCH();
  return 0;
}

int paig_sigma_grad(const double* dsig_a, int na, const double* dsig_b, int nb, const float* u, float* gu,
                    int accumulate, void* stream) {
  PAIG_REQUIRE(u && gu && na >= 0 && nb >= 0 && (na == 0 || dsig_a) && (nb == 0 || dsig_b), "sigma_grad: bad argument");
  hipLaunchKernelGGL(sigma_grad_k, dim3(1), dim3(256), 0, (hipStream_t)stream, dsig_a, na, dsig_b, nb, u, gu,
                     accumulate);
  PAIG_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

template <typename T>
static int stn_fwd(const float* U, const T* theta, float* out, int N, int C, int Hi, int Wi, int Ho, int Wo,
                   void* stream) {
  if (N <= 0) return 0;
  PAIG_REQUIRE(C > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0, "stn_fwd: bad shape");
  const long long total = (long long)N * Ho * Wo;
  const int g = (int)(total / 256 + 1 < 8192 ? total / 256 + 1 : 8192);
  hipLaunchKernelGGL(stn_fwd_k<T>, dim3(g), dim3(256), 0, (hipStream_t)stream, U, theta, out, N, C, Hi, Wi, Ho, Wo);
  PAIG_CHECK_LAUNCH();
  return 0;
}

template <typename T>
static int stn_bwd(const float* U, const T* theta, const float* dout, float* dU, T* dtheta, int N, int C, int Hi,
                   int Wi, int Ho, int Wo, void* stream) {
  if (N <= 0) return 0;
  PAIG_REQUIRE(C > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0, "stn_bwd: bad shape");
  hipLaunchKernelGGL(stn_bwd_k<T>, dim3(N), dim3(256), 0, (hipStream_t)stream, U, theta, dout, dU, dtheta, N, C, Hi,
                     Wi, Ho, Wo);
  PAIG_CHECK_LAUNCH();
  return 0;
}

extern "C" {


int paig_stn_fwd(const float* U, const float* theta, float* out, int N, int C, int Hi, int Wi, int Ho, int Wo,
                 void* stream) {
  return stn_fwd<float>(U, theta, out, N, C, Hi, Wi, Ho, Wo, stream);
}

int paig_stn_bwd(const float* U, const float* theta, const float* dout, float* dU, float* dtheta, int N, int C,
                 int Hi, int Wi, int Ho, int Wo, void* stream) {
  return stn_bwd<float>(U, theta, dout, dU, dtheta, N, C, Hi, Wi, Ho, Wo, stream);
}

int paig_stn_fwd_f64(const float* U, const double* theta, float* out, int N, int C, int Hi, int Wi, int Ho, int Wo,
                     void* stream) {
  return stn_fwd<double>(U, theta, out, N, C, Hi, Wi, Ho, Wo, stream);
}

int paig_stn_bwd_f64(const float* U, const double* theta, const float* dout, float* dU, double* dtheta, int N, int C,
                     int Hi, int Wi, int Ho, int Wo, void* stream) {
  return stn_bwd<double>(U, theta, dout, dU, dtheta, N, C, Hi, Wi, Ho, Wo, stream);
}

}  // extern "C"

#ifdef PAIG_DEC_STAMPS
extern "C" int paig_dec_stamps_read(void* host, size_t bytes) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(paig_dec_stamps), bytes);
}
#endif

// Synthetic dataset rendering on the device: the trajectory integrators and the
// disk rasteriser of nn/datasets/synth.py (_spring_traj / _bounce_traj /
// _gravity_traj, _disk_frames and the composition of render_sequences).
//
//   integrate: one lane per candidate, fp64, the host's update order; the
//     acceptance flag is the host's rejection rule.  Loops run T * sub steps.
//   raster: one block column per (sequence, frame); a lane produces 4 pixels
//     of one row = 12 contiguous bytes of the NHWC uint8 frame.  The object
//     positions of a frame are wave-uniform (indexed by blockIdx only).  A
//     pixel's 4 x 4 subsample tests run only when its centre is within the
//     subsample reach of the disk's rim; elsewhere the count is 0 or 16.
//
// Every product and sum of the host is one numpy operation, rounded on its
// own: this file is compiled without FMA contraction.
#include <stdint.h>

#include "common.h"

#pragma clang fp contract(off)

namespace {

enum { PHYS_SPRING = 0, PHYS_BOUNCE = 1, PHYS_GRAVITY = 2 };

// pos [m, T, K, 2]: the state before each step's `sub` substeps.
template <int K, int PHYS>
__global__ void __launch_bounds__(64)
synth_integrate_k(const double* __restrict__ p0, const double* __restrict__ v0, long long m, int T, int sub, double dt,
                  double size, double radius, double c0, double c1, double* __restrict__ pos,
                  int* __restrict__ valid) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i >= m) return;
  double p[K][2], v[K][2];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    p[j][0] = p0[(i * K + j) * 2];
    p[j][1] = p0[(i * K + j) * 2 + 1];
    v[j][0] = v0[(i * K + j) * 2];
    v[j][1] = v0[(i * K + j) * 2 + 1];
  }
  const double h = dt / (double)sub;
  const double lo = radius, hi = size - radius;
  const double eq2 = 2.0 * c1;
  int ok = 1;
  double* o = pos + i * T * K * 2;
  for (int t = 0; t < T; ++t) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      o[(t * K + j) * 2] = p[j][0];
      o[(t * K + j) * 2 + 1] = p[j][1];
      if (PHYS == PHYS_GRAVITY)   // synth.py:105: every recorded position strictly inside
        ok &= (p[j][0] > lo) & (p[j][0] < hi) & (p[j][1] > lo) & (p[j][1] < hi);
    }
    for (int s = 0; s < sub; ++s) {
      if (PHYS == PHYS_SPRING) {   // synth.py:56-61
        const double dx = p[0][0] - p[1][0], dy = p[0][1] - p[1][1];
        const double n = sqrt(dx * dx + dy * dy) + 1e-8;
        const double f = c0 * (n - eq2);
        const double Fx = f * dx / n, Fy = f * dy / n;
        v[0][0] -= h * Fx;
        v[0][1] -= h * Fy;
        v[1][0] += h * Fx;
        v[1][1] += h * Fy;
#pragma unroll
        for (int j = 0; j < K; ++j) {
          p[j][0] += h * v[j][0];
          p[j][1] += h * v[j][1];
        }
      } else if (PHYS == PHYS_BOUNCE) {   // synth.py:77-80
#pragma unroll
        for (int j = 0; j < K; ++j)
#pragma unroll
          for (int a = 0; a < 2; ++a) {
            const double q = p[j][a] + h * v[j][a];
            const bool l = q < lo, g = q > hi;
            v[j][a] = (l | g) ? -v[j][a] : v[j][a];
            p[j][a] = l ? 2.0 * lo - q : (g ? 2.0 * hi - q : q);
          }
      } else {   // synth.py:96-104
        double acc[K][2];
#pragma unroll
        for (int a = 0; a < K; ++a) {
          acc[a][0] = 0.0;
          acc[a][1] = 0.0;
#pragma unroll
          for (int b = 0; b < K; ++b) {
            if (a == b) continue;
            const double dx = p[b][0] - p[a][0], dy = p[b][1] - p[a][1];
            const double n = fmax(sqrt(dx * dx + dy * dy), 1.0);
            const double n3 = n * n * n;
            acc[a][0] += c0 * dx / n3;
            acc[a][1] += c0 * dy / n3;
          }
        }
#pragma unroll
        for (int j = 0; j < K; ++j) {
          v[j][0] += h * acc[j][0];
          v[j][1] += h * acc[j][1];
          p[j][0] += h * v[j][0];
          p[j][1] += h * v[j][1];
        }
      }
    }
    if (PHYS == PHYS_SPRING) {   // synth.py:62: the state after every step within [radius, size - radius]
#pragma unroll
      for (int j = 0; j < K; ++j)
        ok &= !(p[j][0] < lo) & !(p[j][1] < lo) & !(p[j][0] > hi) & !(p[j][1] > hi);
    }
  }
  valid[i] = ok;
}

// Count of the 16 subsamples of pixel (px, py) inside the disk at (x, y):
// fl(fl(dx dx) + fl(dy dy)) <= r2 with the subsample coordinates
// (s + 0.5) / 4 (exact in fp32 and fp64), as numpy evaluates it.
__device__ __forceinline__ int rim_count(int px, int py, double x, double y, double r2) {
  double dx2[4], dy2[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const double dx = (double)((float)(4 * px + s) + 0.5f) * 0.25 - x;
    const double dy = (double)((float)(4 * py + s) + 0.5f) * 0.25 - y;
    dx2[s] = dx * dx;
    dy2[s] = dy * dy;
  }
  int k = 0;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) k += (dx2[b] + dy2[a]) <= r2 ? 1 : 0;
  return k;
}

// ---- candidates drawn on the device -----------------------------------------
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3",
// SC'11; the Random123 constants).  key = (seed, stream id), counter =
// (candidate low word, candidate high word, round, draw slot): every block of
// four words is a pure function of those, so a candidate does not depend on m
// or on the launch shape.
struct Philox4 {
  uint32_t w[4];
};

__host__ __device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                                          uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t a = (uint64_t)0xD2511F53u * c0, b = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(b >> 32) ^ c1 ^ k0, n1 = (uint32_t)b;
    const uint32_t n2 = (uint32_t)(a >> 32) ^ c3 ^ k1, n3 = (uint32_t)a;
    c0 = n0, c1 = n1, c2 = n2, c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// numpy's double from two 32-bit words: 53 random bits in [0, 1)
__device__ __forceinline__ double u53(uint32_t a, uint32_t b) {
  return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * (1.0 / 9007199254740992.0);
}

enum { DRAW_SLOTS = 4, DRAW_U = 2 * DRAW_SLOTS };

// One lane per candidate.  Uniform u[2 s] / u[2 s + 1] come from words (0, 1)
// / (2, 3) of draw slot s.  Their use, fixed (synth_device.initial_conditions_philox
// is the same arithmetic, operation for operation):
//   spring   u0 u1 centre of mass x y (half: x from the left half with the same u0);
//            u2 pair angle, u3 pair distance factor - 0.5; u4 u5 velocity angles
//            of objects 0 1; u6 u7 their speed factors
//   bounce   u0 u1 position of object 0, u2 u3 of object 1; u4 u5 velocity
//            angles; u6 u7 speed factors (0.5 + 0.5 u)
//   gravity  u0 angle of object 0, u1 orbit radius factor (slot 0 only)
template <int K, int PHYS>
__global__ void __launch_bounds__(64)
synth_draw_k(uint32_t k0, uint32_t k1, uint32_t round, long long m, int half, double size, double rb, double c0,
             double c1, double vmax, double* __restrict__ p0, double* __restrict__ v0, double* __restrict__ udbg) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i >= m) return;
  constexpr int SLOTS = PHYS == PHYS_GRAVITY ? 1 : DRAW_SLOTS;
  constexpr double PI = 3.141592653589793;
  double u[DRAW_U];
#pragma unroll
  for (int s = 0; s < DRAW_SLOTS; ++s) {
    if (s < SLOTS) {
      const Philox4 x = philox4x32_10((uint32_t)i, (uint32_t)((unsigned long long)i >> 32), round, (uint32_t)s, k0, k1);
      u[2 * s] = u53(x.w[0], x.w[1]);
      u[2 * s + 1] = u53(x.w[2], x.w[3]);
    } else {
      u[2 * s] = 0.0;
      u[2 * s + 1] = 0.0;
    }
  }
  if (udbg) {
#pragma unroll
    for (int s = 0; s < DRAW_U; ++s) udbg[i * DRAW_U + s] = u[s];
  }
  double p[K][2], v[K][2];
  if (PHYS == PHYS_SPRING) {
    const double lo = rb + c1, hi = size - (rb + c1);
    const double cx = half ? lo + (size / 2.0 - lo) * u[0] : lo + (hi - lo) * u[0];
    const double cy = lo + (hi - lo) * u[1];
    const double ang = u[2] * 2.0 * PI, r = u[3] + 0.5;
    const double ox = cos(ang) * c1 * r, oy = sin(ang) * c1 * r;
    p[0][0] = ox + cx;
    p[0][1] = oy + cy;
    p[1][0] = -ox + cx;
    p[1][1] = -oy + cy;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const double a = u[4 + j] * 2.0 * PI;
      v[j][0] = cos(a) * vmax * u[6 + j];
      v[j][1] = sin(a) * vmax * u[6 + j];
    }
  } else if (PHYS == PHYS_BOUNCE) {
    const double span = size - 2.0 * rb;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      p[j][0] = rb + span * u[2 * j];
      p[j][1] = rb + span * u[2 * j + 1];
      const double a = u[4 + j] * 2.0 * PI, s = 0.5 + 0.5 * u[6 + j];
      v[j][0] = cos(a) * vmax * s;
      v[j][1] = sin(a) * vmax * s;
    }
  } else {
    const double c = size / 2.0, a0 = u[0] * 2.0 * PI, r = 4.0 + 4.0 * u[1];
    const double sp = sqrt(c0 / r) * 0.35;
    const double ph[3] = {0.0, 2.0 * PI / 3.0, 4.0 * PI / 3.0};
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const double a = a0 + ph[j % 3];
      const double cs = cos(a), sn = sin(a);
      p[j][0] = c + r * cs;
      p[j][1] = c + r * sn;
      v[j][0] = -sn * sp;
      v[j][1] = cs * sp;
    }
  }
#pragma unroll
  for (int j = 0; j < K; ++j) {
    p0[(i * K + j) * 2] = p[j][0];
    p0[(i * K + j) * 2 + 1] = p[j][1];
    v0[(i * K + j) * 2] = v[j][0];
    v0[(i * K + j) * 2 + 1] = v[j][1];
  }
}

// bg [n, npix] = clip(U - 0.2, 0, 1), U = (word >> 8) 2^-24 in fp32: one lane
// per 4 pixels = the four words of counter (quad low, quad high, round, BG_SLOT).
enum { BG_SLOT = 0x6267 };

__global__ void __launch_bounds__(256)
synth_bg_k(uint32_t k0, uint32_t k1, uint32_t round, long long quads, float* __restrict__ bg) {
  const long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (q >= quads) return;
  const Philox4 x = philox4x32_10((uint32_t)q, (uint32_t)((unsigned long long)q >> 32), round, (uint32_t)BG_SLOT, k0, k1);
  float4 o;
  float* of = reinterpret_cast<float*>(&o);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float uf = (float)(x.w[e] >> 8) * (1.0f / 16777216.0f);
    of[e] = fminf(fmaxf(uf - 0.2f, 0.0f), 1.0f);
  }
  *reinterpret_cast<float4*>(bg + 4 * q) = o;
}

// Acceptance flags -> row indices, in candidate order: one block walks the
// flags 256 at a time; a lane's slot is the running count + the counts of the
// waves before its own + the set lanes before it in its wave's ballot.  No
// atomics: the order of rows is the order of the candidates, always.
// totals (nullable, int64 [3]) accumulates {calls, min(accepted, n), n -
// min(accepted, n)}: calls on one stream are ordered, so lane 0's plain
// read-add-store is exact.
__global__ void __launch_bounds__(256)
synth_compact_k(const int* __restrict__ valid, long long m, long long* __restrict__ rows, long long n,
                int* __restrict__ count, long long* __restrict__ totals) {
  __shared__ int wtot[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  long long base = 0;   // accepted so far (block-uniform)
  for (long long s = 0; s < m; s += 256) {
    const long long i = s + tid;
    const bool f = i < m && valid[i] != 0;
    const unsigned long long b = __ballot(f);
    const int pre = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) wtot[w] = __popcll(b);
    __syncthreads();
    int before = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = wtot[k];
      before += k < w ? c : 0;
      tot += c;
    }
    const long long at = base + before + pre;
    if (f && at < n) rows[at] = i;
    base += tot;
    __syncthreads();
  }
  const long long got = base < n ? base : n;
  for (long long i = got + tid; i < n; i += 256) rows[i] = -1;
  if (tid == 0) {
    count[0] = (int)got;
    count[1] = (int)base;
    if (totals) {
      totals[0] += 1;
      totals[1] += got;
      totals[2] += n - got;
    }
  }
}

// out [n, T, size, size, 3] uint8; grid (n * T, blocks per frame); lane q of a
// frame renders pixels 4q .. 4q+3 (one row: size % 4 == 0).  m > 0 (the _ex
// entry): rows come from the device unchecked, and a sequence whose row is
// outside [0, m) is left as it is.
template <int K>
__global__ void __launch_bounds__(256)
synth_raster_k(const double* __restrict__ pos, const long long* __restrict__ rows, long long m, int T, int size,
               double radius, const float* __restrict__ bg, uint8_t* __restrict__ out) {
  const long long f = blockIdx.x;               // frame = i * T + t (< 2^31)
  const long long i = blockIdx.x / (unsigned)T;
  const int t = (int)(f - i * T);
  const int q = blockIdx.y * blockDim.x + threadIdx.x;
  const int npix = size * size;
  if (4 * q >= npix) return;
  const long long r = rows ? rows[i] : i;       // wave-uniform
  if (m > 0 && (r < 0 || r >= m)) return;
  const double* P = pos + (r * T + t) * (K * 2);
  const int py = (4 * q) / size, px0 = (4 * q) - py * size;

  // a subsample lies within 0.375 * sqrt(2) < 0.531 of its pixel's centre
  constexpr double REACH = 0.54;
  const double r2 = radius * radius;
  const double out2 = (radius + REACH) * (radius + REACH);
  const double in2 = radius > REACH ? (radius - REACH) * (radius - REACH) : -1.0;

  int cnt[4][3];
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int c = 0; c < 3; ++c) cnt[e][c] = 0;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const double x = P[2 * j], y = P[2 * j + 1];   // scalar loads
    const double dyc = ((double)py + 0.5) - y;
    const double dyc2 = dyc * dyc;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double dxc = ((double)(px0 + e) + 0.5) - x;
      const double dc2 = dxc * dxc + dyc2;
      int k;
      if (dc2 > out2) k = 0;
      else if (dc2 < in2) k = 16;
      else k = rim_count(px0 + e, py, x, y, r2);
      cnt[e][2 - (j % 3)] = k;
    }
  }

  unsigned w[3] = {0u, 0u, 0u};
  if (bg) {
    const float4 b = *reinterpret_cast<const float4*>(bg + i * npix + 4 * q);
    const float bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float v = fmaxf(bv[e], (float)cnt[e][c] * 0.0625f);
        v = fminf(fmaxf(v, 0.0f), 1.0f);
        const unsigned byte = (unsigned)(v * 255.0f);
        const int o = e * 3 + c;
        w[o >> 2] |= byte << (8 * (o & 3));
      }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const unsigned byte = (unsigned)(cnt[e][c] * 255) >> 4;
        const int o = e * 3 + c;
        w[o >> 2] |= byte << (8 * (o & 3));
      }
  }
  // 12 contiguous bytes per lane, 768 per wave (4-byte aligned: frame and row
  // sizes are multiples of 12)
  unsigned* dst = reinterpret_cast<unsigned*>(out + f * (3LL * npix) + 12LL * q);
  dst[0] = w[0];
  dst[1] = w[1];
  dst[2] = w[2];
}

}  // namespace

extern "C" {

int paig_synth_integrate(int phys, const double* p0, const double* v0, long long m, int K, int T, int sub, double dt,
                         double size, double radius, double c0, double c1, double* pos, int* valid, void* stream) {
  PAIG_REQUIRE(phys >= PHYS_SPRING && phys <= PHYS_GRAVITY, "synth_integrate: phys=%d (0 spring, 1 bounce, 2 gravity)",
               phys);
  PAIG_REQUIRE(K == 2 || K == 3, "synth_integrate: K=%d (2 or 3)", K);
  PAIG_REQUIRE(K == (phys == PHYS_GRAVITY ? 3 : 2), "synth_integrate: K=%d does not match phys=%d", K, phys);
  PAIG_REQUIRE(m >= 0 && T > 0 && sub > 0 && m <= 0x7fffffffLL * 64, "synth_integrate: m=%lld T=%d sub=%d", m, T, sub);
  if (m == 0) return 0;
  PAIG_REQUIRE(p0 && v0 && pos && valid, "synth_integrate: null operand");
  const dim3 grid((unsigned)((m + 63) / 64)), block(64);
  hipStream_t st = (hipStream_t)stream;
  if (phys == PHYS_SPRING)
    hipLaunchKernelGGL((synth_integrate_k<2, PHYS_SPRING>), grid, block, 0, st, p0, v0, m, T, sub, dt, size, radius, c0,
                       c1, pos, valid);
  else if (phys == PHYS_BOUNCE)
    hipLaunchKernelGGL((synth_integrate_k<2, PHYS_BOUNCE>), grid, block, 0, st, p0, v0, m, T, sub, dt, size, radius, c0,
                       c1, pos, valid);
  else
    hipLaunchKernelGGL((synth_integrate_k<3, PHYS_GRAVITY>), grid, block, 0, st, p0, v0, m, T, sub, dt, size, radius,
                       c0, c1, pos, valid);
  PAIG_CHECK_LAUNCH();
  return 0;
}

static int synth_raster_launch(const char* who, const double* pos, const long long* rows, long long m, long long n,
                               int T, int K, int size, double radius, const float* bg, unsigned char* out,
                               void* stream) {
  PAIG_REQUIRE(K == 2 || K == 3, "%s: K=%d (2 or 3)", who, K);
  PAIG_REQUIRE(size > 0 && size % 4 == 0 && size <= 4096, "%s: size=%d (a multiple of 4, <= 4096)", who, size);
  PAIG_REQUIRE(n >= 0 && T > 0 && n * T <= 0x7fffffffLL, "%s: n=%lld T=%d (n * T < 2^31)", who, n, T);
  if (n == 0) return 0;
  PAIG_REQUIRE(pos && out, "%s: null operand", who);
  PAIG_REQUIRE(((uintptr_t)out % 4) == 0 && ((uintptr_t)bg % 16) == 0, "%s: out must be 4-byte and bg 16-byte aligned",
               who);
  const int quads = size * size / 4;
  // the block size (whole waves) that leaves the fewest idle lanes per frame
  int bs = 256, waste = cdiv(quads, 256) * 256 - quads;
  for (int b = 192; b >= 64; b -= 64) {
    const int w = cdiv(quads, b) * b - quads;
    if (w < waste) bs = b, waste = w;
  }
  const dim3 grid((unsigned)(n * T), (unsigned)cdiv(quads, bs)), block(bs);
  PAIG_REQUIRE(grid.y <= 65535u, "%s: size=%d too large", who, size);
  hipStream_t st = (hipStream_t)stream;
  if (K == 2)
    hipLaunchKernelGGL(synth_raster_k<2>, grid, block, 0, st, pos, rows, m, T, size, radius, bg, out);
  else
    hipLaunchKernelGGL(synth_raster_k<3>, grid, block, 0, st, pos, rows, m, T, size, radius, bg, out);
  PAIG_CHECK_LAUNCH();
  return 0;
}

int paig_synth_raster(const double* pos, const long long* rows, long long n, int T, int K, int size, double radius,
                      const float* bg, unsigned char* out, void* stream) {
  return synth_raster_launch("synth_raster", pos, rows, 0, n, T, K, size, radius, bg, out, stream);
}

int paig_synth_raster_ex(const double* pos, const long long* rows, long long m, long long n, int T, int K, int size,
                         double radius, const float* bg, unsigned char* out, void* stream) {
  PAIG_REQUIRE(m > 0 && rows, "synth_raster_ex: m=%lld (> 0) and rows are required", m);
  return synth_raster_launch("synth_raster_ex", pos, rows, m, n, T, K, size, radius, bg, out, stream);
}

int paig_synth_draw(int phys, long long seed, long long stream_id, long long round, long long m, int K, int half,
                    double size, double radius, double c0, double c1, double vmax, double* p0, double* v0, double* u,
                    void* stream) {
  PAIG_REQUIRE(phys >= PHYS_SPRING && phys <= PHYS_GRAVITY, "synth_draw: phys=%d (0 spring, 1 bounce, 2 gravity)", phys);
  PAIG_REQUIRE(K == (phys == PHYS_GRAVITY ? 3 : 2), "synth_draw: K=%d does not match phys=%d", K, phys);
  PAIG_REQUIRE(seed >= 0 && seed <= 0xffffffffLL && stream_id >= 0 && stream_id <= 0xffffffffLL && round >= 0 &&
                   round <= 0xffffffffLL,
               "synth_draw: seed=%lld stream=%lld round=%lld (each in [0, 2^32))", seed, stream_id, round);
  PAIG_REQUIRE(m >= 0 && m <= 0x7fffffffLL * 64, "synth_draw: m=%lld", m);
  if (m == 0) return 0;
  PAIG_REQUIRE(p0 && v0, "synth_draw: null operand");
  const dim3 grid((unsigned)((m + 63) / 64)), block(64);
  hipStream_t st = (hipStream_t)stream;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)stream_id, rd = (uint32_t)round;
  if (phys == PHYS_SPRING)
    hipLaunchKernelGGL((synth_draw_k<2, PHYS_SPRING>), grid, block, 0, st, k0, k1, rd, m, half, size, radius, c0, c1,
                       vmax, p0, v0, u);
  else if (phys == PHYS_BOUNCE)
    hipLaunchKernelGGL((synth_draw_k<2, PHYS_BOUNCE>), grid, block, 0, st, k0, k1, rd, m, half, size, radius, c0, c1,
                       vmax, p0, v0, u);
  else
    hipLaunchKernelGGL((synth_draw_k<3, PHYS_GRAVITY>), grid, block, 0, st, k0, k1, rd, m, half, size, radius, c0, c1,
                       vmax, p0, v0, u);
  PAIG_CHECK_LAUNCH();
  return 0;
}

int paig_synth_background(long long seed, long long stream_id, long long round, long long n, int size, float* bg,
                          void* stream) {
  PAIG_REQUIRE(seed >= 0 && seed <= 0xffffffffLL && stream_id >= 0 && stream_id <= 0xffffffffLL && round >= 0 &&
                   round <= 0xffffffffLL,
               "synth_background: seed=%lld stream=%lld round=%lld (each in [0, 2^32))", seed, stream_id, round);
  PAIG_REQUIRE(n >= 0 && size > 0 && size % 4 == 0 && size <= 4096, "synth_background: n=%lld size=%d", n, size);
  if (n == 0) return 0;
  PAIG_REQUIRE(bg && ((uintptr_t)bg % 16) == 0, "synth_background: bg must be 16-byte aligned");
  const long long quads = n * (long long)(size * size / 4);
  PAIG_REQUIRE(quads <= 0x7fffffffLL * 256, "synth_background: n=%lld too large", n);
  hipLaunchKernelGGL(synth_bg_k, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (uint32_t)seed, (uint32_t)stream_id, (uint32_t)round, quads, bg);
  PAIG_CHECK_LAUNCH();
  return 0;
}

int paig_synth_compact(const int* valid, long long m, long long* rows, long long n, int* count, long long* totals,
                       void* stream) {
  PAIG_REQUIRE(m >= 0 && m <= 0x7fffffffLL && n >= 0, "synth_compact: m=%lld n=%lld", m, n);
  PAIG_REQUIRE(count && (m == 0 || valid) && (n == 0 || rows), "synth_compact: null operand");
  hipLaunchKernelGGL(synth_compact_k, dim3(1), dim3(256), 0, (hipStream_t)stream, valid, m, rows, n, count, totals);
  PAIG_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

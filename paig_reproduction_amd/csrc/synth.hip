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

// out [n, T, size, size, 3] uint8; grid (n * T, blocks per frame); lane q of a
// frame renders pixels 4q .. 4q+3 (one row: size % 4 == 0).
template <int K>
__global__ void __launch_bounds__(256)
synth_raster_k(const double* __restrict__ pos, const long long* __restrict__ rows, int T, int size, double radius,
               const float* __restrict__ bg, uint8_t* __restrict__ out) {
  const long long f = blockIdx.x;               // frame = i * T + t (< 2^31)
  const long long i = blockIdx.x / (unsigned)T;
  const int t = (int)(f - i * T);
  const int q = blockIdx.y * blockDim.x + threadIdx.x;
  const int npix = size * size;
  if (4 * q >= npix) return;
  const long long r = rows ? rows[i] : i;       // wave-uniform
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

int paig_synth_raster(const double* pos, const long long* rows, long long n, int T, int K, int size, double radius,
                      const float* bg, unsigned char* out, void* stream) {
  PAIG_REQUIRE(K == 2 || K == 3, "synth_raster: K=%d (2 or 3)", K);
  PAIG_REQUIRE(size > 0 && size % 4 == 0 && size <= 4096, "synth_raster: size=%d (a multiple of 4, <= 4096)", size);
  PAIG_REQUIRE(n >= 0 && T > 0 && n * T <= 0x7fffffffLL, "synth_raster: n=%lld T=%d (n * T < 2^31)", n, T);
  if (n == 0) return 0;
  PAIG_REQUIRE(pos && out, "synth_raster: null operand");
  PAIG_REQUIRE(((uintptr_t)out % 4) == 0 && ((uintptr_t)bg % 16) == 0,
               "synth_raster: out must be 4-byte and bg 16-byte aligned");
  const int quads = size * size / 4;
  // the block size (whole waves) that leaves the fewest idle lanes per frame
  int bs = 256, waste = cdiv(quads, 256) * 256 - quads;
  for (int b = 192; b >= 64; b -= 64) {
    const int w = cdiv(quads, b) * b - quads;
    if (w < waste) bs = b, waste = w;
  }
  const dim3 grid((unsigned)(n * T), (unsigned)cdiv(quads, bs)), block(bs);
  PAIG_REQUIRE(grid.y <= 65535u, "synth_raster: size=%d too large", size);
  hipStream_t st = (hipStream_t)stream;
  if (K == 2)
    hipLaunchKernelGGL(synth_raster_k<2>, grid, block, 0, st, pos, rows, T, size, radius, bg, out);
  else
    hipLaunchKernelGGL(synth_raster_k<3>, grid, block, 0, st, pos, rows, T, size, radius, bg, out);
  PAIG_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

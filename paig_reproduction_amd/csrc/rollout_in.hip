// Interaction-network rollout cell: one relation network shared by all ordered
// pairs of objects and one object network shared by all objects, all R steps
// in one launch, and its backpropagation through time.
//
//   s_i   = [(pos_i - s) / s, vel_i / s]                 s = frame side / 2, K = D / 2 objects
//   e_ij  = tanh(W_r2 tanh(W_r1 [s_i, s_j] + b_r1) + b_r2)   every ordered pair j != i (receiver first)
//   a_i   = sum_{j != i} e_ij                            in increasing j
//   y_i   = W_o2 tanh(W_o1 [s_i, a_i] + b_o1) + b_o2
//   pos_i' = pos_i + s y_i[:2];  vel_i' = vel_i + s y_i[2:]
//
// The reference has no counterpart: this is a learned cell in the place of
// cells.py's equations inside the rollout loop physics_models.py:231-239,
// same pos_vel_seq layout as paig_rollout_fwd.
//
// Layout of one block (rollout_lstm.hip's): 16 sequences (the M of a 16x16x4
// f32 MFMA tile) and one wave per 16 hidden units.  The M rows of a tile are
// the 16 sequences of one ordered pair, or of one object; a step walks the
// K (K - 1) pairs and then the K objects.  Each wave holds the B operands of
// its 16 hidden units (W_r1, W_r2, W_o1 rows; one 4x16 tile per VGPR) in
// registers for the whole rollout.  Activations cross waves through LDS only
// (transposed, [unit][row]: A-operand reads are consecutive words, accumulator
// writes 16-byte stores).  The moving state lives in the A-operand layout in
// every wave: lane (row, k) holds component k of every object's s_i.  The
// read-out W_o2 is split over the waves (each multiplies its own 16 hidden
// units) and summed in wave order by every lane that needs the value.  Four
// block barriers per step, no atomics, no cross-lane operand staging.
// Products are exact f32 (v_mfma_f32_16x16x4_f32).
#include <algorithm>

#include "rollout_learned.h"

namespace {

constexpr int IN_HMAX = 128;   // hidden units (8 waves of 16)
constexpr int IN_ROWS = 16;    // sequences per block

static_assert(IN_ROWS == LEARNED_ROWS, "the grid of LEARNED_DISPATCH");

// the saved state of one forward (floats from the workspace base), then the
// backward's own buffers; every region a multiple of 4 floats.  Row of a
// pair: ((b R + t) P + p), p = i (K - 1) + (j < i ? j : j - 1); of an object:
// ((b R + t) K + i)
struct InWs {
  size_t xr, h1, e, xo, ho, dz1, dz2, dzo, dy, gemm, colsum, total;
  size_t gemm_floats;
};
static InWs in_ws(int B, int D, int H, int R) {
  const int K = D / 2, P = K * (K - 1);
  const size_t pr = (size_t)B * R * P, orows = (size_t)B * R * K;
  InWs w;
  size_t o = 0;
  w.xr = o, o += pr * 8;            // [s_i, s_j]
  w.h1 = o, o += pr * H;            // first relation activation
  w.e = o, o += pr * H;             // second relation activation e_ij
  w.xo = o, o += orows * (4 + H);   // [s_i, a_i]
  w.ho = o, o += orows * H;         // object hidden activation
  w.dz1 = o, o += pr * H;
  w.dz2 = o, o += pr * H;
  w.dzo = o, o += orows * H;
  w.dy = o, o += orows * 4;
  size_t g = paig_gemm_workspace(H, 8, (int)pr);
  g = std::max(g, paig_gemm_workspace(H, H, (int)pr));
  g = std::max(g, paig_gemm_workspace(H, 4 + H, (int)orows));
  g = std::max(g, paig_gemm_workspace(4, H, (int)orows));
  g = (g + 3) & ~(size_t)3;
  w.gemm = o, o += g;
  w.gemm_floats = g;
  w.colsum = o, o += (paig_colsum_workspace((int)pr, H) + 3) & ~(size_t)3;
  w.total = o;
  return w;
}

// column of component c (0, 1: position; 2, 3: velocity) of object i in a
// pos_vel_seq row [pos (D) | vel (D)]
__device__ __forceinline__ int in_col(int i, int c, int D) { return c < 2 ? 2 * i + c : D + 2 * i + (c - 2); }
__device__ __forceinline__ int in_pair(int i, int j, int K) { return i * (K - 1) + (j < i ? j : j - 1); }

// K objects, KH >= H / 4 k-steps of a hidden vector (weights past H are zero)
template <int K, int KH>
__global__ void __launch_bounds__(512)
in_fwd_k(const float* __restrict__ pos0, long long pos0_ld, const float* __restrict__ vel0,
         const float* __restrict__ w_r1, const float* __restrict__ b_r1, const float* __restrict__ w_r2,
         const float* __restrict__ b_r2, const float* __restrict__ w_o1, const float* __restrict__ b_o1,
         const float* __restrict__ w_o2, const float* __restrict__ b_o2, float S, float* __restrict__ pvs,
         float* __restrict__ sv_xr, float* __restrict__ sv_h1, float* __restrict__ sv_e, float* __restrict__ sv_xo,
         float* __restrict__ sv_ho, int B, int H, int R) {
  constexpr int D = 2 * K, D2 = 4 * K, P = K * (K - 1);
  constexpr int HU = (4 * KH + 15) / 16 * 16;   // hidden units with a row in LDS
  __shared__ __attribute__((aligned(16))) float h1T[P][HU * IN_ROWS];   // [pair][unit][row]
  __shared__ __attribute__((aligned(16))) float aT[K][HU * IN_ROWS];    // [object][unit][row]
  __shared__ __attribute__((aligned(16))) float hoT[K][HU * IN_ROWS];
  __shared__ __attribute__((aligned(16))) float yp[8][K][4 * IN_ROWS];  // read-out partials: [wave][object][col][row]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, NW = blockDim.x >> 6;
  const int ar = lane & 15, ak = lane >> 4;   // A operand: row ar, k offset ak; C: column ar, rows 4 ak + r
  const int row0 = blockIdx.x * IN_ROWS;
  const int j = 16 * w + ar;                  // hidden unit of this lane's B / C column
  const bool jv = j < H;
  const int HO = 4 + H;                       // W_o1's row length

  // ---- stationary B operands: k-step ks -> W[j][4 ks + ak]
  float wr1[2], wr2[KH], wo1[1 + KH], wo2[4];
  wr1[0] = jv ? w_r1[(long long)j * 8 + ak] : 0.f;
  wr1[1] = jv ? w_r1[(long long)j * 8 + 4 + ak] : 0.f;
  wo1[0] = jv ? w_o1[(long long)j * HO + ak] : 0.f;
#pragma unroll
  for (int q = 0; q < KH; ++q) {
    const int k = 4 * q + ak;
    wr2[q] = (jv && k < H) ? w_r2[(long long)j * H + k] : 0.f;
    wo1[1 + q] = (jv && k < H) ? w_o1[(long long)j * HO + 4 + k] : 0.f;
  }
  // read-out over this wave's own 16 hidden units: B[k][n = ar] = W_o2[n][16 w + 4 q + ak]
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int k = 16 * w + 4 * q + ak;
    wo2[q] = (ar < 4 && k < H) ? w_o2[(long long)ar * H + k] : 0.f;
  }
  const float br1 = jv ? b_r1[j] : 0.f, br2 = jv ? b_r2[j] : 0.f, bo1 = jv ? b_o1[j] : 0.f, bo2 = b_o2[ak];
  // ---- the moving state in A-operand layout: lane (ar, ak) holds component ak of every object of sequence row0 + ar
  const int arow = row0 + ar;
  const bool av = arow < B;
  float sv[K];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    float v = 0.f;
    if (av) {
      if (ak < 2) v = pos0[(long long)arow * pos0_ld + 2 * i + ak];
      else if (vel0) v = vel0[((long long)i * B + arow) * 2 + (ak - 2)];
    }
    sv[i] = v;
    if (w == 0 && av) pvs[(long long)arow * (R + 1) * D2 + in_col(i, ak, D)] = v;
  }
  // units past this block's waves are read (4 KH may exceed 16 NW) and never written: zeros
  for (int i = threadIdx.x; i < P * HU * IN_ROWS; i += blockDim.x) (&h1T[0][0])[i] = 0.f;
  for (int i = threadIdx.x; i < K * HU * IN_ROWS; i += blockDim.x) (&aT[0][0])[i] = 0.f, (&hoT[0][0])[i] = 0.f;
  __syncthreads();

  for (int t = 0; t < R; ++t) {
    float x[K];
#pragma unroll
    for (int i = 0; i < K; ++i) x[i] = ak < 2 ? (sv[i] - S) / S : sv[i] / S;
    // ---- relation layer 1, every ordered pair (receiver i first)
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
      for (int jj = 0; jj < K; ++jj) {
        if (jj == i) continue;
        const int p = in_pair(i, jj, K);
        f32x4 acc = {br1, br1, br1, br1};
        acc = mfma4(x[i], wr1[0], acc);
        acc = mfma4(x[jj], wr1[1], acc);
        f32x4 h;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          h[r] = jv ? tanhf(acc[r]) : 0.f;
          const int row = row0 + 4 * ak + r;
          if (sv_h1 && jv && row < B) sv_h1[(((long long)row * R + t) * P + p) * H + j] = h[r];
        }
        *reinterpret_cast<f32x4*>(&h1T[p][j * IN_ROWS + 4 * ak]) = h;
        if (sv_xr && w == 0 && av) {
          float* o = sv_xr + (((long long)arow * R + t) * P + p) * 8;
          o[ak] = x[i], o[4 + ak] = x[jj];
        }
      }
    if (sv_xo && w == 0 && av) {
#pragma unroll
      for (int i = 0; i < K; ++i) sv_xo[(((long long)arow * R + t) * K + i) * HO + ak] = x[i];
    }
    __syncthreads();
    // ---- relation layer 2 and the sum over senders
    f32x4 acc2[P];
#pragma unroll
    for (int p = 0; p < P; ++p) acc2[p] = f32x4{br2, br2, br2, br2};
#pragma unroll
    for (int q = 0; q < KH; ++q)
#pragma unroll
      for (int p = 0; p < P; ++p) acc2[p] = mfma4(h1T[p][(4 * q + ak) * IN_ROWS + ar], wr2[q], acc2[p]);
#pragma unroll
    for (int i = 0; i < K; ++i) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int jj = 0; jj < K; ++jj) {
        if (jj == i) continue;
        const int p = in_pair(i, jj, K);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = jv ? tanhf(acc2[p][r]) : 0.f;
          const int row = row0 + 4 * ak + r;
          if (sv_e && jv && row < B) sv_e[(((long long)row * R + t) * P + p) * H + j] = e;
          a[r] += e;
        }
      }
      *reinterpret_cast<f32x4*>(&aT[i][j * IN_ROWS + 4 * ak]) = a;
      if (sv_xo && jv) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = row0 + 4 * ak + r;
          if (row < B) sv_xo[(((long long)row * R + t) * K + i) * HO + 4 + j] = a[r];
        }
      }
    }
    __syncthreads();
    // ---- object layer 1
    f32x4 acc3[K];
#pragma unroll
    for (int i = 0; i < K; ++i) acc3[i] = mfma4(x[i], wo1[0], f32x4{bo1, bo1, bo1, bo1});
#pragma unroll
    for (int q = 0; q < KH; ++q)
#pragma unroll
      for (int i = 0; i < K; ++i) acc3[i] = mfma4(aT[i][(4 * q + ak) * IN_ROWS + ar], wo1[1 + q], acc3[i]);
#pragma unroll
    for (int i = 0; i < K; ++i) {
      f32x4 h;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        h[r] = jv ? tanhf(acc3[i][r]) : 0.f;
        const int row = row0 + 4 * ak + r;
        if (sv_ho && jv && row < B) sv_ho[(((long long)row * R + t) * K + i) * H + j] = h[r];
      }
      *reinterpret_cast<f32x4*>(&hoT[i][j * IN_ROWS + 4 * ak]) = h;
    }
    __syncthreads();
    // ---- read-out partial over this wave's hidden units
#pragma unroll
    for (int i = 0; i < K; ++i) {
      f32x4 pa = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int q = 0; q < 4; ++q) pa = mfma4(hoT[i][(16 * w + 4 * q + ak) * IN_ROWS + ar], wo2[q], pa);
      if (ar < 4) *reinterpret_cast<f32x4*>(&yp[w][i][ar * IN_ROWS + 4 * ak]) = pa;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < K; ++i) {
      float y = bo2;
      for (int ww = 0; ww < NW; ++ww) y += yp[ww][i][ak * IN_ROWS + ar];
      sv[i] = sv[i] + S * y;
      if (w == 0 && av) pvs[((long long)arow * (R + 1) + t + 1) * D2 + in_col(i, ak, D)] = sv[i];
    }
  }
}

// Backward through time: t = R .. 1 in one launch, carrying the position /
// velocity adjoints in the A-operand layout.  Stationary B operands: W_o2
// (dh_o = dy W_o2), the a-columns of W_o1 (da = dz_o W_o1[:, 4:]), W_r2 (dh_1
// = dz_2 W_r2) and this wave's rows of W_o1[:, :4] and W_r1 (the state
// adjoints, summed over the waves in wave order).  da_i fans out to every
// e_ij of receiver i; the adjoint of s_i sums its receiver pairs, its sender
// pairs and its object row, in that order.
template <int K, int KH>
__global__ void __launch_bounds__(512)
in_bwd_k(const float* __restrict__ dpos_roll, const float* __restrict__ dpvs, const float* __restrict__ w_r1,
         const float* __restrict__ w_r2, const float* __restrict__ w_o1, const float* __restrict__ w_o2, float S,
         const float* __restrict__ sv_h1, const float* __restrict__ sv_e, const float* __restrict__ sv_ho,
         float* __restrict__ dz1_out, float* __restrict__ dz2_out, float* __restrict__ dzo_out,
         float* __restrict__ dy_out, float* __restrict__ dpos0, float* __restrict__ dvel0, int B, int H, int R) {
  constexpr int D = 2 * K, D2 = 4 * K, P = K * (K - 1);
  constexpr int HU = (4 * KH + 15) / 16 * 16;
  __shared__ __attribute__((aligned(16))) float zoT[K][HU * IN_ROWS];   // [object][unit][row]
  __shared__ __attribute__((aligned(16))) float z2T[P][HU * IN_ROWS];   // [pair][unit][row]
  __shared__ __attribute__((aligned(16))) float z1T[P][HU * IN_ROWS];
  __shared__ __attribute__((aligned(16))) float xpo[8][K][4 * IN_ROWS];   // ds_i partials of the object row: [wave][object][col][row]
  __shared__ __attribute__((aligned(16))) float xpr[8][P][8 * IN_ROWS];   // d[s_i, s_j] partials: [wave][pair][col][row]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, NW = blockDim.x >> 6;
  const int ar = lane & 15, ak = lane >> 4;
  const int row0 = blockIdx.x * IN_ROWS;
  const int j = 16 * w + ar;
  const bool jv = j < H;
  const int HO = 4 + H;

  float wo1a[KH], wr2t[KH], wo1s[4], wr1t[4];
  const float wo2t = jv ? w_o2[(long long)ak * H + j] : 0.f;   // B[k = ak][j] = W_o2[ak][j]
#pragma unroll
  for (int q = 0; q < KH; ++q) {   // B[k = m][j], m = 4 q + ak
    const int m = 4 * q + ak;
    wo1a[q] = (jv && m < H) ? w_o1[(long long)m * HO + 4 + j] : 0.f;
    wr2t[q] = (jv && m < H) ? w_r2[(long long)m * H + j] : 0.f;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {    // B[k = m][n = ar], m in this wave's units
    const int m = 16 * w + 4 * q + ak;
    wo1s[q] = (ar < 4 && m < H) ? w_o1[(long long)m * HO + ar] : 0.f;
    wr1t[q] = (ar < 8 && m < H) ? w_r1[(long long)m * 8 + ar] : 0.f;
  }

  const int arow = row0 + ar;
  const bool av = arow < B;
  float ga[K];
#pragma unroll
  for (int i = 0; i < K; ++i) ga[i] = 0.f;
  for (int i = threadIdx.x; i < K * HU * IN_ROWS; i += blockDim.x) (&zoT[0][0])[i] = 0.f;
  for (int i = threadIdx.x; i < P * HU * IN_ROWS; i += blockDim.x) (&z2T[0][0])[i] = 0.f, (&z1T[0][0])[i] = 0.f;
  __syncthreads();

  for (int s = R - 1; s >= 0; --s) {
    // ---- adjoints arriving at step s + 1's outputs; dy_i = s (d pos_i', d vel_i'); object layer 2 and tanh'
#pragma unroll
    for (int i = 0; i < K; ++i) {
      if (av) {
        if (dpos_roll && ak < 2) ga[i] += dpos_roll[((long long)arow * R + s) * D + 2 * i + ak];
        if (dpvs) ga[i] += dpvs[((long long)arow * (R + 1) + s + 1) * D2 + in_col(i, ak, D)];
      }
      const float dya = S * ga[i];
      if (w == 0 && av) dy_out[(((long long)arow * R + s) * K + i) * 4 + ak] = dya;
      const f32x4 dho = mfma4(dya, wo2t, f32x4{0.f, 0.f, 0.f, 0.f});
      f32x4 dz;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + 4 * ak + r;
        const bool ok = jv && row < B;
        const long long at = (((long long)row * R + s) * K + i) * H + j;
        const float h = ok ? sv_ho[at] : 0.f;
        dz[r] = ok ? dho[r] * (1.f - h * h) : 0.f;
        if (ok) dzo_out[at] = dz[r];
      }
      *reinterpret_cast<f32x4*>(&zoT[i][j * IN_ROWS + 4 * ak]) = dz;
    }
    __syncthreads();
    // ---- object layer 1: da_i (fanned out to every e_ij of receiver i) and this wave's share of ds_i
    f32x4 da[K];
#pragma unroll
    for (int i = 0; i < K; ++i) da[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < KH; ++q)
#pragma unroll
      for (int i = 0; i < K; ++i) da[i] = mfma4(zoT[i][(4 * q + ak) * IN_ROWS + ar], wo1a[q], da[i]);
#pragma unroll
    for (int i = 0; i < K; ++i) {
      f32x4 px = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int q = 0; q < 4; ++q) px = mfma4(zoT[i][(16 * w + 4 * q + ak) * IN_ROWS + ar], wo1s[q], px);
      if (ar < 4) *reinterpret_cast<f32x4*>(&xpo[w][i][ar * IN_ROWS + 4 * ak]) = px;
#pragma unroll
      for (int jj = 0; jj < K; ++jj) {
        if (jj == i) continue;
        const int p = in_pair(i, jj, K);
        f32x4 dz;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = row0 + 4 * ak + r;
          const bool ok = jv && row < B;
          const long long at = (((long long)row * R + s) * P + p) * H + j;
          const float e = ok ? sv_e[at] : 0.f;
          dz[r] = ok ? da[i][r] * (1.f - e * e) : 0.f;
          if (ok) dz2_out[at] = dz[r];
        }
        *reinterpret_cast<f32x4*>(&z2T[p][j * IN_ROWS + 4 * ak]) = dz;
      }
    }
    __syncthreads();
    // ---- relation layer 2
    f32x4 dh[P];
#pragma unroll
    for (int p = 0; p < P; ++p) dh[p] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < KH; ++q)
#pragma unroll
      for (int p = 0; p < P; ++p) dh[p] = mfma4(z2T[p][(4 * q + ak) * IN_ROWS + ar], wr2t[q], dh[p]);
#pragma unroll
    for (int p = 0; p < P; ++p) {
      f32x4 dz;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + 4 * ak + r;
        const bool ok = jv && row < B;
        const long long at = (((long long)row * R + s) * P + p) * H + j;
        const float h = ok ? sv_h1[at] : 0.f;
        dz[r] = ok ? dh[p][r] * (1.f - h * h) : 0.f;
        if (ok) dz1_out[at] = dz[r];
      }
      *reinterpret_cast<f32x4*>(&z1T[p][j * IN_ROWS + 4 * ak]) = dz;
    }
    __syncthreads();
    // ---- relation layer 1: this wave's share of d[s_i, s_j]
#pragma unroll
    for (int p = 0; p < P; ++p) {
      f32x4 px = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int q = 0; q < 4; ++q) px = mfma4(z1T[p][(16 * w + 4 * q + ak) * IN_ROWS + ar], wr1t[q], px);
      if (ar < 8) *reinterpret_cast<f32x4*>(&xpr[w][p][ar * IN_ROWS + 4 * ak]) = px;
    }
    __syncthreads();
    // ---- ds_i: receiver pairs, sender pairs, object row; each summed over the waves in wave order
#pragma unroll
    for (int i = 0; i < K; ++i) {
      float ds = 0.f;
#pragma unroll
      for (int jj = 0; jj < K; ++jj) {
        if (jj == i) continue;
        float v = 0.f;
        for (int ww = 0; ww < NW; ++ww) v += xpr[ww][in_pair(i, jj, K)][ak * IN_ROWS + ar];
        ds += v;
      }
#pragma unroll
      for (int jj = 0; jj < K; ++jj) {
        if (jj == i) continue;
        float v = 0.f;
        for (int ww = 0; ww < NW; ++ww) v += xpr[ww][in_pair(jj, i, K)][(4 + ak) * IN_ROWS + ar];
        ds += v;
      }
      float v = 0.f;
      for (int ww = 0; ww < NW; ++ww) v += xpo[ww][i][ak * IN_ROWS + ar];
      ds += v;
      ga[i] += ds / S;
    }
  }
  if (w == 0 && av) {
#pragma unroll
    for (int i = 0; i < K; ++i) {
      float v = ga[i];
      if (dpvs) v += dpvs[(long long)arow * (R + 1) * D2 + in_col(i, ak, D)];
      if (ak < 2) dpos0[(long long)arow * D + 2 * i + ak] = v;
      else if (dvel0) dvel0[((long long)i * B + arow) * 2 + (ak - 2)] = v;
    }
  }
}

static int in_shape_ok(const char* who, int B, int D, int H, int R) {
  if ((D != 4 && D != 6) || H < 4 || H > IN_HMAX || H % 4 != 0) {
    paig_set_error("%s: unsupported shape D=%d H=%d (D in {4, 6}, H a multiple of 4 in [4, %d])", who, D, H, IN_HMAX);
    return PAIG_E_UNSUPPORTED;
  }
  PAIG_REQUIRE(B >= 0 && R >= 1 && (long long)B * R * 6 * (4 + H) < (1ll << 31), "%s: B=%d R=%d out of range", who, B, R);
  return 0;
}

static int in_ws_ok(const char* who, const void* ws, size_t ws_bytes, const InWs& L) {
  if (ws_bytes < L.total * sizeof(float)) {
    paig_set_error("%s: workspace of %zu bytes, %zu needed", who, ws_bytes, L.total * sizeof(float));
    return PAIG_E_UNSUPPORTED;
  }
  PAIG_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "%s: workspace not 16-byte aligned", who);
  return 0;
}

}  // namespace

extern "C" {

size_t paig_rollout_in_workspace(int B, int D, int H, int R) {
  if (B <= 0 || (D != 4 && D != 6) || H <= 0 || R <= 0) return 0;
  return in_ws(B, D, H, R).total * sizeof(float);
}

int paig_rollout_in_fwd(const float* pos0, long long pos0_ld, const float* vel0, const float* w_r1, const float* b_r1,
                        const float* w_r2, const float* b_r2, const float* w_o1, const float* b_o1, const float* w_o2,
                        const float* b_o2, float half, float* pvs, void* ws, size_t ws_bytes, int B, int D, int H,
                        int R, void* stream) {
  if (int rc = in_shape_ok("paig_rollout_in_fwd", B, D, H, R)) return rc;
  if (B == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  PAIG_REQUIRE(pos0 && w_r1 && b_r1 && w_r2 && b_r2 && w_o1 && b_o1 && w_o2 && b_o2 && pvs,
               "paig_rollout_in_fwd: null operand");
  PAIG_REQUIRE(half > 0.f, "paig_rollout_in_fwd: half=%g", (double)half);
  float *xr = nullptr, *h1 = nullptr, *e = nullptr, *xo = nullptr, *ho = nullptr;
  if (ws) {
    const InWs L = in_ws(B, D, H, R);
    if (int rc = in_ws_ok("paig_rollout_in_fwd", ws, ws_bytes, L)) return rc;
    float* f = (float*)ws;
    xr = f + L.xr, h1 = f + L.h1, e = f + L.e, xo = f + L.xo, ho = f + L.ho;
  }
  LEARNED_DISPATCH(in_fwd_k, pos0, pos0_ld, vel0, w_r1, b_r1, w_r2, b_r2, w_o1, b_o1, w_o2, b_o2, half, pvs, xr, h1, e,
                   xo, ho, B, H, R);
  PAIG_CHECK_LAUNCH();
  return 0;
}

int paig_rollout_in_bwd(const float* dpos_roll, const float* dpvs, const float* w_r1, const float* w_r2,
                        const float* w_o1, const float* w_o2, float half, float* dpos0, float* dvel0, float* dw_r1,
                        float* db_r1, float* dw_r2, float* db_r2, float* dw_o1, float* db_o1, float* dw_o2,
                        float* db_o2, int accumulate, void* ws, size_t ws_bytes, int B, int D, int H, int R,
                        void* stream) {
  if (int rc = in_shape_ok("paig_rollout_in_bwd", B, D, H, R)) return rc;
  if (B == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  PAIG_REQUIRE(w_r1 && w_r2 && w_o1 && w_o2 && dpos0 && dw_r1 && db_r1 && dw_r2 && db_r2 && dw_o1 && db_o1 && dw_o2 &&
                   db_o2 && ws,
               "paig_rollout_in_bwd: null operand");
  PAIG_REQUIRE(half > 0.f, "paig_rollout_in_bwd: half=%g", (double)half);
  const InWs L = in_ws(B, D, H, R);
  if (int rc = in_ws_ok("paig_rollout_in_bwd", ws, ws_bytes, L)) return rc;
  float* f = (float*)ws;
  float *dz1 = f + L.dz1, *dz2 = f + L.dz2, *dzo = f + L.dzo, *dy = f + L.dy;
  LEARNED_DISPATCH(in_bwd_k, dpos_roll, dpvs, w_r1, w_r2, w_o1, w_o2, half, f + L.h1, f + L.e, f + L.ho, dz1, dz2, dzo,
                   dy, dpos0, dvel0, B, H, R);
  PAIG_CHECK_LAUNCH();
  // ---- weight gradients: sums over all pair / object rows, off the serial chain
  const int K = D / 2, pr = B * R * K * (K - 1), orows = B * R * K, HO = 4 + H;
  const float beta = accumulate ? 1.f : 0.f;
  int rc;
  if ((rc = learned_wgrad(H, 8, pr, dz1, f + L.xr, beta, dw_r1, f + L.gemm, L.gemm_floats, stream))) return rc;
  if ((rc = learned_wgrad(H, H, pr, dz2, f + L.h1, beta, dw_r2, f + L.gemm, L.gemm_floats, stream))) return rc;
  if ((rc = learned_wgrad(H, HO, orows, dzo, f + L.xo, beta, dw_o1, f + L.gemm, L.gemm_floats, stream))) return rc;
  if ((rc = learned_wgrad(4, H, orows, dy, f + L.ho, beta, dw_o2, f + L.gemm, L.gemm_floats, stream))) return rc;
  // ---- bias gradients: column sums in a fixed order
  if ((rc = paig_colsum(dz1, pr, H, H, db_r1, accumulate, f + L.colsum, stream))) return rc;
  if ((rc = paig_colsum(dz2, pr, H, H, db_r2, accumulate, f + L.colsum, stream))) return rc;
  if ((rc = paig_colsum(dzo, orows, H, H, db_o1, accumulate, f + L.colsum, stream))) return rc;
  return paig_colsum(dy, orows, 4, 4, db_o2, accumulate, f + L.colsum, stream);
}

}  // extern "C"

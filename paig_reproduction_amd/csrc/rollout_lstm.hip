// Black-box rollout cell: an LSTM (nn.LSTMCell gate order i, f, g, o) with a
// linear read-out that moves positions and velocities, all R steps in one
// launch, and its backpropagation through time.
//
//   x_t = [(pos_t - s) / s, vel_t / s]                  s = frame side / 2
//   z   = W_ih x_t + b_ih + W_hh h_t + b_hh             h_0 = c_0 = 0
//   c'  = sig(z_f) c + sig(z_i) tanh(z_g);  h' = sig(z_o) tanh(c')
//   y   = W_p h' + b_p;  pos' = pos + s y[:D];  vel' = vel + s y[D:]
//
// The reference has no working counterpart (its "lstm" table entry cannot be
// called by its rollout, physics_models.py:233); this is the learned cell in
// the place of cells.py's equations, same pos_vel_seq layout as
// paig_rollout_fwd.
//
// Layout of one block: 16 sequences (the M of a 16x16x4 f32 MFMA tile) and one
// wave per 16 hidden units.  The kernel is a serial chain of R small matrix
// products, so the weights stay where the chain needs no memory round trip:
// each wave holds the B operands of its four gate tiles (W_ih | W_hh rows of
// its 16 hidden units, one 4x16 tile per VGPR) in registers for the whole
// rollout.  h_t crosses waves through LDS (transposed, [k][row], so the A
// operand reads are conflict-free and the accumulator writes are 16-byte
// stores); the four gates of one hidden unit land in the same lane, so the
// cell update needs no exchange.  The read-out is split over the waves (each
// multiplies its own 16 hidden units) and summed in wave order by every lane
// that needs the value: two block barriers per step, no atomics.
// Products are exact f32 (v_mfma_f32_16x16x4_f32).
#include <algorithm>

#include "rollout_learned.h"

namespace {

constexpr int LSTM_HMAX = 128;   // hidden units (8 waves of 16)
constexpr int LSTM_ROWS = 16;    // sequences per block

static_assert(LSTM_ROWS == LEARNED_ROWS, "the grid of LEARNED_DISPATCH");
// finite for every finite x: exp(-x) = inf gives 1 / inf = 0
__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

// the saved state of one forward (floats from the workspace base), then the
// backward's own buffers; every region a multiple of 4 floats
struct LstmWs {
  size_t gates, c, hn, hp, x, dz, dy, gemm, colsum, total;
  size_t gemm_floats;
};
static LstmWs lstm_ws(int B, int D, int H, int R) {
  const size_t rows = (size_t)B * R;
  LstmWs w;
  size_t o = 0;
  w.gates = o, o += rows * 4 * H;
  w.c = o, o += rows * H;
  w.hn = o, o += rows * H;
  w.hp = o, o += rows * H;
  w.x = o, o += rows * 2 * D;
  w.dz = o, o += rows * 4 * H;
  w.dy = o, o += rows * 2 * D;
  size_t g = paig_gemm_workspace(4 * H, 2 * D, (int)rows);
  g = std::max(g, paig_gemm_workspace(4 * H, H, (int)rows));
  g = std::max(g, paig_gemm_workspace(2 * D, H, (int)rows));
  g = (g + 3) & ~(size_t)3;
  w.gemm = o, o += g;
  w.gemm_floats = g;
  w.colsum = o, o += (paig_colsum_workspace((int)rows, 4 * H) + 3) & ~(size_t)3;
  w.total = o;
  return w;
}

// KX = 2D / 4 k-steps of x, KH >= H / 4 k-steps of h (weights past H are zero)
template <int KX, int KH>
__global__ void __launch_bounds__(512)
lstm_fwd_k(const float* __restrict__ pos0, long long pos0_ld, const float* __restrict__ vel0,
           const float* __restrict__ w_ih, const float* __restrict__ w_hh, const float* __restrict__ b_ih,
           const float* __restrict__ b_hh, const float* __restrict__ w_p, const float* __restrict__ b_p, float S,
           float* __restrict__ pvs, float* __restrict__ sv_gates, float* __restrict__ sv_c, float* __restrict__ sv_hn,
           float* __restrict__ sv_hp, float* __restrict__ sv_x, int B, int H, int R) {
  constexpr int D = 2 * KX, D2 = 4 * KX;
  __shared__ __attribute__((aligned(16))) float hT[2][LSTM_HMAX * LSTM_ROWS];   // h transposed: [k][row]
  __shared__ __attribute__((aligned(16))) float yp[8][16 * LSTM_ROWS];          // read-out partials: [wave][col][row]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, NW = blockDim.x >> 6;
  const int ar = lane & 15, ak = lane >> 4;   // A operand: row ar, k offset ak; C: column ar, rows 4 ak + r
  const int row0 = blockIdx.x * LSTM_ROWS;
  const int j = 16 * w + ar;                  // hidden unit of this lane's B / C column
  const bool jv = j < H;

  // ---- stationary B operands: gate g, k-step ks -> W[g H + j][4 ks + ak]
  float wg[4][KX + KH], bz[4], wp[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
#pragma unroll
    for (int ks = 0; ks < KX; ++ks) wg[g][ks] = jv ? w_ih[(long long)(g * H + j) * D2 + 4 * ks + ak] : 0.f;
#pragma unroll
    for (int q = 0; q < KH; ++q) {
      const int k = 4 * q + ak;
      wg[g][KX + q] = (jv && k < H) ? w_hh[(long long)(g * H + j) * H + k] : 0.f;
    }
    bz[g] = jv ? b_ih[g * H + j] + b_hh[g * H + j] : 0.f;
  }
  // read-out over this wave's own 16 hidden units: B[k][n = ar] = W_p[n][16 w + 4 q + ak]
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int k = 16 * w + 4 * q + ak;
    wp[q] = (ar < D2 && k < H) ? w_p[(long long)ar * H + k] : 0.f;
  }
  // ---- the moving state in A-operand layout: lane (ar, ak) holds column 4 ks + ak of sequence row0 + ar
  const int arow = row0 + ar;
  const bool av = arow < B;
  float sv[KX], bp[KX];
#pragma unroll
  for (int ks = 0; ks < KX; ++ks) {
    const int col = 4 * ks + ak;
    bp[ks] = b_p[col];
    float v = 0.f;
    if (av) {
      if (col < D) v = pos0[(long long)arow * pos0_ld + col];
      else if (vel0) v = vel0[((long long)((col - D) >> 1) * B + arow) * 2 + ((col - D) & 1)];
    }
    sv[ks] = v;
    if (w == 0 && av) pvs[(long long)arow * (R + 1) * D2 + col] = v;
  }
  for (int i = threadIdx.x; i < 2 * LSTM_HMAX * LSTM_ROWS; i += blockDim.x) (&hT[0][0])[i] = 0.f;
  float c[4] = {0.f, 0.f, 0.f, 0.f}, hprev[4] = {0.f, 0.f, 0.f, 0.f};
  __syncthreads();

  for (int t = 0; t < R; ++t) {
    const float* cur = hT[t & 1];
    float* nxt = hT[(t + 1) & 1];
    float xa[KX];
#pragma unroll
    for (int ks = 0; ks < KX; ++ks) xa[ks] = (4 * ks + ak < D) ? (sv[ks] - S) / S : sv[ks] / S;
    f32x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = f32x4{bz[g], bz[g], bz[g], bz[g]};
#pragma unroll
    for (int ks = 0; ks < KX; ++ks)
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g] = mfma4(xa[ks], wg[g][ks], acc[g]);
#pragma unroll
    for (int q = 0; q < KH; ++q) {
      const float a = cur[(4 * q + ak) * LSTM_ROWS + ar];
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g] = mfma4(a, wg[g][KX + q], acc[g]);
    }
    // ---- cell update: the four gates of (row 4 ak + r, unit j) are in this lane
    f32x4 hn;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float gi = sigm(acc[0][r]), gf = sigm(acc[1][r]), gg = tanhf(acc[2][r]), go = sigm(acc[3][r]);
      c[r] = gf * c[r] + gi * gg;
      hn[r] = jv ? go * tanhf(c[r]) : 0.f;
      const int row = row0 + 4 * ak + r;
      if (sv_gates && jv && row < B) {
        const long long rt = (long long)row * R + t;
        float* gt = sv_gates + rt * 4 * H + j;
        gt[0] = gi, gt[H] = gf, gt[2 * H] = gg, gt[3 * H] = go;
        sv_c[rt * H + j] = c[r];
        sv_hn[rt * H + j] = hn[r];
        sv_hp[rt * H + j] = hprev[r];
      }
      hprev[r] = hn[r];
    }
    *reinterpret_cast<f32x4*>(nxt + j * LSTM_ROWS + 4 * ak) = hn;
    if (sv_x && w == 0 && av) {
#pragma unroll
      for (int ks = 0; ks < KX; ++ks) sv_x[((long long)arow * R + t) * D2 + 4 * ks + ak] = xa[ks];
    }
    __syncthreads();
    // ---- read-out partial over this wave's hidden units
    f32x4 pa = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q) pa = mfma4(nxt[(16 * w + 4 * q + ak) * LSTM_ROWS + ar], wp[q], pa);
    *reinterpret_cast<f32x4*>(&yp[w][ar * LSTM_ROWS + 4 * ak]) = pa;
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < KX; ++ks) {
      float y = bp[ks];
      for (int ww = 0; ww < NW; ++ww) y += yp[ww][(4 * ks + ak) * LSTM_ROWS + ar];
      sv[ks] = sv[ks] + S * y;
      if (w == 0 && av) pvs[((long long)arow * (R + 1) + t + 1) * D2 + 4 * ks + ak] = sv[ks];
    }
  }
}

// Backward through time: t = R .. 1 in one launch, carrying dh, dc (in the
// accumulator layout) and the position / velocity adjoints (in the A-operand
// layout).  Stationary B operands: W_p (dh += dy W_p), W_hh (dh_prev = dz
// W_hh, K = 4 H split per gate over four accumulators) and this wave's rows
// of W_ih (dx = dz W_ih, summed over the waves in wave order).
template <int KX, int KH>
__global__ void __launch_bounds__(512)
lstm_bwd_k(const float* __restrict__ dpos_roll, const float* __restrict__ dpvs, const float* __restrict__ w_ih,
           const float* __restrict__ w_hh, const float* __restrict__ w_p, float S, const float* __restrict__ sv_gates,
           const float* __restrict__ sv_c, float* __restrict__ dz_out, float* __restrict__ dy_out,
           float* __restrict__ dpos0, float* __restrict__ dvel0, int B, int H, int R) {
  constexpr int D = 2 * KX, D2 = 4 * KX;
  __shared__ __attribute__((aligned(16))) float dzT[4 * LSTM_HMAX * LSTM_ROWS];   // [gate][unit][row]
  __shared__ __attribute__((aligned(16))) float xp[8][16 * LSTM_ROWS];            // dx partials: [wave][col][row]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, NW = blockDim.x >> 6;
  const int ar = lane & 15, ak = lane >> 4;
  const int row0 = blockIdx.x * LSTM_ROWS;
  const int j = 16 * w + ar;
  const bool jv = j < H;

  float whh[4][KH], wih[4][4], wpt[KX];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
#pragma unroll
    for (int q = 0; q < KH; ++q) {   // B[k = g H + m][j] = W_hh[g H + m][j], m = 4 q + ak
      const int m = 4 * q + ak;
      whh[g][q] = (jv && m < H) ? w_hh[(long long)(g * H + m) * H + j] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {    // B[k = g H + m][n = ar] = W_ih[g H + m][n], m in this wave's units
      const int m = 16 * w + 4 * q + ak;
      wih[g][q] = (ar < D2 && m < H) ? w_ih[(long long)(g * H + m) * D2 + ar] : 0.f;
    }
  }
#pragma unroll
  for (int ks = 0; ks < KX; ++ks) wpt[ks] = jv ? w_p[(long long)(4 * ks + ak) * H + j] : 0.f;   // B[k = n][j] = W_p[n][j]

  const int arow = row0 + ar;
  const bool av = arow < B;
  float ga[KX];
#pragma unroll
  for (int ks = 0; ks < KX; ++ks) ga[ks] = 0.f;
  f32x4 dh = {0.f, 0.f, 0.f, 0.f};
  float dc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int i = threadIdx.x; i < 4 * LSTM_HMAX * LSTM_ROWS; i += blockDim.x) dzT[i] = 0.f;

  // the saved gates and cell states of a step, in the accumulator layout
  // (zeros for rows past B and units past H: their dz is then zero);
  // fetched one step ahead of the serial chain
  float G[4][4], CN[4], CP[4], nG[4][4], nCN[4], nCP[4];
  auto fetch = [&](int s, float (&g4)[4][4], float (&cn)[4], float (&cp)[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + 4 * ak + r;
      const bool ok = jv && row < B;
      const long long rt = (long long)row * R + s;
#pragma unroll
      for (int g = 0; g < 4; ++g) g4[g][r] = ok ? sv_gates[rt * 4 * H + g * H + j] : 0.f;
      cn[r] = ok ? sv_c[rt * H + j] : 0.f;
      cp[r] = (ok && s > 0) ? sv_c[(rt - 1) * H + j] : 0.f;
    }
  };
  fetch(R - 1, nG, nCN, nCP);
  __syncthreads();

  for (int s = R - 1; s >= 0; --s) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int g = 0; g < 4; ++g) G[g][r] = nG[g][r];
      CN[r] = nCN[r], CP[r] = nCP[r];
    }
    // ---- adjoints arriving at step s + 1's outputs; dy = s (d pos', d vel')
    float dya[KX];
#pragma unroll
    for (int ks = 0; ks < KX; ++ks) {
      const int col = 4 * ks + ak;
      if (av) {
        if (dpos_roll && col < D) ga[ks] += dpos_roll[((long long)arow * R + s) * D + col];
        if (dpvs) ga[ks] += dpvs[((long long)arow * (R + 1) + s + 1) * D2 + col];
      }
      dya[ks] = S * ga[ks];
      if (w == 0 && av) dy_out[((long long)arow * R + s) * D2 + col] = dya[ks];
    }
    f32x4 dht = dh;
#pragma unroll
    for (int ks = 0; ks < KX; ++ks) dht = mfma4(dya[ks], wpt[ks], dht);
    // ---- gate adjoints
    f32x4 dzv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float gi = G[0][r], gf = G[1][r], gg = G[2][r], go = G[3][r];
      const float tc = tanhf(CN[r]);
      const float dct = dc[r] + dht[r] * go * (1.f - tc * tc);
      dzv[0][r] = dct * gg * gi * (1.f - gi);
      dzv[1][r] = dct * CP[r] * gf * (1.f - gf);
      dzv[2][r] = dct * gi * (1.f - gg * gg);
      dzv[3][r] = dht[r] * tc * go * (1.f - go);
      dc[r] = dct * gf;
      const int row = row0 + 4 * ak + r;
      if (jv && row < B) {
        float* o = dz_out + ((long long)row * R + s) * 4 * H + j;
        o[0] = dzv[0][r], o[H] = dzv[1][r], o[2 * H] = dzv[2][r], o[3 * H] = dzv[3][r];
      }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) *reinterpret_cast<f32x4*>(dzT + (g * LSTM_HMAX + j) * LSTM_ROWS + 4 * ak) = dzv[g];
    __syncthreads();
    if (s > 0) fetch(s - 1, nG, nCN, nCP);
    // ---- dh of the previous step and this wave's share of dx
    f32x4 a4[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) a4[g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < KH; ++q)
#pragma unroll
      for (int g = 0; g < 4; ++g) a4[g] = mfma4(dzT[(g * LSTM_HMAX + 4 * q + ak) * LSTM_ROWS + ar], whh[g][q], a4[g]);
    dh = (a4[0] + a4[1]) + (a4[2] + a4[3]);
    f32x4 px = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        px = mfma4(dzT[(g * LSTM_HMAX + 16 * w + 4 * q + ak) * LSTM_ROWS + ar], wih[g][q], px);
    *reinterpret_cast<f32x4*>(&xp[w][ar * LSTM_ROWS + 4 * ak]) = px;
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < KX; ++ks) {
      float dx = 0.f;
      for (int ww = 0; ww < NW; ++ww) dx += xp[ww][(4 * ks + ak) * LSTM_ROWS + ar];
      ga[ks] += dx / S;
    }
  }
  if (w == 0 && av) {
#pragma unroll
    for (int ks = 0; ks < KX; ++ks) {
      const int col = 4 * ks + ak;
      float v = ga[ks];
      if (dpvs) v += dpvs[(long long)arow * (R + 1) * D2 + col];
      if (col < D) dpos0[(long long)arow * D + col] = v;
      else if (dvel0) dvel0[((long long)((col - D) >> 1) * B + arow) * 2 + ((col - D) & 1)] = v;
    }
  }
}

static int lstm_shape_ok(const char* who, int B, int D, int H, int R) {
  if ((D != 4 && D != 6) || H < 4 || H > LSTM_HMAX || H % 4 != 0) {
    paig_set_error("%s: unsupported shape D=%d H=%d (D in {4, 6}, H a multiple of 4 in [4, %d])", who, D, H, LSTM_HMAX);
    return PAIG_E_UNSUPPORTED;
  }
  PAIG_REQUIRE(B >= 0 && R >= 1 && (long long)B * R * 4 * H < (1ll << 31), "%s: B=%d R=%d out of range", who, B, R);
  return 0;
}

}  // namespace

extern "C" {

size_t paig_rollout_lstm_workspace(int B, int D, int H, int R) {
  if (B <= 0 || D <= 0 || H <= 0 || R <= 0) return 0;
  return lstm_ws(B, D, H, R).total * sizeof(float);
}

int paig_rollout_lstm_fwd(const float* pos0, long long pos0_ld, const float* vel0, const float* w_ih,
                          const float* w_hh, const float* b_ih, const float* b_hh, const float* w_p, const float* b_p,
                          float half, float* pvs, void* ws, size_t ws_bytes, int B, int D, int H, int R,
                          void* stream) {
  if (int rc = lstm_shape_ok("paig_rollout_lstm_fwd", B, D, H, R)) return rc;
  if (B == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  PAIG_REQUIRE(pos0 && w_ih && w_hh && b_ih && b_hh && w_p && b_p && pvs, "paig_rollout_lstm_fwd: null operand");
  PAIG_REQUIRE(half > 0.f, "paig_rollout_lstm_fwd: half=%g", (double)half);
  float *g = nullptr, *c = nullptr, *hn = nullptr, *hp = nullptr, *x = nullptr;
  if (ws) {
    const LstmWs L = lstm_ws(B, D, H, R);
    PAIG_REQUIRE(ws_bytes >= L.total * sizeof(float) && (reinterpret_cast<uintptr_t>(ws) & 15) == 0,
                 "paig_rollout_lstm_fwd: workspace of %zu bytes, %zu needed (16-byte aligned)", ws_bytes,
                 L.total * sizeof(float));
    float* f = (float*)ws;
    g = f + L.gates, c = f + L.c, hn = f + L.hn, hp = f + L.hp, x = f + L.x;
  }
  LEARNED_DISPATCH(lstm_fwd_k, pos0, pos0_ld, vel0, w_ih, w_hh, b_ih, b_hh, w_p, b_p, half, pvs, g, c, hn, hp, x, B, H,
                   R);
  PAIG_CHECK_LAUNCH();
  return 0;
}

int paig_rollout_lstm_bwd(const float* dpos_roll, const float* dpvs, const float* w_ih, const float* w_hh,
                          const float* w_p, float half, float* dpos0, float* dvel0, float* dw_ih, float* dw_hh,
                          float* db_ih, float* db_hh, float* dw_p, float* db_p, int accumulate, void* ws,
                          size_t ws_bytes, int B, int D, int H, int R, void* stream) {
  if (int rc = lstm_shape_ok("paig_rollout_lstm_bwd", B, D, H, R)) return rc;
  if (B == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  PAIG_REQUIRE(w_ih && w_hh && w_p && dpos0 && dw_ih && dw_hh && db_ih && db_hh && dw_p && db_p && ws,
               "paig_rollout_lstm_bwd: null operand");
  PAIG_REQUIRE(half > 0.f, "paig_rollout_lstm_bwd: half=%g", (double)half);
  const LstmWs L = lstm_ws(B, D, H, R);
  PAIG_REQUIRE(ws_bytes >= L.total * sizeof(float) && (reinterpret_cast<uintptr_t>(ws) & 15) == 0,
               "paig_rollout_lstm_bwd: workspace of %zu bytes, %zu needed (16-byte aligned)", ws_bytes,
               L.total * sizeof(float));
  float* f = (float*)ws;
  float *dz = f + L.dz, *dy = f + L.dy;
  LEARNED_DISPATCH(lstm_bwd_k, dpos_roll, dpvs, w_ih, w_hh, w_p, half, f + L.gates, f + L.c, dz, dy, dpos0, dvel0, B, H,
                   R);
  PAIG_CHECK_LAUNCH();
  // ---- weight gradients: sums over all B R rows, off the serial chain
  const int rows = B * R, H4 = 4 * H, D2 = 2 * D;
  const float beta = accumulate ? 1.f : 0.f;
  int rc;
  if ((rc = learned_wgrad(H4, D2, rows, dz, f + L.x, beta, dw_ih, f + L.gemm, L.gemm_floats, stream))) return rc;
  if ((rc = learned_wgrad(H4, H, rows, dz, f + L.hp, beta, dw_hh, f + L.gemm, L.gemm_floats, stream))) return rc;
  if ((rc = learned_wgrad(D2, H, rows, dy, f + L.hn, beta, dw_p, f + L.gemm, L.gemm_floats, stream))) return rc;
  // ---- bias gradients: column sums in a fixed order
  if ((rc = paig_colsum(dz, rows, H4, H4, db_ih, accumulate, f + L.colsum, stream))) return rc;
  if ((rc = paig_colsum(dz, rows, H4, H4, db_hh, accumulate, f + L.colsum, stream))) return rc;
  return paig_colsum(dy, rows, D2, D2, db_p, accumulate, f + L.colsum, stream);
}

}  // extern "C"

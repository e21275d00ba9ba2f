// What the two learned rollout cells (rollout_lstm.hip, rollout_in.hip) share:
// their f32 MFMA step, the (K, KH) launch dispatch of their kernels and the
// weight-gradient GEMM of their backwards.  Both lay a block out as 16
// sequences by one wave per 16 hidden units.
#pragma once

#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int LEARNED_ROWS = 16;   // sequences per block (the M of a 16x16x4 f32 MFMA tile)

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// dW [M][N] (= or +=, beta) A^T B over `rows` rows of A [rows][M] and B [rows][N]
static int learned_wgrad(int M, int N, int rows, const float* A, const float* B, float beta, float* dW, float* ws,
                         size_t ws_floats, void* stream) {
  return paig_gemm(1, 0, M, N, rows, 1.f, A, M, B, N, beta, dW, N, nullptr, 0, 0, nullptr, 0, nullptr, ws, ws_floats,
                   stream);
}

}  // namespace

// Launches KERNEL<K, KH> for the caller's B, D, H on its stream st; KH: the
// bucket of H, the smallest instantiated count of hidden k-steps >= H / 4
#define LEARNED_DISPATCH(KERNEL, ...)                                                                      \
  do {                                                                                                     \
    const int kh = H / 4;                                                                                  \
    const dim3 grid(cdiv(B, LEARNED_ROWS)), block(64 * cdiv(H, 16));                                       \
    if (D == 4 && kh <= 8) hipLaunchKernelGGL((KERNEL<2, 8>), grid, block, 0, st, __VA_ARGS__);            \
    else if (D == 4 && kh <= 16) hipLaunchKernelGGL((KERNEL<2, 16>), grid, block, 0, st, __VA_ARGS__);     \
    else if (D == 4 && kh <= 25) hipLaunchKernelGGL((KERNEL<2, 25>), grid, block, 0, st, __VA_ARGS__);     \
    else if (D == 4) hipLaunchKernelGGL((KERNEL<2, 32>), grid, block, 0, st, __VA_ARGS__);                 \
    else if (kh <= 8) hipLaunchKernelGGL((KERNEL<3, 8>), grid, block, 0, st, __VA_ARGS__);                 \
    else if (kh <= 16) hipLaunchKernelGGL((KERNEL<3, 16>), grid, block, 0, st, __VA_ARGS__);               \
    else if (kh <= 25) hipLaunchKernelGGL((KERNEL<3, 25>), grid, block, 0, st, __VA_ARGS__);               \
    else hipLaunchKernelGGL((KERNEL<3, 32>), grid, block, 0, st, __VA_ARGS__);                             \
  } while (0)

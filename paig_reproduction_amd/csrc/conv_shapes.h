// (CIN, COUT, H, KS) of the ShallowUNet(hidden 8) convolutions at 32 x 32, the
// shapes both MFMA tiers instantiate (conv_mfma.hip: all it has;
// conv_split.hip: the head of its lists).  FWD: forward and dgrad kernel
// shapes (a dgrad's shape is (layer Cout, layer Cin)); WG: weight gradients;
// UP: the convs whose input is the fused 2x upsample (c7, c10).
#pragma once
#define PAIG_SUNET32_FWD(X)                                                                               \
  X(3, 8, 32, 3) X(8, 8, 32, 3) X(8, 16, 16, 3) X(16, 16, 16, 3) X(16, 32, 8, 3) X(32, 32, 8, 3)         \
  X(32, 16, 16, 3) X(16, 16, 32, 3) X(24, 8, 32, 3) X(8, 2, 32, 1) X(16, 8, 16, 3) X(8, 24, 32, 3)       \
  X(2, 8, 32, 1) X(32, 16, 8, 3) X(16, 32, 16, 3)
#define PAIG_SUNET32_WG(X)                                                                                \
  X(3, 8, 32, 3) X(8, 8, 32, 3) X(8, 16, 16, 3) X(16, 16, 16, 3) X(16, 32, 8, 3) X(32, 32, 8, 3)         \
  X(32, 16, 16, 3) X(16, 16, 32, 3) X(24, 8, 32, 3) X(8, 2, 32, 1)
#define PAIG_SUNET32_UP(X) X(32, 16, 16, 3) X(16, 16, 32, 3)

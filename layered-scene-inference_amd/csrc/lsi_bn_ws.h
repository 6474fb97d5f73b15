// The batch-norm workspace, shared by lsi_bn.hip and the convolution kernels
// that leave the statistics there in their epilogue.
#pragma once

// Batch-norm workspace layout per group, in floats (lsi_bn.hip; the convolution
// kernels that accumulate the statistics in their epilogue write the same
// places): [0] arrival counter (int), [ACC, ACC + 4096) the accumulators -- both
// zero between launches --, from CONST the 2 C constants of the second pass and
// (backward) the group's C sums of dz.
#define LSI_BN_WS_ACC 16
#define LSI_BN_WS_CONST (16 + 4096)
#define LSI_BN_WS_STRIDE (16 + 4096 + 3 * 2048)
// Statistics left by a convolution's epilogue (lsi_conv2d_*_bnstats): plain sums
// of y and y * y in `lsi_bn_stat_slots(C)` copies of the accumulators (slot s of
// a group: ACC + s * 2 C; thousands of workgroups adding to the same two cache
// lines would take ~8 ns each, one after the other), folded, turned into the
// constants and cleared by lsi_bn_relu_norm.
// The hand-over is checked on the device: the producer's first workgroup of a
// group leaves LSI_BN_TAG(C, groups) in the group's word [1]; lsi_bn_relu_norm
// expects exactly that tag, the kernels that accumulate their own statistics
// (lsi_bn_relu_fwd / _bwd) expect 0.  A kernel that finds something else writes
// NaN constants (its output is NaN: loud in any loss), and clears accumulators
// and tag, so that the calls after it are right again.
#define LSI_BN_WS_TAG 1
#define LSI_BN_TAG(C, groups) (0x5A000000 | (((groups) & 0xfff) << 12) | ((C) & 0xfff))
static inline int lsi_bn_stat_slots(int C) {
  int ns = 1;
  while (ns < 32 && 2 * ns * 2 * C <= 4096) ns *= 2;
  return ns;
}

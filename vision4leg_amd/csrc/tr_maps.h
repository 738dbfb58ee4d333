// vision4leg_amd — lane -> LDS offset maps of the conv weight-grads' transposed operand reads (ds_read_b64_tr_b16, gfx950).
// Plain constexpr arithmetic with no HIP in it: csrc/bwd.h builds its addresses from these functions and
// tools/host/tr_maps_check.cpp replays them on the CPU against the element-by-element gathers they replace.
//
// The instruction, per group of 16 consecutive lanes: lane 4q + p supplies the address of block row q, columns 4p .. 4p+3
// (4 contiguous 16-bit elements, 8-byte aligned); lane i receives column i of the four rows, row q in element q. With the block's
// rows = contraction indices and its columns = the operand's 16 rows, two reads (h = 0, 1) give lane (fr = lane & 15, g = lane >> 4)
// the elements k = 8g .. 8g+7 of row fr: the operand of mma_k32 (common.h). So in every map below the lane's k is
//   tr_k(lane, h) = 8 (lane >> 4) + 4 h + ((lane & 15) >> 2)      and its first column is      tr_c(lane) = 4 (lane & 3).
// All offsets are in elements of the 16-bit operand type.
#pragma once
#if defined(__HIPCC__)
#define V4L_TRMAP __host__ __device__ constexpr
#else
#define V4L_TRMAP constexpr
#endif

namespace v4l {
namespace trmap {

constexpr int LC1 = 40;      // c1 rows [225 pixels][32 ci + 8]
constexpr int LT = 72;       // dc2 rows [48 pixels][64 co + 8]; rows 36..47 are zeros
constexpr int LD1 = 40;      // dc1 rows [256 pixels][32 co + 8]; rows 225..255 are zeros
constexpr int L3 = 72;       // conv3 weight-grad: dc3 rows [17][64 co + 8] (row 16: zeros), c2 rows [C2R][64 ci + 8]
constexpr int C2R = 36 + 15; // c2 rows 36..50 are zeros: the zero K half reads row 36 + a tap's offset (<= 2*6 + 2 rows)

V4L_TRMAP int tr_k(int lane, int h) { return 8 * (lane >> 4) + 4 * h + ((lane & 15) >> 2); }
V4L_TRMAP int tr_c(int lane) { return 4 * (lane & 3); }

// ---- dW2 += dc2^T col(c1): K = output pixel pos = 32 st + k (pos >= 36: dc2 reads a zero row, c1 only stays in bounds: pixel 0)
// A (c1): address = dw2_a_lane(st, lane, h) + dw2_a_tile(kt); rows = c1 pixels (2 oy + ky, 2 ox + kx), columns = ci 16 (kt & 1) ..+15
V4L_TRMAP int dw2_a_lane(int st, int lane, int h) {
  const int pos = st * 32 + tr_k(lane, h), pp = pos < 36 ? pos : 0, oy = pp / 6, ox = pp - oy * 6;
  return (2 * oy * 15 + 2 * ox) * LC1 + tr_c(lane);
}
V4L_TRMAP int dw2_a_tile(int kt) {
  const int tap = kt >> 1, ky = tap >> 2, kx = tap & 3;
  return (ky * 15 + kx) * LC1 + (kt & 1) * 16;
}
// B (dc2 [pixel][co]): address = dw2_b_lane(st, lane, h) + 16 c for co tile c
V4L_TRMAP int dw2_b_lane(int st, int lane, int h) {
  const int pos = st * 32 + tr_k(lane, h);
  return (pos < 36 ? pos : 36) * LT + tr_c(lane);
}

// ---- dW1 += dc1^T col(image): K = output pixel pos = 32 st + k (pos >= 225: dc1 rows are zeros, the image reads pixel 0)
// A (one image channel [64][64]): address = dw1_a_lane(st, lane, h) + dw1_a_tile(kyt); the block's 16 columns are the k-tile's two
// kernel rows ky = 2 kyt + {0, 1} x 8 kx, so lane 4q + p points at image row 4 oy + ky0 + (p >> 1), columns 4 ox + 4 (p & 1) ..+3
V4L_TRMAP int dw1_a_lane(int st, int lane, int h) {
  const int pos = st * 32 + tr_k(lane, h), pp = pos < 225 ? pos : 0, oy = pp / 15, ox = pp - oy * 15, p = lane & 3;
  return (4 * oy + (p >> 1)) * 64 + 4 * ox + 4 * (p & 1);
}
V4L_TRMAP int dw1_a_tile(int kyt) { return 2 * kyt * 64; }
// B (dc1 [pixel][co]): address = dw1_b_lane(st, lane, h) + 16 c
V4L_TRMAP int dw1_b_lane(int st, int lane, int h) { return (st * 32 + tr_k(lane, h)) * LD1 + tr_c(lane); }

// ---- dW3 += dc3^T col(c2): K = output pixel pos = 4 oy + ox < 16 in lane groups 0 and 1; groups 2 and 3 (k >= 16) read zero rows
// A (c2 [pixel][ci]): address = dw3_a_lane(lane, h) + dw3_a_tile(kt)
V4L_TRMAP int dw3_a_lane(int lane, int h) {
  const int pos = tr_k(lane, h);
  return (pos < 16 ? (pos >> 2) * 6 + (pos & 3) : 36) * L3 + tr_c(lane);
}
V4L_TRMAP int dw3_a_tile(int kt) {
  const int tap = kt >> 2, ky = tap / 3, kx = tap - ky * 3;
  return (ky * 6 + kx) * L3 + (kt & 3) * 16;
}
// B (dc3 [pixel][co]): address = dw3_b_lane(lane, h) + 16 c
V4L_TRMAP int dw3_b_lane(int lane, int h) {
  const int pos = tr_k(lane, h);
  return (pos < 16 ? pos : 16) * L3 + tr_c(lane);
}

}  // namespace trmap
}  // namespace v4l

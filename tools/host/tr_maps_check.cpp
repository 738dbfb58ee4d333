// CPU check of csrc/tr_maps.h (the lane -> LDS offset maps of the conv weight-grads' transposed operand reads): the transposed
// read is emulated on index-filled images, and for all 64 lanes and every (step, tile) the fragment it delivers must equal, element
// for element, what the gather expressions it replaces (csrc/bwd.h, the `TR == false` paths) read; every lane address must be
// 8-byte aligned and keep its 4 elements inside the image. No GPU, no HIP:
//   g++ -std=c++17 -O1 [-fsanitize=address,undefined] tools/host/tr_maps_check.cpp -o tr_maps_check && ./tr_maps_check
#include <cstdio>
#include <vector>
#include "../../vision4leg_amd/csrc/tr_maps.h"

using namespace v4l::trmap;

static int g_fail = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      if (g_fail++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
    }                                                     \
  } while (0)

constexpr int ZERO = -1;  // what an element of a zeroed pad row holds; every other element holds its own offset

// [rows][ld] image whose element (r, c) holds r * ld + c, rows >= zrow0 hold ZERO
static std::vector<int> index_image(int rows, int ld, int zrow0) {
  std::vector<int> v((size_t)rows * ld);
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < ld; ++c) v[(size_t)r * ld + c] = r < zrow0 ? r * ld + c : ZERO;
  return v;
}

// ds_read_b64_tr_b16 of one wave: off[lane] = the lane's element offset -> out[lane][0..3]
static void tr_read(const std::vector<int>& img, const int (&off)[64], int (&out)[64][4], const char* what) {
  for (int l = 0; l < 64; ++l) {
    CHECK((off[l] * 2) % 8 == 0, "%s: lane %d offset %d is not 8-byte aligned", what, l, off[l]);
    CHECK(off[l] >= 0 && (size_t)off[l] + 4 <= img.size(), "%s: lane %d offset %d out of bounds (%zu)", what, l, off[l], img.size());
  }
  for (int l = 0; l < 64; ++l) {
    const int grp = l & ~15, i = l & 15;
    for (int q = 0; q < 4; ++q) {
      const int o = off[grp + 4 * q + (i >> 2)] + (i & 3);  // column i of block row q: element i & 3 of lane 4q + (i >> 2)
      out[l][q] = o >= 0 && (size_t)o < img.size() ? img[o] : -2;
    }
  }
}

// the fragment two reads build: frag[lane][j], j = 4 h + q
template <class F>
static void tr_frag(const std::vector<int>& img, F lane_off, int (&frag)[64][8], const char* what) {
  for (int h = 0; h < 2; ++h) {
    int off[64], out[64][4];
    for (int l = 0; l < 64; ++l) off[l] = lane_off(l, h);
    tr_read(img, off, out, what);
    for (int l = 0; l < 64; ++l)
      for (int q = 0; q < 4; ++q) frag[l][4 * h + q] = out[l][q];
  }
}

int main() {
  int frag[64][8];
  // ---------------------------------------------------------------- dW2
  {
    const std::vector<int> c1 = index_image(225, LC1, 225), dc2 = index_image(48, LT, 36);
    for (int st = 0; st < 2; ++st) {
      for (int kt = 0; kt < 32; ++kt) {
        tr_frag(c1, [&](int l, int h) { return dw2_a_lane(st, l, h) + dw2_a_tile(kt); }, frag, "dW2 A");
        for (int l = 0; l < 64; ++l) {
          const int fr = l & 15, g = l >> 4, tap = kt >> 1, ci = (kt & 1) * 16 + fr, ky = tap >> 2, kx = tap & 3;
          for (int j = 0; j < 8; ++j) {
            const int pos = st * 32 + g * 8 + j, pp = pos < 36 ? pos : 0, oy = pp / 6, ox = pp - oy * 6;
            const int want = ((2 * oy + ky) * 15 + 2 * ox + kx) * LC1 + ci;
            CHECK(frag[l][j] == want, "dW2 A st %d kt %d lane %d j %d: %d != %d", st, kt, l, j, frag[l][j], want);
          }
        }
      }
      for (int c = 0; c < 4; ++c) {
        tr_frag(dc2, [&](int l, int h) { return dw2_b_lane(st, l, h) + 16 * c; }, frag, "dW2 B");
        for (int l = 0; l < 64; ++l)
          for (int j = 0; j < 8; ++j) {
            const int pos = st * 32 + (l >> 4) * 8 + j, want = pos < 36 ? pos * LT + c * 16 + (l & 15) : ZERO;  // dc2^T[co][pos], zeros from 36
            CHECK(frag[l][j] == want, "dW2 B st %d c %d lane %d j %d: %d != %d", st, c, l, j, frag[l][j], want);
          }
      }
    }
  }
  // ---------------------------------------------------------------- dW1
  {
    const std::vector<int> img = index_image(64, 64, 64), dc1 = index_image(256, LD1, 225);
    for (int st = 0; st < 8; ++st) {
      for (int kyt = 0; kyt < 4; ++kyt) {
        tr_frag(img, [&](int l, int h) { return dw1_a_lane(st, l, h) + dw1_a_tile(kyt); }, frag, "dW1 A");
        for (int l = 0; l < 64; ++l) {
          const int fr = l & 15, g = l >> 4, ky = kyt * 2 + (fr >> 3), kx = fr & 7;
          for (int j = 0; j < 8; ++j) {
            const int pos = st * 32 + g * 8 + j, pp = pos < 225 ? pos : 0, oy = pp / 15, ox = pp - oy * 15;
            const int want = (4 * oy) * 64 + 4 * ox + ky * 64 + kx;
            CHECK(frag[l][j] == want, "dW1 A st %d kyt %d lane %d j %d: %d != %d", st, kyt, l, j, frag[l][j], want);
          }
        }
      }
      for (int c = 0; c < 2; ++c) {
        tr_frag(dc1, [&](int l, int h) { return dw1_b_lane(st, l, h) + 16 * c; }, frag, "dW1 B");
        for (int l = 0; l < 64; ++l)
          for (int j = 0; j < 8; ++j) {
            const int pos = st * 32 + (l >> 4) * 8 + j, want = pos < 225 ? pos * LD1 + c * 16 + (l & 15) : ZERO;  // dc1^T[co][pos], zeros from 225
            CHECK(frag[l][j] == want, "dW1 B st %d c %d lane %d j %d: %d != %d", st, c, l, j, frag[l][j], want);
          }
      }
    }
  }
  // ---------------------------------------------------------------- dW3
  {
    const std::vector<int> c2 = index_image(C2R, L3, 36), dc3 = index_image(17, L3, 16);
    for (int kt = 0; kt < 36; ++kt) {
      tr_frag(c2, [&](int l, int h) { return dw3_a_lane(l, h) + dw3_a_tile(kt); }, frag, "dW3 A");
      for (int l = 0; l < 64; ++l) {
        const int fr = l & 15, g = l >> 4, tap = kt >> 2, ky = tap / 3, kx = tap - ky * 3;
        for (int j = 0; j < 8; ++j) {
          const int pos = (g & 1) * 8 + j;
          const int want = g < 2 ? (ky * 6 + kx) * L3 + (kt & 3) * 16 + fr + ((pos >> 2) * 6 + (pos & 3)) * L3 : ZERO;
          CHECK(frag[l][j] == want, "dW3 A kt %d lane %d j %d: %d != %d", kt, l, j, frag[l][j], want);
        }
      }
    }
    for (int c = 0; c < 4; ++c) {
      tr_frag(dc3, [&](int l, int h) { return dw3_b_lane(l, h) + 16 * c; }, frag, "dW3 B");
      for (int l = 0; l < 64; ++l)
        for (int j = 0; j < 8; ++j) {
          const int g = l >> 4, want = g < 2 ? ((g & 1) * 8 + j) * L3 + c * 16 + (l & 15) : ZERO;
          CHECK(frag[l][j] == want, "dW3 B c %d lane %d j %d: %d != %d", c, l, j, frag[l][j], want);
        }
    }
  }
  if (g_fail) { printf("%d mismatches\n", g_fail); return 1; }
  printf("OK\n");
  return 0;
}

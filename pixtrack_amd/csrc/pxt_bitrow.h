// A row of a binary image tile as one 128-bit word, for the box morphology of occlusion_mask_kernel
// (pxt_occlusion.hip) and rb_scene_kernel (pxt_raster.hip): a 64-column tile sits in bits 32..95, up to 32 columns of
// its neighbours on either side.  Erosion and dilation along x are shift-AND / shift-OR steps on the word, along y AND /
// OR over the neighbouring rows' words.
#pragma once
#include "pxt_common.h"

namespace pxt {

struct OcRow {
  unsigned long long lo, hi;
};
__device__ inline OcRow oc_and(OcRow a, OcRow b) { return {a.lo & b.lo, a.hi & b.hi}; }
__device__ inline OcRow oc_or(OcRow a, OcRow b) { return {a.lo | b.lo, a.hi | b.hi}; }
__device__ inline OcRow oc_shl(OcRow a, int s) {  // towards higher columns; 0 < s < 64
  return {a.lo << s, (a.hi << s) | (a.lo >> (64 - s))};
}
__device__ inline OcRow oc_shr(OcRow a, int s) {
  return {(a.lo >> s) | (a.hi << (64 - s)), a.hi >> s};
}
// the tile's own 64 columns: bits 32..95
__device__ inline unsigned long long oc_core(OcRow a) { return (a.lo >> 32) | (a.hi << 32); }

// The image's columns 0 .. W - 1 as bits of the row word of the tile whose first column is x0: bits 32 - x0 ..
// 32 - x0 + W - 1, clipped to [0, 128).
__device__ inline OcRow oc_image_columns(int x0, int W) {
  OcRow in_cols = {0ull, 0ull};
  const int b_lo = max(32 - x0, 0), b_hi = (int)min((long long)32 - x0 + W, (long long)128);
  for (int b = 0; b < 2; ++b) {
    const int lo = max(b_lo - 64 * b, 0), hi = min(b_hi - 64 * b, 64);
    unsigned long long mbits = 0ull;
    if (hi > lo) mbits = ((hi - lo) == 64 ? ~0ull : ((1ull << (hi - lo)) - 1ull)) << lo;
    (b == 0 ? in_cols.lo : in_cols.hi) = mbits;
  }
  return in_cols;
}

// Dilation of a row along x by radius rd, in doubling shifts.
__device__ inline OcRow oc_dilate_x(OcRow d, int rd) {
  for (int covered = 0, step = 1; covered < rd; step *= 2) {
    const int sft = min(step, rd - covered);
    d = oc_or(d, oc_or(oc_shl(d, sft), oc_shr(d, sft)));
    covered += sft;
  }
  return d;
}

// Four bits -> four 0 / 1 bytes of a dword.
__device__ inline unsigned oc_bytes(unsigned b4) {
  return (b4 & 1u) | ((b4 & 2u) << 7) | ((b4 & 4u) << 14) | ((b4 & 8u) << 21);
}

}  // namespace pxt

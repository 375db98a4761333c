// One point's feature-metric terms: THE statement of the LM's per-point arithmetic (pxt_lm.hip), shared with the
// kernels that must reproduce it - pxt_lm_information (pxt_lm_info.hip: g and H in the LM's order of operations) and
// pxt_score_pose_hypotheses (pxt_reloc.hip: the LM's first logged cost).  A point is served by a lane group, four
// consecutive channels per lane; what follows is the order in which one lane, then the group, forms the point's terms:
//   transform_point -> point_in_window (projection, validity) -> bilinear_weights -> PXT_LM_POINT_CH per channel
//   (residual and central-difference map gradients over the 12-texel cross footprint) or PXT_LM_POINT_CH_COST (2 x 2
//   taps, cost only) -> lm_group_sum over the group -> robust_loss -> point_jacobian -> point_normal_terms.
// How a kernel ADDRESSES the footprint (row pointers and float masks in the LM, 32-bit byte offsets and bit masks in the
// information kernel) is its own business; operation order and parenthesisation in here decide the bits of all three.
#pragma once

#include "pxt_common.h"

namespace pxt {

__device__ inline void robust_loss(int kind, float alpha, float scale, float x, float& loss,
                                   float& w) {
  // pixloc losses.py: scaled_loss(x, fn, a) = (a^2 fn(x/a^2), fn'(x/a^2)).
  if (kind == 0) {
    loss = x;
    w = 1.f;
    return;
  }
  float a2 = scale * scale;
  float y = x / a2;
  float l, d;
  if (kind == 1) {  // huber
    if (y <= 1.f) {
      l = y;
      d = 1.f;
    } else {
      float sy = sqrtf(y);
      l = 2.f * sy - 1.f;
      d = fmaxf(1.1920929e-07f, 1.f / sy);
    }
  } else {  // barron(alpha)
    if (alpha == 0.f) {
      l = 2.f * log1pf(fminf(0.5f * y, 33e37f));
      d = 2.f / (y + 2.f);
    } else if (alpha == 2.f) {
      l = y;
      d = 1.f;
    } else {
      float beta = fmaxf(fabsf(alpha - 2.f), 1e-7f);
      float as = (alpha >= 0.f ? 1.f : -1.f) * fmaxf(fabsf(alpha), 1e-7f);
      l = 2.f * (beta / as) * (powf(y / beta + 1.f, 0.5f * alpha) - 1.f);
      d = powf(y / beta + 1.f, 0.5f * alpha - 1.f);
    }
  }
  loss = l * a2;
  w = d;
}

// Sum over the LG lanes of a point's group, every lane receiving the total.  The first four butterfly
// steps are DPP moves inside a 16-lane row (quad_perm xor 1 / xor 2, row_half_mirror, row_mirror: for values
// that are already uniform over the smaller group a mirror is as good as an xor); only the 32-lane step
// crosses rows (one ds_bpermute).  (Six sums x five dependent __shfl_xor = 3.2k cycles per point round with
// hipcc's ds_bpermute lowering; stamps.)
__device__ inline float lm_dpp_add(float v, int ctrl_tag) {
  const int iv = __builtin_bit_cast(int, v);
  int o;
  if (ctrl_tag == 0) o = __builtin_amdgcn_update_dpp(iv, iv, 0xB1, 0xF, 0xF, false);        // quad_perm [1,0,3,2]
  else if (ctrl_tag == 1) o = __builtin_amdgcn_update_dpp(iv, iv, 0x4E, 0xF, 0xF, false);   // quad_perm [2,3,0,1]
  else if (ctrl_tag == 2) o = __builtin_amdgcn_update_dpp(iv, iv, 0x141, 0xF, 0xF, false);  // row_half_mirror
  else o = __builtin_amdgcn_update_dpp(iv, iv, 0x140, 0xF, 0xF, false);                     // row_mirror
  return v + __builtin_bit_cast(float, o);
}

// LG (lanes per point) is 8 or 32 (`wide`), wave-uniform at run time.
__device__ inline float lm_group_sum(float v, bool wide) {
  v = lm_dpp_add(v, 0);
  v = lm_dpp_add(v, 1);
  v = lm_dpp_add(v, 2);
  if (wide) {
    v = lm_dpp_add(v, 3);
    v += __shfl_xor(v, 16, PXT_WAVE);
  }
  return v;
}

// The same for a compile-time group width of 8, 16 or 32 lanes.
template <int LG>
__device__ inline float lm_group_sum_t(float v) {
  v = lm_dpp_add(v, 0);
  v = lm_dpp_add(v, 1);
  v = lm_dpp_add(v, 2);
  if (LG >= 16) v = lm_dpp_add(v, 3);
  if (LG >= 32) v += __shfl_xor(v, 16, PXT_WAVE);
  return v;
}

// Sum over the 16 lanes of a DPP row, every lane receiving the total (a fixed tree: the same bits in every workgroup).
__device__ inline float lm_row16_sum(float v) {
  v = lm_dpp_add(v, 0);
  v = lm_dpp_add(v, 1);
  v = lm_dpp_add(v, 2);
  return lm_dpp_add(v, 3);
}

// p = R X + t, the pose as 12 floats (row-major R, then t).
__host__ __device__ inline void transform_point(const float* T, float X, float Y, float Z, float& px, float& py, float& pz) {
  px = T[0] * X + T[1] * Y + T[2] * Z + T[9];
  py = T[3] * X + T[4] * Y + T[5] * Z + T[10];
  pz = T[6] * X + T[7] * Y + T[8] * Z + T[11];
}

// The validity rule: `valid` so far (in range, mask bit) is narrowed by the projection's own test (project_point: in
// front of the camera, inside the distortion model's range, inside the image) and by (u, v) lying at least `pad`
// texels inside the W x H map.  (In/out, not returned: with a returned value lm_refine_kernel's code moves.)
__host__ __device__ inline void point_in_window(const Cam& cam, float px, float py, float pz, bool& valid, int W, int H, float pad,
                                       float& u, float& v, float* Jw /* 6 or nullptr */) {
  valid = project_point(cam, px, py, pz, u, v, Jw) && valid;
  valid = valid && (u >= pad) && (v >= pad) && (u <= (float)(W - 1) - pad) && (v <= (float)(H - 1) - pad);
}

// Texel (ix0, iy0) and the weights of the 2 x 2 bilinear taps at (u, v): w00 at (ix0, iy0), w10 at (ix0 + 1, iy0), ...
__device__ inline void bilinear_weights(float u, float v, int& ix0, int& iy0, float& w00, float& w10, float& w01,
                                        float& w11) {
  const float fu = floorf(u), fv = floorf(v);
  ix0 = (int)fu;
  iy0 = (int)fv;
  const float ax = u - fu, ay = v - fv;
  w00 = (1.f - ax) * (1.f - ay);
  w10 = ax * (1.f - ay);
  w01 = (1.f - ax) * ay;
  w11 = ax * ay;
}

// The 2 x 2 texels the sparse sampler (pxt_lm.hip sample_level) reads for a valid point at (u, v) of an FW x FH level
// whose map holds the window [x0, x0 + W) x [y0, y0 + H): columns ix0 / x1 and rows iy0 / y1 in WINDOW coordinates, the
// fractions and the masks of the second column / row (0.f where it would leave the full level; the texel is still read,
// clamped onto the first).  All four texels are read whatever their weights.  Shared with the reference pass's tile
// marking (pxt_unet.hip reference_tiles_mark), which must name exactly the texels the sampler will read.
struct SampleTexels {
  int ix0, iy0, x1, y1;
  float ax, ay, mx, my;
};
__host__ __device__ inline int clamp_int(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__host__ __device__ inline SampleTexels sample_texels(float u, float v, int FW, int FH, int x0, int y0, int W, int H) {
  SampleTexels t;
  const float fu = floorf(u), fv = floorf(v);
  const int ix0f = (int)fu, iy0f = (int)fv;
  t.ax = u - fu;
  t.ay = v - fv;
  const int x1f = ix0f + 1 < FW ? ix0f + 1 : FW - 1, y1f = iy0f + 1 < FH ? iy0f + 1 : FH - 1;
  t.mx = (ix0f + 1 < FW) ? 1.f : 0.f;
  t.my = (iy0f + 1 < FH) ? 1.f : 0.f;
  // window coordinates (the caller's window holds every texel a valid point reads; the clamps only keep a caller's
  // mistake from reading outside the buffer)
  t.ix0 = clamp_int(ix0f - x0, 0, W - 1);
  t.iy0 = clamp_int(iy0f - y0, 0, H - 1);
  t.x1 = clamp_int(x1f - x0, 0, W - 1);
  t.y1 = clamp_int(y1f - y0, 0, H - 1);
  return t;
}

// One channel of a point: residual and central-difference map gradients from the 12-texel cross footprint of the five
// bilinear taps (centre, x +- 1, y +- 1) around texel (ix0, iy0) = row 1, column 1 of the 4 x 4 neighbourhood - rows 0,3
// use columns 1,2; rows 1,2 use columns 0..3 - added to the six sums that cross the lane group: s_cost = sum r^2,
// A = gradF^T r (2), B = gradF^T gradF (3).  aRC is texel (row R, column C) times its mask (1.f inside the map, 0.f
// outside: grid_sample padding_mode='zeros'), f the reference value.  A macro, not a function: lm_refine_kernel's code
// must not move (256 VGPRs, spilling), and only the same tokens at the call site guarantee that.
#define PXT_LM_POINT_CH(w00_, w10_, w01_, w11_, a01_, a02_, a10_, a11_, a12_, a13_, a20_, a21_, a22_, a23_, a31_, a32_, \
                        f_, s_cost_, A0_, A1_, B00_, B01_, B11_)                                                        \
  {                                                                                                                     \
    const float a01 = (a01_), a02 = (a02_), a10 = (a10_), a11 = (a11_), a12 = (a12_), a13 = (a13_), a20 = (a20_),       \
                a21 = (a21_), a22 = (a22_), a23 = (a23_), a31 = (a31_), a32 = (a32_);                                   \
    const float F = (w00_) * a11 + (w10_) * a12 + (w01_) * a21 + (w11_) * a22;                                          \
    const float Fxp = (w00_) * a12 + (w10_) * a13 + (w01_) * a22 + (w11_) * a23;                                        \
    const float Fxm = (w00_) * a10 + (w10_) * a11 + (w01_) * a20 + (w11_) * a21;                                        \
    const float Fyp = (w00_) * a21 + (w10_) * a22 + (w01_) * a31 + (w11_) * a32;                                        \
    const float Fym = (w00_) * a01 + (w10_) * a02 + (w01_) * a11 + (w11_) * a12;                                        \
    const float gx = 0.5f * (Fxp - Fxm), gy = 0.5f * (Fyp - Fym);                                                       \
    const float r = F - (f_);                                                                                           \
    (s_cost_) += r * r;                                                                                                 \
    (A0_) += r * gx;                                                                                                    \
    (A1_) += r * gy;                                                                                                    \
    (B00_) += gx * gx;                                                                                                  \
    (B01_) += gx * gy;                                                                                                  \
    (B11_) += gy * gy;                                                                                                  \
  }

// The cost alone, from the centre tap's 2 x 2 texels: the first lines of the body above.
#define PXT_LM_POINT_CH_COST(w00_, w10_, w01_, w11_, a11_, a12_, a21_, a22_, f_, s_cost_)    \
  {                                                                                          \
    const float a11 = (a11_), a12 = (a12_), a21 = (a21_), a22 = (a22_);                      \
    const float F = (w00_) * a11 + (w10_) * a12 + (w01_) * a21 + (w11_) * a22;               \
    const float r = F - (f_);                                                                \
    (s_cost_) += r * r;                                                                      \
  }

// Jp = d(u,v)/d(delta) = Jw (2x3) * [I | -[p]x] (3x6), translation columns first (J0, J1: its two rows).
__device__ inline void point_jacobian(const float* Jw, float px, float py, float pz, float* J0, float* J1) {
  J0[0] = Jw[0]; J0[1] = Jw[1]; J0[2] = Jw[2];
  J1[0] = Jw[3]; J1[1] = Jw[4]; J1[2] = Jw[5];
  // -[p]x = [[0, pz, -py], [-pz, 0, px], [py, -px, 0]]
  J0[3] = -Jw[1] * pz + Jw[2] * py;
  J0[4] = Jw[0] * pz - Jw[2] * px;
  J0[5] = -Jw[0] * py + Jw[1] * px;
  J1[3] = -Jw[4] * pz + Jw[5] * py;
  J1[4] = Jw[3] * pz - Jw[5] * px;
  J1[5] = -Jw[3] * py + Jw[4] * px;
}

// One point's contribution to g (dst[0..5]) and the upper triangle of H (dst[6..26], row-major) from the six
// group-reduced scalars A, B and the point's weight: J = gradF (C x 2) * Jp (2 x 6)  =>  J^T r = Jp^T A,
// J^T J = Jp^T B Jp.  ADD: added to what dst holds; else stored, as a sum that starts at 0.f.
template <bool ADD>
__device__ __forceinline__ void point_normal_terms(float* dst, float wgt, const float* J0, const float* J1, float A0,
                                                   float A1, float B00, float B01, float B11) {
  float M0[6], M1[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    M0[k] = B00 * J0[k] + B01 * J1[k];
    M1[k] = B01 * J0[k] + B11 * J1[k];
    dst[k] = (ADD ? dst[k] : 0.f) + wgt * (J0[k] * A0 + J1[k] * A1);
  }
  int idx = 6;
#pragma unroll
  for (int k = 0; k < 6; ++k)
#pragma unroll
    for (int l = k; l < 6; ++l, ++idx) dst[idx] = (ADD ? dst[idx] : 0.f) + wgt * (J0[k] * M0[l] + J1[k] * M1[l]);
}

}  // namespace pxt

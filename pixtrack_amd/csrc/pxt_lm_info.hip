// The LM's normal equations at a given pose, evaluated ONCE (pxt_lm_information, include/pixtrack_hip.h).
//
// For each of n_problems independent (points, level, pose) problems one launch forms the sums of one LM iteration at
// the given pose - sum rho, n_valid, sum w |r|^2, sum w, g = sum w J^T r and the upper triangle of the UNDAMPED
// H = sum w J^T J - and a second small launch folds them into a 48-float record.  Validity, projection, the 12-texel
// cross footprint of the five bilinear taps, the central-difference map gradients, w_unc = conf_query * conf_ref and
// rho / rho' are those of lm_accumulate (pxt_lm.hip), restated here (that file holds 256 VGPRs, is pinned by its tests
// and stays untouched); the parameter order is the LM's delta (translation 3, rotation 3, left update).
//
// Mapping
//  * A point is owned by a lane GROUP as in the LM (4 consecutive channels per lane, dwordx4 texel reads: 32 lanes per
//    point for C > 32, 8 otherwise), and J^T J = Jp^T (gradF^T gradF) Jp: six scalars per point cross the group.
//  * TWO points are in flight per group: both points' footprints are requested before either is consumed (the scoring
//    kernel's lesson, DESIGN.md 3.4: one point per group per trip left the memory pipe idle behind every reduction).
//  * The points of ONE problem are dealt round-robin to the groups of n_wgs workgroups (blockIdx.x), the problems are
//    blockIdx.y.  n_wgs depends on the problem's n_points and C only (about four points per group, at most
//    kInfoMaxWgs), so a problem's summation order does not depend on what else is in the launch.
//  * Inside a workgroup the group leaders' 31 sums are folded in a fixed order through LDS; across a problem's
//    workgroups the partials go to the workspace and the fold kernel (one wave per problem) adds them in workgroup
//    order - the kernel boundary orders the partials; no atomics anywhere.
//  * The parameter record of a problem (device workspace, or the kernel-argument segment for up to two problems), the
//    pose and the LM record's status words are read through vector loads (pointers made opaque VGPR values, as
//    pxt_reloc.hip does): the pose may have been written by the kernel just ahead in the stream.
#include "pxt_common.h"

#include <algorithm>

namespace pxt {
namespace {

constexpr int kInfoBlock = 256;
constexpr int kInfoWaves = kInfoBlock / PXT_WAVE;
constexpr int kInfoMaxGroups = kInfoBlock / 8;  // groups per workgroup at 8 lanes per point
constexpr int kInfoMaxWgs = 128;                // workgroups per problem, at most
constexpr int kInfoPointsPerGroup = 4;          // target; more when n_wgs is capped
constexpr int kInfoAcc = 32;                    // floats per partial: words 0..30 of the record, one pad
constexpr int kInfoGrpStride = 33;              // padded: leaders of one wave hit distinct LDS banks
constexpr int kInfoArgProblems = 2;             // parameter records that travel as kernel arguments

struct InfoParams {  // 128 bytes
  const float* p3d;
  const uint8_t* mask;
  const float* fmap;
  const float* fref;
  const float* pose;
  float* out;
  int n, h, w, C, cs, ndist, pose_is_record, n_wgs;
  float cam[10];
  int pad_[2];
};
static_assert(sizeof(InfoParams) == 128, "parameter records are read as aligned vectors");

struct InfoArgs {
  InfoParams p[kInfoArgProblems];
};

struct InfoConf {
  int pad, loss, min_valid;
  float loss_alpha, loss_scale;
};

template <typename T>
__device__ __forceinline__ const T* vector_pointer(const T* p) {
  asm volatile("" : "+v"(p));  // an opaque VGPR value: the loads through it are vector loads
  return p;
}

// A value every lane loaded alike (parameter record, pose), moved to a scalar register: what was read through a vector
// load stays uniform for the compiler from here on (addresses, loop bounds and the camera cost no VGPRs).
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float uniform(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
template <typename T>
__device__ __forceinline__ T* uniform(T* p) {
  const unsigned long long v = (unsigned long long)p;
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
  return (T*)(((unsigned long long)hi << 32) | lo);
}

// pixloc scaled_loss(x, fn, a) = (a^2 fn(x / a^2), fn'(x / a^2)): the LM's robust_loss (pxt_lm.hip).
__device__ inline void info_robust_loss(int kind, float alpha, float scale, float x, float& loss, float& w) {
  if (kind == 0) {
    loss = x;
    w = 1.f;
    return;
  }
  const float a2 = scale * scale;
  const float y = x / a2;
  float l, d;
  if (kind == 1) {  // huber
    if (y <= 1.f) {
      l = y;
      d = 1.f;
    } else {
      const float sy = sqrtf(y);
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
      const float beta = fmaxf(fabsf(alpha - 2.f), 1e-7f);
      const float as = (alpha >= 0.f ? 1.f : -1.f) * fmaxf(fabsf(alpha), 1e-7f);
      l = 2.f * (beta / as) * (powf(y / beta + 1.f, 0.5f * alpha) - 1.f);
      d = powf(y / beta + 1.f, 0.5f * alpha - 1.f);
    }
  }
  loss = l * a2;
  w = d;
}

// Sum over a point's lane group, every lane receiving the total: the LM's fixed butterfly (DPP inside a 16-lane row,
// one cross-row step for 32 lanes), so a point's six scalars are formed in the LM's order.
__device__ inline float info_dpp_add(float v, int ctrl_tag) {
  const int iv = __builtin_bit_cast(int, v);
  int o;
  if (ctrl_tag == 0) o = __builtin_amdgcn_update_dpp(iv, iv, 0xB1, 0xF, 0xF, false);        // quad_perm [1,0,3,2]
  else if (ctrl_tag == 1) o = __builtin_amdgcn_update_dpp(iv, iv, 0x4E, 0xF, 0xF, false);   // quad_perm [2,3,0,1]
  else if (ctrl_tag == 2) o = __builtin_amdgcn_update_dpp(iv, iv, 0x141, 0xF, 0xF, false);  // row_half_mirror
  else o = __builtin_amdgcn_update_dpp(iv, iv, 0x140, 0xF, 0xF, false);                     // row_mirror
  return v + __builtin_bit_cast(float, o);
}

__device__ inline float info_group_sum(float v, bool wide) {
  v = info_dpp_add(v, 0);
  v = info_dpp_add(v, 1);
  v = info_dpp_add(v, 2);
  if (wide) {
    v = info_dpp_add(v, 3);
    v += __shfl_xor(v, 16, PXT_WAVE);
  }
  return v;
}

// One point's terms added to the group's sums, in the record's order: acc[0] sum rho, [1] n_valid, [2] sum w |r|^2,
// [3] sum w, [4..9] g, [10..30] upper H.  J = gradF (C x 2) * Jp (2 x 6)  =>  J^T r = Jp^T A,  J^T J = Jp^T B Jp.
__device__ inline void info_add_point(float* acc, float wgt, float rcost, float r2, const float* Jw, float px, float py,
                                      float pz, float A0, float A1, float B00, float B01, float B11) {
  // Jp = d(u,v)/d(delta) = Jw (2x3) * [I | -[p]x] (3x6), translation columns first.
  float J0[6], J1[6];
  J0[0] = Jw[0]; J0[1] = Jw[1]; J0[2] = Jw[2];
  J1[0] = Jw[3]; J1[1] = Jw[4]; J1[2] = Jw[5];
  J0[3] = -Jw[1] * pz + Jw[2] * py;
  J0[4] = Jw[0] * pz - Jw[2] * px;
  J0[5] = -Jw[0] * py + Jw[1] * px;
  J1[3] = -Jw[4] * pz + Jw[5] * py;
  J1[4] = Jw[3] * pz - Jw[5] * px;
  J1[5] = -Jw[3] * py + Jw[4] * px;
  acc[0] += rcost;
  acc[1] += 1.f;
  acc[2] += wgt * r2;
  acc[3] += wgt;
  float M0[6], M1[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    M0[k] = B00 * J0[k] + B01 * J1[k];
    M1[k] = B01 * J0[k] + B11 * J1[k];
    acc[4 + k] += wgt * (J0[k] * A0 + J1[k] * A1);
  }
  int idx = 10;
#pragma unroll
  for (int k = 0; k < 6; ++k)
#pragma unroll
    for (int l = k; l < 6; ++l) acc[idx++] += wgt * (J0[k] * M0[l] + J1[k] * M1[l]);
}

// What a point needs between its projection and its arithmetic.
struct InfoPoint {
  bool valid;
  int n;  // clamped into the bank: an invalid point's loads stay in bounds and are discarded
  float px, py, pz, Jw[6];
  float w00, w10, w01, w11;
  unsigned xo[4], yo[4];  // BYTE offsets of the 4 columns / 4 rows of the neighbourhood, clamped into the map (32-bit:
                          // one VGPR per address beside the map's scalar base; the entry point bounds the map's size)
  int xin, yin;           // bit k: column / row k lies inside the map (outside counts as zero: grid_sample 'zeros')
  // 1.f where texel (row r, column c) lies inside the map, else 0.f
  __device__ __forceinline__ float in(int r, int c) const { return ((yin >> r) & (xin >> c) & 1) ? 1.f : 0.f; }
};

// Reads at a scalar base (named as global memory: the pointer was rebuilt from two scalar halves) + 32-bit byte offset.
typedef const __attribute__((address_space(1))) char* InfoGlobal;
typedef float InfoVec4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 info_texel(const float* base, unsigned byte_offset) {
  const InfoVec4 v = *(const __attribute__((address_space(1))) InfoVec4*)((InfoGlobal)base + byte_offset);
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ float info_word(const float* base, unsigned byte_offset) {
  return *(const __attribute__((address_space(1))) float*)((InfoGlobal)base + byte_offset);
}

__device__ inline const InfoParams* info_params(const InfoParams* ws_params, int from_args, int prob) {
  const InfoParams* base = from_args ? (const InfoParams*)__builtin_amdgcn_kernarg_segment_ptr() : ws_params;
  return vector_pointer(base + prob);
}

// -> false when the problem is skipped (its LM record reports failed / a status).
__device__ inline bool info_load_pose(const InfoParams* q, float* T) {
  const float4* tp = (const float4*)vector_pointer(q->pose);
  const float4 a = tp[0], b = tp[1], d = tp[2];
  T[0] = a.x; T[1] = a.y; T[2] = a.z; T[3] = a.w;
  T[4] = b.x; T[5] = b.y; T[6] = b.z; T[7] = b.w;
  T[8] = d.x; T[9] = d.y; T[10] = d.z; T[11] = d.w;
#pragma unroll
  for (int i = 0; i < 12; ++i) T[i] = uniform(T[i]);
  if (uniform(q->pose_is_record)) {
    const float4 st = tp[3];  // failed, status, total iterations, completion word
    if (uniform(st.x) != 0.f || uniform(st.y) != 0.f) return false;
  }
  return true;
}

__global__ __launch_bounds__(kInfoBlock) void lm_info_accumulate_kernel(const InfoArgs args, const InfoParams* ws_params,
                                                                        float* partials, const InfoConf cf,
                                                                        const int from_args) {
  __shared__ float part[kInfoMaxGroups * kInfoGrpStride];
  const int prob = blockIdx.y, b = blockIdx.x;
  const InfoParams* q = info_params(ws_params, from_args, prob);
  const int n_wgs = uniform(q->n_wgs);
  if (b >= n_wgs) return;  // (workgroup-uniform)
  float T[12];
  if (!info_load_pose(q, T)) return;  // skipped: the fold kernel marks the record

  const int N = uniform(q->n), W = uniform(q->w), H = uniform(q->h), C = uniform(q->C), cs = uniform(q->cs);
  const bool wide = C > 32;
  const int LG = wide ? 32 : 8;
  const int GPW = PXT_WAVE / LG, G = kInfoWaves * GPW;  // groups per wave / per workgroup
  const int lane = threadIdx.x & (PXT_WAVE - 1);
  const int sub = lane & (LG - 1);
  const int grp = (threadIdx.x / PXT_WAVE) * GPW + lane / LG;
  float c10[10];
  {
    const float* c = q->cam;
#pragma unroll
    for (int i = 0; i < 10; ++i) c10[i] = uniform(c[i]);
  }
  const Cam cam = make_cam(c10, uniform(q->ndist));
  const float* p3d = uniform(q->p3d);
  const uint8_t* mask = uniform(q->mask);
  const float* fmap = uniform(q->fmap);
  const float* fref = uniform(q->fref);
  const float pad = (float)cf.pad;

  float acc[kInfoAcc];
#pragma unroll
  for (int k = 0; k < kInfoAcc; ++k) acc[k] = 0.f;

  // point i of the problem -> group (i mod TG) of the problem's TG groups; a group takes its points two at a time
  const int TG = n_wgs * G;
  const int first = b * G + grp;
#pragma unroll 1
  for (int i0 = first; i0 < N; i0 += 2 * TG) {
    InfoPoint pt[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      InfoPoint& p = pt[j];
      const int i = i0 + j * TG;
      bool valid = i < N;
      p.n = min(i, N - 1);
      const float X = info_word(p3d, 12u * (unsigned)p.n), Y = info_word(p3d, 12u * (unsigned)p.n + 4u),
                  Z = info_word(p3d, 12u * (unsigned)p.n + 8u);
      if (mask) valid = valid && *((const __attribute__((address_space(1))) uint8_t*)mask + (unsigned)p.n) != 0;
      p.px = T[0] * X + T[1] * Y + T[2] * Z + T[9];
      p.py = T[3] * X + T[4] * Y + T[5] * Z + T[10];
      p.pz = T[6] * X + T[7] * Y + T[8] * Z + T[11];
      float u, v;
      valid = project_point(cam, p.px, p.py, p.pz, u, v, p.Jw) && valid;
      valid = valid && (u >= pad) && (v >= pad) && (u <= (float)(W - 1) - pad) && (v <= (float)(H - 1) - pad);
      if (!valid) u = v = 0.f;  // (u, v may be anything, NaN included: keep the address arithmetic defined)
      p.valid = valid;
      const float fu = floorf(u), fv = floorf(v);
      const int ix0 = (int)fu, iy0 = (int)fv;
      const float ax = u - fu, ay = v - fv;
      p.w00 = (1.f - ax) * (1.f - ay); p.w10 = ax * (1.f - ay); p.w01 = (1.f - ax) * ay; p.w11 = ax * ay;
      p.xin = p.yin = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int xx = ix0 - 1 + k, yy = iy0 - 1 + k;
        p.xin |= (xx >= 0 && xx < W) ? 1 << k : 0;
        p.yin |= (yy >= 0 && yy < H) ? 1 << k : 0;
        p.xo[k] = (unsigned)(min(max(xx, 0), W - 1) * cs) * 4u;
        p.yo[k] = (unsigned)(min(max(yy, 0), H - 1) * W * cs) * 4u;
      }
    }

    float s_cost[2] = {0.f, 0.f}, A0[2] = {0.f, 0.f}, A1[2] = {0.f, 0.f}, B00[2] = {0.f, 0.f}, B01[2] = {0.f, 0.f},
          B11[2] = {0.f, 0.f};
#pragma unroll 1
    for (int c0 = 4 * sub; c0 < C; c0 += 4 * LG) {
      // 12-texel cross footprint per point: rows 0,3 use columns 1,2; rows 1,2 use columns 0..3.  Both points' 13 reads
      // are issued before the arithmetic of either.
      float4 t01[2], t02[2], t10[2], t11[2], t12[2], t13[2], t20[2], t21[2], t22[2], t23[2], t31[2], t32[2], fr[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const InfoPoint& p = pt[j];
        const unsigned cb = 4u * (unsigned)c0;
        t01[j] = info_texel(fmap, p.yo[0] + p.xo[1] + cb);
        t02[j] = info_texel(fmap, p.yo[0] + p.xo[2] + cb);
        t10[j] = info_texel(fmap, p.yo[1] + p.xo[0] + cb);
        t11[j] = info_texel(fmap, p.yo[1] + p.xo[1] + cb);
        t12[j] = info_texel(fmap, p.yo[1] + p.xo[2] + cb);
        t13[j] = info_texel(fmap, p.yo[1] + p.xo[3] + cb);
        t20[j] = info_texel(fmap, p.yo[2] + p.xo[0] + cb);
        t21[j] = info_texel(fmap, p.yo[2] + p.xo[1] + cb);
        t22[j] = info_texel(fmap, p.yo[2] + p.xo[2] + cb);
        t23[j] = info_texel(fmap, p.yo[2] + p.xo[3] + cb);
        t31[j] = info_texel(fmap, p.yo[3] + p.xo[1] + cb);
        t32[j] = info_texel(fmap, p.yo[3] + p.xo[2] + cb);
        fr[j] = info_texel(fref, 4u * (unsigned)(p.n * cs) + cb);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const InfoPoint& p = pt[j];
        const float w00 = p.w00, w10 = p.w10, w01 = p.w01, w11 = p.w11;
        const float m01 = p.in(0, 1), m02 = p.in(0, 2);
        const float m10 = p.in(1, 0), m11 = p.in(1, 1), m12 = p.in(1, 2), m13 = p.in(1, 3);
        const float m20 = p.in(2, 0), m21 = p.in(2, 1), m22 = p.in(2, 2), m23 = p.in(2, 3);
        const float m31 = p.in(3, 1), m32 = p.in(3, 2);
#define PXT_INFO_CH(q_)                                                                                       \
  {                                                                                                           \
    const float a01 = t01[j].q_ * m01, a02 = t02[j].q_ * m02, a10 = t10[j].q_ * m10, a11 = t11[j].q_ * m11,   \
                a12 = t12[j].q_ * m12, a13 = t13[j].q_ * m13, a20 = t20[j].q_ * m20, a21 = t21[j].q_ * m21,   \
                a22 = t22[j].q_ * m22, a23 = t23[j].q_ * m23, a31 = t31[j].q_ * m31, a32 = t32[j].q_ * m32;   \
    const float F = w00 * a11 + w10 * a12 + w01 * a21 + w11 * a22;                                            \
    const float Fxp = w00 * a12 + w10 * a13 + w01 * a22 + w11 * a23;                                          \
    const float Fxm = w00 * a10 + w10 * a11 + w01 * a20 + w11 * a21;                                          \
    const float Fyp = w00 * a21 + w10 * a22 + w01 * a31 + w11 * a32;                                          \
    const float Fym = w00 * a01 + w10 * a02 + w01 * a11 + w11 * a12;                                          \
    const float gx = 0.5f * (Fxp - Fxm), gy = 0.5f * (Fyp - Fym);                                             \
    const float r = F - fr[j].q_;                                                                             \
    s_cost[j] += r * r;                                                                                       \
    A0[j] += r * gx;                                                                                          \
    A1[j] += r * gy;                                                                                          \
    B00[j] += gx * gx;                                                                                        \
    B01[j] += gx * gy;                                                                                        \
    B11[j] += gy * gy;                                                                                        \
  }
        PXT_INFO_CH(x) PXT_INFO_CH(y) PXT_INFO_CH(z) PXT_INFO_CH(w)
#undef PXT_INFO_CH
      }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const InfoPoint& p = pt[j];
      // confidence: bilinear sample of channel C (one address for the whole group)
      const unsigned cb = 4u * (unsigned)C;
      const float q11 = info_word(fmap, p.yo[1] + p.xo[1] + cb) * p.in(1, 1);
      const float q12 = info_word(fmap, p.yo[1] + p.xo[2] + cb) * p.in(1, 2);
      const float q21 = info_word(fmap, p.yo[2] + p.xo[1] + cb) * p.in(2, 1);
      const float q22 = info_word(fmap, p.yo[2] + p.xo[2] + cb) * p.in(2, 2);
      const float wq = p.w00 * q11 + p.w10 * q12 + p.w01 * q21 + p.w11 * q22;
      const float wref = info_word(fref, 4u * (unsigned)(p.n * cs) + cb);
      const float sc = info_group_sum(s_cost[j], wide);
      const float a0 = info_group_sum(A0[j], wide), a1 = info_group_sum(A1[j], wide);
      const float b00 = info_group_sum(B00[j], wide), b01 = info_group_sum(B01[j], wide),
                  b11 = info_group_sum(B11[j], wide);
      float rcost, wl;
      info_robust_loss(cf.loss, cf.loss_alpha, cf.loss_scale, sc, rcost, wl);
      const float wgt = wl * (wref * wq);
      if (p.valid)  // group-uniform: an invalid point contributes nothing (weight 0, not counted)
        info_add_point(acc, wgt, rcost, sc, p.Jw, p.px, p.py, p.pz, a0, a1, b00, b01, b11);
    }
  }

  if (sub == 0) {
#pragma unroll
    for (int k = 0; k < kInfoAcc - 1; ++k) part[grp * kInfoGrpStride + k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < kInfoAcc) {  // the groups' sums in a fixed order
    float v = 0.f;
    if (threadIdx.x < kInfoAcc - 1)
      for (int g = 0; g < G; ++g) v += part[g * kInfoGrpStride + threadIdx.x];
    partials[((size_t)prob * kInfoMaxWgs + b) * kInfoAcc + threadIdx.x] = v;
  }
}

// One wave per problem: the workgroups' partials in workgroup order, then the record; word 47 last.
__global__ __launch_bounds__(PXT_WAVE) void lm_info_fold_kernel(const InfoArgs args, const InfoParams* ws_params,
                                                                const float* partials, const InfoConf cf,
                                                                const int from_args) {
  __shared__ float rec[kInfoAcc];
  const int prob = blockIdx.x;
  const InfoParams* q = info_params(ws_params, from_args, prob);
  float* out = uniform(q->out);
  float T[12];
  const bool run = info_load_pose(q, T);
  if (!run) {
    if (threadIdx.x == 0) __hip_atomic_store(&out[47], -1.f, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    return;
  }
  const int n_wgs = uniform(q->n_wgs);
  if (threadIdx.x < kInfoAcc) {
    const float* p = partials + (size_t)prob * kInfoMaxWgs * kInfoAcc + threadIdx.x;
    float v = 0.f;
    for (int b = 0; b < n_wgs; ++b) v += p[(size_t)b * kInfoAcc];
    rec[threadIdx.x] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {  // one thread writes the record, so that its release covers every word
    for (int k = 0; k < kInfoAcc - 1; ++k) out[k] = rec[k];
    out[31] = 0.f;
    for (int k = 0; k < 12; ++k) out[32 + k] = T[k];
    out[44] = out[45] = out[46] = 0.f;
    const float ok = rec[1] >= (float)cf.min_valid ? 1.f : -2.f;  // -2: evaluated, but the LM would call it failed
    __hip_atomic_store(&out[47], ok, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

int info_workgroups(int n_points, int C) {
  const int groups = kInfoBlock / (C > 32 ? 32 : 8);
  const int per_wg = groups * kInfoPointsPerGroup;
  return std::max(1, std::min(kInfoMaxWgs, (n_points + per_wg - 1) / per_wg));
}

size_t info_params_bytes(int n_problems) { return ((size_t)n_problems * sizeof(InfoParams) + 255) / 256 * 256; }

// Pinned staging records, a ring of four per thread and device (as the LM batch keeps them): a slot is reused only
// after the copy that read it has completed.
struct InfoStageSlot {
  InfoParams* host = nullptr;
  hipEvent_t copied = nullptr;
};
constexpr int kInfoStageSlots = 4;

}  // namespace
}  // namespace pxt

using namespace pxt;

extern "C" int64_t pxt_lm_information_workspace_bytes(int32_t n_problems) {
  if (n_problems < 1 || n_problems > PXT_LM_INFO_MAX_PROBLEMS) return PXT_E_ARG;
  return (int64_t)(info_params_bytes(n_problems) + (size_t)n_problems * kInfoMaxWgs * kInfoAcc * sizeof(float));
}

extern "C" int pxt_lm_information(const pxt_lm_info_problem* problems, int32_t n_problems, const pxt_lm_conf* conf,
                                  void* workspace, void* stream) {
  if (!problems || !conf || !workspace) return PXT_E_ARG;
  if (n_problems < 1 || n_problems > PXT_LM_INFO_MAX_PROBLEMS) return PXT_E_ARG;
  if (((uintptr_t)workspace % 16) != 0) return PXT_E_ARG;
  if (conf->pad < 0 || conf->loss < 0 || conf->loss > 2 || conf->min_valid < 0) return PXT_E_ARG;
  const int K = n_problems;
  const bool from_args = K <= kInfoArgProblems;
  InfoArgs args = {};
  InfoParams* rec = args.p;
  InfoStageSlot* slot = nullptr;
  if (!from_args) {
    static thread_local InfoStageSlot stage[16][kInfoStageSlots];
    static thread_local int stage_next[16] = {0};
    int dev_id = 0;
    PXT_HIP_CHECK(hipGetDevice(&dev_id));
    if (dev_id < 0 || dev_id >= 16) return PXT_E_ARG;
    slot = &stage[dev_id][stage_next[dev_id]];
    stage_next[dev_id] = (stage_next[dev_id] + 1) % kInfoStageSlots;
    if (!slot->host) {
      PXT_HIP_CHECK(hipHostMalloc((void**)&slot->host, PXT_LM_INFO_MAX_PROBLEMS * sizeof(InfoParams), hipHostMallocDefault));
      PXT_HIP_CHECK(hipEventCreateWithFlags(&slot->copied, hipEventDisableTiming));
    } else {
      PXT_HIP_CHECK(hipEventSynchronize(slot->copied));
    }
    rec = slot->host;
  }
  int max_wgs = 1;
  for (int k = 0; k < K; ++k) {
    const pxt_lm_info_problem& q = problems[k];
    const pxt_lm_level& l = q.level;
    if (!q.p3d || !q.pose || !q.out || q.n_points < 1) return PXT_E_ARG;
    if (!l.fmap || !l.fref || l.C < 4 || (l.C % 4) != 0 || (l.cstride % 4) != 0 || l.cstride < l.C + 1 || l.h < 2 ||
        l.w < 2)
      return PXT_E_ARG;
    if (l.ndist != 0 && l.ndist != 2 && l.ndist != 4) return PXT_E_ARG;
    if (((uintptr_t)l.fmap % 16) != 0 || ((uintptr_t)l.fref % 16) != 0 || ((uintptr_t)q.pose % 16) != 0 ||
        ((uintptr_t)q.out % 4) != 0)
      return PXT_E_ARG;
    // (byte offsets inside the map and the reference records are 32-bit in the kernel)
    if ((long long)l.h * l.w * l.cstride >= (1ll << 30) || (long long)q.n_points * l.cstride >= (1ll << 30)) return PXT_E_ARG;
    for (int j = 0; j < k; ++j)
      if (problems[j].out == q.out) return PXT_E_ARG;
    InfoParams& P = rec[k];
    P.p3d = q.p3d;
    P.mask = q.point_mask;
    P.fmap = l.fmap;
    P.fref = l.fref;
    P.pose = q.pose;
    P.out = q.out;
    P.n = q.n_points;
    P.h = l.h; P.w = l.w; P.C = l.C; P.cs = l.cstride; P.ndist = l.ndist;
    P.pose_is_record = q.pose_is_lm_record != 0;
    P.n_wgs = info_workgroups(q.n_points, l.C);
    for (int i = 0; i < 10; ++i) P.cam[i] = l.cam[i];
    P.pad_[0] = P.pad_[1] = 0;
    max_wgs = std::max(max_wgs, P.n_wgs);
  }
  InfoConf cf;
  cf.pad = conf->pad;
  cf.loss = conf->loss;
  cf.min_valid = conf->min_valid;
  cf.loss_alpha = conf->loss_alpha;
  cf.loss_scale = conf->loss_scale;
  hipStream_t s = (hipStream_t)stream;
  const InfoParams* ws_params = (const InfoParams*)workspace;
  float* partials = (float*)((char*)workspace + info_params_bytes(K));
  if (!from_args) {
    PXT_HIP_CHECK(hipMemcpyAsync(workspace, slot->host, (size_t)K * sizeof(InfoParams), hipMemcpyHostToDevice, s));
    PXT_HIP_CHECK(hipEventRecord(slot->copied, s));
  }
  hipLaunchKernelGGL(lm_info_accumulate_kernel, dim3(max_wgs, K), dim3(kInfoBlock), 0, s, args, ws_params, partials, cf,
                     (int)from_args);
  PXT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(lm_info_fold_kernel, dim3(K), dim3(PXT_WAVE), 0, s, args, ws_params, (const float*)partials, cf,
                     (int)from_args);
  PXT_HIP_CHECK(hipGetLastError());
  return PXT_OK;
}

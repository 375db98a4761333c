// The LM's normal equations at a given pose, evaluated ONCE (pxt_lm_information, include/pixtrack_hip.h).
//
// For each of n_problems independent (points, level, pose) problems one launch forms the sums of one LM iteration at
// the given pose - sum rho, n_valid, sum w |r|^2, sum w, g = sum w J^T r and the upper triangle of the UNDAMPED
// H = sum w J^T J - and a second small launch folds them into a 48-float record.  Validity, projection, the 12-texel
// cross footprint of the five bilinear taps, the central-difference map gradients, w_unc = conf_query * conf_ref and
// rho / rho' are the LM's own (pxt_lm_point.h, which lm_accumulate is written in as well); the parameter order is the
// LM's delta (translation 3, rotation 3, left update).
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
#include "pxt_lm_point.h"

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

// One point's terms added to the group's sums, in the record's order: acc[0] sum rho, [1] n_valid, [2] sum w |r|^2,
// [3] sum w, [4..9] g, [10..30] upper H.
__device__ inline void info_add_point(float* acc, float wgt, float rcost, float r2, const float* Jw, float px, float py,
                                      float pz, float A0, float A1, float B00, float B01, float B11) {
  float J0[6], J1[6];
  point_jacobian(Jw, px, py, pz, J0, J1);
  acc[0] += rcost;
  acc[1] += 1.f;
  acc[2] += wgt * r2;
  acc[3] += wgt;
  point_normal_terms<true>(acc + 4, wgt, J0, J1, A0, A1, B00, B01, B11);
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
  const float* pose = vector_pointer(q->pose);
  load_pose12(pose, T);
#pragma unroll
  for (int i = 0; i < 12; ++i) T[i] = uniform(T[i]);
  if (uniform(q->pose_is_record)) {
    const float4 st = ((const float4*)pose)[3];  // failed, status, total iterations, completion word
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
      transform_point(T, X, Y, Z, p.px, p.py, p.pz);
      float u, v;
      point_in_window(cam, p.px, p.py, p.pz, valid, W, H, pad, u, v, p.Jw);
      if (!valid) u = v = 0.f;  // (u, v may be anything, NaN included: keep the address arithmetic defined)
      p.valid = valid;
      int ix0, iy0;
      bilinear_weights(u, v, ix0, iy0, p.w00, p.w10, p.w01, p.w11);
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
#define PXT_INFO_CH(q_)                                                                                          \
  PXT_LM_POINT_CH(w00, w10, w01, w11, t01[j].q_ * m01, t02[j].q_ * m02, t10[j].q_ * m10, t11[j].q_ * m11,          \
                  t12[j].q_ * m12, t13[j].q_ * m13, t20[j].q_ * m20, t21[j].q_ * m21, t22[j].q_ * m22,             \
                  t23[j].q_ * m23, t31[j].q_ * m31, t32[j].q_ * m32, fr[j].q_, s_cost[j], A0[j], A1[j], B00[j],    \
                  B01[j], B11[j])
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
      const float sc = lm_group_sum(s_cost[j], wide);
      const float a0 = lm_group_sum(A0[j], wide), a1 = lm_group_sum(A1[j], wide);
      const float b00 = lm_group_sum(B00[j], wide), b01 = lm_group_sum(B01[j], wide),
                  b11 = lm_group_sum(B11[j], wide);
      float rcost, wl;
      robust_loss(cf.loss, cf.loss_alpha, cf.loss_scale, sc, rcost, wl);
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

using InfoStage = StageRing<InfoParams, PXT_LM_INFO_MAX_PROBLEMS>;

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
  InfoStage::Slot* slot = nullptr;
  if (!from_args) {
    static thread_local InfoStage stage;
    if (const int rc = stage.acquire(&slot)) return rc;
    rec = slot->host;
  }
  int max_wgs = 1;
  for (int k = 0; k < K; ++k) {
    const pxt_lm_info_problem& q = problems[k];
    const pxt_lm_level& l = q.level;
    if (!q.p3d || !q.pose || !q.out || q.n_points < 1) return PXT_E_ARG;
    if (const int rc = check_level(l)) return rc;
    if (((uintptr_t)q.pose % 16) != 0 || ((uintptr_t)q.out % 4) != 0) return PXT_E_ARG;
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

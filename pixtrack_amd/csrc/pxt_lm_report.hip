// Which points carried the pose: the POINT terms of one LM iteration at a given pose, written out instead of summed
// (pxt_lm_point_report, include/pixtrack_hip.h).
//
// The reference keeps a refinement's point set at debug >= 2 (pixtrack/localization/tracker.py:26-30, filled from
// pixtrack/localization/pixloc_pose_refiners.py:200-271) and leaves everything per point - where it projects, whether
// the optimiser counted it, its residual and weights - to pixloc's plots.  The LM kernel forms those terms for every
// point on every iteration and drops them; this is the fourth consumer of pxt_lm_point.h (after lm_accumulate, the
// information kernel and the hypothesis scorer) and the one that keeps them: an 8-float record per point and a 16-float
// summary per problem.  Validity, projection, the 2 x 2 bilinear taps of the centre sample (PXT_LM_POINT_CH_COST: only
// the cost is needed - no map gradients, no Jacobian), w_unc = conf_query * conf_ref and rho / rho' are the LM's own.
//
// Mapping (pxt_lm_info.hip's, which see for the reasons)
//  * A point is owned by a lane GROUP as in the LM (4 consecutive channels per lane, dwordx4 texel reads: 32 lanes per
//    point for C > 32, 8 otherwise); TWO points are in flight per group.
//  * The points of ONE problem are dealt round-robin to the groups of n_wgs workgroups (blockIdx.x), the problems are
//    blockIdx.y.  n_wgs depends on the problem's n_points and C only, so a problem's summation order does not depend on
//    what else is in the launch.
//  * A point's record is 32 contiguous bytes: the group's lane 0 stores words 0..3, lane 1 words 4..7 (one dwordx4
//    each; every lane of the group holds the reduced values).  Plain vector stores.
//  * The group leaders' 8 sums are folded in a fixed order through LDS; across a problem's workgroups the partials go to
//    the workspace and the fold kernel (one wave per problem) adds them in workgroup order and writes the summary, word
//    15 last.  No atomics anywhere.  (The counts are sums of 1.f: exact below 2^24 points, which the entry point bounds.)
//  * The parameter record, the pose and the LM record's status words are read through vector loads: the pose may have
//    been written by the kernel just ahead in the stream.
#include "pxt_common.h"
#include "pxt_lm_point.h"

#include <algorithm>

namespace pxt {
namespace {

constexpr int kRepBlock = 256;
constexpr int kRepWaves = kRepBlock / PXT_WAVE;
constexpr int kRepMaxGroups = kRepBlock / 8;  // groups per workgroup at 8 lanes per point
constexpr int kRepMaxWgs = 128;               // workgroups per problem, at most
constexpr int kRepPointsPerGroup = 4;         // target; more when n_wgs is capped
constexpr int kRepAcc = 8;                    // floats per partial: words 0..7 of the summary
constexpr int kRepGrpStride = 9;              // padded: leaders of one wave hit distinct LDS banks
constexpr int kRepArgProblems = 2;            // parameter records that travel as kernel arguments

struct RepParams {  // 144 bytes
  const float* p3d;
  const uint8_t* mask;
  const float* fmap;
  const float* fref;
  const float* pose;
  float* points;
  float* summary;
  int n, h, w, C, cs, ndist, pose_is_record, n_wgs;
  float inlier_weight;
  float cam[10];
  int pad_[3];
};
static_assert(sizeof(RepParams) == 144, "parameter records are read as aligned vectors");

struct RepArgs {
  RepParams p[kRepArgProblems];
};

struct RepConf {
  int pad, loss, min_valid;
  float loss_alpha, loss_scale;
};

// What a point needs between its projection and its arithmetic.
struct RepPoint {
  bool valid, live;  // live: the point exists (i < N)
  int n;             // clamped into the bank: an invalid point's loads stay in bounds and are discarded
  int i;
  float code, u, v;
  float w00, w10, w01, w11;
  unsigned xo[2], yo[2];  // BYTE offsets of the 2 columns / rows of the taps, clamped into the map
  int xin, yin;           // bit k: column / row k lies inside the map (outside counts as zero: grid_sample 'zeros')
  __device__ __forceinline__ float in(int r, int c) const { return ((yin >> r) & (xin >> c) & 1) ? 1.f : 0.f; }
};

typedef const __attribute__((address_space(1))) char* RepGlobal;
typedef float RepVec4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 rep_texel(const float* base, unsigned byte_offset) {
  const RepVec4 v = *(const __attribute__((address_space(1))) RepVec4*)((RepGlobal)base + byte_offset);
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ float rep_word(const float* base, unsigned byte_offset) {
  return *(const __attribute__((address_space(1))) float*)((RepGlobal)base + byte_offset);
}

__device__ inline const RepParams* rep_params(const RepParams* ws_params, int from_args, int prob) {
  const RepParams* base = from_args ? (const RepParams*)__builtin_amdgcn_kernarg_segment_ptr() : ws_params;
  return vector_pointer(base + prob);
}

// -> false when the problem is skipped (its LM record reports failed / a status).
__device__ __forceinline__ bool rep_load_pose(const RepParams* q, float* T) {
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

// project_point's own "in front of the camera" and "inside the distortion model's range" tests, for the reject code
// (validity itself is point_in_window's).
__device__ inline bool rep_projectable(const Cam& c, float x, float y, float z) {
  if (!(z > kCamEps)) return false;
  if (c.ndist <= 0) return true;
  const float iz = 1.0f / fmaxf(z, kCamEps);
  const float xn = x * iz, yn = y * iz;
  const float r2 = xn * xn + yn * yn;
  const float disc = 9.f * c.k1 * c.k1 - 20.f * c.k2;
  const bool limited = ((c.k2 > 0.f) && (disc > 0.f)) || ((c.k2 <= 0.f) && (c.k1 > 0.f));
  if (!limited) return true;
  const float limit = (c.k2 > 0.f) ? (sqrtf(fmaxf(disc, 0.f)) - 3.f * c.k1) / (10.f * c.k2) : 1.f / (3.f * c.k1);
  return r2 < fabsf(limit);
}

__global__ __launch_bounds__(kRepBlock) void lm_report_points_kernel(const RepArgs args, const RepParams* ws_params,
                                                                     float* partials, const RepConf cf,
                                                                     const int from_args) {
  __shared__ float part[kRepMaxGroups * kRepGrpStride];
  const int prob = blockIdx.y, b = blockIdx.x;
  const RepParams* q = rep_params(ws_params, from_args, prob);
  const int n_wgs = uniform(q->n_wgs);
  if (b >= n_wgs) return;  // (workgroup-uniform)
  float T[12];
  if (!rep_load_pose(q, T)) return;  // skipped: the fold kernel marks the summary

  const int N = uniform(q->n), W = uniform(q->w), H = uniform(q->h), C = uniform(q->C), cs = uniform(q->cs);
  const bool wide = C > 32;
  const int LG = wide ? 32 : 8;
  const int GPW = PXT_WAVE / LG, G = kRepWaves * GPW;  // groups per wave / per workgroup
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
  float* points = uniform(q->points);
  const float inlier_weight = uniform(q->inlier_weight);
  const float pad = (float)cf.pad;

  float acc[kRepAcc];
#pragma unroll
  for (int k = 0; k < kRepAcc; ++k) acc[k] = 0.f;

  // point i of the problem -> group (i mod TG) of the problem's TG groups; a group takes its points two at a time
  const int TG = n_wgs * G;
  const int first = b * G + grp;
#pragma unroll 1
  for (int i0 = first; i0 < N; i0 += 2 * TG) {
    RepPoint pt[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      RepPoint& p = pt[j];
      p.i = i0 + j * TG;
      p.live = p.i < N;
      p.n = min(p.i, N - 1);
      const float X = rep_word(p3d, 12u * (unsigned)p.n), Y = rep_word(p3d, 12u * (unsigned)p.n + 4u),
                  Z = rep_word(p3d, 12u * (unsigned)p.n + 8u);
      bool kept = true;
      if (mask) kept = *((const __attribute__((address_space(1))) uint8_t*)mask + (unsigned)p.n) != 0;
      float px, py, pz;
      transform_point(T, X, Y, Z, px, py, pz);
      bool valid = p.live && kept;
      float u, v;
      point_in_window(cam, px, py, pz, valid, W, H, pad, u, v, nullptr);
      p.valid = valid;
      p.code = valid ? 0.f : (!kept ? 1.f : (!rep_projectable(cam, px, py, pz) ? 2.f : 3.f));
      const float nan = __builtin_nanf("");
      p.u = pz > kCamEps ? u : nan;
      p.v = pz > kCamEps ? v : nan;
      if (!valid) u = v = 0.f;  // (u, v may be anything, NaN included: keep the address arithmetic defined)
      int ix0, iy0;
      bilinear_weights(u, v, ix0, iy0, p.w00, p.w10, p.w01, p.w11);
      p.xin = p.yin = 0;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int xx = ix0 + k, yy = iy0 + k;
        p.xin |= (xx >= 0 && xx < W) ? 1 << k : 0;
        p.yin |= (yy >= 0 && yy < H) ? 1 << k : 0;
        p.xo[k] = (unsigned)(min(max(xx, 0), W - 1) * cs) * 4u;
        p.yo[k] = (unsigned)(min(max(yy, 0), H - 1) * W * cs) * 4u;
      }
    }

    float s_cost[2] = {0.f, 0.f};
#pragma unroll 1
    for (int c0 = 4 * sub; c0 < C; c0 += 4 * LG) {
      // both points' 5 reads are issued before the arithmetic of either
      float4 t11[2], t12[2], t21[2], t22[2], fr[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const RepPoint& p = pt[j];
        const unsigned cb = 4u * (unsigned)c0;
        t11[j] = rep_texel(fmap, p.yo[0] + p.xo[0] + cb);
        t12[j] = rep_texel(fmap, p.yo[0] + p.xo[1] + cb);
        t21[j] = rep_texel(fmap, p.yo[1] + p.xo[0] + cb);
        t22[j] = rep_texel(fmap, p.yo[1] + p.xo[1] + cb);
        fr[j] = rep_texel(fref, 4u * (unsigned)(p.n * cs) + cb);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const RepPoint& p = pt[j];
        const float m11 = p.in(0, 0), m12 = p.in(0, 1), m21 = p.in(1, 0), m22 = p.in(1, 1);
#define PXT_REP_CH(q_)                                                                                           \
  PXT_LM_POINT_CH_COST(p.w00, p.w10, p.w01, p.w11, t11[j].q_ * m11, t12[j].q_ * m12, t21[j].q_ * m21, t22[j].q_ * m22, \
                       fr[j].q_, s_cost[j])
        PXT_REP_CH(x) PXT_REP_CH(y) PXT_REP_CH(z) PXT_REP_CH(w)
#undef PXT_REP_CH
      }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const RepPoint& p = pt[j];
      // confidence: bilinear sample of channel C (one address for the whole group)
      const unsigned cb = 4u * (unsigned)C;
      const float q11 = rep_word(fmap, p.yo[0] + p.xo[0] + cb) * p.in(0, 0);
      const float q12 = rep_word(fmap, p.yo[0] + p.xo[1] + cb) * p.in(0, 1);
      const float q21 = rep_word(fmap, p.yo[1] + p.xo[0] + cb) * p.in(1, 0);
      const float q22 = rep_word(fmap, p.yo[1] + p.xo[1] + cb) * p.in(1, 1);
      const float wq = p.w00 * q11 + p.w10 * q12 + p.w01 * q21 + p.w11 * q22;
      const float wref = rep_word(fref, 4u * (unsigned)(p.n * cs) + cb);
      const float sc = lm_group_sum(s_cost[j], wide);
      float rcost, wl;
      robust_loss(cf.loss, cf.loss_alpha, cf.loss_scale, sc, rcost, wl);
      const float wunc = wref * wq;
      const float ok = p.valid ? 1.f : 0.f;
      if (p.valid) {  // group-uniform: an invalid point contributes nothing
        acc[0] += rcost;
        acc[1] += 1.f;
        acc[2] += wl >= inlier_weight ? 1.f : 0.f;
        acc[3] += wl * wunc;
        acc[4] += wunc;
      } else if (p.live) {
        acc[5] += p.code == 1.f ? 1.f : 0.f;
        acc[6] += p.code == 2.f ? 1.f : 0.f;
        acc[7] += p.code == 3.f ? 1.f : 0.f;
      }
      if (points && p.live && sub < 2) {  // the record's two halves, one 16-byte store each
        const float4 lo = make_float4(ok, p.u, p.v, p.valid ? sc : 0.f);
        const float4 hi = make_float4(p.valid ? rcost : 0.f, p.valid ? wl : 0.f, p.valid ? wunc : 0.f, p.code);
        const float4 half = sub == 0 ? lo : hi;
        RepVec4 o;
        o.x = half.x; o.y = half.y; o.z = half.z; o.w = half.w;
        ((__attribute__((address_space(1))) RepVec4*)points)[2 * (size_t)p.i + sub] = o;
      }
    }
  }

  if (sub == 0) {
#pragma unroll
    for (int k = 0; k < kRepAcc; ++k) part[grp * kRepGrpStride + k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < kRepAcc) {  // the groups' sums in a fixed order
    float v = 0.f;
    for (int g = 0; g < G; ++g) v += part[g * kRepGrpStride + threadIdx.x];
    partials[((size_t)prob * kRepMaxWgs + b) * kRepAcc + threadIdx.x] = v;
  }
}

// One wave per problem: the workgroups' partials in workgroup order, then the summary; word 15 last.
__global__ __launch_bounds__(PXT_WAVE) void lm_report_fold_kernel(const RepArgs args, const RepParams* ws_params,
                                                                  const float* partials, const RepConf cf,
                                                                  const int from_args) {
  __shared__ float rec[kRepAcc];
  const int prob = blockIdx.x;
  const RepParams* q = rep_params(ws_params, from_args, prob);
  float* out = uniform(q->summary);
  float T[12];
  const bool run = rep_load_pose(q, T);
  if (!run) {
    if (threadIdx.x == 0) __hip_atomic_store(&out[15], -1.f, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    return;
  }
  const int n_wgs = uniform(q->n_wgs);
  if (threadIdx.x < kRepAcc) {
    const float* p = partials + (size_t)prob * kRepMaxWgs * kRepAcc + threadIdx.x;
    float v = 0.f;
    for (int b = 0; b < n_wgs; ++b) v += p[(size_t)b * kRepAcc];
    rec[threadIdx.x] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {  // one thread writes the summary, so that its release covers every word
    for (int k = 0; k < kRepAcc; ++k) out[k] = rec[k];
    for (int k = kRepAcc; k < 15; ++k) out[k] = 0.f;
    const float ok = rec[1] >= (float)cf.min_valid ? 1.f : -2.f;  // -2: evaluated, but the LM would call it failed
    __hip_atomic_store(&out[15], ok, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

int rep_workgroups(int n_points, int C) {
  const int groups = kRepBlock / (C > 32 ? 32 : 8);
  const int per_wg = groups * kRepPointsPerGroup;
  return std::max(1, std::min(kRepMaxWgs, (n_points + per_wg - 1) / per_wg));
}

size_t rep_params_bytes(int n_problems) { return ((size_t)n_problems * sizeof(RepParams) + 255) / 256 * 256; }

using RepStage = StageRing<RepParams, PXT_LM_REPORT_MAX_PROBLEMS>;

}  // namespace
}  // namespace pxt

using namespace pxt;

extern "C" int64_t pxt_lm_point_report_workspace_bytes(int32_t n_problems) {
  if (n_problems < 1 || n_problems > PXT_LM_REPORT_MAX_PROBLEMS) return PXT_E_ARG;
  return (int64_t)(rep_params_bytes(n_problems) + (size_t)n_problems * kRepMaxWgs * kRepAcc * sizeof(float));
}

extern "C" int pxt_lm_point_report(const pxt_lm_report_problem* problems, int32_t n_problems, const pxt_lm_conf* conf,
                                   void* workspace, void* stream) {
  if (!problems || !conf || !workspace) return PXT_E_ARG;
  if (n_problems < 1 || n_problems > PXT_LM_REPORT_MAX_PROBLEMS) return PXT_E_ARG;
  if (((uintptr_t)workspace % 16) != 0) return PXT_E_ARG;
  if (conf->pad < 0 || conf->loss < 0 || conf->loss > 2 || conf->min_valid < 0) return PXT_E_ARG;
  const int K = n_problems;
  const bool from_args = K <= kRepArgProblems;
  RepArgs args = {};
  RepParams* rec = args.p;
  RepStage::Slot* slot = nullptr;
  if (!from_args) {
    static thread_local RepStage stage;
    if (const int rc = stage.acquire(&slot)) return rc;
    rec = slot->host;
  }
  int max_wgs = 1;
  for (int k = 0; k < K; ++k) {
    const pxt_lm_report_problem& q = problems[k];
    const pxt_lm_level& l = q.level;
    if (!q.p3d || !q.pose || !q.summary || q.n_points < 1 || q.n_points > (1 << 24)) return PXT_E_ARG;
    if (const int rc = check_level(l)) return rc;
    if (((uintptr_t)q.pose % 16) != 0 || ((uintptr_t)q.summary % 4) != 0 || ((uintptr_t)q.points % 16) != 0) return PXT_E_ARG;
    if (!(q.inlier_weight == q.inlier_weight)) return PXT_E_ARG;  // NaN
    // (byte offsets inside the map and the reference records are 32-bit in the kernel)
    if ((long long)l.h * l.w * l.cstride >= (1ll << 30) || (long long)q.n_points * l.cstride >= (1ll << 30)) return PXT_E_ARG;
    for (int j = 0; j < k; ++j)
      if (problems[j].summary == q.summary || (q.points && problems[j].points == q.points)) return PXT_E_ARG;
    RepParams& P = rec[k];
    P.p3d = q.p3d;
    P.mask = q.point_mask;
    P.fmap = l.fmap;
    P.fref = l.fref;
    P.pose = q.pose;
    P.points = q.points;
    P.summary = q.summary;
    P.n = q.n_points;
    P.h = l.h; P.w = l.w; P.C = l.C; P.cs = l.cstride; P.ndist = l.ndist;
    P.pose_is_record = q.pose_is_lm_record != 0;
    P.n_wgs = rep_workgroups(q.n_points, l.C);
    P.inlier_weight = q.inlier_weight;
    for (int i = 0; i < 10; ++i) P.cam[i] = l.cam[i];
    P.pad_[0] = P.pad_[1] = P.pad_[2] = 0;
    max_wgs = std::max(max_wgs, P.n_wgs);
  }
  RepConf cf;
  cf.pad = conf->pad;
  cf.loss = conf->loss;
  cf.min_valid = conf->min_valid;
  cf.loss_alpha = conf->loss_alpha;
  cf.loss_scale = conf->loss_scale;
  hipStream_t s = (hipStream_t)stream;
  const RepParams* ws_params = (const RepParams*)workspace;
  float* partials = (float*)((char*)workspace + rep_params_bytes(K));
  if (!from_args) {
    PXT_HIP_CHECK(hipMemcpyAsync(workspace, slot->host, (size_t)K * sizeof(RepParams), hipMemcpyHostToDevice, s));
    PXT_HIP_CHECK(hipEventRecord(slot->copied, s));
  }
  hipLaunchKernelGGL(lm_report_points_kernel, dim3(max_wgs, K), dim3(kRepBlock), 0, s, args, ws_params, partials, cf,
                     (int)from_args);
  PXT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(lm_report_fold_kernel, dim3(K), dim3(PXT_WAVE), 0, s, args, ws_params, (const float*)partials, cf,
                     (int)from_args);
  PXT_HIP_CHECK(hipGetLastError());
  return PXT_OK;
}

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
// The mapping of points to lanes and workgroups, the folds, the loads and the launch are the evaluation frame's
// (pxt_lm_eval.h, which see for the reasons).  This kernel's own:
//  * A point's record is 32 contiguous bytes: the group's lane 0 stores words 0..3, lane 1 words 4..7 (one dwordx4
//    each; every lane of the group holds the reduced values).  Plain vector stores.
//  * The group leaders fold 8 sums.  (The counts are sums of 1.f: exact below 2^24 points, which the entry point bounds.)
#include "pxt_lm_eval.h"

namespace pxt {
namespace {

constexpr int kRepAcc = 8;        // floats per partial: words 0..7 of the summary
constexpr int kRepGrpStride = 9;  // padded: leaders of one wave hit distinct LDS banks

struct RepParams {  // 144 bytes
  const float* p3d;
  const uint8_t* mask;
  const float* fmap;
  const float* fref;
  const float* pose;
  float* points;
  float* out;  // the summary
  int n, h, w, C, cs, ndist, pose_is_record, n_wgs;
  float inlier_weight;
  float cam[10];
  int pad_[3];
};
static_assert(sizeof(RepParams) == 144, "parameter records are read as aligned vectors");

// What a point needs between its projection and its arithmetic.
struct RepPoint : EvalPoint<2, 0> {
  bool valid, live;  // live: the point exists (i < N)
  int i;
  float code, u, v;
};

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

__global__ __launch_bounds__(kEvalBlock) void lm_report_points_kernel(const EvalArgs<RepParams> args,
                                                                      const RepParams* ws_params, float* partials,
                                                                      const EvalConf cf, const int from_args) {
  __shared__ float part[kEvalMaxGroups * kRepGrpStride];
  const int prob = blockIdx.y, b = blockIdx.x;
  const RepParams* q = eval_params(ws_params, from_args, prob);
  const int n_wgs = uniform(q->n_wgs);
  if (b >= n_wgs) return;  // (workgroup-uniform)
  float T[12];
  if (!eval_load_pose(q, T)) return;  // skipped: the fold kernel marks the summary

  PXT_EVAL_LANES(q);  // declares N, W, H, C, cs, wide, LG, G, sub, grp, cam, p3d, mask, fmap, fref
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
      const float X = eval_word(p3d, 12u * (unsigned)p.n), Y = eval_word(p3d, 12u * (unsigned)p.n + 4u),
                  Z = eval_word(p3d, 12u * (unsigned)p.n + 8u);
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
      PXT_EVAL_PLACE(p, ix0, iy0, W, H, cs);
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
        t11[j] = eval_texel(fmap, p.yo[0] + p.xo[0] + cb);
        t12[j] = eval_texel(fmap, p.yo[0] + p.xo[1] + cb);
        t21[j] = eval_texel(fmap, p.yo[1] + p.xo[0] + cb);
        t22[j] = eval_texel(fmap, p.yo[1] + p.xo[1] + cb);
        fr[j] = eval_texel(fref, 4u * (unsigned)(p.n * cs) + cb);
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
      PXT_EVAL_CONFIDENCE(p, fmap, fref, C, cs);  // declares wq, wref (and cb, c_, q11..q22)
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
        EvalVec4 o;
        o.x = half.x; o.y = half.y; o.z = half.z; o.w = half.w;
        ((__attribute__((address_space(1))) EvalVec4*)points)[2 * (size_t)p.i + sub] = o;
      }
    }
  }

  eval_fold_groups<kRepAcc, kRepGrpStride, kRepAcc>(part, acc, sub, grp, G, partials, prob, b);
}

// One wave per problem: the summary's 8 sums, zeros; word 15 last.
__global__ __launch_bounds__(PXT_WAVE) void lm_report_fold_kernel(const EvalArgs<RepParams> args, const RepParams* ws_params,
                                                                  const float* partials, const EvalConf cf,
                                                                  const int from_args) {
  // declares prob, q, out, T, rec; RETURNS when the problem is skipped
  PXT_EVAL_FOLD_SUMS(RepParams, kRepAcc, 15, ws_params, from_args, partials);
  if (threadIdx.x == 0) {
    for (int k = 0; k < kRepAcc; ++k) out[k] = rec[k];
    for (int k = kRepAcc; k < 15; ++k) out[k] = 0.f;
    PXT_EVAL_FOLD_DONE(15, cf);  // reads rec[1], stores out[LAST]
  }
}

}  // namespace
}  // namespace pxt

using namespace pxt;

extern "C" int64_t pxt_lm_point_report_workspace_bytes(int32_t n_problems) {
  return eval_workspace_bytes<RepParams, kRepAcc>(n_problems, PXT_LM_REPORT_MAX_PROBLEMS);
}

extern "C" int pxt_lm_point_report(const pxt_lm_report_problem* problems, int32_t n_problems, const pxt_lm_conf* conf,
                                   void* workspace, void* stream) {
  const auto fill = [&](int k, RepParams& r) {
    const pxt_lm_report_problem& q = problems[k];
    if (!q.summary || q.n_points > (1 << 24)) return PXT_E_ARG;
    if (((uintptr_t)q.summary % 4) != 0 || ((uintptr_t)q.points % 16) != 0) return PXT_E_ARG;
    if (!(q.inlier_weight == q.inlier_weight)) return PXT_E_ARG;  // NaN
    for (int j = 0; j < k; ++j)
      if (problems[j].summary == q.summary || (q.points && problems[j].points == q.points)) return PXT_E_ARG;
    r.points = q.points;
    r.out = q.summary;
    r.inlier_weight = q.inlier_weight;
    return PXT_OK;
  };
  return eval_launch<RepParams, PXT_LM_REPORT_MAX_PROBLEMS>(problems, n_problems, conf, workspace, stream, fill,
                                                            lm_report_points_kernel, lm_report_fold_kernel);
}

// The LM's normal equations at a given pose, evaluated ONCE (pxt_lm_information, include/pixtrack_hip.h).
//
// For each of n_problems independent (points, level, pose) problems one launch forms the sums of one LM iteration at
// the given pose - sum rho, n_valid, sum w |r|^2, sum w, g = sum w J^T r and the upper triangle of the UNDAMPED
// H = sum w J^T J - and a second small launch folds them into a 48-float record.  Validity, projection, the 12-texel
// cross footprint of the five bilinear taps, the central-difference map gradients, w_unc = conf_query * conf_ref and
// rho / rho' are the LM's own (pxt_lm_point.h, which lm_accumulate is written in as well); the parameter order is the
// LM's delta (translation 3, rotation 3, left update).
//
// The mapping of points to lanes and workgroups, the folds, the loads and the launch are the evaluation frame's
// (pxt_lm_eval.h, which see for the reasons).  This kernel's own: J^T J = Jp^T (gradF^T gradF) Jp, so six scalars per
// point cross the group, and the group leaders fold 31 sums.
#include "pxt_lm_eval.h"

namespace pxt {
namespace {

constexpr int kInfoAcc = 32;        // floats per partial: words 0..30 of the record, one pad
constexpr int kInfoGrpStride = 33;  // padded: leaders of one wave hit distinct LDS banks

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

// What a point needs between its projection and its arithmetic: the 4 x 4 neighbourhood around the sample.
struct InfoPoint : EvalPoint<4, -1> {
  bool valid;
  float px, py, pz, Jw[6];
};

__global__ __launch_bounds__(kEvalBlock) void lm_info_accumulate_kernel(const EvalArgs<InfoParams> args,
                                                                        const InfoParams* ws_params, float* partials,
                                                                        const EvalConf cf, const int from_args) {
  __shared__ float part[kEvalMaxGroups * kInfoGrpStride];
  const int prob = blockIdx.y, b = blockIdx.x;
  const InfoParams* q = eval_params(ws_params, from_args, prob);
  const int n_wgs = uniform(q->n_wgs);
  if (b >= n_wgs) return;  // (workgroup-uniform)
  float T[12];
  if (!eval_load_pose(q, T)) return;  // skipped: the fold kernel marks the record
  PXT_EVAL_LANES(q);  // declares N, W, H, C, cs, wide, LG, G, sub, grp, cam, p3d, mask, fmap, fref
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
      const float X = eval_word(p3d, 12u * (unsigned)p.n), Y = eval_word(p3d, 12u * (unsigned)p.n + 4u),
                  Z = eval_word(p3d, 12u * (unsigned)p.n + 8u);
      if (mask) valid = valid && *((const __attribute__((address_space(1))) uint8_t*)mask + (unsigned)p.n) != 0;
      transform_point(T, X, Y, Z, p.px, p.py, p.pz);
      float u, v;
      point_in_window(cam, p.px, p.py, p.pz, valid, W, H, pad, u, v, p.Jw);
      if (!valid) u = v = 0.f;  // (u, v may be anything, NaN included: keep the address arithmetic defined)
      p.valid = valid;
      int ix0, iy0;
      bilinear_weights(u, v, ix0, iy0, p.w00, p.w10, p.w01, p.w11);
      PXT_EVAL_PLACE(p, ix0, iy0, W, H, cs);
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
        t01[j] = eval_texel(fmap, p.yo[0] + p.xo[1] + cb);
        t02[j] = eval_texel(fmap, p.yo[0] + p.xo[2] + cb);
        t10[j] = eval_texel(fmap, p.yo[1] + p.xo[0] + cb);
        t11[j] = eval_texel(fmap, p.yo[1] + p.xo[1] + cb);
        t12[j] = eval_texel(fmap, p.yo[1] + p.xo[2] + cb);
        t13[j] = eval_texel(fmap, p.yo[1] + p.xo[3] + cb);
        t20[j] = eval_texel(fmap, p.yo[2] + p.xo[0] + cb);
        t21[j] = eval_texel(fmap, p.yo[2] + p.xo[1] + cb);
        t22[j] = eval_texel(fmap, p.yo[2] + p.xo[2] + cb);
        t23[j] = eval_texel(fmap, p.yo[2] + p.xo[3] + cb);
        t31[j] = eval_texel(fmap, p.yo[3] + p.xo[1] + cb);
        t32[j] = eval_texel(fmap, p.yo[3] + p.xo[2] + cb);
        fr[j] = eval_texel(fref, 4u * (unsigned)(p.n * cs) + cb);
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
      PXT_EVAL_CONFIDENCE(p, fmap, fref, C, cs);  // declares wq, wref (and cb, c_, q11..q22)
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
  eval_fold_groups<kInfoAcc, kInfoGrpStride, kInfoAcc - 1>(part, acc, sub, grp, G, partials, prob, b);
}

// One wave per problem: the record's 31 sums, a zero, the pose that was evaluated, zeros; word 47 last.
__global__ __launch_bounds__(PXT_WAVE) void lm_info_fold_kernel(const EvalArgs<InfoParams> args, const InfoParams* ws_params,
                                                                const float* partials, const EvalConf cf,
                                                                const int from_args) {
  // declares prob, q, out, T, rec; RETURNS when the problem is skipped
  PXT_EVAL_FOLD_SUMS(InfoParams, kInfoAcc, 47, ws_params, from_args, partials);
  if (threadIdx.x == 0) {
    for (int k = 0; k < kInfoAcc - 1; ++k) out[k] = rec[k];
    out[31] = 0.f;
    for (int k = 0; k < 12; ++k) out[32 + k] = T[k];
    out[44] = out[45] = out[46] = 0.f;
    PXT_EVAL_FOLD_DONE(47, cf);  // reads rec[1], stores out[LAST]
  }
}

}  // namespace
}  // namespace pxt

using namespace pxt;

extern "C" int64_t pxt_lm_information_workspace_bytes(int32_t n_problems) {
  return eval_workspace_bytes<InfoParams, kInfoAcc>(n_problems, PXT_LM_INFO_MAX_PROBLEMS);
}

extern "C" int pxt_lm_information(const pxt_lm_info_problem* problems, int32_t n_problems, const pxt_lm_conf* conf,
                                  void* workspace, void* stream) {
  const auto fill = [&](int k, InfoParams& r) {
    const pxt_lm_info_problem& q = problems[k];
    if (!q.out || ((uintptr_t)q.out % 4) != 0) return PXT_E_ARG;
    for (int j = 0; j < k; ++j)
      if (problems[j].out == q.out) return PXT_E_ARG;
    r.out = q.out;
    return PXT_OK;
  };
  return eval_launch<InfoParams, PXT_LM_INFO_MAX_PROBLEMS>(problems, n_problems, conf, workspace, stream, fill,
                                                           lm_info_accumulate_kernel, lm_info_fold_kernel);
}

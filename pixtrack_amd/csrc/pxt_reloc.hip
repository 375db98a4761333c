// Scoring of pose hypotheses for relocalisation (pxt_score_pose_hypotheses, include/pixtrack_hip.h).
//
// One launch scores M poses against ONE query feature map (the LM's layout: HWC float32, descriptor L2-normalised over
// C channels, confidence at channel C, cstride = round4(C + 1)).  Hypothesis h owns the points [begin, begin + count)
// of one flat bank (p3d, reference records, optional point mask) and gets four sums over its VALID points:
//   out[h] = { sum rho(|F_q - F_ref|^2), n_valid, sum w * rho, sum w },  w = conf_query * conf_ref.
// Projection, bilinear taps, the group sum and rho are the LM's own (pxt_lm_point.h, which lm_accumulate is written in
// as well; the validity rule is point_in_window's, by hand): out[h][0] / out[h][1] is the masked-mean cost
// pxt_lm_refine logs at k = 0 of its first iteration for the same pose, points and level, out[h][1] its k = 1.
//
// Mapping: one workgroup per hypothesis (384 hypotheses on 256 CUs: no inter-workgroup exchange), 16 waves; a point
// is owned by a lane GROUP as in the LM (4 consecutive channels per lane, dwordx4 texel reads: 32 lanes per point at
// C = 128, 8 for C <= 32).  A group's leader keeps its four running sums in registers; at the end the groups' sums
// are folded in a fixed order through LDS, so a hypothesis's values depend on its own inputs only - not on M, on the
// other hypotheses or on the run.  No atomics anywhere.
//
// The camera (kernel argument), the pose and the range of a hypothesis (device arrays: M is bounded by memory, not by
// the kernel-argument segment) are read through vector loads (pointers made opaque VGPR values, as the renderer's
// camera is: DESIGN.md section 7).
#include "pxt_common.h"
#include "pxt_lm_point.h"

namespace pxt {
namespace {

constexpr int kRelocBlock = 1024;
constexpr int kRelocWaves = kRelocBlock / PXT_WAVE;

struct RelocParams {
  const float* fmap;
  const float* p3d;
  const float* fref;
  const uint8_t* valid;
  const float* poses;    // [M][12]
  const int32_t* ranges; // [M][2] {begin, count}
  float* out;            // [M][4]
  int h, w, C, cs, ndist, n_total, pad, loss;
  float loss_alpha, loss_scale;
  float cam[10];
};

template <int LG>
__global__ __launch_bounds__(kRelocBlock) void reloc_score_kernel(const RelocParams P) {
  constexpr int GPW = PXT_WAVE / LG;          // groups per wave
  constexpr int kGroups = kRelocWaves * GPW;  // groups per workgroup
  __shared__ float part[kGroups][4];
  const int hyp = blockIdx.x;
  const int lane = threadIdx.x & (PXT_WAVE - 1);
  const int sub = lane & (LG - 1);
  const int grp = (threadIdx.x / PXT_WAVE) * GPW + lane / LG;

  float c10[10];
  {  // (through the kernarg segment pointer: taking the address of the by-value argument would copy it to scratch)
    const float* c = vector_pointer(((const RelocParams*)__builtin_amdgcn_kernarg_segment_ptr())->cam);
#pragma unroll
    for (int i = 0; i < 10; ++i) c10[i] = c[i];
  }
  const Cam cam = make_cam(c10, P.ndist);
  float T[12];
  load_pose12(vector_pointer(P.poses + (size_t)hyp * 12), T);
  const int2 rg = *(const int2*)vector_pointer(P.ranges + (size_t)hyp * 2);
  const int begin = rg.x, count = rg.y;
  // a range outside the bank is reported (NaN cost, n_valid = -1) instead of read
  const bool bad = begin < 0 || count < 0 || (long long)begin + count > (long long)P.n_total;

  const int W = P.w, H = P.h, C = P.C, cs = P.cs;
  const float pad = (float)P.pad;
  float s_rho = 0.f, s_n = 0.f, s_wrho = 0.f, s_w = 0.f;  // meaningful in each group's lane 0

#pragma unroll 1
  for (int i = grp; !bad && i < count; i += kGroups) {
    const int n = begin + i;
    const float X = P.p3d[3 * (size_t)n], Y = P.p3d[3 * (size_t)n + 1], Z = P.p3d[3 * (size_t)n + 2];
    bool valid = P.valid ? P.valid[n] != 0 : true;
    float px, py, pz, u, v;
    transform_point(T, X, Y, Z, px, py, pz);
    // point_in_window() by hand: through the call this kernel's generated code changes (two scalar ANDs swap operands)
    valid = project_point(cam, px, py, pz, u, v, nullptr) && valid;
    valid = valid && (u >= pad) && (v >= pad) && (u <= (float)(W - 1) - pad) && (v <= (float)(H - 1) - pad);
    if (!valid) continue;  // group-uniform

    int ix0, iy0;
    float w00, w10, w01, w11;
    bilinear_weights(u, v, ix0, iy0, w00, w10, w01, w11);
    // the 2 x 2 taps; a texel outside the map counts as zero (the LM's masks), addresses clamped into the map
    const float mx1 = (ix0 + 1 < W) ? 1.f : 0.f, my1 = (iy0 + 1 < H) ? 1.f : 0.f;
    const float mx0 = (ix0 >= 0) ? 1.f : 0.f, my0 = (iy0 >= 0) ? 1.f : 0.f;
    const int x0 = min(max(ix0, 0), W - 1), x1 = min(max(ix0 + 1, 0), W - 1);
    const int y0 = min(max(iy0, 0), H - 1), y1 = min(max(iy0 + 1, 0), H - 1);
    const float m11 = my0 * mx0, m12 = my0 * mx1, m21 = my1 * mx0, m22 = my1 * mx1;
    const float* p00 = P.fmap + ((size_t)y0 * W + x0) * cs;
    const float* p10 = P.fmap + ((size_t)y0 * W + x1) * cs;
    const float* p01 = P.fmap + ((size_t)y1 * W + x0) * cs;
    const float* p11 = P.fmap + ((size_t)y1 * W + x1) * cs;
    const float* fr = P.fref + (size_t)n * cs;

    float s_cost = 0.f;
#pragma unroll 1
    for (int c0 = 4 * sub; c0 < C; c0 += 4 * LG) {
      const float4 t11 = *(const float4*)(p00 + c0), t12 = *(const float4*)(p10 + c0);
      const float4 t21 = *(const float4*)(p01 + c0), t22 = *(const float4*)(p11 + c0);
      const float4 f = *(const float4*)(fr + c0);
#define PXT_RELOC_CH(q) \
  PXT_LM_POINT_CH_COST(w00, w10, w01, w11, t11.q * m11, t12.q * m12, t21.q * m21, t22.q * m22, f.q, s_cost)
      PXT_RELOC_CH(x) PXT_RELOC_CH(y) PXT_RELOC_CH(z) PXT_RELOC_CH(w)
#undef PXT_RELOC_CH
    }
    const float q11 = p00[C] * m11, q12 = p10[C] * m12, q21 = p01[C] * m21, q22 = p11[C] * m22;
    const float wq = w00 * q11 + w10 * q12 + w01 * q21 + w11 * q22;
    const float wref = fr[C];
    s_cost = lm_group_sum_t<LG>(s_cost);
    float rho, wl;  // (the loss's derivative is not used here)
    robust_loss(P.loss, P.loss_alpha, P.loss_scale, s_cost, rho, wl);
    const float wgt = wref * wq;
    s_rho += rho;
    s_n += 1.f;
    s_wrho += wgt * rho;
    s_w += wgt;
  }
  if (sub == 0) {
    part[grp][0] = s_rho;
    part[grp][1] = s_n;
    part[grp][2] = s_wrho;
    part[grp][3] = s_w;
  }
  __syncthreads();
  if (threadIdx.x == 0) {  // the groups' sums in a fixed order
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int g = 0; g < kGroups; ++g) {
      o.x += part[g][0];
      o.y += part[g][1];
      o.z += part[g][2];
      o.w += part[g][3];
    }
    if (bad) o = make_float4(__builtin_nanf(""), -1.f, __builtin_nanf(""), __builtin_nanf(""));
    *(float4*)(P.out + (size_t)hyp * 4) = o;
  }
}

}  // namespace
}  // namespace pxt

using namespace pxt;

extern "C" int pxt_score_pose_hypotheses(const pxt_reloc_map* map, const pxt_reloc_bank* bank, const float* poses,
                                         const int32_t* ranges, int32_t n_hypotheses, const pxt_lm_conf* conf, float* out,
                                         void* stream) {
  if (!map || !bank || !poses || !ranges || !conf || !out) return PXT_E_ARG;
  if (n_hypotheses <= 0) return PXT_E_ARG;
  if (const int rc = check_level(map->fmap, bank->fref, map->h, map->w, map->C, map->cstride, map->ndist)) return rc;
  if (!bank->p3d || bank->n_points < 1) return PXT_E_ARG;
  if (((uintptr_t)poses % 16) != 0 || ((uintptr_t)ranges % 8) != 0 || ((uintptr_t)out % 16) != 0) return PXT_E_ARG;
  if (conf->pad < 0 || conf->loss < 0 || conf->loss > 2) return PXT_E_ARG;
  RelocParams P;
  P.fmap = map->fmap;
  P.p3d = bank->p3d;
  P.fref = bank->fref;
  P.valid = bank->valid;
  P.poses = poses;
  P.ranges = ranges;
  P.out = out;
  P.h = map->h; P.w = map->w; P.C = map->C; P.cs = map->cstride; P.ndist = map->ndist;
  P.n_total = bank->n_points;
  P.pad = conf->pad;
  P.loss = conf->loss;
  P.loss_alpha = conf->loss_alpha;
  P.loss_scale = conf->loss_scale;
  for (int i = 0; i < 10; ++i) P.cam[i] = map->cam[i];
  hipStream_t s = (hipStream_t)stream;
  if (map->C <= 32)
    hipLaunchKernelGGL(reloc_score_kernel<8>, dim3(n_hypotheses), dim3(kRelocBlock), 0, s, P);
  else
    hipLaunchKernelGGL(reloc_score_kernel<32>, dim3(n_hypotheses), dim3(kRelocBlock), 0, s, P);
  PXT_HIP_CHECK(hipGetLastError());
  return PXT_OK;
}

// Scoring of pose hypotheses for relocalisation (pxt_score_pose_hypotheses, include/pixtrack_hip.h).
//
// One launch scores M poses against ONE query feature map (the LM's layout: HWC float32, descriptor L2-normalised over
// C channels, confidence at channel C, cstride = round4(C + 1)).  Hypothesis h owns the points [begin, begin + count)
// of one flat bank (p3d, reference records, optional point mask) and gets four sums over its VALID points:
//   out[h] = { sum rho(|F_q - F_ref|^2), n_valid, sum w * rho, sum w },  w = conf_query * conf_ref.
// Validity, projection, bilinear taps and rho are those of lm_accumulate (pxt_lm.hip), restated here (that file is
// pinned by its tests and stays untouched): out[h][0] / out[h][1] is the masked-mean cost pxt_lm_refine logs at k = 0
// of its first iteration for the same pose, points and level, out[h][1] its k = 1.
//
// Mapping: one workgroup per hypothesis (384 hypotheses on 256 CUs: no inter-workgroup exchange), 16 waves; a point
// is owned by a lane GROUP as in the LM (4 consecutive channels per lane, dwordx4 texel reads: 32 lanes per point at
// C = 128, 8 for C <= 32).  A group's leader keeps its four running sums in registers; at the end the groups' sums
// are folded in a fixed order through LDS, so a hypothesis's values depend on its own inputs only - not on M, on the
// other hypotheses or on the run.  No atomics anywhere.
//
// The camera (kernel argument), the pose and the range of a hypothesis (device arrays: M is bounded by memory, not by
// the kernel-argument segment) are read through vector loads (pointers made opaque VGPR values, as the renderer's
// camera_pointer does: DESIGN.md section 7).
#include "pxt_common.h"

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

// pixloc scaled_loss(x, fn, a) = a^2 fn(x / a^2): the LM's robust_loss (pxt_lm.hip), the loss value only.
__device__ inline float reloc_rho(int kind, float alpha, float scale, float x) {
  if (kind == 0) return x;
  const float a2 = scale * scale;
  const float y = x / a2;
  float l;
  if (kind == 1) {  // huber
    l = y <= 1.f ? y : 2.f * sqrtf(y) - 1.f;
  } else {  // barron(alpha)
    if (alpha == 0.f) {
      l = 2.f * log1pf(fminf(0.5f * y, 33e37f));
    } else if (alpha == 2.f) {
      l = y;
    } else {
      const float beta = fmaxf(fabsf(alpha - 2.f), 1e-7f);
      const float as = (alpha >= 0.f ? 1.f : -1.f) * fmaxf(fabsf(alpha), 1e-7f);
      l = 2.f * (beta / as) * (powf(y / beta + 1.f, 0.5f * alpha) - 1.f);
    }
  }
  return l * a2;
}

// Sum over a point's LG lanes (every lane receives the total): the LM's fixed butterfly (DPP inside a 16-lane row, one
// cross-row step for 32 lanes), so a point's squared distance is formed in the LM's order.
__device__ inline float reloc_dpp_add(float v, int ctrl_tag) {
  const int iv = __builtin_bit_cast(int, v);
  int o;
  if (ctrl_tag == 0) o = __builtin_amdgcn_update_dpp(iv, iv, 0xB1, 0xF, 0xF, false);        // quad_perm [1,0,3,2]
  else if (ctrl_tag == 1) o = __builtin_amdgcn_update_dpp(iv, iv, 0x4E, 0xF, 0xF, false);   // quad_perm [2,3,0,1]
  else if (ctrl_tag == 2) o = __builtin_amdgcn_update_dpp(iv, iv, 0x141, 0xF, 0xF, false);  // row_half_mirror
  else o = __builtin_amdgcn_update_dpp(iv, iv, 0x140, 0xF, 0xF, false);                     // row_mirror
  return v + __builtin_bit_cast(float, o);
}

template <int LG>
__device__ inline float reloc_group_sum(float v) {
  v = reloc_dpp_add(v, 0);
  v = reloc_dpp_add(v, 1);
  v = reloc_dpp_add(v, 2);
  if (LG >= 16) v = reloc_dpp_add(v, 3);
  if (LG >= 32) v += __shfl_xor(v, 16, PXT_WAVE);
  return v;
}

template <typename T>
__device__ __forceinline__ const T* vector_pointer(const T* p) {
  asm volatile("" : "+v"(p));  // an opaque VGPR value: the loads through it are vector loads
  return p;
}

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
  {
    const float4* tp = (const float4*)vector_pointer(P.poses + (size_t)hyp * 12);
    const float4 a = tp[0], b = tp[1], d = tp[2];
    T[0] = a.x; T[1] = a.y; T[2] = a.z; T[3] = a.w;
    T[4] = b.x; T[5] = b.y; T[6] = b.z; T[7] = b.w;
    T[8] = d.x; T[9] = d.y; T[10] = d.z; T[11] = d.w;
  }
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
    const float px = T[0] * X + T[1] * Y + T[2] * Z + T[9];
    const float py = T[3] * X + T[4] * Y + T[5] * Z + T[10];
    const float pz = T[6] * X + T[7] * Y + T[8] * Z + T[11];
    float u, v;
    valid = project_point(cam, px, py, pz, u, v, nullptr) && valid;
    valid = valid && (u >= pad) && (v >= pad) && (u <= (float)(W - 1) - pad) && (v <= (float)(H - 1) - pad);
    if (!valid) continue;  // group-uniform

    const float fu = floorf(u), fv = floorf(v);
    const int ix0 = (int)fu, iy0 = (int)fv;
    const float ax = u - fu, ay = v - fv;
    const float w00 = (1.f - ax) * (1.f - ay), w10 = ax * (1.f - ay), w01 = (1.f - ax) * ay, w11 = ax * ay;
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
#define PXT_RELOC_CH(q)                                                                                       \
  {                                                                                                           \
    const float a11 = t11.q * m11, a12 = t12.q * m12, a21 = t21.q * m21, a22 = t22.q * m22;                   \
    const float F = w00 * a11 + w10 * a12 + w01 * a21 + w11 * a22;                                            \
    const float r = F - f.q;                                                                                  \
    s_cost += r * r;                                                                                          \
  }
      PXT_RELOC_CH(x) PXT_RELOC_CH(y) PXT_RELOC_CH(z) PXT_RELOC_CH(w)
#undef PXT_RELOC_CH
    }
    const float q11 = p00[C] * m11, q12 = p10[C] * m12, q21 = p01[C] * m21, q22 = p11[C] * m22;
    const float wq = w00 * q11 + w10 * q12 + w01 * q21 + w11 * q22;
    const float wref = fr[C];
    s_cost = reloc_group_sum<LG>(s_cost);
    const float rho = reloc_rho(P.loss, P.loss_alpha, P.loss_scale, s_cost);
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
  if (!map->fmap || map->C < 4 || (map->C % 4) != 0 || (map->cstride % 4) != 0 || map->cstride < map->C + 1 ||
      map->h < 2 || map->w < 2)
    return PXT_E_ARG;
  if (map->ndist != 0 && map->ndist != 2 && map->ndist != 4) return PXT_E_ARG;
  if (!bank->p3d || !bank->fref || bank->n_points < 1) return PXT_E_ARG;
  if (((uintptr_t)map->fmap % 16) != 0 || ((uintptr_t)bank->fref % 16) != 0 || ((uintptr_t)poses % 16) != 0 ||
      ((uintptr_t)ranges % 8) != 0 || ((uintptr_t)out % 16) != 0)
    return PXT_E_ARG;
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

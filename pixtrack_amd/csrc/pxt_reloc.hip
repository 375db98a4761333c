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
//
// pxt_score_pose_hypotheses_depth is the depth counterpart: the same poses, ranges and bank
// points, scored against the frame's SENSOR DEPTH image instead of a feature map.  A point of a hypothesis either lies
// on the sensed surface or it does not: per point one 12-byte read of the point, one byte of the mask and ONE 2-byte
// gather - no descriptors - so a whole placement grid (lateral position x distance per bank entry, relocalizer.py) is
// scored in one launch and only its best go on to the feature scorer above.  Per point n of hypothesis h (skipped
// where valid[n] == 0): p = transform_point(T_h, X_n), (u, v) = project_point(p) - the LM's projection - and the pixel
// (floor(u + 0.5), floor(v + 0.5)), pxt_points_visible's addressing (texel k's centre is at coordinate k); a point the
// projection refuses or whose pixel is outside the image counts nowhere.  Otherwise n_in counts it, raw = sensor[y][x],
// raw != 0 counts in n_measured, and with d = float(raw) * sensor_scale and r = d - p.z (each ONE fp32 operation, not
// contracted): |r| <= tolerance counts in n_agree (equality agrees), r > tolerance in n_behind (the sensor sees past
// the point: the object is not there); a NaN counts in neither.  out[h] = {n_in, n_measured, n_agree, n_behind}, a
// range outside the bank {-1, -1, -1, -1} without a read.
//
// Mapping: ONE WAVE per hypothesis, four hypotheses per workgroup of 256 threads; the lanes stride over the points,
// four points per lane and trip, so that four independent 2-byte gathers are in flight per lane (the kernel is bound by
// the latency of those gathers: a placement grid's hypotheses land all over the image).  The four counts are integers
// from ballot and population count, kept wave-uniform: no atomics, no LDS, and a hypothesis's four words depend on its
// own inputs only - not on M, its index, its neighbours in the workgroup or the run.  Lane 0 stores them as one 16-byte
// vector store.
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

constexpr int kDepthWaves = 4;                       // hypotheses per workgroup
constexpr int kDepthBlock = kDepthWaves * PXT_WAVE;
constexpr int kDepthFlight = 4;                      // points per lane and trip
constexpr int kDepthMaxHypotheses = 1 << 22;
constexpr long long kDepthMaxPixels = 1ll << 28;

struct RelocDepthParams {
  const float* p3d;
  const uint8_t* valid;
  const float* poses;      // [M][12]
  const int32_t* ranges;   // [M][2] {begin, count}
  const uint16_t* sensor;  // [H][W]
  int32_t* out;            // [M][4]
  int M, W, H, ndist, n_total;
  float sensor_scale, tolerance;
  float cam[10];
};

// r = raw * scale - pz as two fp32 operations: whatever the file's flags, the product is rounded before the difference.
__device__ __forceinline__ float depth_residual(unsigned raw, float scale, float pz) {
#pragma clang fp contract(off)
  const float d = (float)raw * scale;
  const float r = d - pz;
  return r;
}

__global__ __launch_bounds__(kDepthBlock) void reloc_depth_kernel(const RelocDepthParams P) {
  const int lane = threadIdx.x & (PXT_WAVE - 1);
  const int hyp = blockIdx.x * kDepthWaves + threadIdx.x / PXT_WAVE;  // wave-uniform
  if (hyp >= P.M) return;

  float c10[10];
  {  // (through the kernarg segment pointer: taking the address of the by-value argument would copy it to scratch)
    const float* c = vector_pointer(((const RelocDepthParams*)__builtin_amdgcn_kernarg_segment_ptr())->cam);
#pragma unroll
    for (int i = 0; i < 10; ++i) c10[i] = c[i];
  }
  const Cam cam = make_cam(c10, P.ndist);
  float T[12];
  load_pose12(vector_pointer(P.poses + (size_t)hyp * 12), T);
  const int2 rg = *(const int2*)vector_pointer(P.ranges + (size_t)hyp * 2);
  const int begin = rg.x, count = rg.y;
  int4* const out = (int4*)(P.out + (size_t)hyp * 4);
  // a range outside the bank is reported instead of read
  if (begin < 0 || count < 0 || (long long)begin + count > (long long)P.n_total) {
    if (lane == 0) *out = make_int4(-1, -1, -1, -1);
    return;
  }

  const int W = P.W, H = P.H;
  const float scale = P.sensor_scale, tol = P.tolerance;
  int n_in = 0, n_measured = 0, n_agree = 0, n_behind = 0;  // wave-uniform
  // without a mask the byte of the point's index is read from the points themselves (n < n_total <= their bytes) and
  // ignored: the load stays unconditional, so it is issued with the point's and not waited for on its own
  const uint8_t* const mask_bytes = P.valid ? P.valid : (const uint8_t*)P.p3d;
  const unsigned no_mask = P.valid ? 0u : 1u;

#pragma unroll 1
  for (int base = 0; base < count; base += PXT_WAVE * kDepthFlight) {
    // Three branch-free phases, each over the trip's four points: a wait for one point's loads is a wait for every load
    // issued before it (one in-order counter), so the loads of a phase are issued together and consumed together.  A
    // lane past the end of the range re-reads the range's last point and a point that is not in the image reads
    // sensor[0]; neither counts.
    bool in[kDepthFlight];
    float X[kDepthFlight], Y[kDepthFlight], Z[kDepthFlight], pz[kDepthFlight];
    unsigned mask[kDepthFlight], raw[kDepthFlight];
#pragma unroll
    for (int k = 0; k < kDepthFlight; ++k) {  // 1. the points and their mask bytes
      const int i = base + k * PXT_WAVE + lane;
      const size_t n = (size_t)begin + min(i, count - 1);
      X[k] = P.p3d[3 * n];
      Y[k] = P.p3d[3 * n + 1];
      Z[k] = P.p3d[3 * n + 2];
      mask[k] = mask_bytes[n] | no_mask;
      in[k] = i < count;
    }
#pragma unroll
    for (int k = 0; k < kDepthFlight; ++k) {  // 2. the projections; the four 2-byte gathers
      float px, py, u, v;
      transform_point(T, X[k], Y[k], Z[k], px, py, pz[k]);
      const bool projects = project_point(cam, px, py, pz[k], u, v, nullptr);
      const float xt = floorf(u + 0.5f), yt = floorf(v + 0.5f);  // the nearest texel: texel k's centre is at k
      const bool inside = (xt >= 0.f) & (yt >= 0.f) & (xt < (float)W) & (yt < (float)H);
      in[k] = in[k] & (mask[k] != 0u) & projects & inside;
      const size_t texel = in[k] ? (size_t)(int)yt * W + (int)xt : 0;
      raw[k] = P.sensor[texel];
    }
#pragma unroll
    for (int k = 0; k < kDepthFlight; ++k) {  // 3. the four counts
      const float r = depth_residual(raw[k], scale, pz[k]);
      n_in += __popcll(__ballot(in[k]));
      n_measured += __popcll(__ballot(in[k] & (raw[k] != 0u)));
      n_agree += __popcll(__ballot(in[k] & (fabsf(r) <= tol)));
      n_behind += __popcll(__ballot(in[k] & (r > tol)));
    }
  }
  if (lane == 0) *out = make_int4(n_in, n_measured, n_agree, n_behind);
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

extern "C" int pxt_score_pose_hypotheses_depth(const pxt_reloc_bank* bank, const float* poses, const int32_t* ranges,
                                               int32_t n_hypotheses, const uint16_t* sensor, int32_t width, int32_t height,
                                               float sensor_scale, float tolerance, const float* cam10_host, int32_t ndist,
                                               int32_t* out, void* stream) {
  if (!bank || !poses || !ranges || !sensor || !cam10_host || !out) return PXT_E_ARG;
  if (n_hypotheses < 1 || n_hypotheses > kDepthMaxHypotheses) return PXT_E_ARG;
  if (width < 1 || height < 1 || (long long)width * height > kDepthMaxPixels) return PXT_E_ARG;
  if (ndist != 0 && ndist != 2 && ndist != 4) return PXT_E_ARG;
  if (!bank->p3d || bank->n_points < 1 || ((uintptr_t)bank->p3d % 4) != 0) return PXT_E_ARG;
  if (((uintptr_t)poses % 16) != 0 || ((uintptr_t)ranges % 8) != 0 || ((uintptr_t)out % 16) != 0 ||
      ((uintptr_t)sensor % 2) != 0)
    return PXT_E_ARG;
  // the camera is the one the sensor image was taken with (as pxt_points_visible holds it to its plane)
  if (!(cam10_host[0] == (float)width && cam10_host[1] == (float)height)) return PXT_E_ARG;
  RelocDepthParams P;
  P.p3d = bank->p3d;
  P.valid = bank->valid;
  P.poses = poses;
  P.ranges = ranges;
  P.sensor = sensor;
  P.out = out;
  P.M = n_hypotheses;
  P.W = width;
  P.H = height;
  P.ndist = ndist;
  P.n_total = bank->n_points;
  P.sensor_scale = sensor_scale;
  P.tolerance = tolerance;
  for (int i = 0; i < 10; ++i) P.cam[i] = cam10_host[i];
  const unsigned grid = ((unsigned)n_hypotheses + kDepthWaves - 1) / kDepthWaves;
  hipLaunchKernelGGL(reloc_depth_kernel, dim3(grid), dim3(kDepthBlock), 0, (hipStream_t)stream, P);
  PXT_HIP_CHECK(hipGetLastError());
  return PXT_OK;
}

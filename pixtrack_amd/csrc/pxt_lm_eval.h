// The evaluation frame of the kernels that evaluate ONE LM iteration at a given pose without taking the step:
// pxt_lm_information (pxt_lm_info.hip: the 12-texel cross with gradients, 31 sums) and pxt_lm_point_report
// (pxt_lm_report.hip: 2 x 2 taps with the cost only, 8 sums and a record per point).  What a point's terms ARE is
// pxt_lm_point.h's; stated here, once, is everything around them.
//
// Mapping
//  * A point is owned by a lane GROUP as in the LM (4 consecutive channels per lane, dwordx4 texel reads: 32 lanes per
//    point for C > 32, 8 otherwise).  TWO points are in flight per group: both points' footprints are requested before
//    either is consumed (the scoring kernel's lesson, DESIGN.md 3.4: one point per group per trip left the memory pipe
//    idle behind every reduction).
//  * The points of ONE problem are dealt round-robin to the groups of n_wgs workgroups (blockIdx.x), the problems are
//    blockIdx.y.  n_wgs depends on the problem's n_points and C only (about four points per group, at most
//    kEvalMaxWgs), so a problem's summation order does not depend on what else is in the launch.
//  * Inside a workgroup the group leaders' sums are folded in a fixed order through LDS; across a problem's workgroups
//    the partials go to the workspace and the fold kernel (one wave per problem) adds them in workgroup order - the
//    kernel boundary orders the partials; no atomics anywhere.  The record's last word is stored last, with
//    system-scope release: a host may poll it in pinned memory.
//  * The parameter record of a problem (device workspace, or the kernel-argument segment for up to two problems), the
//    pose and the LM record's status words are read through vector loads (pointers made opaque VGPR values, as
//    pxt_reloc.hip does): the pose may have been written by the kernel just ahead in the stream.
//
// A parameter record type P (its size and field offsets are the kernel's own: they are in the generated code) names
// the common fields alike: p3d, mask, fmap, fref, pose, out, n, h, w, C, cs, ndist, pose_is_record, n_wgs, cam[10].
#pragma once

#include "pxt_common.h"
#include "pxt_lm_point.h"

#include <algorithm>

namespace pxt {

constexpr int kEvalBlock = 256;
constexpr int kEvalWaves = kEvalBlock / PXT_WAVE;
constexpr int kEvalMaxGroups = kEvalBlock / 8;  // groups per workgroup at 8 lanes per point
constexpr int kEvalMaxWgs = 128;                // workgroups per problem, at most
constexpr int kEvalPointsPerGroup = 4;          // target; more when n_wgs is capped
constexpr int kEvalArgProblems = 2;             // parameter records that travel as kernel arguments

template <typename P>
struct EvalArgs {
  P p[kEvalArgProblems];
};

struct EvalConf {
  int pad, loss, min_valid;
  float loss_alpha, loss_scale;
};

// ---- loads ----------------------------------------------------------------------------------------------------
// Reads at a scalar base (named as global memory: the pointer was rebuilt from two scalar halves) + 32-bit byte offset.
typedef const __attribute__((address_space(1))) char* EvalGlobal;
typedef float EvalVec4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 eval_texel(const float* base, unsigned byte_offset) {
  const EvalVec4 v = *(const __attribute__((address_space(1))) EvalVec4*)((EvalGlobal)base + byte_offset);
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ float eval_word(const float* base, unsigned byte_offset) {
  return *(const __attribute__((address_space(1))) float*)((EvalGlobal)base + byte_offset);
}

template <typename P>
__device__ __forceinline__ const P* eval_params(const P* ws_params, int from_args, int prob) {
  const P* base = from_args ? (const P*)__builtin_amdgcn_kernarg_segment_ptr() : ws_params;
  return vector_pointer(base + prob);
}

// -> false when the problem is skipped (its LM record reports failed / a status).
template <typename P>
__device__ inline bool eval_load_pose(const P* q, float* T) {
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

// ---- lane mapping -----------------------------------------------------------------------------------------------
// A lane's place in its workgroup and the problem's record in scalars, as locals of the kernel: N, W, H, C, cs, wide, LG
// (lanes per group), G (groups per workgroup), sub (the lane in its group), grp (the group in its workgroup), cam, p3d,
// mask, fmap, fref.  (A macro: as members of a struct the same reads leave the kernels' code elsewhere.)
#define PXT_EVAL_LANES(q)                                                                                              \
  const int N = uniform((q)->n), W = uniform((q)->w), H = uniform((q)->h), C = uniform((q)->C), cs = uniform((q)->cs); \
  const bool wide = C > 32;                                                                                            \
  const int LG = wide ? 32 : 8;                                                                                        \
  const int GPW = PXT_WAVE / LG, G = kEvalWaves * GPW; /* groups per wave / per workgroup */                           \
  const int lane = threadIdx.x & (PXT_WAVE - 1);                                                                       \
  const int sub = lane & (LG - 1);                                                                                     \
  const int grp = (threadIdx.x / PXT_WAVE) * GPW + lane / LG;                                                          \
  float c10[10];                                                                                                       \
  {                                                                                                                    \
    const float* c = (q)->cam;                                                                                         \
    _Pragma("unroll") for (int i = 0; i < 10; ++i) c10[i] = uniform(c[i]);                                             \
  }                                                                                                                    \
  const Cam cam = make_cam(c10, uniform((q)->ndist));                                                                  \
  const float* p3d = uniform((q)->p3d);                                                                                \
  const uint8_t* mask = uniform((q)->mask);                                                                            \
  const float* fmap = uniform((q)->fmap);                                                                              \
  const float* fref = uniform((q)->fref)

// ---- footprint ------------------------------------------------------------------------------------------------
// Where a point reads: TAPS columns / rows of the map starting at texel (ix0 + ORIGIN, iy0 + ORIGIN), (ix0, iy0) being
// the bilinear sample's first texel - 4 from -1 for the 12-texel cross, 2 from 0 for the 2 x 2 taps.
template <int TAPS, int ORIGIN>
struct EvalPoint {
  static constexpr int kTaps = TAPS, kOrigin = ORIGIN;
  int n;  // clamped into the bank: an invalid point's loads stay in bounds and are discarded
  float w00, w10, w01, w11;
  unsigned xo[TAPS], yo[TAPS];  // BYTE offsets of the columns / rows, clamped into the map (32-bit: one VGPR per address
                                // beside the map's scalar base; the entry point bounds the map's size)
  int xin, yin;                 // bit k: column / row k lies inside the map (outside counts as zero: grid_sample 'zeros')
  // 1.f where texel (row r, column c) lies inside the map, else 0.f
  __device__ __forceinline__ float in(int r, int c) const { return ((yin >> r) & (xin >> c) & 1) ? 1.f : 0.f; }
};

// Fills p's offsets and masks from the sample's first texel (ix0, iy0).  (A macro: as a function, member or free, the same
// loop leaves the information kernel's code elsewhere.)
#define PXT_EVAL_PLACE(p, ix0, iy0, W, H, cs)                               \
  do {                                                                      \
    (p).xin = (p).yin = 0;                                                  \
    _Pragma("unroll") for (int k = 0; k < (p).kTaps; ++k) {                 \
      const int xx = (ix0) + (p).kOrigin + k, yy = (iy0) + (p).kOrigin + k; \
      (p).xin |= (xx >= 0 && xx < (W)) ? 1 << k : 0;                        \
      (p).yin |= (yy >= 0 && yy < (H)) ? 1 << k : 0;                        \
      (p).xo[k] = (unsigned)(min(max(xx, 0), (W)-1) * (cs)) * 4u;           \
      (p).yo[k] = (unsigned)(min(max(yy, 0), (H)-1) * (W) * (cs)) * 4u;     \
    }                                                                       \
  } while (0)

// Declares wq, the confidence of p's sample - channel C at the sample's own 2 x 2 texels (one address for the whole
// group) - and wref, the reference's.  (A macro for the same reason.)
#define PXT_EVAL_CONFIDENCE(p, fmap, fref, C, cs)                                                   \
  const int c_ = -(p).kOrigin; /* the sample's first row / column among p's taps */                 \
  const unsigned cb = 4u * (unsigned)(C);                                                           \
  const float q11 = eval_word(fmap, (p).yo[c_] + (p).xo[c_] + cb) * (p).in(c_, c_);                 \
  const float q12 = eval_word(fmap, (p).yo[c_] + (p).xo[c_ + 1] + cb) * (p).in(c_, c_ + 1);         \
  const float q21 = eval_word(fmap, (p).yo[c_ + 1] + (p).xo[c_] + cb) * (p).in(c_ + 1, c_);         \
  const float q22 = eval_word(fmap, (p).yo[c_ + 1] + (p).xo[c_ + 1] + cb) * (p).in(c_ + 1, c_ + 1); \
  const float wq = (p).w00 * q11 + (p).w10 * q12 + (p).w01 * q21 + (p).w11 * q22;                   \
  const float wref = eval_word(fref, 4u * (unsigned)((p).n * (cs)) + cb)

// ---- folds ----------------------------------------------------------------------------------------------------
// The group leaders' sums -> LDS -> the workgroup's partial (ACC floats, WORDS of them meaningful), in a fixed order.
template <int ACC, int STRIDE, int WORDS>
__device__ __forceinline__ void eval_fold_groups(float* part, const float* acc, int sub, int grp, int G,
                                                 float* partials, int prob, int b) {
  if (sub == 0) {
#pragma unroll
    for (int k = 0; k < WORDS; ++k) part[grp * STRIDE + k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < ACC) {  // the groups' sums in a fixed order
    float v = 0.f;
    if (WORDS == ACC || threadIdx.x < WORDS)
      for (int g = 0; g < G; ++g) v += part[g * STRIDE + threadIdx.x];
    partials[((size_t)prob * kEvalMaxWgs + b) * ACC + threadIdx.x] = v;
  }
}

// The fold kernel, one wave per problem, is PXT_EVAL_FOLD_SUMS, thread 0 writing the record's words from rec and T (one
// thread, so that its release covers every word) and PXT_EVAL_FOLD_DONE.  This declares prob, q, out (the record), T
// (the pose) and rec (LDS: ACC floats, the workgroups' partials added in workgroup order); a skipped problem gets word
// LAST = -1 and the kernel returns.  (Macros: rec handed to a function, or the skip as a flag from one, moves one of
// the two fold kernels' code - whether rec[1] is read again behind the record's stores is decided by such things.)
#define PXT_EVAL_FOLD_SUMS(P, ACC, LAST, ws_params, from_args, partials)                                     \
  __shared__ float rec[ACC];                                                                                 \
  const int prob = blockIdx.x;                                                                               \
  const P* q = eval_params(ws_params, from_args, prob);                                                      \
  float* out = uniform(q->out);                                                                              \
  float T[12];                                                                                               \
  const bool run = eval_load_pose(q, T);                                                                     \
  if (!run) {                                                                                                \
    if (threadIdx.x == 0) __hip_atomic_store(&out[LAST], -1.f, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM); \
    return;                                                                                                  \
  }                                                                                                          \
  const int n_wgs = uniform(q->n_wgs);                                                                       \
  if (threadIdx.x < (ACC)) {                                                                                 \
    const float* p = (partials) + (size_t)prob * kEvalMaxWgs * (ACC) + threadIdx.x;                          \
    float v = 0.f;                                                                                           \
    for (int b = 0; b < n_wgs; ++b) v += p[(size_t)b * (ACC)];                                               \
    rec[threadIdx.x] = v;                                                                                    \
  }                                                                                                          \
  __syncthreads()

// Word LAST, stored last with system-scope release: 1 ok; -2 evaluated, but the LM would call it failed (rec[1]: n_valid).
#define PXT_EVAL_FOLD_DONE(LAST, cf)                             \
  const float ok = rec[1] >= (float)(cf).min_valid ? 1.f : -2.f; \
  __hip_atomic_store(&out[LAST], ok, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM)

// ---- host -----------------------------------------------------------------------------------------------------
inline int eval_workgroups(int n_points, int C) {
  const int groups = kEvalBlock / (C > 32 ? 32 : 8);
  const int per_wg = groups * kEvalPointsPerGroup;
  return std::max(1, std::min(kEvalMaxWgs, (n_points + per_wg - 1) / per_wg));
}

template <typename P>
size_t eval_params_bytes(int n_problems) {
  return ((size_t)n_problems * sizeof(P) + 255) / 256 * 256;
}

// The parameter records, then ACC floats per workgroup of every problem.
template <typename P, int ACC>
int64_t eval_workspace_bytes(int n_problems, int max_problems) {
  if (n_problems < 1 || n_problems > max_problems) return PXT_E_ARG;
  return (int64_t)(eval_params_bytes<P>(n_problems) + (size_t)n_problems * kEvalMaxWgs * ACC * sizeof(float));
}

// One launch of K problems: the checks both entry points make, the parameter records (kernel arguments for up to
// kEvalArgProblems problems, else a pinned staging slot copied to the workspace ahead of the launch) and the two
// kernels.  fill(k, rec) checks what is the entry point's own of problem k and sets its own fields of rec (zeroed, the
// common fields are set here); Problem names the common fields as pxt_lm_info_problem does.
template <typename P, int MAX_PROBLEMS, typename Problem, typename Fill, typename PointsKernel, typename FoldKernel>
int eval_launch(const Problem* problems, int n_problems, const pxt_lm_conf* conf, void* workspace, void* stream, Fill fill,
                PointsKernel points_kernel, FoldKernel fold_kernel) {
  if (!problems || !conf || !workspace) return PXT_E_ARG;
  if (n_problems < 1 || n_problems > MAX_PROBLEMS) return PXT_E_ARG;
  if (((uintptr_t)workspace % 16) != 0) return PXT_E_ARG;
  if (conf->pad < 0 || conf->loss < 0 || conf->loss > 2 || conf->min_valid < 0) return PXT_E_ARG;
  const EvalConf cf = {conf->pad, conf->loss, conf->min_valid, conf->loss_alpha, conf->loss_scale};
  const int K = n_problems;
  const bool from_args = K <= kEvalArgProblems;
  using Stage = StageRing<P, MAX_PROBLEMS>;
  EvalArgs<P> args = {};
  P* rec = args.p;
  typename Stage::Slot* slot = nullptr;
  if (!from_args) {
    static thread_local Stage stage;
    if (const int rc = stage.acquire(&slot)) return rc;
    rec = slot->host;
  }
  int max_wgs = 1;
  for (int k = 0; k < K; ++k) {
    const Problem& q = problems[k];
    const pxt_lm_level& l = q.level;
    if (!q.p3d || !q.pose || q.n_points < 1) return PXT_E_ARG;
    if (const int rc = check_level(l)) return rc;
    if (((uintptr_t)q.pose % 16) != 0) return PXT_E_ARG;
    // (byte offsets inside the map and the reference records are 32-bit in the kernel)
    if ((long long)l.h * l.w * l.cstride >= (1ll << 30) || (long long)q.n_points * l.cstride >= (1ll << 30)) return PXT_E_ARG;
    P& r = rec[k];
    r = P();
    if (const int rc = fill(k, r)) return rc;
    r.p3d = q.p3d;
    r.mask = q.point_mask;
    r.fmap = l.fmap;
    r.fref = l.fref;
    r.pose = q.pose;
    r.n = q.n_points;
    r.h = l.h; r.w = l.w; r.C = l.C; r.cs = l.cstride; r.ndist = l.ndist;
    r.pose_is_record = q.pose_is_lm_record != 0;
    r.n_wgs = eval_workgroups(q.n_points, l.C);
    for (int i = 0; i < 10; ++i) r.cam[i] = l.cam[i];
    max_wgs = std::max(max_wgs, r.n_wgs);
  }
  hipStream_t s = (hipStream_t)stream;
  const P* ws_params = (const P*)workspace;
  float* partials = (float*)((char*)workspace + eval_params_bytes<P>(K));
  if (!from_args) {
    PXT_HIP_CHECK(hipMemcpyAsync(workspace, slot->host, (size_t)K * sizeof(P), hipMemcpyHostToDevice, s));
    PXT_HIP_CHECK(hipEventRecord(slot->copied, s));
  }
  hipLaunchKernelGGL(points_kernel, dim3(max_wgs, K), dim3(kEvalBlock), 0, s, args, ws_params, partials, cf, (int)from_args);
  PXT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(fold_kernel, dim3(K), dim3(PXT_WAVE), 0, s, args, ws_params, (const float*)partials, cf, (int)from_args);
  PXT_HIP_CHECK(hipGetLastError());
  return PXT_OK;
}

}  // namespace pxt

// Mesh-free pose evaluation: the Depth renders of P (estimated, ground-truth) pose pairs compared pixel by pixel in one
// call (pxt_depth_agreement, include/pixtrack_hip.h; no reference counterpart).
//
// pxt_pose_errors (pxt_eval.hip) scores a run on model vertices; an object that exists only as an SfM model and a NeRF
// has none.  The renderer's own Depth image at the two poses gives the BOP benchmark's Visible Surface Discrepancy, the
// silhouette IoU and the mean depth error on the overlap instead (pixtrack_amd/render_evaluation.py turns the counts
// below into those figures).  This file is the comparison: an HBM streaming reduction, 2 x 16 B read per pixel.
//
// Arithmetic (all fp32; no multiplication stands next to an addition, so -ffp-contract=on has nothing to fuse)
//  * vis(v) = v.w >= min_alpha && v.x > 0 (pxt_points_from_depth's base test); q(v) = v.x / v.w, correctly rounded;
//    both = vis(e) && vis(g); dq = |q(e) - q(g)|; within_k = both && dq < tq[k] (strict; false for a NaN).
//  * The thresholds arrive divided by the depth-to-SfM-unit factor (the host rounds tau / z_scale once): no depth is
//    ever multiplied.  Slots k >= n_taus hold 0.0, which no |.| is below: their counts are 0 without a branch.
//  * A `both` pixel whose dq is NaN or inf counts in n_both, is within no threshold and is left out of sum and max.
//
// Mapping
//  * grid = (ceil(W H / 1024), P), 256 threads: a workgroup's share of a pair is 1024 consecutive pixels, four per
//    lane, all eight 16-byte loads of a lane issued before the first use (a wave's load covers 1 KiB contiguous).
//    Pixels past W H read nothing and are invisible.
//  * Predicates are counted per wave: ballot + population count, in scalar registers (19 counters: n_est, n_gt, n_both
//    and 16 thresholds; the loops over them are unrolled, so no counter is indexed at run time and nothing spills).
//  * The float sum and max: four pixels in order per lane, the wave butterfly (every lane ends with the same bits), the
//    four waves in wave order through LDS, one partial record (24 words, laid out like the output record) per
//    workgroup to workspace[pair][block], one lane per word.
//  * The fold kernel (one wave per pair): lane l adds blocks l, l + 64, ... in that order, then the butterfly, and
//    lane 0 writes the record.  A fixed order whatever P: a pair's record depends on its own two images and the
//    thresholds only.  (Not one lane over all blocks: 2^28 pixels are 262144 partials, and the tree keeps the
//    summation error at a few ulps.)  No atomics, two launches, no host synchronisation.
#include "pxt_common.h"

namespace pxt {
namespace {

constexpr int kDaBlock = 256;
constexpr int kDaWaves = kDaBlock / PXT_WAVE;
constexpr int kDaPix = 4;                          // pixels per lane
constexpr int kDaShare = kDaBlock * kDaPix;        // pixels per workgroup
constexpr int kDaTaus = PXT_DEPTH_AGREE_MAX_TAUS;
constexpr int kDaRec = PXT_DEPTH_AGREE_RECORD;     // words per partial and per record
constexpr int kDaMaxPairs = 65535;                 // gridDim.y
constexpr int64_t kDaMaxPixels = (int64_t)1 << 28;
static_assert(kDaRec == 8 + kDaTaus && kDaRec % 4 == 0, "record layout");

struct DaArgs {
  const float4* est;  // [P][H][W]: .x = composited depth * depth_scale, .w = alpha
  const float4* gt;
  int npix, n_blocks;
  float min_alpha;
  float tq[kDaTaus];  // slots >= n_taus: 0.0
  uint32_t* partials;  // [P][n_blocks][kDaRec]
};

__device__ __forceinline__ bool da_vis(const float4 v, float min_alpha) { return v.w >= min_alpha && v.x > 0.f; }
__device__ __forceinline__ uint32_t da_bits(float v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ float da_float(uint32_t v) { return __builtin_bit_cast(float, v); }
__device__ __forceinline__ uint32_t da_count(bool p) { return (uint32_t)__popcll(__ballot(p)); }

// word 4 is a float sum, word 5 a float max, every other word an integer count
__device__ __forceinline__ uint32_t da_combine(int word, uint32_t a, uint32_t b) {
  if (word == 4) return da_bits(da_float(a) + da_float(b));
  if (word == 5) return da_bits(fmaxf(da_float(a), da_float(b)));
  return a + b;
}

__global__ __launch_bounds__(kDaBlock) void depth_agreement_kernel(const DaArgs a) {
  __shared__ uint32_t red[kDaWaves][kDaRec];
  const int pair = blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
  const size_t base = (size_t)pair * (size_t)a.npix;
  float4 e[kDaPix], g[kDaPix];
#pragma unroll
  for (int j = 0; j < kDaPix; ++j) {
    const int i = b * kDaShare + j * kDaBlock + tid;
    e[j] = g[j] = make_float4(0.f, 0.f, 0.f, 0.f);  // invisible
    if (i < a.npix) {
      e[j] = a.est[base + i];
      g[j] = a.gt[base + i];
    }
  }
  // .y and .z count as used, behind the last load: one 128-bit load per pixel and image (not two 32-bit loads 12 bytes
  // apart), all eight in flight together
#pragma unroll
  for (int j = 0; j < kDaPix; ++j) asm volatile("" : : "v"(e[j].y), "v"(e[j].z), "v"(g[j].y), "v"(g[j].z));
  uint32_t n_est = 0, n_gt = 0, n_both = 0, within[kDaTaus];
#pragma unroll
  for (int k = 0; k < kDaTaus; ++k) within[k] = 0;
  float sum = 0.f, mx = 0.f;
#pragma unroll
  for (int j = 0; j < kDaPix; ++j) {
    const bool ve = da_vis(e[j], a.min_alpha), vg = da_vis(g[j], a.min_alpha), both = ve && vg;
    n_est += da_count(ve);
    n_gt += da_count(vg);
    n_both += da_count(both);
    const float qe = e[j].x / e[j].w, qg = g[j].x / g[j].w;
    const float dq = both ? fabsf(qe - qg) : __builtin_nanf("");  // a NaN is below no threshold
    const bool finite = dq <= 3.402823466e+38f;                   // false for NaN and inf
    sum += finite ? dq : 0.f;
    mx = finite ? fmaxf(mx, dq) : mx;
#pragma unroll
    for (int k = 0; k < kDaTaus; ++k) within[k] += da_count(dq < a.tq[k]);
  }
#pragma unroll
  for (int m = 1; m < PXT_WAVE; m <<= 1) {
    sum += __shfl_xor(sum, m, PXT_WAVE);
    mx = fmaxf(mx, __shfl_xor(mx, m, PXT_WAVE));
  }
  if ((tid & (PXT_WAVE - 1)) == 0) {
    uint32_t* r = red[tid / PXT_WAVE];
    r[0] = n_est; r[1] = n_gt; r[2] = n_both; r[3] = 0;
    r[4] = da_bits(sum); r[5] = da_bits(mx); r[6] = 0; r[7] = 0;
#pragma unroll
    for (int k = 0; k < kDaTaus; ++k) r[8 + k] = within[k];
  }
  __syncthreads();
  if (tid < kDaRec) {
    uint32_t v = red[0][tid];
    for (int w = 1; w < kDaWaves; ++w) v = da_combine(tid, v, red[w][tid]);
    a.partials[((size_t)pair * a.n_blocks + b) * kDaRec + tid] = v;
  }
}

// One wave per pair: lane l folds blocks l, l + 64, ... in order, the butterfly folds the lanes, lane 0 writes.
__global__ __launch_bounds__(PXT_WAVE) void depth_agreement_fold_kernel(const uint32_t* __restrict__ partials,
                                                                        const int n_blocks, const int n_taus,
                                                                        uint32_t* __restrict__ records) {
  const int pair = blockIdx.x, lane = threadIdx.x;
  const uint4* p = (const uint4*)(partials + (size_t)pair * n_blocks * kDaRec);
  uint32_t v[kDaRec];
#pragma unroll
  for (int w = 0; w < kDaRec; ++w) v[w] = 0;  // (+0.0 for the sum and the max)
#pragma unroll 1
  for (int b = lane; b < n_blocks; b += PXT_WAVE) {
#pragma unroll
    for (int c = 0; c < kDaRec / 4; ++c) {
      const uint4 t = p[(size_t)b * (kDaRec / 4) + c];
      v[4 * c + 0] = da_combine(4 * c + 0, v[4 * c + 0], t.x);
      v[4 * c + 1] = da_combine(4 * c + 1, v[4 * c + 1], t.y);
      v[4 * c + 2] = da_combine(4 * c + 2, v[4 * c + 2], t.z);
      v[4 * c + 3] = da_combine(4 * c + 3, v[4 * c + 3], t.w);
    }
  }
#pragma unroll
  for (int m = 1; m < PXT_WAVE; m <<= 1) {
#pragma unroll
    for (int w = 0; w < kDaRec; ++w) v[w] = da_combine(w, v[w], (uint32_t)__shfl_xor((int)v[w], m, PXT_WAVE));
  }
  if (lane == 0) {
    uint32_t* rec = records + (size_t)pair * kDaRec;
    v[3] = v[0] + v[1] - v[2];
    v[6] = (uint32_t)n_taus;
    v[7] = 1u;
#pragma unroll
    for (int w = 0; w < kDaRec; ++w) rec[w] = v[w];
  }
}

bool da_sizes_ok(int n_pairs, int width, int height) {
  return n_pairs >= 1 && n_pairs <= kDaMaxPairs && width >= 1 && height >= 1 && (int64_t)width * height <= kDaMaxPixels;
}
int da_blocks(int width, int height) { return (int)(((int64_t)width * height + kDaShare - 1) / kDaShare); }

}  // namespace
}  // namespace pxt

using namespace pxt;

extern "C" int64_t pxt_depth_agreement_workspace_bytes(int32_t n_pairs, int32_t width, int32_t height) {
  if (!da_sizes_ok(n_pairs, width, height)) return PXT_E_ARG;
  return (int64_t)n_pairs * da_blocks(width, height) * kDaRec * (int64_t)sizeof(uint32_t);
}

extern "C" int pxt_depth_agreement(const float* depth_est, const float* depth_gt, int32_t n_pairs, int32_t width,
                                   int32_t height, float min_alpha, const float* tq_host, int32_t n_taus,
                                   uint32_t* records, void* workspace, void* stream) {
  if (!depth_est || !depth_gt || !tq_host || !records || !workspace) return PXT_E_ARG;
  if (!da_sizes_ok(n_pairs, width, height) || n_taus < 1 || n_taus > kDaTaus) return PXT_E_ARG;
  if (((uintptr_t)depth_est % 16) != 0 || ((uintptr_t)depth_gt % 16) != 0 || ((uintptr_t)records % 4) != 0 ||
      ((uintptr_t)workspace % 16) != 0)
    return PXT_E_ARG;
  DaArgs a;
  a.est = (const float4*)depth_est;
  a.gt = (const float4*)depth_gt;
  a.npix = width * height;
  a.n_blocks = da_blocks(width, height);
  a.min_alpha = min_alpha;
  for (int k = 0; k < kDaTaus; ++k) a.tq[k] = k < n_taus ? tq_host[k] : 0.f;
  a.partials = (uint32_t*)workspace;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(depth_agreement_kernel, dim3(a.n_blocks, n_pairs), dim3(kDaBlock), 0, s, a);
  PXT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(depth_agreement_fold_kernel, dim3(n_pairs), dim3(PXT_WAVE), 0, s, (const uint32_t*)a.partials,
                     a.n_blocks, (int)n_taus, records);
  PXT_HIP_CHECK(hipGetLastError());
  return PXT_OK;
}

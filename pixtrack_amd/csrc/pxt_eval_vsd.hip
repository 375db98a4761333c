// BOP's sensor-depth Visible Surface Discrepancy: the Depth renders of P (estimated, ground-truth) pose pairs compared
// with each other AND with the frame's sensor depth image, pixel by pixel, in one call (pxt_sensor_vsd,
// include/pixtrack_hip.h; no reference counterpart).
//
// pxt_depth_agreement (pxt_eval_render.hip) takes the two render silhouettes as the visibility masks.  With the 16-bit
// depth image a data set such as YCB-Video keeps beside every colour frame, the masks are BOP's (Hodan et al., ECCV
// 2018 / BOP 2019, visib_mode = bop19): a pixel an occluder hides counts neither for nor against the estimate, and the
// visible fraction of the object falls out of the same counts (pixtrack_amd/sensor_evaluation.py makes the figures).
// This file is the comparison: an HBM streaming reduction, 2 x 16 B + 2 B read per pixel (+ 4 B of a shared, cache-
// resident ray plane).
//
// Arithmetic (all fp32).  Every product and difference is rounded on its own: they go through __fmul_rn / __fsub_rn,
// each a single IEEE operation that -ffp-contract=on cannot fuse with its neighbour (the file needs no flag of its own).
//  * sil(v) = v.w >= min_alpha && v.x > 0; q(v) = v.x / v.w (pxt_depth_agreement's reading).
//  * r = ray[y][x] (1.0f without a plane); d_e = q(e) * r; d_g = q(g) * r; d_s = (float(raw) * sensor_q) * r, raw the
//    sensor count at (x + shift_x, y + shift_y), 0 when that position is outside the image.
//  * vis(d, sil) = sil && (d - d_s <= delta_q || raw == 0); vis_g = vis(d_g, sil(g));
//    vis_e = vis(d_e, sil(e)) || (vis_g && sil(e)); inter = vis_g && vis_e; dd = |d_e - d_g|;
//    within_k = inter && dd < tq[k] (strict; false for a NaN).  Slots k >= n_taus hold 0.0, which no |.| is below.
//  * An `inter` pixel whose dd is NaN or inf counts in n_inter, is within no threshold and is left out of sum and max.
//
// Mapping (depth_agreement_kernel's)
//  * grid = (ceil(W H / 1024), P), 256 threads: a workgroup's share of a pair is 1024 consecutive pixels, four per
//    lane; the eight 16-byte loads, the four 2-byte sensor loads and the four ray loads of a lane are all issued before
//    the first use.  A wave's sensor load covers 128 contiguous bytes.  Pixels past W H read nothing and are invisible.
//  * The shift: the sensor position of every pixel is tested against [0, W) x [0, H) before its load, so no address
//    leaves the pair's own H x W counts - a shifted row neither reads the next row's start nor the next pair.  Without
//    a shift (the block-uniform common case) the sensor index is the pixel index and no division is done.
//  * Predicates are counted per wave: ballot + population count, in scalar registers (22 counters, loops unrolled).
//  * The float sum and max: four pixels in order per lane, the wave butterfly, the four waves in wave order through LDS,
//    one partial record (32 words, laid out like the output record) per workgroup to workspace[pair][block].
//  * The fold kernel (one wave per pair): lane l adds blocks l, l + 64, ... in that order, then the butterfly, and lane
//    0 writes the record.  A fixed order whatever P: a pair's record depends on its own three images, the ray plane,
//    the shift and the scalars only.  No atomics, two launches, no host synchronisation.
#include "pxt_common.h"

namespace pxt {
namespace {

constexpr int kSvBlock = 256;
constexpr int kSvWaves = kSvBlock / PXT_WAVE;
constexpr int kSvPix = 4;                          // pixels per lane
constexpr int kSvShare = kSvBlock * kSvPix;        // pixels per workgroup
constexpr int kSvTaus = PXT_SENSOR_VSD_MAX_TAUS;
constexpr int kSvRec = PXT_SENSOR_VSD_RECORD;      // words per partial and per record
constexpr int kSvMaxPairs = 65535;                 // gridDim.y
constexpr int64_t kSvMaxPixels = (int64_t)1 << 28;
constexpr int kSvMaxShift = 32767;
static_assert(kSvRec == 16 + kSvTaus && kSvRec % 4 == 0 && kSvRec <= kSvBlock, "record layout");

struct SvArgs {
  const float4* est;  // [P][H][W]: .x = composited depth * depth_scale, .w = alpha
  const float4* gt;
  const uint16_t* sensor;  // [P][H][W]
  const float* ray;        // [H][W] or nullptr
  int npix, n_blocks, width, height, shift_x, shift_y;
  float min_alpha, sensor_q, delta_q;
  float tq[kSvTaus];   // slots >= n_taus: 0.0
  uint32_t* partials;  // [P][n_blocks][kSvRec]
};

__device__ __forceinline__ bool sv_sil(const float4 v, float min_alpha) { return v.w >= min_alpha && v.x > 0.f; }
__device__ __forceinline__ uint32_t sv_bits(float v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ float sv_float(uint32_t v) { return __builtin_bit_cast(float, v); }
__device__ __forceinline__ uint32_t sv_count(bool p) { return (uint32_t)__popcll(__ballot(p)); }

// word 4 is a float sum, word 5 a float max, every other word an integer count
__device__ __forceinline__ uint32_t sv_combine(int word, uint32_t a, uint32_t b) {
  if (word == 4) return sv_bits(sv_float(a) + sv_float(b));
  if (word == 5) return sv_bits(fmaxf(sv_float(a), sv_float(b)));
  return a + b;
}

__global__ __launch_bounds__(kSvBlock) void sensor_vsd_kernel(const SvArgs a) {
  __shared__ uint32_t red[kSvWaves][kSvRec];
  const int pair = blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
  const size_t base = (size_t)pair * (size_t)a.npix;
  const bool shifted = (a.shift_x | a.shift_y) != 0;  // uniform
  float4 e[kSvPix], g[kSvPix];
  float r[kSvPix];
  uint32_t raw[kSvPix];
  // the sensor position of every pixel first (integer division only with a shift), then all sixteen loads
  int si[kSvPix];  // index into the pair's own H x W counts, or -1: nothing is read
#pragma unroll
  for (int j = 0; j < kSvPix; ++j) {
    const int i = b * kSvShare + j * kSvBlock + tid;
    si[j] = i < a.npix ? i : -1;
    if (shifted && i < a.npix) {
      const int y = i / a.width, x = i - y * a.width;
      const int xs = x + a.shift_x, ys = y + a.shift_y;
      si[j] = (xs >= 0 && xs < a.width && ys >= 0 && ys < a.height) ? ys * a.width + xs : -1;
    }
  }
#pragma unroll
  for (int j = 0; j < kSvPix; ++j) {
    const int i = b * kSvShare + j * kSvBlock + tid;
    e[j] = g[j] = make_float4(0.f, 0.f, 0.f, 0.f);  // invisible
    r[j] = 1.f;
    raw[j] = 0;
    if (i < a.npix) {
      e[j] = a.est[base + i];
      g[j] = a.gt[base + i];
      if (a.ray) r[j] = a.ray[i];
    }
    if (si[j] >= 0) raw[j] = a.sensor[base + si[j]];
  }
  // .y and .z count as used, behind the last load: one 128-bit load per pixel and image, all in flight together
#pragma unroll
  for (int j = 0; j < kSvPix; ++j) asm volatile("" : : "v"(e[j].y), "v"(e[j].z), "v"(g[j].y), "v"(g[j].z));
  uint32_t n_ve = 0, n_vg = 0, n_inter = 0, n_se = 0, n_sg = 0, n_meas = 0, within[kSvTaus];
#pragma unroll
  for (int k = 0; k < kSvTaus; ++k) within[k] = 0;
  float sum = 0.f, mx = 0.f;
#pragma unroll
  for (int j = 0; j < kSvPix; ++j) {
    const bool se = sv_sil(e[j], a.min_alpha), sg = sv_sil(g[j], a.min_alpha), none = raw[j] == 0;
    const float de = __fmul_rn(e[j].x / e[j].w, r[j]), dg = __fmul_rn(g[j].x / g[j].w, r[j]);
    const float ds = __fmul_rn(__fmul_rn((float)raw[j], a.sensor_q), r[j]);
    const bool vg = sg && (__fsub_rn(dg, ds) <= a.delta_q || none);
    const bool ve = se && (__fsub_rn(de, ds) <= a.delta_q || none || vg);
    const bool inter = vg && ve;
    n_se += sv_count(se);
    n_sg += sv_count(sg);
    n_meas += sv_count(!none);
    n_ve += sv_count(ve);
    n_vg += sv_count(vg);
    n_inter += sv_count(inter);
    const float dd = inter ? fabsf(__fsub_rn(de, dg)) : __builtin_nanf("");  // a NaN is below no threshold
    const bool finite = dd <= 3.402823466e+38f;                              // false for NaN and inf
    sum += finite ? dd : 0.f;
    mx = finite ? fmaxf(mx, dd) : mx;
#pragma unroll
    for (int k = 0; k < kSvTaus; ++k) within[k] += sv_count(dd < a.tq[k]);
  }
#pragma unroll
  for (int m = 1; m < PXT_WAVE; m <<= 1) {
    sum += __shfl_xor(sum, m, PXT_WAVE);
    mx = fmaxf(mx, __shfl_xor(mx, m, PXT_WAVE));
  }
  if ((tid & (PXT_WAVE - 1)) == 0) {
    uint32_t* w = red[tid / PXT_WAVE];
    w[0] = n_ve; w[1] = n_vg; w[2] = n_inter; w[3] = 0;
    w[4] = sv_bits(sum); w[5] = sv_bits(mx); w[6] = 0; w[7] = 0;
    w[8] = n_se; w[9] = n_sg; w[10] = n_meas;
#pragma unroll
    for (int k = 11; k < 16; ++k) w[k] = 0;
#pragma unroll
    for (int k = 0; k < kSvTaus; ++k) w[16 + k] = within[k];
  }
  __syncthreads();
  if (tid < kSvRec) {
    uint32_t v = red[0][tid];
    for (int w = 1; w < kSvWaves; ++w) v = sv_combine(tid, v, red[w][tid]);
    a.partials[((size_t)pair * a.n_blocks + b) * kSvRec + tid] = v;
  }
}

// One wave per pair: lane l folds blocks l, l + 64, ... in order, the butterfly folds the lanes, lane 0 writes.
__global__ __launch_bounds__(PXT_WAVE) void sensor_vsd_fold_kernel(const uint32_t* __restrict__ partials,
                                                                   const int n_blocks, const int n_taus,
                                                                   uint32_t* __restrict__ records) {
  const int pair = blockIdx.x, lane = threadIdx.x;
  const uint4* p = (const uint4*)(partials + (size_t)pair * n_blocks * kSvRec);
  uint32_t v[kSvRec];
#pragma unroll
  for (int w = 0; w < kSvRec; ++w) v[w] = 0;  // (+0.0 for the sum and the max)
#pragma unroll 1
  for (int b = lane; b < n_blocks; b += PXT_WAVE) {
#pragma unroll
    for (int c = 0; c < kSvRec / 4; ++c) {
      const uint4 t = p[(size_t)b * (kSvRec / 4) + c];
      v[4 * c + 0] = sv_combine(4 * c + 0, v[4 * c + 0], t.x);
      v[4 * c + 1] = sv_combine(4 * c + 1, v[4 * c + 1], t.y);
      v[4 * c + 2] = sv_combine(4 * c + 2, v[4 * c + 2], t.z);
      v[4 * c + 3] = sv_combine(4 * c + 3, v[4 * c + 3], t.w);
    }
  }
#pragma unroll
  for (int m = 1; m < PXT_WAVE; m <<= 1) {
#pragma unroll
    for (int w = 0; w < kSvRec; ++w) v[w] = sv_combine(w, v[w], (uint32_t)__shfl_xor((int)v[w], m, PXT_WAVE));
  }
  if (lane == 0) {
    uint32_t* rec = records + (size_t)pair * kSvRec;
    v[3] = v[0] + v[1] - v[2];
    v[6] = (uint32_t)n_taus;
    v[7] = 1u;
#pragma unroll
    for (int w = 0; w < kSvRec; ++w) rec[w] = v[w];
  }
}

bool sv_sizes_ok(int n_pairs, int width, int height) {
  return n_pairs >= 1 && n_pairs <= kSvMaxPairs && width >= 1 && height >= 1 && (int64_t)width * height <= kSvMaxPixels;
}
int sv_blocks(int width, int height) { return (int)(((int64_t)width * height + kSvShare - 1) / kSvShare); }

}  // namespace
}  // namespace pxt

using namespace pxt;

extern "C" int64_t pxt_sensor_vsd_workspace_bytes(int32_t n_pairs, int32_t width, int32_t height) {
  if (!sv_sizes_ok(n_pairs, width, height)) return PXT_E_ARG;
  return (int64_t)n_pairs * sv_blocks(width, height) * kSvRec * (int64_t)sizeof(uint32_t);
}

extern "C" int pxt_sensor_vsd(const float* depth_est, const float* depth_gt, const uint16_t* sensor, const float* ray,
                              int32_t n_pairs, int32_t width, int32_t height, int32_t shift_x, int32_t shift_y,
                              float min_alpha, float sensor_q, float delta_q, const float* tq_host, int32_t n_taus,
                              uint32_t* records, void* workspace, void* stream) {
  if (!depth_est || !depth_gt || !sensor || !tq_host || !records || !workspace) return PXT_E_ARG;
  if (!sv_sizes_ok(n_pairs, width, height) || n_taus < 1 || n_taus > kSvTaus) return PXT_E_ARG;
  if (shift_x < -kSvMaxShift || shift_x > kSvMaxShift || shift_y < -kSvMaxShift || shift_y > kSvMaxShift) return PXT_E_ARG;
  if (((uintptr_t)depth_est % 16) != 0 || ((uintptr_t)depth_gt % 16) != 0 || ((uintptr_t)sensor % 2) != 0 ||
      ((uintptr_t)ray % 4) != 0 || ((uintptr_t)records % 4) != 0 || ((uintptr_t)workspace % 16) != 0)
    return PXT_E_ARG;
  SvArgs a;
  a.est = (const float4*)depth_est;
  a.gt = (const float4*)depth_gt;
  a.sensor = sensor;
  a.ray = ray;
  a.npix = width * height;
  a.n_blocks = sv_blocks(width, height);
  a.width = width;
  a.height = height;
  a.shift_x = shift_x;
  a.shift_y = shift_y;
  a.min_alpha = min_alpha;
  a.sensor_q = sensor_q;
  a.delta_q = delta_q;
  for (int k = 0; k < kSvTaus; ++k) a.tq[k] = k < n_taus ? tq_host[k] : 0.f;
  a.partials = (uint32_t*)workspace;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sensor_vsd_kernel, dim3(a.n_blocks, n_pairs), dim3(kSvBlock), 0, s, a);
  PXT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(sensor_vsd_fold_kernel, dim3(n_pairs), dim3(PXT_WAVE), 0, s, (const uint32_t*)a.partials,
                     a.n_blocks, (int)n_taus, records);
  PXT_HIP_CHECK(hipGetLastError());
  return PXT_OK;
}

// Reference points back-projected from a Depth render (pxt_points_from_depth; no reference counterpart).
//
// The reference refines a frame on the SfM points of the nearest mapping image (pixloc_pose_refiners.py:282-290).  This
// file makes a point set from the frame's own Depth render instead: a lattice of the pixels that are safely inside the
// silhouette, back-projected along the renderer's own rays (make_ray, pxt_ngp.hip) into SfM object coordinates.
//
// It is an HBM streaming pass (16 B per pixel read once, the eroded neighbours out of L1 / L2, <= n_max pixels read
// again) in three launches on one stream:
//   accept   one lane per pixel, dwordx4 loads: base test + erosion -> one 64-bit ballot word per 64 pixels and the
//            number of accepted pixels per workgroup segment
//   stride   every workgroup sums the segment counts (integers: the sum does not depend on the order), derives the
//            lattice stride s from it and counts its own segment's lattice candidates
//   compact  a workgroup's first output slot = the candidates of all segments before it; inside the segment the ballot
//            words and a lane prefix give each candidate its slot.  Slots follow the pixels' row-major order and no
//            atomic decides an index, so the output is a pure function of the input.
#include "pxt_common.h"

#include <cmath>

namespace pxt {

constexpr int kPtsSeg = 1024;             // pixels per workgroup: 256 lanes x 4 trips
constexpr int kPtsTrips = kPtsSeg / 256;  // one ballot word per wave and trip
constexpr int kPtsWords = kPtsSeg / 64;
constexpr int kPtsHead = 16;              // ints in front of the segment counts: [0] A, [1] s

struct PtsArgs {
  const float4* depth;  // [H][W]: .x = composited depth * depth_scale, .w = alpha
  int W, H, npix, nseg, erode, n_max;
  float min_alpha;
  int* head;                 // [kPtsHead]
  int* seg_accepted;         // [nseg]
  int* seg_candidates;       // [nseg]
  unsigned long long* bits;  // [nseg * kPtsWords]: bit i % 64 of word i / 64 = pixel i accepted
};

struct PtsProjection {
  float M[9], b[3];  // p = b + z * M (dxn, dyn, 1)^T
  float focal, depth_scale;
};

__device__ __forceinline__ bool pts_base_test(const float4 v, float min_alpha) { return v.w >= min_alpha && v.x > 0.f; }

// Sum of `v` over the workgroup's 256 lanes, returned to all of them.
__device__ inline int pts_block_sum(int v, int* s4) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, PXT_WAVE);
  __syncthreads();  // (s4 may still be read from the previous sum)
  if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s4[0] + s4[1]) + (s4[2] + s4[3]);
}

// The smallest s >= 1 with s * s * n_max >= A, in integer arithmetic (the float square root only picks the start).
__device__ inline int pts_stride(int A, int n_max) {
  int s = (int)sqrtf((float)A / (float)n_max);
  if (s < 1) s = 1;
  while (s > 1 && (long long)(s - 1) * (s - 1) * n_max >= (long long)A) --s;
  while ((long long)s * s * n_max < (long long)A) ++s;
  return s;
}

// Ballot of the wave's 64 pixels of trip j that are accepted and lie on the lattice x % s == s / 2, y % s == s / 2.
__device__ __forceinline__ unsigned long long pts_candidate_word(const PtsArgs& a, int s, int j, int& x, int& y) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * kPtsSeg + j * 256 + threadIdx.x;
  const unsigned long long w = a.bits[blockIdx.x * kPtsWords + j * 4 + wave];  // (bits of pixels >= npix are 0)
  y = i / a.W;
  x = i - y * a.W;
  const bool cand = ((w >> lane) & 1ull) != 0ull && (x % s) == s / 2 && (y % s) == s / 2;
  return __ballot(cand);
}

__global__ __launch_bounds__(256) void points_accept_kernel(const PtsArgs a) {
  __shared__ int s_cnt[kPtsWords];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int e = a.erode;
#pragma unroll
  for (int j = 0; j < kPtsTrips; ++j) {
    const int i = blockIdx.x * kPtsSeg + j * 256 + threadIdx.x;
    bool ok = false;
    if (i < a.npix) {
      ok = pts_base_test(a.depth[i], a.min_alpha);
      const int y = i / a.W, x = i - y * a.W;
      // the (2e + 1)^2 square: one that leaves the image fails; every pixel of it passes the base test
      if (ok && e > 0 && (x < e || y < e || x + e >= a.W || y + e >= a.H)) ok = false;
      if (ok && e > 0) {
        for (int dy = -e; dy <= e; ++dy)
          for (int dx = -e; dx <= e; ++dx)
            if ((dx != 0 || dy != 0) && ok) ok = pts_base_test(a.depth[i + dy * a.W + dx], a.min_alpha);
      }
    }
    const unsigned long long m = __ballot(ok);
    if (lane == 0) {
      a.bits[blockIdx.x * kPtsWords + j * 4 + wave] = m;
      s_cnt[j * 4 + wave] = __popcll(m);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = 0;
    for (int k = 0; k < kPtsWords; ++k) c += s_cnt[k];
    a.seg_accepted[blockIdx.x] = c;
  }
}

__global__ __launch_bounds__(256) void points_stride_kernel(const PtsArgs a) {
  __shared__ int s4[4];
  int part = 0;
  for (int b = threadIdx.x; b < a.nseg; b += 256) part += a.seg_accepted[b];
  const int A = pts_block_sum(part, s4);
  const int s = pts_stride(A, a.n_max);
  int c = 0, x, y;
#pragma unroll
  for (int j = 0; j < kPtsTrips; ++j) c += __popcll(pts_candidate_word(a, s, j, x, y));
  c = pts_block_sum((threadIdx.x & 63) == 0 ? c : 0, s4);
  if (threadIdx.x == 0) {
    a.seg_candidates[blockIdx.x] = c;
    if (blockIdx.x == 0) {
      a.head[0] = A;
      a.head[1] = s;
    }
  }
}

__global__ __launch_bounds__(256) void points_compact_kernel(const PtsArgs a, const PtsProjection pj, float* __restrict__ p3d,
                                                             uint8_t* __restrict__ slot_valid, int* __restrict__ record) {
  __shared__ int s4[4];
  __shared__ int s_cnt[kPtsWords];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int A = a.head[0], s = a.head[1];
  int before = 0, all = 0;
  for (int b = threadIdx.x; b < a.nseg; b += 256) {
    const int c = a.seg_candidates[b];
    all += c;
    if (b < (int)blockIdx.x) before += c;
  }
  before = pts_block_sum(before, s4);
  all = pts_block_sum(all, s4);
  unsigned long long m[kPtsTrips];
  int xs[kPtsTrips], ys[kPtsTrips];
#pragma unroll
  for (int j = 0; j < kPtsTrips; ++j) {
    m[j] = pts_candidate_word(a, s, j, xs[j], ys[j]);
    if (lane == 0) s_cnt[j * 4 + wave] = __popcll(m[j]);
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kPtsTrips; ++j) {
    if (((m[j] >> lane) & 1ull) == 0ull) continue;
    int slot = before;  // the segment's words come in pixel order: trip-major, then wave
    for (int k = 0; k < j * 4 + wave; ++k) slot += s_cnt[k];
    slot += __popcll(m[j] & ((1ull << lane) - 1ull));
    if (slot >= a.n_max) continue;  // the tail is cut (record[3] > n_max tells)
    const float4 v = a.depth[blockIdx.x * kPtsSeg + j * 256 + threadIdx.x];
    const float z = v.x / (v.w * pj.depth_scale);
    const float dxn = ((float)xs[j] + 0.5f - 0.5f * (float)a.W) / pj.focal;
    const float dyn = ((float)ys[j] + 0.5f - 0.5f * (float)a.H) / pj.focal;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      p3d[3 * (size_t)slot + c] = pj.b[c] + z * (pj.M[3 * c] * dxn + pj.M[3 * c + 1] * dyn + pj.M[3 * c + 2]);
    slot_valid[slot] = 1;
  }
  // unused slots: the camera centre, which the sampler rejects at the reference pose (z > kCamEps fails)
  const int n_points = min(all, a.n_max);
  for (int slot = n_points + blockIdx.x * 256 + threadIdx.x; slot < a.n_max; slot += gridDim.x * 256) {
    p3d[3 * (size_t)slot + 0] = pj.b[0];
    p3d[3 * (size_t)slot + 1] = pj.b[1];
    p3d[3 * (size_t)slot + 2] = pj.b[2];
    slot_valid[slot] = 0;
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
    record[0] = A;
    record[1] = s;
    record[2] = n_points;
    record[3] = all;
  }
}

static inline int64_t pts_round64(int64_t v) { return (v + 63) / 64 * 64; }
static inline bool pts_size_ok(int w, int h) { return w >= 1 && h >= 1 && w <= 16384 && h <= 16384; }

}  // namespace pxt

using namespace pxt;

extern "C" int64_t pxt_points_from_depth_workspace_bytes(int32_t width, int32_t height) {
  if (!pts_size_ok(width, height)) return -1;
  const int64_t nseg = ((int64_t)width * height + kPtsSeg - 1) / kPtsSeg;
  return pts_round64(kPtsHead * 4) + pts_round64(2 * nseg * 4) + nseg * kPtsWords * 8;
}

extern "C" int pxt_points_from_depth(const float* depth, int32_t width, int32_t height, const float* xform_host, float focal,
                                     float depth_scale, float min_alpha, int32_t erode, int32_t n_max, float* p3d,
                                     uint8_t* slot_valid, int32_t* record, void* workspace, void* stream) {
  if (!depth || !xform_host || !p3d || !slot_valid || !record || !workspace || !pts_size_ok(width, height)) return PXT_E_ARG;
  if (erode < 0 || erode > 2 || n_max < 1 || n_max > (1 << 24) || !(focal > 0.f) || !(depth_scale > 0.f)) return PXT_E_ARG;
  if (((uintptr_t)depth % 16) != 0 || ((uintptr_t)workspace % 8) != 0 || ((uintptr_t)record % 4) != 0) return PXT_E_ARG;
  PtsArgs a;
  a.depth = (const float4*)depth;
  a.W = width;
  a.H = height;
  a.npix = width * height;
  a.nseg = (a.npix + kPtsSeg - 1) / kPtsSeg;
  a.erode = erode;
  a.n_max = n_max;
  a.min_alpha = min_alpha;
  char* ws = (char*)workspace;
  a.head = (int*)ws;
  a.seg_accepted = (int*)(ws + pts_round64(kPtsHead * 4));
  a.seg_candidates = a.seg_accepted + a.nseg;
  a.bits = (unsigned long long*)(ws + pts_round64(kPtsHead * 4) + pts_round64(2 * (int64_t)a.nseg * 4));
  PtsProjection pj;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) pj.M[3 * r + c] = xform_host[4 * r + c];
    pj.b[r] = xform_host[4 * r + 3];
  }
  pj.focal = focal;
  pj.depth_scale = depth_scale;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(points_accept_kernel, dim3(a.nseg), dim3(256), 0, s, a);
  hipLaunchKernelGGL(points_stride_kernel, dim3(a.nseg), dim3(256), 0, s, a);
  hipLaunchKernelGGL(points_compact_kernel, dim3(a.nseg), dim3(256), 0, s, a, pj, p3d, slot_valid, (int*)record);
  PXT_HIP_CHECK(hipGetLastError());
  return PXT_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// The same selection for up to PXT_POINTS_MAX_VIEWS depth planes of a mesh template's frame call in ONE chain of three
// launches (pxt_points_from_depth_views).  The grid is the concatenation of the views' 1024-pixel segments; a workgroup
// finds its view in the per-view first-segment table (uniform per workgroup), the stride pass sums and the compact pass
// prefixes over its own view's segments only.  The back-projection follows the mesh rasteriser's pixel rule (pixel
// centres at integer coordinates, fx fy cx cy) in single fp32 operations, so that mesh_render.points_reference restates
// it bit for bit.  The view table travels in the kernel arguments: no upload, no staging block.
// ---------------------------------------------------------------------------------------------------------------------
namespace pxt {

struct PtvView {
  float f[PXT_MESH_VIEW];  // R row-major, t, fx fy cx cy, near, depth_q, 0 0: what the frame call drew the plane with
  const float4* depth;     // [H][W]: .x = z * depth_q, .w = 1 on a covered pixel
  int W, H, npix;
  int seg0;  // the view's first segment in the grid
};

struct PtvArgs {
  PtvView v[PXT_POINTS_MAX_VIEWS];
  int n_views, nseg, erode, n_max;  // nseg: all views' segments
  float min_alpha;
  int* head;                 // [PXT_POINTS_MAX_VIEWS][2]: A, s per view
  int* seg_accepted;         // [nseg]
  int* seg_candidates;       // [nseg]
  unsigned long long* bits;  // [nseg * kPtsWords]
};

// The workgroup's view: the last one whose first segment is not behind blockIdx.x (every view has a segment).
__device__ __forceinline__ int ptv_view_of(const PtvArgs& a) {
  int v = 0;
  for (int k = 1; k < a.n_views; ++k)
    if ((int)blockIdx.x >= a.v[k].seg0) v = k;
  return v;
}

__device__ __forceinline__ int ptv_segments(const PtvArgs& a, int v) { return (a.v[v].npix + kPtsSeg - 1) / kPtsSeg; }

// pts_candidate_word for the segment `lb` of a view of width W (the bits of pixels >= npix are 0).
__device__ __forceinline__ unsigned long long ptv_candidate_word(const PtvArgs& a, int W, int lb, int s, int j, int& x, int& y) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lb * kPtsSeg + j * 256 + threadIdx.x;
  const unsigned long long w = a.bits[(size_t)blockIdx.x * kPtsWords + j * 4 + wave];
  y = i / W;
  x = i - y * W;
  const bool cand = ((w >> lane) & 1ull) != 0ull && (x % s) == s / 2 && (y % s) == s / 2;
  return __ballot(cand);
}

// R^T q in the order the header states: p_j = (R_0j q_0 + R_1j q_1) + R_2j q_2, every step one fp32 operation.
__device__ __forceinline__ void ptv_to_object(const float* f, float q0, float q1, float q2, float* p) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < 3; ++j) p[j] = (f[j] * q0 + f[3 + j] * q1) + f[6 + j] * q2;
}

__device__ __forceinline__ void ptv_back_project(const float* f, float d, int x, int y, float* p) {
#pragma clang fp contract(off)
  const float z = d / f[17];
  const float xn = ((float)x - f[14]) / f[12];
  const float yn = ((float)y - f[15]) / f[13];
  const float c0 = z * xn, c1 = z * yn;
  ptv_to_object(f, c0 - f[9], c1 - f[10], z - f[11], p);
}

__global__ __launch_bounds__(256) void points_views_accept_kernel(const PtvArgs a) {
  __shared__ int s_cnt[kPtsWords];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int v = ptv_view_of(a);
  const float4* __restrict__ depth = a.v[v].depth;
  const int W = a.v[v].W, H = a.v[v].H, npix = a.v[v].npix, lb = blockIdx.x - a.v[v].seg0;
  const int e = a.erode;
#pragma unroll
  for (int j = 0; j < kPtsTrips; ++j) {
    const int i = lb * kPtsSeg + j * 256 + threadIdx.x;
    bool ok = false;
    if (i < npix) {
      ok = pts_base_test(depth[i], a.min_alpha);
      const int y = i / W, x = i - y * W;
      // the (2e + 1)^2 square: one that leaves the image fails; every pixel of it passes the base test
      if (ok && e > 0 && (x < e || y < e || x + e >= W || y + e >= H)) ok = false;
      if (ok && e > 0) {
        for (int dy = -e; dy <= e; ++dy)
          for (int dx = -e; dx <= e; ++dx)
            if ((dx != 0 || dy != 0) && ok) ok = pts_base_test(depth[i + dy * W + dx], a.min_alpha);
      }
    }
    const unsigned long long m = __ballot(ok);
    if (lane == 0) {
      a.bits[(size_t)blockIdx.x * kPtsWords + j * 4 + wave] = m;
      s_cnt[j * 4 + wave] = __popcll(m);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = 0;
    for (int k = 0; k < kPtsWords; ++k) c += s_cnt[k];
    a.seg_accepted[blockIdx.x] = c;
  }
}

__global__ __launch_bounds__(256) void points_views_stride_kernel(const PtvArgs a) {
  __shared__ int s4[4];
  const int v = ptv_view_of(a);
  const int seg0 = a.v[v].seg0, nseg = ptv_segments(a, v), lb = blockIdx.x - seg0;
  int part = 0;
  for (int b = threadIdx.x; b < nseg; b += 256) part += a.seg_accepted[seg0 + b];
  const int A = pts_block_sum(part, s4);
  const int s = pts_stride(A, a.n_max);
  int c = 0, x, y;
#pragma unroll
  for (int j = 0; j < kPtsTrips; ++j) c += __popcll(ptv_candidate_word(a, a.v[v].W, lb, s, j, x, y));
  c = pts_block_sum((threadIdx.x & 63) == 0 ? c : 0, s4);
  if (threadIdx.x == 0) {
    a.seg_candidates[blockIdx.x] = c;
    if (lb == 0) {
      a.head[2 * v] = A;
      a.head[2 * v + 1] = s;
    }
  }
}

__global__ __launch_bounds__(256) void points_views_compact_kernel(const PtvArgs a, float* __restrict__ p3d_all,
                                                                   uint8_t* __restrict__ valid_all, int* __restrict__ records) {
  __shared__ int s4[4];
  __shared__ int s_cnt[kPtsWords];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int v = ptv_view_of(a);
  const int seg0 = a.v[v].seg0, nseg = ptv_segments(a, v), lb = blockIdx.x - seg0;
  float f[PXT_MESH_VIEW];
#pragma unroll
  for (int k = 0; k < 18; ++k) f[k] = a.v[v].f[k];
  const float4* __restrict__ depth = a.v[v].depth;
  float* __restrict__ p3d = p3d_all + (size_t)v * a.n_max * 3;
  uint8_t* __restrict__ slot_valid = valid_all + (size_t)v * a.n_max;
  const int A = a.head[2 * v], s = a.head[2 * v + 1];
  int before = 0, all = 0;
  for (int b = threadIdx.x; b < nseg; b += 256) {
    const int c = a.seg_candidates[seg0 + b];
    all += c;
    if (b < lb) before += c;
  }
  before = pts_block_sum(before, s4);
  all = pts_block_sum(all, s4);
  unsigned long long m[kPtsTrips];
  int xs[kPtsTrips], ys[kPtsTrips];
#pragma unroll
  for (int j = 0; j < kPtsTrips; ++j) {
    m[j] = ptv_candidate_word(a, a.v[v].W, lb, s, j, xs[j], ys[j]);
    if (lane == 0) s_cnt[j * 4 + wave] = __popcll(m[j]);
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kPtsTrips; ++j) {
    if (((m[j] >> lane) & 1ull) == 0ull) continue;
    int slot = before;  // the segment's words come in pixel order: trip-major, then wave
    for (int k = 0; k < j * 4 + wave; ++k) slot += s_cnt[k];
    slot += __popcll(m[j] & ((1ull << lane) - 1ull));
    if (slot >= a.n_max) continue;  // the tail is cut (record[3] > n_max tells)
    const float4 d = depth[lb * kPtsSeg + j * 256 + threadIdx.x];
    float p[3];
    ptv_back_project(f, d.x, xs[j], ys[j], p);
    p3d[3 * (size_t)slot + 0] = p[0];
    p3d[3 * (size_t)slot + 1] = p[1];
    p3d[3 * (size_t)slot + 2] = p[2];
    slot_valid[slot] = 1;
  }
  // unused slots: the camera centre R^T (-t), which the sampler rejects at the frame's pose (z > kCamEps fails)
  const int n_points = min(all, a.n_max);
  float c[3];
  ptv_to_object(f, -f[9], -f[10], -f[11], c);
  for (int slot = n_points + lb * 256 + threadIdx.x; slot < a.n_max; slot += nseg * 256) {
    p3d[3 * (size_t)slot + 0] = c[0];
    p3d[3 * (size_t)slot + 1] = c[1];
    p3d[3 * (size_t)slot + 2] = c[2];
    slot_valid[slot] = 0;
  }
  if (lb == nseg - 1 && threadIdx.x == 0) {
    int* record = records + 4 * v;
    record[0] = A;
    record[1] = s;
    record[2] = n_points;
    record[3] = all;
  }
}

constexpr int kPtvHeadBytes = PXT_POINTS_MAX_VIEWS * 2 * 4;  // (a multiple of 64)

// The segments of all views, or -1 when a count or a size is out of range.
static inline int64_t ptv_total_segments(int32_t n_views, const int32_t* sizes) {
  if (n_views < 1 || n_views > PXT_POINTS_MAX_VIEWS || !sizes) return -1;
  int64_t nseg = 0;
  for (int k = 0; k < n_views; ++k) {
    if (!pts_size_ok(sizes[2 * k], sizes[2 * k + 1])) return -1;
    nseg += ((int64_t)sizes[2 * k] * sizes[2 * k + 1] + kPtsSeg - 1) / kPtsSeg;
  }
  return nseg;
}

}  // namespace pxt

extern "C" int64_t pxt_points_from_depth_views_workspace_bytes(int32_t n_views, const int32_t* sizes) {
  const int64_t nseg = ptv_total_segments(n_views, sizes);
  if (nseg < 0) return -1;
  return kPtvHeadBytes + pts_round64(2 * nseg * 4) + nseg * kPtsWords * 8;
}

extern "C" int pxt_points_from_depth_views(const float* const* depth, const int32_t* sizes, const float* views, int32_t n_views,
                                           float min_alpha, int32_t erode, int32_t n_max, float* p3d, uint8_t* slot_valid,
                                           int32_t* records, void* workspace, void* stream) {
  if (!depth || !sizes || !views || !p3d || !slot_valid || !records || !workspace) return PXT_E_ARG;
  const int64_t nseg = ptv_total_segments(n_views, sizes);
  if (nseg < 0) return PXT_E_ARG;
  if (erode < 0 || erode > 2 || n_max < 1 || n_max > (1 << 24)) return PXT_E_ARG;
  if (((uintptr_t)workspace % 16) != 0 || ((uintptr_t)p3d % 4) != 0 || ((uintptr_t)slot_valid % 4) != 0 ||
      ((uintptr_t)records % 4) != 0)
    return PXT_E_ARG;
  PtvArgs a;
  int seg0 = 0;
  for (int k = 0; k < n_views; ++k) {
    const float* f = views + (size_t)k * PXT_MESH_VIEW;
    for (int i = 0; i < PXT_MESH_VIEW; ++i)
      if (!std::isfinite(f[i])) return PXT_E_ARG;
    if (!(f[12] > 0.f) || !(f[13] > 0.f) || !(f[17] > 0.f)) return PXT_E_ARG;
    if (!depth[k] || ((uintptr_t)depth[k] % 16) != 0) return PXT_E_ARG;
    PtvView& v = a.v[k];
    for (int i = 0; i < PXT_MESH_VIEW; ++i) v.f[i] = f[i];
    v.depth = (const float4*)depth[k];
    v.W = sizes[2 * k];
    v.H = sizes[2 * k + 1];
    v.npix = v.W * v.H;
    v.seg0 = seg0;
    seg0 += (v.npix + kPtsSeg - 1) / kPtsSeg;
  }
  for (int k = n_views; k < PXT_POINTS_MAX_VIEWS; ++k) a.v[k] = PtvView{};
  a.n_views = n_views;
  a.nseg = (int)nseg;
  a.erode = erode;
  a.n_max = n_max;
  a.min_alpha = min_alpha;
  char* ws = (char*)workspace;
  a.head = (int*)ws;
  a.seg_accepted = (int*)(ws + kPtvHeadBytes);
  a.seg_candidates = a.seg_accepted + a.nseg;
  a.bits = (unsigned long long*)(ws + kPtvHeadBytes + pts_round64(2 * nseg * 4));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(points_views_accept_kernel, dim3(a.nseg), dim3(256), 0, s, a);
  hipLaunchKernelGGL(points_views_stride_kernel, dim3(a.nseg), dim3(256), 0, s, a);
  hipLaunchKernelGGL(points_views_compact_kernel, dim3(a.nseg), dim3(256), 0, s, a, p3d, slot_valid, (int*)records);
  PXT_HIP_CHECK(hipGetLastError());
  return PXT_OK;
}

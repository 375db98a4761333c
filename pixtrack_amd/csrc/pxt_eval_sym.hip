// Symmetry-aware pose errors of a finished run: BOP's MSSD and MSPD of F frames against ground truth in one call
// (pxt_symmetric_pose_errors, include/pixtrack_hip.h).
//
// The BOP benchmark scores a pose with the Maximum Symmetry-aware Surface / Projection Distance: the maximum over the
// model points of the 3D (2D, after projection) distance between the point under the estimate and under the ground truth,
// minimised over the object's set of symmetry transforms (pixtrack_amd/symmetry.py builds the set).  That is F * S * V
// transform-project-compare triples from a few kilobytes of input; the reference has no counterpart.
//
// Arithmetic (fp32, per frame f, symmetry s, vertex i; u_i the centred vertex)
//  * Hoisted, once per vertex and workgroup: a = T_rel u (T_rel = T_gt^-1 T_est, evaluation.relative_poses' form) and
//    pe = pi(T_est u).  Per triple: w = S_s u, d3^2 = |a - w|^2 - the relative form of pxt_eval.hip,
//    |T_est v - T_gt S v| = |T_rel v - S v|, object-sized numbers only - and d2^2 = |pe - pi(T_gt w)|^2 with
//    pi(p) = (fx p.x / p.z + cx, fy p.y / p.z + cy), two IEEE divisions.  d2^2 is +inf when either z is not a positive
//    finite number.  Every transform is the same chain of fmaf, so that T_est = T_gt (T_rel = I exactly) with S_0 = I
//    gives w = u = a and pe == pi(T_gt w) bit for bit: MSSD and MSPD are 0.0 exactly.
//  * SQUARED distances are compared (max over i, then min over s); one sqrtf per figure at the very end (monotone and
//    correctly rounded, as in pxt_eval.hip).
//
// Mapping
//  * A lane owns ONE symmetry (12 floats in registers) and walks vertices; it keeps two running maxima and the inner
//    loop has no cross-lane traffic at all.  256 threads = SL symmetry lanes x VL vertex lanes, SL = the power of two
//    >= min(S, 64), VL = 256 / SL: S = 1 is 256 vertex lanes, S >= 64 is one wave per vertex lane.
//  * grid = (ceil(V / 4096), F, ceil(S / SL)).  A workgroup takes 4096 vertices in LDS tiles of 512 (two float4 per
//    vertex: {u, pe.x}, {a, pe.y}; 16 KiB), staged by all 256 threads with the hoisted arithmetic; vertex lane vl then
//    reads entries vl, vl + VL, ...  With SL = 64 a wave reads one address (a broadcast); with smaller SL the 64 / SL
//    addresses of a wave are consecutive 16-byte words.  The staging is repeated per symmetry chunk: 1 / SL of the work.
//    Both ends stay busy: S = 1, V = 2^20 is 256 workgroups per frame of 16 vertices a lane, S = 630, V = 300 is 10
//    workgroups per frame of 75 vertices a lane.
//  * The frame's 40 floats are read through vector loads (40 lanes of wave 0, which also ballots "not finite") into
//    LDS once per workgroup - they may have been written by a kernel just ahead in the stream; a non-finite one ends
//    the workgroup at once.  The matrices go from LDS into scalar registers next to their use - T_rel, T_est where a
//    tile is staged, T_gt for the inner loop; all 40 floats held throughout spilled scalar registers into vector lanes
//    (106 SGPRs; now 64 SGPRs, 64 VGPRs, no scratch: 8 waves per SIMD).
//  * Reduction: lanes of one symmetry through a wave butterfly over the vertex-lane bits, the four waves through LDS, the
//    squared maxima to workspace[frame][block][2][S_pad]; the fold kernel (256 threads per frame) takes the maximum over
//    the blocks per symmetry, the (value, index) minimum over the set - lowest index on a tie, lanes by butterfly, waves
//    through LDS - and writes the record.  max and min are order-independent: a frame's record depends on its own 40
//    floats, the vertices and the set only.  No atomics.
//
// Tails
//  * Vertices: a tile's live entries are rounded up to a multiple of VL; the entries past the end are copies of the
//    block's last vertex (a duplicate changes no maximum), so the inner loop has no bounds test.
//  * Symmetries: S is rounded up to S_pad = chunks * SL; a lane past S evaluates symmetry S - 1 again and writes its
//    slot, which the fold kernel never reads.  Utilisation is S / S_pad: 315 / 320, 630 / 640, worst 65 / 128.
//
// VALU per triple (counted in the source; the ISA's figure is in DESIGN 3.10): S u 9 fma, d3^2 3 sub + 1 mul + 2 fma,
// max 1, T_gt w 9 fma, two divisions about 10 each, pixel 2 fma, d2^2 2 sub + 1 mul + 1 fma, validity 3, max 1: about 55.
#include "pxt_common.h"

#include <algorithm>

namespace pxt {
namespace {

constexpr int kSyBlock = 256;
constexpr int kSyWaves = kSyBlock / PXT_WAVE;
constexpr int kSyTile = 512;                   // vertices per LDS tile (two float4 each: 16 KiB)
constexpr int kSyVerts = 4096;                 // vertices per workgroup
constexpr int kSyFrame = PXT_SYM_ERR_FRAME;    // floats per frame: rel, est, gt, fx fy cx cy
constexpr int kSyMaxVertices = 1 << 20;
constexpr int kSyMaxFrames = 65535;            // gridDim.y
constexpr float kSyFltMax = 3.402823466e+38f;
static_assert(kSyTile % kSyBlock == 0 && kSyVerts % kSyTile == 0, "tile staging");
static_assert(kSyFrame == 40 && kSyFrame <= PXT_WAVE, "one lane per frame float");

// R row-major in T[0..8], t in T[9..11]; the same fmaf chain wherever a point is transformed
__device__ __forceinline__ void sy_transform(const float* T, float x, float y, float z, float& ox, float& oy, float& oz) {
  ox = fmaf(T[0], x, fmaf(T[1], y, fmaf(T[2], z, T[9])));
  oy = fmaf(T[3], x, fmaf(T[4], y, fmaf(T[5], z, T[10])));
  oz = fmaf(T[6], x, fmaf(T[7], y, fmaf(T[8], z, T[11])));
}

// K = fx, fy, cx, cy.  -> false when z is not a positive finite number (px, py are then meaningless)
__device__ __forceinline__ bool sy_project(const float* K, float x, float y, float z, float& px, float& py) {
  px = fmaf(K[0], x / z, K[2]);
  py = fmaf(K[1], y / z, K[3]);
  return z > 0.f && z <= kSyFltMax;
}

// The frame's 40 floats: vector loads (the 40 lanes are of wave 0) -> LDS.  -> false when a value is not finite.
__device__ __forceinline__ bool sy_load_frame(const float* frames, int frame, float* frame_s, int* bad_s) {
  if (threadIdx.x < PXT_WAVE) {
    float v = 0.f;
    if (threadIdx.x < kSyFrame) frame_s[threadIdx.x] = v = frames[(size_t)frame * kSyFrame + threadIdx.x];
    const unsigned long long bad = __ballot(!(fabsf(v) <= kSyFltMax));  // true for NaN
    if (threadIdx.x == 0) *bad_s = bad != 0ull;
  }
  __syncthreads();
  return uniform(*bad_s) == 0;
}

// 12 floats of the frame from LDS into scalar registers
__device__ __forceinline__ void sy_uniform12(const float* src, float* T) {
#pragma unroll
  for (int i = 0; i < 12; ++i) T[i] = uniform(src[i]);
}

__global__ __launch_bounds__(kSyBlock) void sym_errors_kernel(const float* __restrict__ vertices, const int V,
                                                              const float* __restrict__ syms, const int S,
                                                              const int sl_log2, const float* __restrict__ frames,
                                                              float* __restrict__ partials) {
  __shared__ float4 tile_a[kSyTile];  // u.x, u.y, u.z, pe.x (+inf: the estimate's z is no positive finite number)
  __shared__ float4 tile_b[kSyTile];  // a.x, a.y, a.z, pe.y
  __shared__ float frame_s[kSyFrame];
  __shared__ int bad_s;
  __shared__ float red[kSyWaves][PXT_WAVE][2];
  const int b = blockIdx.x, frame = blockIdx.y, chunk = blockIdx.z, tid = threadIdx.x;
  if (!sy_load_frame(frames, frame, frame_s, &bad_s)) return;  // (workgroup-uniform) the fold kernel marks the record

  const int SL = 1 << sl_log2, VL = kSyBlock >> sl_log2;
  const int vl = tid >> sl_log2;
  const int s = chunk * SL + (tid & (SL - 1));
  float Sm[12];
  {
    const float* sp = syms + 12 * (size_t)min(s, S - 1);  // a lane past S repeats the last symmetry
#pragma unroll
    for (int i = 0; i < 12; ++i) Sm[i] = sp[i];
  }

  float m3 = 0.f, m2 = 0.f;  // squared maxima
  const int v0 = b * kSyVerts, v1 = min(V, v0 + kSyVerts);
#pragma unroll 1
  for (int t0 = v0; t0 < v1; t0 += kSyTile) {
    const int n = min(kSyTile, v1 - t0);
    const int n_pad = (n + VL - 1) & ~(VL - 1);  // VL divides kSyTile: n_pad <= kSyTile
    if (t0 != v0) __syncthreads();               // the previous tile has been read by every wave
#pragma unroll 1
    for (int k = tid; k < n_pad; k += kSyBlock) {
      float T_rel[12], T_est[12], K[4];  // scalar registers, read where they are used: see the header
      sy_uniform12(frame_s, T_rel);
      sy_uniform12(frame_s + 12, T_est);
#pragma unroll
      for (int i = 0; i < 4; ++i) K[i] = uniform(frame_s[36 + i]);
      const size_t o = 3 * (size_t)(t0 + min(k, n - 1));  // past the end: the last vertex again
      const float ux = vertices[o], uy = vertices[o + 1], uz = vertices[o + 2];
      float ax, ay, az, ex, ey, ez, px, py;
      sy_transform(T_rel, ux, uy, uz, ax, ay, az);
      sy_transform(T_est, ux, uy, uz, ex, ey, ez);
      if (!sy_project(K, ex, ey, ez, px, py)) px = __builtin_inff();
      tile_a[k] = make_float4(ux, uy, uz, px);
      tile_b[k] = make_float4(ax, ay, az, py);
    }
    __syncthreads();
    float T_gt[12], K[4];
    sy_uniform12(frame_s + 24, T_gt);
#pragma unroll
    for (int i = 0; i < 4; ++i) K[i] = uniform(frame_s[36 + i]);
#pragma unroll 2
    for (int k = vl; k < n_pad; k += VL) {
      const float4 A = tile_a[k], Bv = tile_b[k];
      float wx, wy, wz, gx, gy, gz, qx, qy;
      sy_transform(Sm, A.x, A.y, A.z, wx, wy, wz);
      const float dx = Bv.x - wx, dy = Bv.y - wy, dz = Bv.z - wz;
      m3 = fmaxf(m3, fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
      sy_transform(T_gt, wx, wy, wz, gx, gy, gz);
      const bool ok = sy_project(K, gx, gy, gz, qx, qy) && A.w <= kSyFltMax;
      const float ex = A.w - qx, ey = Bv.w - qy;
      m2 = fmaxf(m2, ok ? fmaf(ey, ey, ex * ex) : __builtin_inff());
    }
  }

  // lanes of one symmetry (the vertex-lane bits of the lane index) -> wave -> workgroup -> workspace
  for (int m = SL; m < PXT_WAVE; m <<= 1) {
    m3 = fmaxf(m3, __shfl_xor(m3, m, PXT_WAVE));
    m2 = fmaxf(m2, __shfl_xor(m2, m, PXT_WAVE));
  }
  red[tid / PXT_WAVE][tid & (PXT_WAVE - 1)][0] = m3;
  red[tid / PXT_WAVE][tid & (PXT_WAVE - 1)][1] = m2;
  __syncthreads();
  if (tid < SL) {
    float r3 = red[0][tid][0], r2 = red[0][tid][1];
#pragma unroll
    for (int w = 1; w < kSyWaves; ++w) {
      r3 = fmaxf(r3, red[w][tid][0]);
      r2 = fmaxf(r2, red[w][tid][1]);
    }
    const size_t S_pad = (size_t)gridDim.z * SL;
    float* p = partials + ((size_t)frame * gridDim.x + b) * 2 * S_pad + (size_t)chunk * SL + tid;
    p[0] = r3;
    p[S_pad] = r2;
  }
}

// the smaller value; on a tie the lower index
__device__ __forceinline__ void sy_take(float& bv, int& bi, float v, int i) {
  if (v < bv || (v == bv && i < bi)) {
    bv = v;
    bi = i;
  }
}

// One workgroup per frame: per symmetry the maximum over the blocks, then the minimum over the set, then the record.
__global__ __launch_bounds__(kSyBlock) void sym_errors_fold_kernel(const float* __restrict__ frames, const int V,
                                                                   const int S, const int S_pad, const int n_blocks,
                                                                   const float* __restrict__ partials,
                                                                   float* __restrict__ records) {
  __shared__ float frame_s[kSyFrame];
  __shared__ int bad_s;
  __shared__ float red_v[kSyWaves][2];
  __shared__ int red_i[kSyWaves][2];
  const int frame = blockIdx.x, tid = threadIdx.x;
  float* rec = records + (size_t)frame * PXT_SYM_ERR_RECORD;
  if (!sy_load_frame(frames, frame, frame_s, &bad_s)) {
    if (tid == 0) rec[7] = -1.f;  // nothing else is written
    return;
  }
  float bv[2] = {__builtin_inff(), __builtin_inff()};
  int bi[2] = {0x7fffffff, 0x7fffffff};
  const float* base = partials + (size_t)frame * n_blocks * 2 * S_pad;
  for (int s = tid; s < S; s += kSyBlock) {
    float m3 = base[s], m2 = base[S_pad + s];
    for (int b = 1; b < n_blocks; ++b) {
      m3 = fmaxf(m3, base[(size_t)b * 2 * S_pad + s]);
      m2 = fmaxf(m2, base[(size_t)b * 2 * S_pad + S_pad + s]);
    }
    sy_take(bv[0], bi[0], m3, s);
    sy_take(bv[1], bi[1], m2, s);
  }
#pragma unroll
  for (int m = 1; m < PXT_WAVE; m <<= 1) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const float ov = __shfl_xor(bv[j], m, PXT_WAVE);
      const int oi = __shfl_xor(bi[j], m, PXT_WAVE);
      sy_take(bv[j], bi[j], ov, oi);
    }
  }
  if ((tid & (PXT_WAVE - 1)) == 0) {
    red_v[tid / PXT_WAVE][0] = bv[0]; red_v[tid / PXT_WAVE][1] = bv[1];
    red_i[tid / PXT_WAVE][0] = bi[0]; red_i[tid / PXT_WAVE][1] = bi[1];
  }
  __syncthreads();
  if (tid >= PXT_SYM_ERR_RECORD) return;
  float v = 0.f;
  if (tid < 4) {
    const int j = tid >> 1;
    float fv = red_v[0][j];
    int fi = red_i[0][j];
    for (int w = 1; w < kSyWaves; ++w) sy_take(fv, fi, red_v[w][j], red_i[w][j]);
    if (fi == 0x7fffffff) fi = 0;  // every candidate was a NaN (non-finite vertices or set): no index to report
    v = (tid & 1) ? (float)fi : sqrtf(fv);
  } else if (tid == 4) {
    v = (float)V;
  } else if (tid == 5) {
    v = (float)S;
  } else if (tid == 7) {
    v = 1.f;
  }
  rec[tid] = v;
}

struct SyPlan {
  int sl_log2, chunks, blocks;
  int64_t s_pad;
};

bool sy_plan(int n_frames, int n_syms, int n_vertices, SyPlan& p) {
  if (n_frames < 1 || n_frames > kSyMaxFrames || n_vertices < 1 || n_vertices > kSyMaxVertices || n_syms < 1 ||
      n_syms > PXT_SYM_ERR_MAX_SYMS)
    return false;
  p.sl_log2 = 0;
  while ((1 << p.sl_log2) < std::min(n_syms, PXT_WAVE)) ++p.sl_log2;
  const int SL = 1 << p.sl_log2;
  p.chunks = (n_syms + SL - 1) / SL;
  p.blocks = (n_vertices + kSyVerts - 1) / kSyVerts;
  p.s_pad = (int64_t)p.chunks * SL;
  return true;
}

}  // namespace
}  // namespace pxt

using namespace pxt;

extern "C" int64_t pxt_symmetric_pose_errors_workspace_bytes(int32_t n_frames, int32_t n_syms, int32_t n_vertices) {
  SyPlan p;
  if (!sy_plan(n_frames, n_syms, n_vertices, p)) return PXT_E_ARG;
  return (int64_t)n_frames * p.blocks * 2 * p.s_pad * (int64_t)sizeof(float);
}

extern "C" int pxt_symmetric_pose_errors(const float* vertices, int32_t n_vertices, const float* syms, int32_t n_syms,
                                         const float* frames, int32_t n_frames, float* records, void* workspace,
                                         void* stream) {
  if (!vertices || !syms || !frames || !records || !workspace) return PXT_E_ARG;
  SyPlan p;
  if (!sy_plan(n_frames, n_syms, n_vertices, p)) return PXT_E_ARG;
  if (((uintptr_t)vertices % 4) != 0 || ((uintptr_t)syms % 4) != 0 || ((uintptr_t)frames % 4) != 0 ||
      ((uintptr_t)records % 4) != 0 || ((uintptr_t)workspace % 4) != 0)
    return PXT_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  float* partials = (float*)workspace;
  hipLaunchKernelGGL(sym_errors_kernel, dim3(p.blocks, n_frames, p.chunks), dim3(kSyBlock), 0, s, vertices,
                     (int)n_vertices, syms, (int)n_syms, p.sl_log2, frames, partials);
  PXT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(sym_errors_fold_kernel, dim3(n_frames), dim3(kSyBlock), 0, s, frames, (int)n_vertices, (int)n_syms,
                     (int)p.s_pad, p.blocks, (const float*)partials, records);
  PXT_HIP_CHECK(hipGetLastError());
  return PXT_OK;
}

// Depth rasteriser for triangle meshes (pxt_mesh_raster, include/pixtrack_hip.h; pixtrack_amd/mesh_render.py), and
// further down its colour resolve for meshes with vertex colours (pxt_mesh_render) or a texture map
// (pxt_mesh_render_textured).
//
// The reference draws meshes with pytorch3d (pixtrack/utils/pytorch3d_render_utils.py:55-93, render_image) for its
// YCB ground-truth renders; this is the depth part of that for the evaluation stack: BOP's VSD compares depth renders
// of the model's mesh through the camera's real intrinsics.  The rule is stated in the header, restated in numpy by
// mesh_render.rasterize_reference and held to it bit for bit.
//
// Every pixel of a view owns one 64-bit key, (bits of z) << 32 | triangle index, in the workspace; a triangle that
// covers the pixel offers its key with a vector atomicMin.  z > 0, so its bits order as the floats do, and the minimum
// of a totally ordered key does not depend on who arrives first: the image is a pure function of the mesh and the view.
//
// Launches (all on the caller's stream, no host synchronisation)
//  1. rs_clear_kernel: the key planes to "empty", the records to their start values (the status word included), the
//     per-view list counters to 0.
//  2. rs_triangle_kernel, one lane per (view, triangle): the three vertices are transformed in place - the workspace is
//     sized without the vertex count, and a vertex costs about thirty operations - then the culls, the signed area in
//     int64, the bounding box clipped to the image.  A box of at most kRsLaneMax pixels is walked by its lane; a larger
//     one is handed to the whole wave (its set-up travels by lane broadcast, the 64 lanes take a tile of the box per
//     step); one of more than kRsWaveMax pixels goes to the view's list for launch 3 while the list has room, else it
//     takes the wave path too.  Which path a triangle takes changes nothing in the image.
//  3. rs_list_kernel, one workgroup per 16 x 16 pixel tile and view: walks the view's list, skips the entries whose box
//     misses the tile, evaluates the others at its lane's pixel and keeps the smallest key in a register: one atomicMin
//     per pixel at the end.  A full-screen triangle is 1200 workgroups' work, not one wave's.
//  4. rs_resolve_kernel, four pixels per lane: key -> the float4 image, the optional id plane; covered / min z / max z
//     are folded per workgroup and reach the record through integer and bit-pattern atomics.
// The edge functions are products of int32 differences in int64 (exact); they are evaluated per pixel, not stepped.
//
// This file is compiled with -ffp-contract=off (pixtrack_amd/_build.py EXTRA): every product, sum and quotient is
// rounded on its own, as numpy does it.
#include "pxt_bitrow.h"
#include "pxt_common.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

namespace pxt {
namespace {

constexpr int kRsBlock = 256;
constexpr int kRsWaves = kRsBlock / PXT_WAVE;
constexpr int kRsTriBlock = 1024;  // rs_triangle_kernel: one add per workgroup and cause reaches the record
constexpr int kRsResolvePixels = 4;  // rs_resolve_kernel: pixels per lane
constexpr int kRsLaneMax = 32;     // box pixels one lane walks alone
constexpr int kRsWaveMax = 1024;   // box pixels the wave walks together; larger boxes go to the list
constexpr int kRsListCap = 1024;   // list entries per view
constexpr int kRfListCap = 16384;  // ... of pxt_mesh_render_frame (rf_list_kernel)
constexpr int kRfWaveMax = 256;    // ... and its threshold: its list kernel gathers per tile, a tile's worth of box is enough
constexpr int kRsTile = 16;        // rs_list_kernel: kRsTile x kRsTile pixels per workgroup
constexpr int kRsSub = 256;        // sub-pixel steps per pixel
constexpr float kRsGuard = 8388608.f;  // 2^23
constexpr float kRsFltMax = 3.402823466e+38f;
constexpr unsigned long long kRsEmpty = ~0ull;
static_assert(kRsTile * kRsTile == kRsBlock, "one lane per pixel of a tile");

enum { RS_DRAWN = 0, RS_NEAR = 1, RS_GUARD = 2, RS_ZERO = 3, RS_INDEX = 4, RS_OFF = 5 };
// record words
enum { RS_W_COVERED = 0, RS_W_DRAWN = 1, RS_W_NEAR = 2, RS_W_GUARD = 3, RS_W_ZERO = 4, RS_W_INDEX = 5, RS_W_OFF = 6,
       RS_W_ZMIN = 7, RS_W_ZMAX = 8, RS_W_STATUS = 9 };

struct RsView {
  float R[9], t[3], fx, fy, cx, cy, near, depth_q;
};

struct RsTri {
  int x[3], y[3];
  float iz[3];
  long long area;
  int ix0, ix1, iy0, iy1;  // the clipped box, empty when ix0 > ix1 or iy0 > iy1
};

struct RsArgs {
  const float* vertices;
  const int* triangles;
  const float* views;
  int V, T, P, W, H, cap;
  unsigned long long* keys;  // [P][H][W]
  unsigned* list_count;      // [P]
  uint4* list;               // [P][cap]: triangle, ix0 | ix1 << 16, iy0 | iy1 << 16, 0
  float* out_depth;
  int* out_tri;
  unsigned* records;
};

__device__ __forceinline__ bool rs_finite(float v) { return fabsf(v) <= kRsFltMax; }  // false for a NaN

// The view's 20 floats; -> every one of them is finite.
__device__ __forceinline__ bool rs_load_view(const float* __restrict__ v20, RsView* v) {
  bool ok = true;
  float f[PXT_MESH_VIEW];
#pragma unroll
  for (int i = 0; i < PXT_MESH_VIEW; ++i) {
    f[i] = v20[i];
    ok = ok && rs_finite(f[i]);
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) v->R[i] = f[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) v->t[i] = f[9 + i];
  v->fx = f[12]; v->fy = f[13]; v->cx = f[14]; v->cy = f[15];
  v->near = f[16];
  v->depth_q = f[17];
  return ok;
}

// One vertex -> RS_DRAWN (X, Y, iz written), RS_GUARD or RS_NEAR.
__device__ __forceinline__ int rs_vertex(const RsView& v, const float* __restrict__ q, int* X, int* Y, float* iz) {
  const float a = q[0], b = q[1], c = q[2];
  float p[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) p[k] = ((v.R[3 * k] * a + v.R[3 * k + 1] * b) + v.R[3 * k + 2] * c) + v.t[k];
  if (!(rs_finite(p[0]) && rs_finite(p[1]) && rs_finite(p[2]))) return RS_GUARD;
  if (p[2] <= v.near) return RS_NEAR;
  const float x = v.fx * (p[0] / p[2]) + v.cx, y = v.fy * (p[1] / p[2]) + v.cy;
  const float xs = rintf(x * (float)kRsSub), ys = rintf(y * (float)kRsSub);
  if (!(fabsf(xs) < kRsGuard) || !(fabsf(ys) < kRsGuard)) return RS_GUARD;  // a NaN or an infinity fails here too
  *X = (int)xs;
  *Y = (int)ys;
  *iz = 1.0f / p[2];
  return RS_DRAWN;
}

// Triangle t of the view -> its cause (RS_DRAWN: s is complete).  No address outside the vertex array is formed.
__device__ __forceinline__ int rs_setup(const RsView& v, const float* __restrict__ vertices, int V, int ia, int ib,
                                        int ic, int W, int H, RsTri* s) {
  if ((unsigned)ia >= (unsigned)V || (unsigned)ib >= (unsigned)V || (unsigned)ic >= (unsigned)V) return RS_INDEX;
  const int c0 = rs_vertex(v, vertices + 3 * (size_t)ia, &s->x[0], &s->y[0], &s->iz[0]);
  const int c1 = rs_vertex(v, vertices + 3 * (size_t)ib, &s->x[1], &s->y[1], &s->iz[1]);
  const int c2 = rs_vertex(v, vertices + 3 * (size_t)ic, &s->x[2], &s->y[2], &s->iz[2]);
  if (c0 == RS_GUARD || c1 == RS_GUARD || c2 == RS_GUARD) return RS_GUARD;
  if (c0 == RS_NEAR || c1 == RS_NEAR || c2 == RS_NEAR) return RS_NEAR;
  long long area = (long long)(s->x[1] - s->x[0]) * (s->y[2] - s->y[0]) - (long long)(s->y[1] - s->y[0]) * (s->x[2] - s->x[0]);
  if (area == 0) return RS_ZERO;
  if (area < 0) {
    const int tx = s->x[1], ty = s->y[1];
    const float tz = s->iz[1];
    s->x[1] = s->x[2]; s->y[1] = s->y[2]; s->iz[1] = s->iz[2];
    s->x[2] = tx; s->y[2] = ty; s->iz[2] = tz;
    area = -area;
  }
  s->area = area;
  const int lo_x = min(s->x[0], min(s->x[1], s->x[2])), hi_x = max(s->x[0], max(s->x[1], s->x[2]));
  const int lo_y = min(s->y[0], min(s->y[1], s->y[2])), hi_y = max(s->y[0], max(s->y[1], s->y[2]));
  if (hi_x < 0 || hi_y < 0 || (long long)lo_x > (long long)kRsSub * (W - 1) || (long long)lo_y > (long long)kRsSub * (H - 1))
    return RS_OFF;
  s->ix0 = max(0, (lo_x + kRsSub - 1) >> 8);  // arithmetic shifts: floor
  s->iy0 = max(0, (lo_y + kRsSub - 1) >> 8);
  s->ix1 = min(W - 1, hi_x >> 8);
  s->iy1 = min(H - 1, hi_y >> 8);
  return RS_DRAWN;
}

// Pixel (i, j) of the triangle's clipped box: covered, and with a positive finite z?  -> the bits of z.
__device__ __forceinline__ bool rs_pixel(const RsTri& s, int i, int j, unsigned* zbits) {
  const int px = i << 8, py = j << 8;  // inside the box: below 2^23
  long long e[3];
  bool in = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int a = (k + 1) % 3, b = (k + 2) % 3;
    const int dx = s.x[b] - s.x[a], dy = s.y[b] - s.y[a];
    e[k] = (long long)dx * (py - s.y[a]) - (long long)dy * (px - s.x[a]);
    const bool top_left = dy < 0 || (dy == 0 && dx > 0);
    in = in && (e[k] > 0 || (e[k] == 0 && top_left));
  }
  if (!in) return false;
  const float A = (float)s.area;
  const float l0 = (float)e[0] / A, l1 = (float)e[1] / A, l2 = (float)e[2] / A;
  const float inv = (l0 * s.iz[0] + l1 * s.iz[1]) + l2 * s.iz[2];
  const float z = 1.0f / inv;
  if (!(z > 0.f && z <= kRsFltMax)) return false;
  *zbits = __builtin_bit_cast(unsigned, z);
  return true;
}

__device__ __forceinline__ unsigned long long rs_key(unsigned zbits, int tri) {
  return ((unsigned long long)zbits << 32) | (unsigned)tri;
}

__global__ __launch_bounds__(kRsBlock) void rs_clear_kernel(const RsArgs a, const size_t n_units) {
  const size_t stride = (size_t)gridDim.x * kRsBlock;
  const size_t g = (size_t)blockIdx.x * kRsBlock + threadIdx.x;
  ulonglong2* k2 = (ulonglong2*)a.keys;  // the key region is padded to whole 16-byte units
  for (size_t u = g; u < n_units; u += stride) k2[u] = make_ulonglong2(kRsEmpty, kRsEmpty);
  for (size_t u = g; u < (size_t)a.P * PXT_MESH_RASTER_RECORD; u += stride) {
    const int view = (int)(u / PXT_MESH_RASTER_RECORD), w = (int)(u % PXT_MESH_RASTER_RECORD);
    unsigned val = 0u;
    if (w == RS_W_ZMIN) val = 0xffffffffu;
    if (w == RS_W_STATUS) {
      RsView v;
      val = rs_load_view(a.views + (size_t)view * PXT_MESH_VIEW, &v) ? 0u : 0xffffffffu;
    }
    a.records[u] = val;
  }
  for (size_t u = g; u < (size_t)a.P; u += stride) a.list_count[u] = 0u;
}

// The work of one workgroup of launch 2 on a finite view of W x H pixels whose key plane is `keys`; `counts`: six words
// of LDS; a box of more than `wave_max` pixels goes to the list.  a.W, a.H and a.keys are not read:
// pxt_mesh_render_frame's views each have their own.
__device__ __forceinline__ void rs_triangle_view(const RsArgs& a, const RsView& v, const int view, const int W, const int H,
                                                 unsigned long long* __restrict__ keys, unsigned* counts, const int wave_max) {
  const int lane = threadIdx.x & (PXT_WAVE - 1);
  if (threadIdx.x < 6) counts[threadIdx.x] = 0u;
  __syncthreads();
  const int t = blockIdx.x * kRsTriBlock + threadIdx.x;
  RsTri s;
  int cause = -1;  // no triangle
  if (t < a.T) {
    const int* f = a.triangles + 3 * (size_t)t;
    cause = rs_setup(v, a.vertices, a.V, f[0], f[1], f[2], W, H, &s);
  }
  // the counts: the waves' ballots meet in LDS, one add per workgroup and cause reaches the record (thousands of adds
  // to one address cost more than the triangles' own work)
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    const unsigned n = (unsigned)__popcll(__ballot(cause == c));
    if (lane == 0 && n) atomicAdd(&counts[c], n);
  }
  __syncthreads();
  if (threadIdx.x < 6 && counts[threadIdx.x]) {
    const int c = threadIdx.x;
    const int word = c == RS_DRAWN ? RS_W_DRAWN : c == RS_NEAR ? RS_W_NEAR : c == RS_GUARD ? RS_W_GUARD
                     : c == RS_ZERO ? RS_W_ZERO : c == RS_INDEX ? RS_W_INDEX : RS_W_OFF;
    atomicAdd(a.records + (size_t)view * PXT_MESH_RASTER_RECORD + word, counts[c]);
  }
  int npx = 0;
  if (cause == RS_DRAWN && s.ix0 <= s.ix1 && s.iy0 <= s.iy1) npx = (s.ix1 - s.ix0 + 1) * (s.iy1 - s.iy0 + 1);  // < 2^30
  if (npx > wave_max && (s.ix1 | s.iy1) < 65536) {  // to the list while it has room (its boxes are 16-bit)
    const unsigned slot = atomicAdd(a.list_count + view, 1u);
    if (slot < (unsigned)a.cap) {
      a.list[(size_t)view * a.cap + slot] = make_uint4((unsigned)t, (unsigned)s.ix0 | ((unsigned)s.ix1 << 16),
                                                       (unsigned)s.iy0 | ((unsigned)s.iy1 << 16), 0u);
      npx = 0;
    }
  }
  if (npx > 0 && npx <= kRsLaneMax) {
    for (int j = s.iy0; j <= s.iy1; ++j)
      for (int i = s.ix0; i <= s.ix1; ++i) {
        unsigned zb;
        if (rs_pixel(s, i, j, &zb)) atomicMin(keys + (size_t)j * W + i, rs_key(zb, t));
      }
  }
  // the larger boxes, one after the other, by the whole wave
  unsigned long long todo = __ballot(npx > kRsLaneMax);
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    RsTri w;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      w.x[k] = __shfl(s.x[k], src, PXT_WAVE);
      w.y[k] = __shfl(s.y[k], src, PXT_WAVE);
      w.iz[k] = __shfl(s.iz[k], src, PXT_WAVE);
    }
    w.area = ((long long)__shfl((int)(s.area >> 32), src, PXT_WAVE) << 32) |
             (unsigned)__shfl((int)(unsigned)s.area, src, PXT_WAVE);
    w.ix0 = __shfl(s.ix0, src, PXT_WAVE); w.ix1 = __shfl(s.ix1, src, PXT_WAVE);
    w.iy0 = __shfl(s.iy0, src, PXT_WAVE); w.iy1 = __shfl(s.iy1, src, PXT_WAVE);
    const int wt = __shfl(t, src, PXT_WAVE);
    const int bw = w.ix1 - w.ix0 + 1;
    const int ltw = bw > 32 ? 6 : bw > 16 ? 5 : bw > 8 ? 4 : 3;  // the wave's tile: 2^ltw wide, 64 >> ltw high
    const int tw = 1 << ltw, th = PXT_WAVE >> ltw;
    const int lx = lane & (tw - 1), ly = lane >> ltw;
    for (int j0 = w.iy0; j0 <= w.iy1; j0 += th)
      for (int i0 = w.ix0; i0 <= w.ix1; i0 += tw) {
        const int i = i0 + lx, j = j0 + ly;
        unsigned zb;
        if (i <= w.ix1 && j <= w.iy1 && rs_pixel(w, i, j, &zb)) atomicMin(keys + (size_t)j * W + i, rs_key(zb, wt));
      }
  }
}

__global__ __launch_bounds__(kRsTriBlock) void rs_triangle_kernel(const RsArgs a) {
  __shared__ unsigned counts[6];
  const int view = blockIdx.y;
  RsView v;
  if (!rs_load_view(a.views + (size_t)view * PXT_MESH_VIEW, &v)) return;  // the whole workgroup alike
  rs_triangle_view(a, v, view, a.W, a.H, a.keys + (size_t)view * a.W * a.H, counts, kRsWaveMax);
}

// The work of one workgroup of launch 3: tile `tile` of a view of W x H pixels with `tiles_x` tiles per row.
__device__ __forceinline__ void rs_list_view(const RsArgs& a, const RsView& v, const int view, const int W, const int H,
                                             unsigned long long* __restrict__ keys, const int n, const int tiles_x,
                                             const int tile) {
  const int tx0 = (tile % tiles_x) * kRsTile, ty0 = (tile / tiles_x) * kRsTile;
  const int i = tx0 + ((int)threadIdx.x & (kRsTile - 1)), j = ty0 + ((int)threadIdx.x / kRsTile);
  const uint4* list = a.list + (size_t)view * a.cap;
  unsigned long long best = kRsEmpty;
  for (int e = 0; e < n; ++e) {
    const uint4 ent = list[e];
    const int bx0 = (int)(ent.y & 0xffffu), bx1 = (int)(ent.y >> 16), by0 = (int)(ent.z & 0xffffu), by1 = (int)(ent.z >> 16);
    if (bx1 < tx0 || bx0 >= tx0 + kRsTile || by1 < ty0 || by0 >= ty0 + kRsTile) continue;  // the whole workgroup alike
    const int t = (int)ent.x;
    if (t < 0 || t >= a.T) continue;
    const int* f = a.triangles + 3 * (size_t)t;
    RsTri s;
    if (rs_setup(v, a.vertices, a.V, f[0], f[1], f[2], W, H, &s) != RS_DRAWN) continue;
    unsigned zb;
    if (i >= s.ix0 && i <= s.ix1 && j >= s.iy0 && j <= s.iy1 && rs_pixel(s, i, j, &zb)) best = min(best, rs_key(zb, t));
  }
  if (best != kRsEmpty && i < W && j < H) atomicMin(keys + (size_t)j * W + i, best);
}

__global__ __launch_bounds__(kRsBlock) void rs_list_kernel(const RsArgs a, const int tiles_x) {
  const int view = blockIdx.y;
  const int n = (int)min(a.list_count[view], (unsigned)a.cap);
  if (n == 0) return;
  RsView v;
  if (!rs_load_view(a.views + (size_t)view * PXT_MESH_VIEW, &v)) return;  // never: such a view lists nothing
  rs_list_view(a, v, view, a.W, a.H, a.keys + (size_t)view * a.W * a.H, n, tiles_x, (int)blockIdx.x);
}

__global__ __launch_bounds__(kRsBlock) void rs_resolve_kernel(const RsArgs a) {
  __shared__ unsigned red[3][kRsWaves];
  const int view = blockIdx.y, tid = threadIdx.x;
  const size_t wh = (size_t)a.W * a.H;
  const float depth_q = a.views[(size_t)view * PXT_MESH_VIEW + 17];
  unsigned mn = 0xffffffffu, mx = 0u, cnt = 0u;
#pragma unroll
  for (int k = 0; k < kRsResolvePixels; ++k) {
    const size_t pix = ((size_t)blockIdx.x * kRsResolvePixels + k) * kRsBlock + tid;
    if (pix >= wh) continue;
    const unsigned long long key = a.keys[(size_t)view * wh + pix];
    const bool cov = key != kRsEmpty;
    const unsigned zb = (unsigned)(key >> 32);
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (cov) {
      const float d = __builtin_bit_cast(float, zb) * depth_q;
      o = make_float4(d, d, d, 1.0f);
      mn = min(mn, zb);
      mx = max(mx, zb);
      ++cnt;
    }
    ((float4*)a.out_depth)[(size_t)view * wh + pix] = o;
    if (a.out_tri) a.out_tri[(size_t)view * wh + pix] = cov ? (int)(unsigned)(key & 0xffffffffull) : -1;
  }
#pragma unroll
  for (int m = 1; m < PXT_WAVE; m <<= 1) {
    mn = min(mn, (unsigned)__shfl_xor((int)mn, m, PXT_WAVE));
    mx = max(mx, (unsigned)__shfl_xor((int)mx, m, PXT_WAVE));
    cnt += (unsigned)__shfl_xor((int)cnt, m, PXT_WAVE);
  }
  if ((tid & (PXT_WAVE - 1)) == 0) {
    red[0][tid / PXT_WAVE] = cnt;
    red[1][tid / PXT_WAVE] = mn;
    red[2][tid / PXT_WAVE] = mx;
  }
  __syncthreads();
  if (tid == 0) {
    unsigned c = 0u, lo = 0xffffffffu, hi = 0u;
#pragma unroll
    for (int w = 0; w < kRsWaves; ++w) {
      c += red[0][w];
      lo = min(lo, red[1][w]);
      hi = max(hi, red[2][w]);
    }
    if (c) {  // min and max only where they can still move the record: its words only ever move one way
      unsigned* rec = a.records + (size_t)view * PXT_MESH_RASTER_RECORD;
      atomicAdd(rec + RS_W_COVERED, c);
      if (lo < __hip_atomic_load(rec + RS_W_ZMIN, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(rec + RS_W_ZMIN, lo);
      if (hi > __hip_atomic_load(rec + RS_W_ZMAX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(rec + RS_W_ZMAX, hi);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// pxt_mesh_render: the same clear, triangle and list launches, then rs_shade_resolve_kernel instead of
// rs_resolve_kernel.  It writes every requested output from the key plane in one pass: the depth image, the id plane and
// the record as rs_resolve_kernel does, and the colour of the winning triangle at the pixel, for which the triangle is
// set up again from its three vertices (the key holds its index; neighbouring pixels share the gathers).
//
// The pixels of all views are numbered in one row, g = view * W * H + pixel, and a workgroup takes kRsShadePixels of
// them from a multiple of four on: the lane's pixels are g0 + k * kRsBlock + tid (coalesced keys, float4 images and
// ids), the 8-bit results meet in LDS, and then lane tid owns the four pixels g0 + 4 tid ..: bytes 12 (g0 / 4 + tid) of
// the colour plane and 4 (g0 / 4 + tid) of the depth_nz plane, whole aligned dwords whatever W * H is.  A group of four
// that a view shares with its neighbour (or that ends past the last view) is stored bytewise by each view's workgroup.
// What differs between the two colour calls is the shading rule alone: Attr turns the winning triangle's exchanged
// corners and their weights into r, g, b.  RsShade<RsVertexColors> is laid out as the one struct it replaced.
template <class Attr>
struct RsShade {
  Attr attr;
  float* out_rgba;
  unsigned char* out_rgb_u8;
  unsigned char* out_nz;
};

constexpr int kRsShadePixels = kRsBlock * 4;

__device__ __forceinline__ unsigned rs_u8(float c) { return (unsigned)((long long)(c * 255.0f) & 255); }

// pxt_mesh_render's rule: the vertex colours of the exchanged corners idx, c = ((w_0 c_0 + w_1 c_1) + w_2 c_2) / inv.
struct RsVertexColors {
  const float* colors;  // [V][3]
  __device__ __forceinline__ void operator()(int, const int* idx, bool, const float* w, float inv, float* rgb) const {
    const float* c0 = colors + 3 * (size_t)idx[0];
    const float* c1 = colors + 3 * (size_t)idx[1];
    const float* c2 = colors + 3 * (size_t)idx[2];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float c = ((w[0] * c0[ch] + w[1] * c1[ch]) + w[2] * c2[ch]) / inv;
      rgb[ch] = fminf(fmaxf(c, 0.f), 1.0f);  // a NaN -> 0
    }
  }
};

// pxt_mesh_render_textured's rule: the corner UVs of triangle t (exchanged as the vertices were), interpolated as the
// colours are, then one bilinear read of the map: row 0 is v = 1, corners aligned, the border clamped (pytorch3d's
// TexturesUV defaults).  A UV index outside [0, n_uvs) leaves the pixel black; no address outside uvs is formed, and
// the clamps keep the four texels inside the map whatever u and v are.
struct RsTexture {
  const float* uvs;         // [n_uvs][2]
  const int* triangle_uvs;  // [T][3]
  const unsigned* texture;  // [Ht][Wt] dwords: r | g << 8 | b << 16 | ignored << 24
  int n_uvs, Wt, Ht;

  static __device__ __forceinline__ float coordinate(float x, int n, int* i0, int* i1) {
    x = fminf(fmaxf(x, 0.f), (float)(n - 1));  // a NaN -> 0
    const float x0 = floorf(x);
    *i0 = (int)x0;
    *i1 = min(*i0 + 1, n - 1);
    return x - x0;
  }

  __device__ __forceinline__ void operator()(int t, const int*, bool exchanged, const float* w, float inv, float* rgb) const {
    const int* f = triangle_uvs + 3 * (size_t)t;  // t < T: rs_shade checked it
    const int k0 = f[0], k1 = exchanged ? f[2] : f[1], k2 = exchanged ? f[1] : f[2];
    if ((unsigned)k0 >= (unsigned)n_uvs || (unsigned)k1 >= (unsigned)n_uvs || (unsigned)k2 >= (unsigned)n_uvs) return;
    const float* a0 = uvs + 2 * (size_t)k0;
    const float* a1 = uvs + 2 * (size_t)k1;
    const float* a2 = uvs + 2 * (size_t)k2;
    const float u = ((w[0] * a0[0] + w[1] * a1[0]) + w[2] * a2[0]) / inv;
    const float v = ((w[0] * a0[1] + w[1] * a1[1]) + w[2] * a2[1]) / inv;
    int i0, i1, j0, j1;
    const float ax = coordinate(u * (float)(Wt - 1), Wt, &i0, &i1);
    const float ay = coordinate((1.0f - v) * (float)(Ht - 1), Ht, &j0, &j1);
    const unsigned* r0 = texture + (size_t)j0 * Wt;
    const unsigned* r1 = texture + (size_t)j1 * Wt;
    const unsigned t00 = r0[i0], t01 = r0[i1], t10 = r1[i0], t11 = r1[i1];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float c00 = (float)((t00 >> (8 * ch)) & 0xffu) / 255.0f, c01 = (float)((t01 >> (8 * ch)) & 0xffu) / 255.0f;
      const float c10 = (float)((t10 >> (8 * ch)) & 0xffu) / 255.0f, c11 = (float)((t11 >> (8 * ch)) & 0xffu) / 255.0f;
      const float top = c00 + ax * (c01 - c00);
      const float bot = c10 + ax * (c11 - c10);
      const float c = top + ay * (bot - top);
      rgb[ch] = fminf(fmaxf(c, 0.f), 1.0f);
    }
  }
};

// The winning triangle of a pixel, set up for shading as rs_setup does (the same rs_vertex, area and exchange; the
// corner indices follow the exchange), no cull - t won the pixel, so it was drawn.  `ok` is false if it cannot have been.
struct RsShadeTri {
  int x[3], y[3], idx[3];
  float iz[3], A;
  bool exchanged, ok;
};

__device__ __forceinline__ void rs_shade_setup(const RsArgs& a, const RsView& v, int t, RsShadeTri* s) {
  s->ok = false;
  if ((unsigned)t >= (unsigned)a.T) return;
  const int* f = a.triangles + 3 * (size_t)t;
  s->idx[0] = f[0]; s->idx[1] = f[1]; s->idx[2] = f[2];
  if ((unsigned)s->idx[0] >= (unsigned)a.V || (unsigned)s->idx[1] >= (unsigned)a.V || (unsigned)s->idx[2] >= (unsigned)a.V)
    return;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (rs_vertex(v, a.vertices + 3 * (size_t)s->idx[k], &s->x[k], &s->y[k], &s->iz[k]) != RS_DRAWN) return;
  long long area = (long long)(s->x[1] - s->x[0]) * (s->y[2] - s->y[0]) - (long long)(s->y[1] - s->y[0]) * (s->x[2] - s->x[0]);
  if (area == 0) return;
  s->exchanged = area < 0;
  if (s->exchanged) {
    const int tx = s->x[1], ty = s->y[1], ti = s->idx[1];
    const float tz = s->iz[1];
    s->x[1] = s->x[2]; s->y[1] = s->y[2]; s->iz[1] = s->iz[2]; s->idx[1] = s->idx[2];
    s->x[2] = tx; s->y[2] = ty; s->iz[2] = tz; s->idx[2] = ti;
    area = -area;
  }
  s->A = (float)area;
  s->ok = true;
}

// The colour of the set-up triangle t at pixel (i, j) -> rgb, zeros if !s.ok.
template <class Attr>
__device__ __forceinline__ void rs_shade_at(const Attr& attr, const RsShadeTri& s, int t, int i, int j, float* rgb) {
  rgb[0] = rgb[1] = rgb[2] = 0.f;
  if (!s.ok) return;
  const int px = i << 8, py = j << 8;
  float w[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int p = (k + 1) % 3, q = (k + 2) % 3;
    const long long e = (long long)(s.x[q] - s.x[p]) * (py - s.y[p]) - (long long)(s.y[q] - s.y[p]) * (px - s.x[p]);
    const float l = (float)e / s.A;
    w[k] = l * s.iz[k];
  }
  const float inv = (w[0] + w[1]) + w[2];
  attr(t, s.idx, s.exchanged, w, inv, rgb);
}

template <class Attr>
__device__ __forceinline__ void rs_shade(const RsArgs& a, const Attr& attr, const RsView& v, int t, int i, int j,
                                         float* rgb) {
  RsShadeTri s;
  rs_shade_setup(a, v, t, &s);
  rs_shade_at(attr, s, t, i, j, rgb);
}

template <class Attr>
__global__ __launch_bounds__(kRsBlock) void rs_shade_resolve_kernel(const RsArgs a, const RsShade<Attr> o) {
  __shared__ unsigned red[3][kRsWaves];
  __shared__ __attribute__((aligned(16))) unsigned packed[kRsShadePixels];  // r | g << 8 | b << 16 | depth_nz << 24
  const int view = blockIdx.y, tid = threadIdx.x;
  const size_t wh = (size_t)a.W * a.H;
  const size_t start = (size_t)view * wh, end = start + wh;  // the view's pixels in the row of all views
  const size_t g0 = (start & ~(size_t)3) + (size_t)blockIdx.x * kRsShadePixels;
  const bool want_rgb = o.out_rgba || o.out_rgb_u8, want_bytes = o.out_rgb_u8 || o.out_nz;
  RsView v;
  rs_load_view(a.views + (size_t)view * PXT_MESH_VIEW, &v);  // a view that is not finite has no covered pixel
  unsigned mn = 0xffffffffu, mx = 0u, cnt = 0u;
  unsigned long long keys[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const size_t g = g0 + (size_t)k * kRsBlock + tid;
    keys[k] = g >= start && g < end ? a.keys[g] : kRsEmpty;
  }
#pragma unroll 1
  for (int k = 0; k < 4; ++k) {
    const size_t g = g0 + (size_t)k * kRsBlock + tid;
    unsigned pk = 0u;
    if (g >= start && g < end) {
      const unsigned long long key = keys[k];
      const bool cov = key != kRsEmpty;
      const unsigned zb = (unsigned)(key >> 32);
      const int t = (int)(unsigned)(key & 0xffffffffull);
      float d = 0.f, rgb[3] = {0.f, 0.f, 0.f};
      if (cov) {
        d = __builtin_bit_cast(float, zb) * v.depth_q;
        mn = min(mn, zb);
        mx = max(mx, zb);
        ++cnt;
        if (want_rgb) {
          const int pix = (int)(g - start);  // < 2^26
          rs_shade(a, o.attr, v, t, pix % a.W, pix / a.W, rgb);
        }
      }
      const float alpha = cov ? 1.0f : 0.f;
      if (a.out_depth) ((float4*)a.out_depth)[g] = make_float4(d, d, d, alpha);
      if (o.out_rgba) ((float4*)o.out_rgba)[g] = make_float4(rgb[0], rgb[1], rgb[2], alpha);
      if (a.out_tri) a.out_tri[g] = cov ? t : -1;
      pk = rs_u8(rgb[0]) | (rs_u8(rgb[1]) << 8) | (rs_u8(rgb[2]) << 16) | (rs_u8(d) != 0u ? 1u << 24 : 0u);
    }
    if (want_bytes) packed[k * kRsBlock + tid] = pk;
  }
  if (want_bytes) {  // the whole workgroup alike
    __syncthreads();
    const uint4 q = ((const uint4*)packed)[tid];
    const size_t g = g0 + 4 * (size_t)tid;  // a multiple of four
    if (g >= start && g + 4 <= end) {
      if (o.out_rgb_u8) {
        unsigned* p = (unsigned*)(o.out_rgb_u8 + 3 * g);
        p[0] = (q.x & 0xffffffu) | (q.y << 24);
        p[1] = ((q.y >> 8) & 0xffffu) | (q.z << 16);
        p[2] = ((q.z >> 16) & 0xffu) | (q.w << 8);
      }
      if (o.out_nz) *(unsigned*)(o.out_nz + g) = (q.x >> 24) | ((q.y >> 24) << 8) | ((q.z >> 24) << 16) | ((q.w >> 24) << 24);
    } else {
      const unsigned qs[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (g + k < start || g + k >= end) continue;
        if (o.out_rgb_u8) {
          o.out_rgb_u8[3 * (g + k) + 0] = (unsigned char)(qs[k] & 0xffu);
          o.out_rgb_u8[3 * (g + k) + 1] = (unsigned char)((qs[k] >> 8) & 0xffu);
          o.out_rgb_u8[3 * (g + k) + 2] = (unsigned char)((qs[k] >> 16) & 0xffu);
        }
        if (o.out_nz) o.out_nz[g + k] = (unsigned char)(qs[k] >> 24);
      }
    }
  }
#pragma unroll
  for (int m = 1; m < PXT_WAVE; m <<= 1) {
    mn = min(mn, (unsigned)__shfl_xor((int)mn, m, PXT_WAVE));
    mx = max(mx, (unsigned)__shfl_xor((int)mx, m, PXT_WAVE));
    cnt += (unsigned)__shfl_xor((int)cnt, m, PXT_WAVE);
  }
  if ((tid & (PXT_WAVE - 1)) == 0) {
    red[0][tid / PXT_WAVE] = cnt;
    red[1][tid / PXT_WAVE] = mn;
    red[2][tid / PXT_WAVE] = mx;
  }
  __syncthreads();
  if (tid == 0) {
    unsigned c = 0u, lo = 0xffffffffu, hi = 0u;
#pragma unroll
    for (int w = 0; w < kRsWaves; ++w) {
      c += red[0][w];
      lo = min(lo, red[1][w]);
      hi = max(hi, red[2][w]);
    }
    if (c) {  // as rs_resolve_kernel
      unsigned* rec = a.records + (size_t)view * PXT_MESH_RASTER_RECORD;
      atomicAdd(rec + RS_W_COVERED, c);
      if (lo < __hip_atomic_load(rec + RS_W_ZMIN, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(rec + RS_W_ZMIN, lo);
      if (hi > __hip_atomic_load(rec + RS_W_ZMAX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(rec + RS_W_ZMAX, hi);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// pxt_mesh_render_frame: up to PXT_MESH_FRAME_MAX_VIEWS views of one mesh in one call, each with its own size, its own
// supersampling factor S and its own choice of outputs - the two images a tracker frame needs (the depth_nz plane at
// the query camera, the anti-aliased 8-bit image at the reference camera) in four launches.  The first three launches
// are pxt_mesh_raster's bodies on each view's fine lattice (S W x S H): what differs per view - the fine size, where its
// key plane starts, S, where its outputs go - rides in the kernel arguments as a small table, the grid's second
// dimension is the view, and a workgroup beyond its view's own extent exits at once.
//
// rf_resolve_kernel is the new part: one lane per OUTPUT pixel.  It reads the pixel's S x S keys in row-major order,
// sets the winning triangle up again only when the key names another triangle than the previous subsample's (inside a
// triangle all S^2 share one set-up; the three vertex transforms with their divisions are most of a subsample's work),
// shades by the existing rule at the fine pixel, adds in the fixed order and scales by 1 / S^2.  A view's planes start
// on aligned addresses of their own, so the byte planes go out as whole dwords through LDS as in
// rs_shade_resolve_kernel, with only the view's last one to three pixels stored bytewise.
struct RfView {
  int W, H, S, Wf, Hf;     // output size, S, fine size
  size_t key_off;          // the view's first key (an even number: the clear writes pairs)
  float* out_rgba;         // each NULL when the view did not ask for it
  unsigned char* out_rgb_u8;
  float* out_depth;
  unsigned char* out_nz;
};

struct RfArgs {
  RsArgs a;  // W, H unused; keys: all views' planes
  RfView g[PXT_MESH_FRAME_MAX_VIEWS];
};

// The fine view of a view's 20 floats (the header's rule, each step one fp32 operation); -> all of it is finite.
__device__ __forceinline__ bool rf_load_view(const float* __restrict__ v20, const int S, RsView* v) {
  const bool ok = rs_load_view(v20, v);
  const float s = (float)S, h = 0.5f * (float)(S - 1);
  v->fx = v->fx * s;
  v->fy = v->fy * s;
  v->cx = v->cx * s + h;
  v->cy = v->cy * s + h;
  return ok && rs_finite(v->fx) && rs_finite(v->fy) && rs_finite(v->cx) && rs_finite(v->cy);
}

// The work of one lane of launch 1 on a.P views whose floats are a.views; supersample(view) -> the view's S.
template <class SupersampleOf>
__device__ __forceinline__ void rf_clear(const RsArgs& a, const size_t n_units, const SupersampleOf& supersample) {
  const size_t stride = (size_t)gridDim.x * kRsBlock;
  const size_t g = (size_t)blockIdx.x * kRsBlock + threadIdx.x;
  ulonglong2* k2 = (ulonglong2*)a.keys;
  for (size_t u = g; u < n_units; u += stride) k2[u] = make_ulonglong2(kRsEmpty, kRsEmpty);
  if (g < (size_t)a.P * PXT_MESH_RASTER_RECORD) {
    const int view = (int)(g / PXT_MESH_RASTER_RECORD), w = (int)(g % PXT_MESH_RASTER_RECORD);
    unsigned val = 0u;
    if (w == RS_W_ZMIN) val = 0xffffffffu;
    if (w == RS_W_STATUS) {
      RsView v;
      val = rf_load_view(a.views + (size_t)view * PXT_MESH_VIEW, supersample(view), &v) ? 0u : 0xffffffffu;
    }
    a.records[g] = val;
  }
  if (g < (size_t)a.P) a.list_count[g] = 0u;
}

__global__ __launch_bounds__(kRsBlock) void rf_clear_kernel(const RfArgs f, const size_t n_units) {
  rf_clear(f.a, n_units, [&f](int view) { return f.g[view].S; });
}

__global__ __launch_bounds__(kRsTriBlock) void rf_triangle_kernel(const RfArgs f) {
  __shared__ unsigned counts[6];
  const int view = blockIdx.y;
  const RfView& g = f.g[view];
  RsView v;
  if (!rf_load_view(f.a.views + (size_t)view * PXT_MESH_VIEW, g.S, &v)) return;  // the whole workgroup alike
  rs_triangle_view(f.a, v, view, g.Wf, g.Hf, f.a.keys + g.key_off, counts, kRfWaveMax);
}

// Launch 3 of the frame call.  On a fine lattice the triangles of an ordinary mesh are "large" by the thousand (a
// triangle 12 pixels wide is 48 fine pixels wide at S = 4), so the list is longer (kRfListCap) and a tile does not walk
// it entry by entry: the workgroup tests 256 entries at once, one per lane, gathers the few whose box meets its tile in
// LDS, and only those are set up and evaluated by every lane.  The smallest key is kept in a register as in
// rs_list_view; the order in which the entries arrive does not matter to a minimum.
// `g` is the view's table entry; a.list_count[view], a.list + view * a.cap and the mesh of `a` are the view's.
__device__ __forceinline__ void rf_list_view(const RsArgs& a, const RfView& g, const int view, unsigned* hits, unsigned* n_hits) {
  const int tid = threadIdx.x;
  const int W = g.Wf, H = g.Hf;
  const int tiles_x = (W + kRsTile - 1) / kRsTile, tiles_y = (H + kRsTile - 1) / kRsTile;
  if ((int)blockIdx.x >= tiles_x * tiles_y) return;  // the grid is the largest view's
  const int n = (int)min(a.list_count[view], (unsigned)a.cap);
  if (n == 0) return;
  RsView v;
  if (!rf_load_view(a.views + (size_t)view * PXT_MESH_VIEW, g.S, &v)) return;  // never: such a view lists nothing
  const int tx0 = ((int)blockIdx.x % tiles_x) * kRsTile, ty0 = ((int)blockIdx.x / tiles_x) * kRsTile;
  const int i = tx0 + (tid & (kRsTile - 1)), j = ty0 + (tid / kRsTile);
  const uint4* list = a.list + (size_t)view * a.cap;
  unsigned long long best = kRsEmpty;
  for (int base = 0; base < n; base += kRsBlock) {  // the whole workgroup alike
    if (tid == 0) *n_hits = 0u;
    __syncthreads();
    if (base + tid < n) {
      const uint4 ent = list[base + tid];
      const int bx0 = (int)(ent.y & 0xffffu), bx1 = (int)(ent.y >> 16), by0 = (int)(ent.z & 0xffffu), by1 = (int)(ent.z >> 16);
      if (!(bx1 < tx0 || bx0 >= tx0 + kRsTile || by1 < ty0 || by0 >= ty0 + kRsTile)) hits[atomicAdd(n_hits, 1u)] = ent.x;
    }
    __syncthreads();
    const int m = (int)*n_hits;  // <= kRsBlock
    for (int e = 0; e < m; ++e) {
      const int t = (int)hits[e];
      if (t < 0 || t >= a.T) continue;
      const int* tri = a.triangles + 3 * (size_t)t;
      RsTri s;
      if (rs_setup(v, a.vertices, a.V, tri[0], tri[1], tri[2], W, H, &s) != RS_DRAWN) continue;
      unsigned zb;
      if (i >= s.ix0 && i <= s.ix1 && j >= s.iy0 && j <= s.iy1 && rs_pixel(s, i, j, &zb)) best = min(best, rs_key(zb, t));
    }
    __syncthreads();  // hits is rewritten by the next round
  }
  if (best != kRsEmpty && i < W && j < H) atomicMin(a.keys + g.key_off + (size_t)j * W + i, best);
}

__global__ __launch_bounds__(kRsBlock) void rf_list_kernel(const RfArgs f) {
  __shared__ unsigned hits[kRsBlock];
  __shared__ unsigned n_hits;
  rf_list_view(f.a, f.g[blockIdx.y], (int)blockIdx.y, hits, &n_hits);
}

// The work of one workgroup of the resolve on a view whose supersample is S (a template argument: a row of the block
// is unrolled and its keys are loaded before the first is used).
template <class Attr, int S>
__device__ __forceinline__ void rf_resolve_view(const RsArgs& a, const Attr& attr, const RfView& g, const int view,
                                                const int wh, const int p0, unsigned (*red)[kRsWaves], unsigned* packed) {
  const int tid = threadIdx.x;
  const int Wf = g.Wf;
  const bool want_rgb = g.out_rgba || g.out_rgb_u8, want_bytes = g.out_rgb_u8 || g.out_nz;
  const unsigned long long* __restrict__ keys = a.keys + g.key_off;
  const float scale = 1.0f / (float)(S * S);  // exact
  RsView v;
  rf_load_view(a.views + (size_t)view * PXT_MESH_VIEW, S, &v);  // a view that is not finite has no covered pixel
  unsigned mn = 0xffffffffu, mx = 0u, cnt = 0u;
  unsigned long long ahead[4] = {kRsEmpty, kRsEmpty, kRsEmpty, kRsEmpty};
  if (S == 1) {  // one key per pixel: the lane's four are in flight together, as in rs_shade_resolve_kernel
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int pix = p0 + k * kRsBlock + tid;
      if (pix < wh) ahead[k] = keys[pix];
    }
  }
#pragma unroll 1
  for (int k = 0; k < 4; ++k) {
    const int pix = p0 + k * kRsBlock + tid;
    unsigned pk = 0u;
    if (pix < wh) {
      const int i = pix % g.W, j = pix / g.W;
      float acc[4] = {0.f, 0.f, 0.f, 0.f}, d = 0.f;
      RsShadeTri tri;
      tri.ok = false;
      int tri_t = 0;
      bool have = false;
#pragma unroll 1
      for (int sb = 0; sb < S; ++sb) {
        unsigned long long ks[S];  // a row of the block: its keys are in flight together
        if (S == 1) {
          ks[0] = k == 0 ? ahead[0] : k == 1 ? ahead[1] : k == 2 ? ahead[2] : ahead[3];
        } else {
#pragma unroll
          for (int sa = 0; sa < S; ++sa) ks[sa] = keys[(size_t)(S * j + sb) * Wf + (size_t)S * i + sa];
        }
#pragma unroll
        for (int sa = 0; sa < S; ++sa) {
          const unsigned long long key = ks[sa];
          const bool cov = key != kRsEmpty;
          float c[4] = {0.f, 0.f, 0.f, 0.f};
          if (cov) {
            const unsigned zb = (unsigned)(key >> 32);
            const int t = (int)(unsigned)(key & 0xffffffffull);
            mn = min(mn, zb);
            mx = max(mx, zb);
            ++cnt;
            d = __builtin_bit_cast(float, zb) * v.depth_q;  // read for S == 1 alone
            if (want_rgb) {
              if (!have || t != tri_t) {  // neighbouring subsamples mostly share their triangle
                rs_shade_setup(a, v, t, &tri);
                tri_t = t;
                have = true;
              }
              rs_shade_at(attr, tri, t, S * i + sa, S * j + sb, c);
            }
            c[3] = 1.0f;
          }
          if (sa == 0 && sb == 0) {
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) acc[ch] = c[ch];
          } else {
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) acc[ch] = acc[ch] + c[ch];
          }
        }
      }
#pragma unroll
      for (int ch = 0; ch < 4; ++ch) acc[ch] = acc[ch] * scale;
      if (g.out_depth) ((float4*)g.out_depth)[pix] = make_float4(d, d, d, acc[3]);  // S == 1: alpha is 0 or 1
      if (g.out_rgba) ((float4*)g.out_rgba)[pix] = make_float4(acc[0], acc[1], acc[2], acc[3]);
      pk = rs_u8(acc[0]) | (rs_u8(acc[1]) << 8) | (rs_u8(acc[2]) << 16) | (rs_u8(d) != 0u ? 1u << 24 : 0u);
    }
    if (want_bytes) packed[k * kRsBlock + tid] = pk;
  }
  if (want_bytes) {  // the whole workgroup alike
    __syncthreads();
    const uint4 q = ((const uint4*)packed)[tid];
    const int p = p0 + 4 * tid;  // a multiple of four, and the planes are 4-byte aligned
    if (p + 4 <= wh) {
      if (g.out_rgb_u8) {
        unsigned* o = (unsigned*)(g.out_rgb_u8 + 3 * (size_t)p);
        o[0] = (q.x & 0xffffffu) | (q.y << 24);
        o[1] = ((q.y >> 8) & 0xffffu) | (q.z << 16);
        o[2] = ((q.z >> 16) & 0xffu) | (q.w << 8);
      }
      if (g.out_nz) *(unsigned*)(g.out_nz + p) = (q.x >> 24) | ((q.y >> 24) << 8) | ((q.z >> 24) << 16) | ((q.w >> 24) << 24);
    } else {
      const unsigned qs[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (p + k >= wh) continue;
        if (g.out_rgb_u8) {
          g.out_rgb_u8[3 * (size_t)(p + k) + 0] = (unsigned char)(qs[k] & 0xffu);
          g.out_rgb_u8[3 * (size_t)(p + k) + 1] = (unsigned char)((qs[k] >> 8) & 0xffu);
          g.out_rgb_u8[3 * (size_t)(p + k) + 2] = (unsigned char)((qs[k] >> 16) & 0xffu);
        }
        if (g.out_nz) g.out_nz[p + k] = (unsigned char)(qs[k] >> 24);
      }
    }
  }
#pragma unroll
  for (int m = 1; m < PXT_WAVE; m <<= 1) {
    mn = min(mn, (unsigned)__shfl_xor((int)mn, m, PXT_WAVE));
    mx = max(mx, (unsigned)__shfl_xor((int)mx, m, PXT_WAVE));
    cnt += (unsigned)__shfl_xor((int)cnt, m, PXT_WAVE);
  }
  if ((tid & (PXT_WAVE - 1)) == 0) {
    red[0][tid / PXT_WAVE] = cnt;
    red[1][tid / PXT_WAVE] = mn;
    red[2][tid / PXT_WAVE] = mx;
  }
  __syncthreads();
  if (tid == 0) {
    unsigned c = 0u, lo = 0xffffffffu, hi = 0u;
#pragma unroll
    for (int w = 0; w < kRsWaves; ++w) {
      c += red[0][w];
      lo = min(lo, red[1][w]);
      hi = max(hi, red[2][w]);
    }
    if (c) {  // as rs_resolve_kernel
      unsigned* rec = a.records + (size_t)view * PXT_MESH_RASTER_RECORD;
      atomicAdd(rec + RS_W_COVERED, c);
      if (lo < __hip_atomic_load(rec + RS_W_ZMIN, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(rec + RS_W_ZMIN, lo);
      if (hi > __hip_atomic_load(rec + RS_W_ZMAX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(rec + RS_W_ZMAX, hi);
    }
  }
}

template <class Attr>
__global__ __launch_bounds__(kRsBlock) void rf_resolve_kernel(const RfArgs f, const Attr attr) {
  __shared__ unsigned red[3][kRsWaves];
  __shared__ __attribute__((aligned(16))) unsigned packed[kRsShadePixels];  // r | g << 8 | b << 16 | depth_nz << 24
  const int view = blockIdx.y;
  const RfView& g = f.g[view];
  const int wh = g.W * g.H;  // <= 2^26
  const int p0 = (int)blockIdx.x * kRsShadePixels;
  if (p0 >= wh) return;  // the grid is the largest view's; the whole workgroup alike
  if (g.S == 1) rf_resolve_view<Attr, 1>(f.a, attr, g, view, wh, p0, red, packed);
  else if (g.S == 2) rf_resolve_view<Attr, 2>(f.a, attr, g, view, wh, p0, red, packed);
  else rf_resolve_view<Attr, 4>(f.a, attr, g, view, wh, p0, red, packed);
}

// ---------------------------------------------------------------------------------------------------------------------
// pxt_mesh_render_frame_batch: the frame call for views of up to PXT_MESH_BATCH_MAX_MESHES different meshes - K objects
// tracked in lock-step - in one chain.  A view's table entry gains the mesh it draws, its own list and that list's cap;
// the mesh table holds what pxt_mesh_render_frame takes per mesh.  The tables and the views' floats are one record in
// the workspace (at 32 views they do not fit the kernel-argument segment), uploaded ahead of the chain, read-only for
// all of it and addressed uniformly per workgroup.  A workgroup forms the RsArgs of its one view - the view's mesh, its
// 20 floats, its list, its record - and runs the frame call's bodies on it as view 0: the arithmetic is theirs.
struct RbMesh {
  const float* vertices;
  const int* triangles;
  RsVertexColors colors;
  RsTexture texture;
  int V, T, textured;
};

struct RbView {
  RfView g;
  size_t list_off;  // the view's first list entry
  int mesh, cap;    // cap = min(T of the mesh, kRfListCap)
};

struct RbRecord {
  RbMesh mesh[PXT_MESH_BATCH_MAX_MESHES];
  RbView view[PXT_MESH_BATCH_MAX_VIEWS];
  float views[PXT_MESH_BATCH_MAX_VIEWS * PXT_MESH_VIEW];
};

struct RbArgs {
  unsigned long long* keys;
  unsigned* list_count;  // [P]
  uint4* list;           // the views' lists, one after the other
  unsigned* records;
  int P;
};

__device__ __forceinline__ RsArgs rb_view_args(const RbRecord* __restrict__ rec, const RbArgs& b, const int view) {
  const RbView& w = rec->view[view];
  const RbMesh& m = rec->mesh[w.mesh];
  RsArgs a;
  a.vertices = m.vertices; a.triangles = m.triangles; a.views = rec->views + (size_t)view * PXT_MESH_VIEW;
  a.V = m.V; a.T = m.T; a.P = 1; a.W = 0; a.H = 0; a.cap = w.cap;
  a.keys = b.keys;
  a.list_count = b.list_count + view;
  a.list = b.list + w.list_off;
  a.out_depth = nullptr; a.out_tri = nullptr;
  a.records = b.records + (size_t)view * PXT_MESH_RASTER_RECORD;
  return a;
}

__device__ __forceinline__ const RsVertexColors& rb_attr(const RbMesh& m, const RsVertexColors*) { return m.colors; }
__device__ __forceinline__ const RsTexture& rb_attr(const RbMesh& m, const RsTexture*) { return m.texture; }
__device__ __forceinline__ bool rb_takes(const RbMesh& m, const RsVertexColors*) { return !m.textured; }
__device__ __forceinline__ bool rb_takes(const RbMesh& m, const RsTexture*) { return m.textured != 0; }

__global__ __launch_bounds__(kRsBlock) void rb_clear_kernel(const RbRecord* __restrict__ rec, const RbArgs b, const size_t n_units) {
  RsArgs a{};
  a.views = rec->views; a.P = b.P; a.keys = b.keys; a.list_count = b.list_count; a.records = b.records;
  rf_clear(a, n_units, [rec](int view) { return rec->view[view].g.S; });
}

__global__ __launch_bounds__(kRsTriBlock) void rb_triangle_kernel(const RbRecord* __restrict__ rec, const RbArgs b) {
  __shared__ unsigned counts[6];
  const int view = blockIdx.y;
  const RsArgs a = rb_view_args(rec, b, view);
  if ((int)blockIdx.x * kRsTriBlock >= a.T) return;  // the grid is the largest mesh's; the whole workgroup alike
  const RfView g = rec->view[view].g;
  RsView v;
  if (!rf_load_view(a.views, g.S, &v)) return;  // the whole workgroup alike
  rs_triangle_view(a, v, 0, g.Wf, g.Hf, a.keys + g.key_off, counts, kRfWaveMax);
}

__global__ __launch_bounds__(kRsBlock) void rb_list_kernel(const RbRecord* __restrict__ rec, const RbArgs b) {
  __shared__ unsigned hits[kRsBlock];
  __shared__ unsigned n_hits;
  const int view = blockIdx.y;
  const RsArgs a = rb_view_args(rec, b, view);
  const RfView g = rec->view[view].g;
  rf_list_view(a, g, 0, hits, &n_hits);
}

// One launch per shading kind that the call's views use; a view of the other kind exits at once.
template <class Attr>
__global__ __launch_bounds__(kRsBlock) void rb_resolve_kernel(const RbRecord* __restrict__ rec, const RbArgs b) {
  __shared__ unsigned red[3][kRsWaves];
  __shared__ __attribute__((aligned(16))) unsigned packed[kRsShadePixels];
  const int view = blockIdx.y;
  const RbMesh& m = rec->mesh[rec->view[view].mesh];
  if (!rb_takes(m, (const Attr*)nullptr)) return;  // the whole workgroup alike
  const RfView g = rec->view[view].g;
  const int wh = g.W * g.H;  // <= 2^26
  const int p0 = (int)blockIdx.x * kRsShadePixels;
  if (p0 >= wh) return;  // the grid is the largest view's; the whole workgroup alike
  const RsArgs a = rb_view_args(rec, b, view);
  const Attr attr = rb_attr(m, (const Attr*)nullptr);
  if (g.S == 1) rf_resolve_view<Attr, 1>(a, attr, g, 0, wh, p0, red, packed);
  else if (g.S == 2) rf_resolve_view<Attr, 2>(a, attr, g, 0, wh, p0, red, packed);
  else rf_resolve_view<Attr, 4>(a, attr, g, 0, wh, p0, red, packed);
}

// pxt_mesh_render_frame_batch_posed: the views whose pose is the output record of an LM launch queued ahead of the
// call.  One wave, one lane per view, between the parameter record's upload and the clear launch: a posed view's lane
// copies the record's 12 pose floats into the view's floats inside the uploaded parameter record, forms depth_q from t
// and the mesh's radius in float64 (the header's order; the file is compiled -ffp-contract=off, and sqrt and the
// quotient are correctly rounded) and mirrors the 20 floats to views_out, its completion word last.  The rendering
// kernels that follow read the floats from the parameter record as they always do.
struct RbPoseTable {
  const float* record[PXT_MESH_BATCH_MAX_VIEWS];
  double radius[PXT_MESH_BATCH_MAX_VIEWS];
};

__global__ __launch_bounds__(64) void rb_pose_kernel(float* __restrict__ views, const RbPoseTable t, float* views_out, const int P) {
  const int p = threadIdx.x;
  if (p >= P) return;
  const float* rec = t.record[p];
  if (!rec) return;
  float* v = views + (size_t)p * PXT_MESH_VIEW;
  float pose[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) pose[i] = rec[i];
  const float failed = rec[12], status = rec[13];
  const double t0 = (double)pose[9], t1 = (double)pose[10], t2 = (double)pose[11];
  const double norm = __builtin_sqrt((t0 * t0 + t1 * t1) + t2 * t2);
  const float depth_q = (float)(1.0 / (norm + t.radius[p]));
#pragma unroll
  for (int i = 0; i < 12; ++i) v[i] = pose[i];
  v[17] = depth_q;
  if (!views_out) return;
  float* o = views_out + (size_t)p * PXT_MESH_VIEW_OUT;
#pragma unroll
  for (int i = 0; i < 12; ++i) o[i] = pose[i];
#pragma unroll
  for (int i = 12; i < PXT_MESH_VIEW; ++i) o[i] = i == 17 ? depth_q : v[i];
  o[21] = o[22] = o[23] = 0.f;
  // the row (all written by this lane) is visible system-wide before the word: a host may poll it in pinned memory
  __hip_atomic_store(&o[20], (failed == 0.f && status == 0.f) ? 1.f : -1.f, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---------------------------------------------------------------------------------------------------------------------
// pxt_mesh_render_scene_batch: the batch call for objects that share an image.  Views that name the same scene are the
// same camera (checked on the host: size and fx fy cx cy bit for bit, S = 1), so their key planes can be compared pixel
// by pixel: view k is hidden at a pixel where it is covered and another member's z bits are smaller.  The high word of
// an empty key is 0xffffffff, above the bits of every positive finite z: the smallest high word among the other members
// decides, and only the keys' high words are read.
//
// rb_scene_kernel, one workgroup of 256 threads per 64 x 16 tile and view (pxt_occlusion_mask's mapping): the band of
// 16 + 2 r_grow rows x 64 + 2 r_grow columns becomes one 128-bit word per row from two wave ballots of H (outside the
// image H is 0, neutral for the dilation); kScRows band rows per wave trip, their four loads per member in flight
// together.  Dilation by shift-OR along x and row-OR along y, the tile's 16 x 64 bits go out as bytes, four per thread.
// n_hidden is the population of the ballots' own columns on the tile's own rows, n_occluder of the dilated core: one
// integer atomicAdd per workgroup and word onto the record the clear zeroed.  It is launched between the list kernel,
// which finishes the keys, and the resolves: the S = 1 planes it reads were written last and are read again next.
struct RbSceneView {
  unsigned char* occluder;  // [H][W], or NULL: the view wants no plane
  unsigned others;          // bit j: view j is another member of this view's scene
  int reserved;
};

struct RbSceneRecord {
  RbRecord base;
  RbSceneView scene[PXT_MESH_BATCH_MAX_VIEWS];
};
static_assert(PXT_MESH_BATCH_MAX_VIEWS <= 32, "RbSceneView::others holds one bit per view");

constexpr int kScW = 64, kScH = 16, kScMaxR = PXT_MESH_SCENE_MAX_GROW;
constexpr int kScBand = kScH + 2 * kScMaxR;  // staged rows at most
constexpr int kScRows = 2;                   // band rows in flight per wave trip
enum { RS_W_HIDDEN = 10, RS_W_OCCLUDER = 11 };

__global__ __launch_bounds__(kRsBlock) void rb_scene_kernel(const RbSceneRecord* __restrict__ rec, const RbArgs b, const int R) {
  __shared__ OcRow sA[kScBand], sB[kScBand];
  __shared__ unsigned sHidden[kRsWaves], sGrown[kScH];
  const int view = blockIdx.y;
  unsigned char* const out = rec->scene[view].occluder;
  if (!out) return;  // the whole workgroup alike
  const int W = rec->base.view[view].g.W, H = rec->base.view[view].g.H;
  const int tiles_x = (W + kScW - 1) / kScW, tiles_y = (H + kScH - 1) / kScH;
  if ((int)blockIdx.x >= tiles_x * tiles_y) return;  // the grid is the largest view's
  const unsigned others = rec->scene[view].others;
  const unsigned* __restrict__ own_keys = (const unsigned*)(b.keys + rec->base.view[view].g.key_off);
  const int x0 = ((int)blockIdx.x % tiles_x) * kScW, y0 = ((int)blockIdx.x / tiles_x) * kScH;
  const int ah = kScH + 2 * R;  // rows y0 - R .. y0 + kScH + R - 1
  const int tid = threadIdx.x, lane = tid & (PXT_WAVE - 1), wave = tid / PXT_WAVE;
  // band column c of a row sits in ballot c / 64 at bit c % 64; the tile's own columns are c = R .. R + 63
  const unsigned long long core0 = ~0ull << R, core1 = R ? ((1ull << R) - 1ull) : 0ull;
  unsigned n_hidden = 0u;  // wave-uniform
  for (int rb = wave; rb < ah; rb += kRsWaves * kScRows) {
    size_t at[kScRows][2];
    bool inside[kScRows][2];
    unsigned own[kScRows][2], front[kScRows][2];
#pragma unroll
    for (int k = 0; k < kScRows; ++k) {
      const int r = rb + kRsWaves * k, yy = y0 - R + r;
#pragma unroll
      for (int part = 0; part < 2; ++part) {
        const int c = part * 64 + lane, xx = x0 - R + c;
        inside[k][part] = r < ah && c < kScW + 2 * R && yy >= 0 && yy < H && xx >= 0 && xx < W;
        at[k][part] = inside[k][part] ? 2 * ((size_t)yy * W + xx) + 1 : 0;  // the key's high word
        own[k][part] = inside[k][part] ? own_keys[at[k][part]] : 0xffffffffu;
        front[k][part] = 0xffffffffu;
      }
    }
    for (unsigned m = others; m; m &= m - 1u) {  // the whole workgroup alike
      const int j = __ffs((int)m) - 1;
      const unsigned* __restrict__ kj = (const unsigned*)(b.keys + rec->base.view[j].g.key_off);  // W x H as this view's
      unsigned z[kScRows][2];
#pragma unroll
      for (int k = 0; k < kScRows; ++k)
#pragma unroll
        for (int part = 0; part < 2; ++part) z[k][part] = inside[k][part] ? kj[at[k][part]] : 0xffffffffu;
#pragma unroll
      for (int k = 0; k < kScRows; ++k)
#pragma unroll
        for (int part = 0; part < 2; ++part) front[k][part] = min(front[k][part], z[k][part]);
    }
#pragma unroll
    for (int k = 0; k < kScRows; ++k) {
      const int r = rb + kRsWaves * k;
      if (r >= ah) break;  // wave-uniform
      const unsigned long long w0 = __ballot(own[k][0] != 0xffffffffu && front[k][0] < own[k][0]);
      const unsigned long long w1 = __ballot(own[k][1] != 0xffffffffu && front[k][1] < own[k][1]);
      if (r >= R && r < R + kScH) n_hidden += (unsigned)(__popcll(w0 & core0) + __popcll(w1 & core1));
      if (lane == 0) sA[r] = oc_shl(OcRow{w0, w1}, 32 - R);  // column c to bit 32 - R + c; 24 <= 32 - R <= 32
    }
  }
  if (lane == 0) sHidden[wave] = n_hidden;
  __syncthreads();
  if (tid < ah) sB[tid] = oc_dilate_x(sA[tid], R);
  __syncthreads();
  if (tid < kScH) {
    OcRow d = {0ull, 0ull};
    const int rc = tid + R;  // this tile row in the staged band
    for (int q = rc - R; q <= rc + R; ++q) d = oc_or(d, sB[q]);  // 0 <= rc - R, rc + R < ah
    d = oc_and(d, y0 + tid < H ? oc_image_columns(x0, W) : OcRow{0ull, 0ull});  // G lives inside the image
    sA[tid] = d;
    sGrown[tid] = (unsigned)__popcll(oc_core(d));
  }
  __syncthreads();
  {
    const int r = tid >> 4, c4 = (tid & 15) * 4;
    const int yy = y0 + r, xx = x0 + c4;
    const unsigned gbytes = oc_bytes((unsigned)((oc_core(sA[r]) >> c4) & 15ull));
    if (yy < H && xx < W) {
      const size_t px = (size_t)yy * W + xx;
      if ((W & 3) == 0) {  // every row starts 4-byte aligned, as the plane does
        *(unsigned*)(out + px) = gbytes;
      } else {
        for (int j = 0; j < 4 && xx + j < W; ++j) out[px + j] = (unsigned char)((gbytes >> (8 * j)) & 1u);
      }
    }
  }
  if (tid == 0) {
    unsigned h = 0u, g = 0u;
#pragma unroll
    for (int w = 0; w < kRsWaves; ++w) h += sHidden[w];
#pragma unroll
    for (int r = 0; r < kScH; ++r) g += sGrown[r];
    unsigned* record = b.records + (size_t)view * PXT_MESH_RASTER_RECORD;
    if (h) atomicAdd(record + RS_W_HIDDEN, h);
    if (g) atomicAdd(record + RS_W_OCCLUDER, g);
  }
}

constexpr int64_t kRsMaxPixels = (int64_t)1 << 26;
constexpr int kRsMaxViews = 4096, kRsMaxCount = 1 << 24, kRsMaxTexture = 16384;

bool rs_sizes_ok(int P, int T, int W, int H) {
  return P >= 1 && P <= kRsMaxViews && T >= 1 && T <= kRsMaxCount && W >= 1 && H >= 1 && (int64_t)W * H <= kRsMaxPixels;
}
int rs_cap(int T) { return std::min(T, kRsListCap); }
int rf_cap(int T) { return std::min(T, kRfListCap); }
int64_t rs_key_bytes(int P, int W, int H) { return ((int64_t)P * W * H * 8 + 15) / 16 * 16; }
int64_t rs_count_bytes(int P) { return ((int64_t)P * 4 + 15) / 16 * 16; }

// pxt_mesh_render_frame's geometry [P][3] (width, height, S) -> the fine sizes are supported; *keys: the key planes'
// total, each padded to an even number of keys.
bool rf_geometry_ok(int P, int T, const int32_t* geometry, int64_t* keys, int max_views = PXT_MESH_FRAME_MAX_VIEWS) {
  if (P < 1 || P > max_views || T < 1 || T > kRsMaxCount || !geometry) return false;
  int64_t n = 0;
  for (int p = 0; p < P; ++p) {
    const int64_t W = geometry[3 * p], H = geometry[3 * p + 1], S = geometry[3 * p + 2];
    if (W < 1 || H < 1 || W > kRsMaxPixels || H > kRsMaxPixels || !(S == 1 || S == 2 || S == 4)) return false;
    if (W * S * H * S > kRsMaxPixels) return false;  // < 2^58
    n += (W * S * H * S + 1) / 2 * 2;
  }
  *keys = n;
  return true;
}

// View p's table entry from geometry and out_offsets (pxt_mesh_render_frame's rules); *key_off: the running key offset.
// -> the view's planes are aligned, fit their buffers and are at least one.
bool rf_place_view(int p, const int32_t* geometry, const int64_t* out_offsets, char* const* base, const int64_t* out_bytes,
                   int64_t* key_off, RfView* gp) {
  const int64_t pixel_bytes[4] = {16, 3, 16, 1}, align[4] = {16, 4, 16, 4};
  RfView& g = *gp;
  g = RfView{};
  g.W = geometry[3 * p]; g.H = geometry[3 * p + 1]; g.S = geometry[3 * p + 2];
  g.Wf = g.W * g.S; g.Hf = g.H * g.S;
  g.key_off = (size_t)*key_off;
  *key_off += ((int64_t)g.Wf * g.Hf + 1) / 2 * 2;
  char* out[4] = {nullptr, nullptr, nullptr, nullptr};
  bool any = false;
  for (int k = 0; k < 4; ++k) {
    const int64_t off = out_offsets[4 * p + k];
    if (off < 0) continue;
    const int64_t bytes = (int64_t)g.W * g.H * pixel_bytes[k];
    if (!base[k] || (off % align[k]) != 0 || out_bytes[k] < 0 || off > out_bytes[k] || bytes > out_bytes[k] - off)
      return false;
    if (k >= 2 && g.S != 1) return false;  // the depth outputs exist for S = 1 alone
    out[k] = base[k] + off;
    any = true;
  }
  if (!any) return false;
  g.out_rgba = (float*)out[0]; g.out_rgb_u8 = (unsigned char*)out[1];
  g.out_depth = (float*)out[2]; g.out_nz = (unsigned char*)out[3];
  return true;
}

// A mesh's texture arguments are complete, aligned and in range.
bool rs_texture_ok(const float* uvs, int32_t n_uvs, const int32_t* triangle_uvs, const uint8_t* texture, int32_t tex_width,
                   int32_t tex_height) {
  return uvs && triangle_uvs && texture && ((uintptr_t)uvs % 4) == 0 && ((uintptr_t)triangle_uvs % 4) == 0 &&
         ((uintptr_t)texture % 4) == 0 && n_uvs >= 1 && n_uvs <= kRsMaxCount && tex_width >= 1 &&
         tex_width <= kRsMaxTexture && tex_height >= 1 && tex_height <= kRsMaxTexture;
}

template <class Attr>
int rf_launch(const RfArgs& f, const Attr& attr, int64_t n_keys, hipStream_t s) {
  const RsArgs& a = f.a;
  int64_t tiles = 1, res = 1;
  for (int p = 0; p < a.P; ++p) {
    const RfView& g = f.g[p];
    tiles = std::max<int64_t>(tiles, (int64_t)((g.Wf + kRsTile - 1) / kRsTile) * ((g.Hf + kRsTile - 1) / kRsTile));
    res = std::max<int64_t>(res, ((int64_t)g.W * g.H + kRsShadePixels - 1) / kRsShadePixels);
  }
  const size_t n_units = (size_t)(n_keys / 2);
  const size_t clear_work = std::max(n_units, (size_t)a.P * PXT_MESH_RASTER_RECORD);
  const unsigned clear_blocks = (unsigned)std::min<size_t>((clear_work + kRsBlock - 1) / kRsBlock, 8192);
  hipLaunchKernelGGL(rf_clear_kernel, dim3(clear_blocks), dim3(kRsBlock), 0, s, f, n_units);
  PXT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(rf_triangle_kernel, dim3((a.T + kRsTriBlock - 1) / kRsTriBlock, a.P), dim3(kRsTriBlock), 0, s, f);
  PXT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(rf_list_kernel, dim3((unsigned)tiles, a.P), dim3(kRsBlock), 0, s, f);
  PXT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(rf_resolve_kernel<Attr>, dim3((unsigned)res, a.P), dim3(kRsBlock), 0, s, f, attr);
  PXT_HIP_CHECK(hipGetLastError());
  return PXT_OK;
}

// pxt_mesh_render_frame_batch's workspace: the key planes, the list counters, every view's own list (placed by a prefix
// sum of the caps), the parameter record (pxt_mesh_render_scene_batch's is the longer RbSceneRecord).
struct RbLayout {
  int64_t n_keys, count_off, list_off, record_off, bytes;
  int64_t view_list[PXT_MESH_BATCH_MAX_VIEWS];  // first entry of each view's list
};

bool rb_layout(int M, const int32_t* n_triangles, int P, const int32_t* view_mesh, const int32_t* geometry, RbLayout* l,
               size_t record_bytes = sizeof(RbRecord)) {
  if (M < 1 || M > PXT_MESH_BATCH_MAX_MESHES || !n_triangles || !view_mesh) return false;
  for (int m = 0; m < M; ++m)
    if (n_triangles[m] < 1 || n_triangles[m] > kRsMaxCount) return false;
  if (!rf_geometry_ok(P, 1, geometry, &l->n_keys, PXT_MESH_BATCH_MAX_VIEWS)) return false;
  int64_t entries = 0;
  for (int p = 0; p < P; ++p) {
    if (view_mesh[p] < 0 || view_mesh[p] >= M) return false;
    l->view_list[p] = entries;
    entries += rf_cap(n_triangles[view_mesh[p]]);
  }
  l->count_off = l->n_keys * 8;
  l->list_off = l->count_off + rs_count_bytes(P);
  l->record_off = l->list_off + entries * 16;
  l->bytes = l->record_off + (int64_t)(record_bytes + 15) / 16 * 16;
  return true;
}

// The pinned blocks the parameter record is staged in: a ring per thread and device; a block is reused once its
// previous copy has been made (pxt_ngp_render_frame_batch's scheme).
struct RbStageSlot {
  RbSceneRecord* host = nullptr;  // the scene table is copied by pxt_mesh_render_scene_batch alone
  hipEvent_t copied = nullptr;
};
constexpr int kRbStageSlots = 4, kRbStageDevices = 16;

// pxt_mesh_render_frame_batch_posed's own arguments.
struct RbPoseCall {
  const pxt_mesh_view_pose* view_pose;
  float* views_out;
};

// pxt_mesh_render_scene_batch's own arguments.
struct RbSceneCall {
  const int32_t* view_scene;
  int32_t r_grow;
  uint8_t* out_occluder;
  int64_t occluder_bytes;
  const int64_t* occluder_offsets;
};

// The scene table of the P placed views `table` whose floats are `views`; -> every bound of the header holds.
bool rb_place_scenes(const RbSceneCall& c, int P, const RbView* table, const float* views, RbSceneView* scene, bool* any,
                     int64_t* tiles) {
  if (!c.view_scene || !c.occluder_offsets || c.r_grow < 0 || c.r_grow > kScMaxR) return false;
  if (((uintptr_t)c.out_occluder % 4) != 0) return false;
  *any = false;
  for (int p = 0; p < P; ++p) {
    RbSceneView& v = scene[p];
    v = RbSceneView{};
    const int s = c.view_scene[p];
    const int64_t off = c.occluder_offsets[p];
    const RfView& g = table[p].g;
    if (s < -1 || s >= P) return false;
    if (s < 0) {
      if (off >= 0) return false;
      continue;
    }
    if (g.S != 1) return false;
    for (int j = 0; j < P; ++j) {
      if (j == p || c.view_scene[j] != s) continue;
      const RfView& o = table[j].g;
      if (o.W != g.W || o.H != g.H) return false;
      if (std::memcmp(views + (size_t)j * PXT_MESH_VIEW + 12, views + (size_t)p * PXT_MESH_VIEW + 12, 4 * sizeof(float)) != 0)
        return false;
      v.others |= 1u << j;
    }
    if (off < 0) continue;
    const int64_t bytes = (int64_t)g.W * g.H;
    if (!c.out_occluder || (off % 4) != 0 || c.occluder_bytes < 0 || off > c.occluder_bytes || bytes > c.occluder_bytes - off)
      return false;
    v.occluder = c.out_occluder + off;
    *any = true;
    *tiles = std::max<int64_t>(*tiles, (int64_t)((g.W + kScW - 1) / kScW) * ((g.H + kScH - 1) / kScH));
  }
  return true;
}

}  // namespace
}  // namespace pxt

using namespace pxt;

extern "C" int64_t pxt_mesh_raster_workspace_bytes(int32_t n_views, int32_t n_triangles, int32_t width, int32_t height) {
  if (!rs_sizes_ok(n_views, n_triangles, width, height)) return PXT_E_ARG;
  return rs_key_bytes(n_views, width, height) + rs_count_bytes(n_views) + (int64_t)n_views * rs_cap(n_triangles) * 16;
}

extern "C" int pxt_mesh_raster(const float* vertices, int32_t n_vertices, const int32_t* triangles, int32_t n_triangles,
                               const float* views, int32_t n_views, int32_t width, int32_t height, float* out_depth,
                               int32_t* out_tri, uint32_t* records, void* workspace, void* stream) {
  if (!rs_sizes_ok(n_views, n_triangles, width, height) || n_vertices < 1 || n_vertices > kRsMaxCount) return PXT_E_ARG;
  if (!vertices || !triangles || !views || !out_depth || !records || !workspace) return PXT_E_ARG;
  if (((uintptr_t)vertices % 4) != 0 || ((uintptr_t)triangles % 4) != 0 || ((uintptr_t)views % 4) != 0 ||
      ((uintptr_t)out_tri % 4) != 0 || ((uintptr_t)records % 4) != 0 || ((uintptr_t)out_depth % 16) != 0 ||
      ((uintptr_t)workspace % 16) != 0)
    return PXT_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  RsArgs a;
  a.vertices = vertices; a.triangles = (const int*)triangles; a.views = views;
  a.V = n_vertices; a.T = n_triangles; a.P = n_views; a.W = width; a.H = height; a.cap = rs_cap(n_triangles);
  const int64_t key_bytes = rs_key_bytes(n_views, width, height);
  a.keys = (unsigned long long*)workspace;
  a.list_count = (unsigned*)((char*)workspace + key_bytes);
  a.list = (uint4*)((char*)workspace + key_bytes + rs_count_bytes(n_views));
  a.out_depth = out_depth; a.out_tri = (int*)out_tri; a.records = (unsigned*)records;

  const size_t n_units = (size_t)(key_bytes / 16);
  const size_t clear_work = std::max(n_units, (size_t)n_views * PXT_MESH_RASTER_RECORD);
  const unsigned clear_blocks = (unsigned)std::min<size_t>((clear_work + kRsBlock - 1) / kRsBlock, 8192);
  hipLaunchKernelGGL(rs_clear_kernel, dim3(clear_blocks), dim3(kRsBlock), 0, s, a, n_units);
  PXT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(rs_triangle_kernel, dim3((n_triangles + kRsTriBlock - 1) / kRsTriBlock, n_views), dim3(kRsTriBlock), 0, s, a);
  PXT_HIP_CHECK(hipGetLastError());
  const int tiles_x = (width + kRsTile - 1) / kRsTile, tiles_y = (height + kRsTile - 1) / kRsTile;  // product <= 2^26
  hipLaunchKernelGGL(rs_list_kernel, dim3((unsigned)tiles_x * (unsigned)tiles_y, n_views), dim3(kRsBlock), 0, s, a, tiles_x);
  PXT_HIP_CHECK(hipGetLastError());
  const int64_t res_pixels = (int64_t)kRsBlock * kRsResolvePixels;
  const unsigned res_blocks = (unsigned)(((int64_t)width * height + res_pixels - 1) / res_pixels);
  hipLaunchKernelGGL(rs_resolve_kernel, dim3(res_blocks, n_views), dim3(kRsBlock), 0, s, a);
  PXT_HIP_CHECK(hipGetLastError());
  return PXT_OK;
}

// The two colour calls: the shared argument checks, launches 1 to 3 as pxt_mesh_raster makes them and the resolve
// instantiated for the call's shading rule.  `attr_ok` is the caller's verdict on its own arguments.
template <class Attr>
static int rs_render(const float* vertices, int32_t n_vertices, const int32_t* triangles, int32_t n_triangles,
                     const Attr& attr, bool attr_ok, const float* views, int32_t n_views, int32_t width, int32_t height,
                     float* out_rgba, uint8_t* out_rgb_u8, float* out_depth, uint8_t* out_depth_nz, int32_t* out_tri,
                     uint32_t* records, void* workspace, void* stream) {
  if (!rs_sizes_ok(n_views, n_triangles, width, height) || n_vertices < 1 || n_vertices > kRsMaxCount) return PXT_E_ARG;
  if (!vertices || !triangles || !attr_ok || !views || !records || !workspace) return PXT_E_ARG;
  if (!out_rgba && !out_rgb_u8 && !out_depth && !out_depth_nz && !out_tri) return PXT_E_ARG;
  if (((uintptr_t)vertices % 4) != 0 || ((uintptr_t)triangles % 4) != 0 ||
      ((uintptr_t)views % 4) != 0 || ((uintptr_t)out_tri % 4) != 0 || ((uintptr_t)records % 4) != 0 ||
      ((uintptr_t)out_rgb_u8 % 4) != 0 || ((uintptr_t)out_depth_nz % 4) != 0 || ((uintptr_t)out_rgba % 16) != 0 ||
      ((uintptr_t)out_depth % 16) != 0 || ((uintptr_t)workspace % 16) != 0)
    return PXT_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  RsArgs a;
  a.vertices = vertices; a.triangles = (const int*)triangles; a.views = views;
  a.V = n_vertices; a.T = n_triangles; a.P = n_views; a.W = width; a.H = height; a.cap = rs_cap(n_triangles);
  const int64_t key_bytes = rs_key_bytes(n_views, width, height);
  a.keys = (unsigned long long*)workspace;
  a.list_count = (unsigned*)((char*)workspace + key_bytes);
  a.list = (uint4*)((char*)workspace + key_bytes + rs_count_bytes(n_views));
  a.out_depth = out_depth; a.out_tri = (int*)out_tri; a.records = (unsigned*)records;
  RsShade<Attr> o;
  o.attr = attr; o.out_rgba = out_rgba; o.out_rgb_u8 = out_rgb_u8; o.out_nz = out_depth_nz;

  // launches 1 to 3 as pxt_mesh_raster makes them
  const size_t n_units = (size_t)(key_bytes / 16);
  const size_t clear_work = std::max(n_units, (size_t)n_views * PXT_MESH_RASTER_RECORD);
  const unsigned clear_blocks = (unsigned)std::min<size_t>((clear_work + kRsBlock - 1) / kRsBlock, 8192);
  hipLaunchKernelGGL(rs_clear_kernel, dim3(clear_blocks), dim3(kRsBlock), 0, s, a, n_units);
  PXT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(rs_triangle_kernel, dim3((n_triangles + kRsTriBlock - 1) / kRsTriBlock, n_views), dim3(kRsTriBlock), 0, s, a);
  PXT_HIP_CHECK(hipGetLastError());
  const int tiles_x = (width + kRsTile - 1) / kRsTile, tiles_y = (height + kRsTile - 1) / kRsTile;
  hipLaunchKernelGGL(rs_list_kernel, dim3((unsigned)tiles_x * (unsigned)tiles_y, n_views), dim3(kRsBlock), 0, s, a, tiles_x);
  PXT_HIP_CHECK(hipGetLastError());
  // a view's pixels begin up to three past a multiple of four in the row of all views
  const unsigned res_blocks = (unsigned)(((int64_t)width * height + 3 + kRsShadePixels - 1) / kRsShadePixels);
  hipLaunchKernelGGL(rs_shade_resolve_kernel<Attr>, dim3(res_blocks, n_views), dim3(kRsBlock), 0, s, a, o);
  PXT_HIP_CHECK(hipGetLastError());
  return PXT_OK;
}

extern "C" int pxt_mesh_render(const float* vertices, int32_t n_vertices, const int32_t* triangles, int32_t n_triangles,
                               const float* colors, const float* views, int32_t n_views, int32_t width, int32_t height,
                               float* out_rgba, uint8_t* out_rgb_u8, float* out_depth, uint8_t* out_depth_nz,
                               int32_t* out_tri, uint32_t* records, void* workspace, void* stream) {
  RsVertexColors attr;
  attr.colors = colors;
  return rs_render(vertices, n_vertices, triangles, n_triangles, attr, colors && ((uintptr_t)colors % 4) == 0, views,
                   n_views, width, height, out_rgba, out_rgb_u8, out_depth, out_depth_nz, out_tri, records, workspace,
                   stream);
}

extern "C" int pxt_mesh_render_textured(const float* vertices, int32_t n_vertices, const int32_t* triangles,
                                        int32_t n_triangles, const float* uvs, int32_t n_uvs, const int32_t* triangle_uvs,
                                        const uint8_t* texture, int32_t tex_width, int32_t tex_height, const float* views,
                                        int32_t n_views, int32_t width, int32_t height, float* out_rgba,
                                        uint8_t* out_rgb_u8, float* out_depth, uint8_t* out_depth_nz, int32_t* out_tri,
                                        uint32_t* records, void* workspace, void* stream) {
  RsTexture attr;
  attr.uvs = uvs; attr.triangle_uvs = (const int*)triangle_uvs; attr.texture = (const unsigned*)texture;
  attr.n_uvs = n_uvs; attr.Wt = tex_width; attr.Ht = tex_height;
  const bool ok = rs_texture_ok(uvs, n_uvs, triangle_uvs, texture, tex_width, tex_height);
  return rs_render(vertices, n_vertices, triangles, n_triangles, attr, ok, views, n_views, width, height, out_rgba,
                   out_rgb_u8, out_depth, out_depth_nz, out_tri, records, workspace, stream);
}

extern "C" int64_t pxt_mesh_render_frame_workspace_bytes(int32_t n_views, int32_t n_triangles, const int32_t* geometry) {
  int64_t n_keys;
  if (!rf_geometry_ok(n_views, n_triangles, geometry, &n_keys)) return PXT_E_ARG;
  return n_keys * 8 + rs_count_bytes(n_views) + (int64_t)n_views * rf_cap(n_triangles) * 16;
}

extern "C" int pxt_mesh_render_frame(const float* vertices, int32_t n_vertices, const int32_t* triangles,
                                     int32_t n_triangles, const float* colors, const float* uvs, int32_t n_uvs,
                                     const int32_t* triangle_uvs, const uint8_t* texture, int32_t tex_width,
                                     int32_t tex_height, const float* views, int32_t n_views, const int32_t* geometry,
                                     const int64_t* out_offsets, float* out_rgba, uint8_t* out_rgb_u8, float* out_depth,
                                     uint8_t* out_depth_nz, const int64_t* out_bytes, uint32_t* records, void* workspace,
                                     void* stream) {
  int64_t n_keys;
  if (!rf_geometry_ok(n_views, n_triangles, geometry, &n_keys) || n_vertices < 1 || n_vertices > kRsMaxCount) return PXT_E_ARG;
  if (!vertices || !triangles || !views || !out_offsets || !out_bytes || !records || !workspace) return PXT_E_ARG;
  const bool textured = uvs || triangle_uvs || texture;
  if ((colors != nullptr) == textured) return PXT_E_ARG;  // vertex colours or a texture map, one of the two
  if (textured && !rs_texture_ok(uvs, n_uvs, triangle_uvs, texture, tex_width, tex_height)) return PXT_E_ARG;
  if (((uintptr_t)vertices % 4) != 0 || ((uintptr_t)triangles % 4) != 0 || ((uintptr_t)colors % 4) != 0 ||
      ((uintptr_t)views % 4) != 0 || ((uintptr_t)records % 4) != 0 || ((uintptr_t)out_rgb_u8 % 4) != 0 ||
      ((uintptr_t)out_depth_nz % 4) != 0 || ((uintptr_t)out_rgba % 16) != 0 || ((uintptr_t)out_depth % 16) != 0 ||
      ((uintptr_t)workspace % 16) != 0)
    return PXT_E_ARG;
  RfArgs f;
  RsArgs& a = f.a;
  a.vertices = vertices; a.triangles = (const int*)triangles; a.views = views;
  a.V = n_vertices; a.T = n_triangles; a.P = n_views; a.W = 0; a.H = 0; a.cap = rf_cap(n_triangles);
  a.keys = (unsigned long long*)workspace;
  a.list_count = (unsigned*)((char*)workspace + n_keys * 8);
  a.list = (uint4*)((char*)workspace + n_keys * 8 + rs_count_bytes(n_views));
  a.out_depth = nullptr; a.out_tri = nullptr; a.records = (unsigned*)records;
  char* const base[4] = {(char*)out_rgba, (char*)out_rgb_u8, (char*)out_depth, (char*)out_depth_nz};
  int64_t key_off = 0;
  for (int p = 0; p < PXT_MESH_FRAME_MAX_VIEWS; ++p) {
    f.g[p] = RfView{};
    if (p < n_views && !rf_place_view(p, geometry, out_offsets, base, out_bytes, &key_off, &f.g[p])) return PXT_E_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  if (textured) {
    RsTexture attr;
    attr.uvs = uvs; attr.triangle_uvs = (const int*)triangle_uvs; attr.texture = (const unsigned*)texture;
    attr.n_uvs = n_uvs; attr.Wt = tex_width; attr.Ht = tex_height;
    return rf_launch(f, attr, n_keys, s);
  }
  RsVertexColors attr;
  attr.colors = colors;
  return rf_launch(f, attr, n_keys, s);
}

extern "C" int64_t pxt_mesh_render_frame_batch_workspace_bytes(int32_t n_meshes, const int32_t* n_triangles, int32_t n_views,
                                                               const int32_t* view_mesh, const int32_t* geometry) {
  RbLayout l;
  if (!rb_layout(n_meshes, n_triangles, n_views, view_mesh, geometry, &l)) return PXT_E_ARG;
  return l.bytes;
}

// The two batch calls: `scene` is pxt_mesh_render_scene_batch's own arguments, NULL for pxt_mesh_render_frame_batch.
static int rb_render(const pxt_mesh_desc* meshes, int32_t n_meshes, const int32_t* view_mesh, const float* views,
                     int32_t n_views, const int32_t* geometry, const int64_t* out_offsets, float* out_rgba,
                     uint8_t* out_rgb_u8, float* out_depth, uint8_t* out_depth_nz, const int64_t* out_bytes,
                     uint32_t* records, void* workspace, void* stream, const RbSceneCall* scene,
                     const RbPoseCall* posed = nullptr) {
  if (!meshes || n_meshes < 1 || n_meshes > PXT_MESH_BATCH_MAX_MESHES) return PXT_E_ARG;
  int32_t n_triangles[PXT_MESH_BATCH_MAX_MESHES];
  for (int m = 0; m < n_meshes; ++m) n_triangles[m] = meshes[m].n_triangles;
  RbLayout l;
  const size_t record_bytes = scene ? sizeof(RbSceneRecord) : sizeof(RbRecord);
  if (!rb_layout(n_meshes, n_triangles, n_views, view_mesh, geometry, &l, record_bytes)) return PXT_E_ARG;
  if (!views || !out_offsets || !out_bytes || !records || !workspace) return PXT_E_ARG;
  if (((uintptr_t)views % 4) != 0 || ((uintptr_t)records % 4) != 0 || ((uintptr_t)out_rgb_u8 % 4) != 0 ||
      ((uintptr_t)out_depth_nz % 4) != 0 || ((uintptr_t)out_rgba % 16) != 0 || ((uintptr_t)out_depth % 16) != 0 ||
      ((uintptr_t)workspace % 16) != 0)
    return PXT_E_ARG;
  bool kind[2] = {false, false};  // vertex colours, texture: a mesh counts where a view draws it
  for (int m = 0; m < n_meshes; ++m) {
    const pxt_mesh_desc& d = meshes[m];
    if (d.n_vertices < 1 || d.n_vertices > kRsMaxCount || !d.vertices || !d.triangles) return PXT_E_ARG;
    if (((uintptr_t)d.vertices % 4) != 0 || ((uintptr_t)d.triangles % 4) != 0 || ((uintptr_t)d.colors % 4) != 0) return PXT_E_ARG;
    const bool textured = d.uvs || d.triangle_uvs || d.texture;
    if ((d.colors != nullptr) == textured) return PXT_E_ARG;  // vertex colours or a texture map, one of the two
    if (textured && !rs_texture_ok(d.uvs, d.n_uvs, d.triangle_uvs, d.texture, d.tex_width, d.tex_height)) return PXT_E_ARG;
  }
  RbView table[PXT_MESH_BATCH_MAX_VIEWS];
  char* const base[4] = {(char*)out_rgba, (char*)out_rgb_u8, (char*)out_depth, (char*)out_depth_nz};
  int64_t key_off = 0, tiles = 1, res = 1;
  int max_T = 1;
  for (int p = 0; p < n_views; ++p) {
    RbView& w = table[p];
    if (!rf_place_view(p, geometry, out_offsets, base, out_bytes, &key_off, &w.g)) return PXT_E_ARG;
    w.mesh = view_mesh[p];
    w.cap = rf_cap(n_triangles[w.mesh]);
    w.list_off = (size_t)l.view_list[p];
    kind[meshes[w.mesh].colors ? 0 : 1] = true;
    max_T = std::max(max_T, (int)n_triangles[w.mesh]);
    tiles = std::max<int64_t>(tiles, (int64_t)((w.g.Wf + kRsTile - 1) / kRsTile) * ((w.g.Hf + kRsTile - 1) / kRsTile));
    res = std::max<int64_t>(res, ((int64_t)w.g.W * w.g.H + kRsShadePixels - 1) / kRsShadePixels);
  }
  RbSceneView scenes[PXT_MESH_BATCH_MAX_VIEWS] = {};
  bool any_plane = false;
  int64_t scene_tiles = 1;
  if (scene && !rb_place_scenes(*scene, n_views, table, views, scenes, &any_plane, &scene_tiles)) return PXT_E_ARG;
  RbPoseTable poses = {};
  bool any_posed = false;
  if (posed) {
    if (!posed->view_pose || ((uintptr_t)posed->views_out % 4) != 0) return PXT_E_ARG;
    for (int p = 0; p < n_views; ++p) {
      const pxt_mesh_view_pose& q = posed->view_pose[p];
      if (!q.pose_record) continue;
      if (((uintptr_t)q.pose_record % 4) != 0 || !std::isfinite(q.radius) || q.radius < 0.0) return PXT_E_ARG;
      poses.record[p] = q.pose_record;
      poses.radius[p] = q.radius;
      any_posed = true;
    }
  }
  // every argument is checked: from here on the call writes
  hipStream_t s = (hipStream_t)stream;
  static thread_local RbStageSlot stage[kRbStageDevices][kRbStageSlots];
  static thread_local int stage_next[kRbStageDevices] = {0};
  int dev_id = 0;
  PXT_HIP_CHECK(hipGetDevice(&dev_id));
  if (dev_id < 0 || dev_id >= kRbStageDevices) return PXT_E_ARG;
  RbStageSlot& slot = stage[dev_id][stage_next[dev_id]];
  stage_next[dev_id] = (stage_next[dev_id] + 1) % kRbStageSlots;
  if (!slot.host) {
    PXT_HIP_CHECK(hipHostMalloc((void**)&slot.host, sizeof(RbSceneRecord), hipHostMallocDefault));
    PXT_HIP_CHECK(hipEventCreateWithFlags(&slot.copied, hipEventDisableTiming));
  } else {
    PXT_HIP_CHECK(hipEventSynchronize(slot.copied));
  }
  RbRecord* const h = &slot.host->base;
  for (int m = 0; m < PXT_MESH_BATCH_MAX_MESHES; ++m) {
    RbMesh& o = h->mesh[m];
    o = RbMesh{};
    if (m >= n_meshes) continue;
    const pxt_mesh_desc& d = meshes[m];
    o.vertices = d.vertices; o.triangles = (const int*)d.triangles; o.V = d.n_vertices; o.T = d.n_triangles;
    o.textured = d.colors ? 0 : 1;
    o.colors.colors = d.colors;
    if (o.textured) {
      o.texture.uvs = d.uvs; o.texture.triangle_uvs = (const int*)d.triangle_uvs; o.texture.texture = (const unsigned*)d.texture;
      o.texture.n_uvs = d.n_uvs; o.texture.Wt = d.tex_width; o.texture.Ht = d.tex_height;
    }
  }
  for (int p = 0; p < PXT_MESH_BATCH_MAX_VIEWS; ++p) h->view[p] = p < n_views ? table[p] : RbView{};
  std::copy(views, views + (size_t)n_views * PXT_MESH_VIEW, h->views);
  std::fill(h->views + (size_t)n_views * PXT_MESH_VIEW, h->views + PXT_MESH_BATCH_MAX_VIEWS * PXT_MESH_VIEW, 0.f);
  char* const ws = (char*)workspace;
  if (scene) std::copy(scenes, scenes + PXT_MESH_BATCH_MAX_VIEWS, slot.host->scene);
  const RbRecord* rec = (const RbRecord*)(ws + l.record_off);  // the first member of an RbSceneRecord
  PXT_HIP_CHECK(hipMemcpyAsync(ws + l.record_off, slot.host, record_bytes, hipMemcpyHostToDevice, s));
  PXT_HIP_CHECK(hipEventRecord(slot.copied, s));
  if (any_posed) {  // behind the upload, ahead of every launch that reads the views' floats
    hipLaunchKernelGGL(rb_pose_kernel, dim3(1), dim3(64), 0, s, (float*)(ws + l.record_off + offsetof(RbRecord, views)),
                       poses, posed->views_out, (int)n_views);
    PXT_HIP_CHECK(hipGetLastError());
  }
  RbArgs b;
  b.keys = (unsigned long long*)ws;
  b.list_count = (unsigned*)(ws + l.count_off);
  b.list = (uint4*)(ws + l.list_off);
  b.records = (unsigned*)records;
  b.P = n_views;
  const size_t n_units = (size_t)(l.n_keys / 2);
  const size_t clear_work = std::max(n_units, (size_t)n_views * PXT_MESH_RASTER_RECORD);
  const unsigned clear_blocks = (unsigned)std::min<size_t>((clear_work + kRsBlock - 1) / kRsBlock, 8192);
  hipLaunchKernelGGL(rb_clear_kernel, dim3(clear_blocks), dim3(kRsBlock), 0, s, rec, b, n_units);
  PXT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(rb_triangle_kernel, dim3((max_T + kRsTriBlock - 1) / kRsTriBlock, n_views), dim3(kRsTriBlock), 0, s, rec, b);
  PXT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(rb_list_kernel, dim3((unsigned)tiles, n_views), dim3(kRsBlock), 0, s, rec, b);
  PXT_HIP_CHECK(hipGetLastError());
  if (any_plane) {  // the keys are final; before the resolves (see rb_scene_kernel)
    hipLaunchKernelGGL(rb_scene_kernel, dim3((unsigned)scene_tiles, n_views), dim3(kRsBlock), 0, s,
                       (const RbSceneRecord*)(ws + l.record_off), b, (int)scene->r_grow);
    PXT_HIP_CHECK(hipGetLastError());
  }
  if (kind[0]) {
    hipLaunchKernelGGL(rb_resolve_kernel<RsVertexColors>, dim3((unsigned)res, n_views), dim3(kRsBlock), 0, s, rec, b);
    PXT_HIP_CHECK(hipGetLastError());
  }
  if (kind[1]) {
    hipLaunchKernelGGL(rb_resolve_kernel<RsTexture>, dim3((unsigned)res, n_views), dim3(kRsBlock), 0, s, rec, b);
    PXT_HIP_CHECK(hipGetLastError());
  }
  return PXT_OK;
}

extern "C" int pxt_mesh_render_frame_batch(const pxt_mesh_desc* meshes, int32_t n_meshes, const int32_t* view_mesh,
                                           const float* views, int32_t n_views, const int32_t* geometry,
                                           const int64_t* out_offsets, float* out_rgba, uint8_t* out_rgb_u8,
                                           float* out_depth, uint8_t* out_depth_nz, const int64_t* out_bytes,
                                           uint32_t* records, void* workspace, void* stream) {
  return rb_render(meshes, n_meshes, view_mesh, views, n_views, geometry, out_offsets, out_rgba, out_rgb_u8, out_depth,
                   out_depth_nz, out_bytes, records, workspace, stream, nullptr);
}

extern "C" int pxt_mesh_render_frame_batch_posed(const pxt_mesh_desc* meshes, int32_t n_meshes, const int32_t* view_mesh,
                                                 const float* views, int32_t n_views, const int32_t* geometry,
                                                 const int64_t* out_offsets, float* out_rgba, uint8_t* out_rgb_u8,
                                                 float* out_depth, uint8_t* out_depth_nz, const int64_t* out_bytes,
                                                 uint32_t* records, void* workspace, const pxt_mesh_view_pose* view_pose,
                                                 float* views_out, void* stream) {
  const RbPoseCall posed = {view_pose, views_out};
  return rb_render(meshes, n_meshes, view_mesh, views, n_views, geometry, out_offsets, out_rgba, out_rgb_u8, out_depth,
                   out_depth_nz, out_bytes, records, workspace, stream, nullptr, &posed);
}

extern "C" int64_t pxt_mesh_render_scene_batch_workspace_bytes(int32_t n_meshes, const int32_t* n_triangles, int32_t n_views,
                                                               const int32_t* view_mesh, const int32_t* geometry) {
  RbLayout l;
  if (!rb_layout(n_meshes, n_triangles, n_views, view_mesh, geometry, &l, sizeof(RbSceneRecord))) return PXT_E_ARG;
  return l.bytes;
}

extern "C" int pxt_mesh_render_scene_batch(const pxt_mesh_desc* meshes, int32_t n_meshes, const int32_t* view_mesh,
                                           const float* views, int32_t n_views, const int32_t* geometry,
                                           const int64_t* out_offsets, float* out_rgba, uint8_t* out_rgb_u8,
                                           float* out_depth, uint8_t* out_depth_nz, const int64_t* out_bytes,
                                           const int32_t* view_scene, int32_t r_grow, uint8_t* out_occluder,
                                           int64_t occluder_bytes, const int64_t* occluder_offsets, uint32_t* records,
                                           void* workspace, void* stream) {
  const RbSceneCall scene = {view_scene, r_grow, out_occluder, occluder_bytes, occluder_offsets};
  return rb_render(meshes, n_meshes, view_mesh, views, n_views, geometry, out_offsets, out_rgba, out_rgb_u8, out_depth,
                   out_depth_nz, out_bytes, records, workspace, stream, &scene);
}

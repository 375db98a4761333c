// Iso-surface of a scalar lattice as an indexed triangle mesh, and BOP's diameter of a point set
// (pxt_iso_surface_count / pxt_iso_surface_emit / pxt_iso_case_table / pxt_max_pairwise_distance, include/pixtrack_hip.h).
//
// The reference's users get a mesh out of instant-ngp (testbed.compute_and_save_marching_cubes_mesh,
// pixtrack/pose_trackers/pixloc_tracker_ycb.py:94); this is that step for the HIP renderer's density lattice
// (pixtrack_amd/mesh.py), restated in numpy by mesh.iso_surface_reference and held to it bit for bit.
//
// Scheme: marching tetrahedra on the Freudenthal (Kuhn) split.  A cell with base corner c is cut into the six tetrahedra
// {c, c + e_a, c + e_a + e_b, c + (1,1,1)}, one per permutation (a, b, .) of the axes in the order of
// itertools.permutations; all six share the cell's main diagonal and neighbouring cells agree on every face diagonal, so
// the mesh is a closed oriented 2-manifold wherever the surface stays inside the lattice.  The 6 x 16 case table is
// computed by the compiler from the unit cube (make_iso_table below); nothing in it was typed in.
//
// Numbering (what makes the output a pure function of the input):
//  * point p = (z * ny + y) * nx + x; inside when v >= iso (a NaN is outside).
//  * a point owns up to seven edges, E0 +x, E1 +y, E2 +z, E3 +x+y, E4 +y+z, E5 +x+z, E6 +x+y+z; an edge exists when its
//    far end is in the lattice and carries a vertex when its ends differ in inside-ness.  Vertex id = rank of
//    (p, edge type) among the vertex-carrying edges.
//  * triangles by cell (= base point p), then tetrahedron, then triangle within the case.
//
// Launches
//  1. iso_count_kernel, one thread per lattice point: its cell's eight corners (itself and the far ends of its seven
//     edges; the +x neighbours come from the next lane, not from memory) -> edge mask, vertex and triangle counts ->
//     exclusive scan inside the workgroup (wave shuffles, the four waves through LDS).  One record per point: local
//     vertex prefix | local triangle prefix << 11 | mask << 23 | (the cell has triangles) << 30; one (vertices,
//     triangles) total per workgroup of 256 points.
//  2. iso_scan_kernel: workgroups of 1024 threads turn 1024 workgroup totals each into exclusive offsets in place and
//     leave their own total one level up; iso_scan_top_kernel, ONE workgroup, does the same to those (at most 512) and
//     writes the grand totals to counts[0..1].
//  3. iso_emit_kernel (after the caller has read the counts and allocated), one thread per lattice point again: a point
//     whose record holds neither an edge nor a triangle reads nothing else; the others write the vertices of their own
//     edges and their cell's triangles.  A vertex owned by another corner q has the id
//     top[q >> 18] + offset[q >> 8] + prefix[q] + popcount(mask[q] & below(edge type)).
// No atomics anywhere; a float is never summed across threads.
//
// This file is compiled with -ffp-contract=off (pixtrack_amd/_build.py EXTRA): a vertex is
// origin + ((x, y, z) + t * d) * spacing with every product and sum rounded on its own, as numpy does it.
#include "pxt_common.h"

#include <algorithm>

namespace pxt {
namespace {

// ---- the case table, derived at compile time ------------------------------------------------------------------------
// entry[t][code][0] = number of triangles, [1 + 3 i + j] = vertex j of triangle i as (owner corner << 3) | edge type,
// the owner corner being dx | dy << 1 | dz << 2 inside the cell; unused slots are -1.  code bit i = tet corner i inside.
struct IsoTable {
  int8_t e[6][16][8];
};

constexpr int kIsoPerm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
// corner-bit difference (dx | dy << 1 | dz << 2) of an edge's ends -> edge type E0..E6
constexpr int kIsoTypeOfDiff[8] = {-1, 0, 1, 3, 2, 5, 4, 6};
// edge type -> corner bits of its far end
constexpr int kIsoFarCorner[7] = {1, 2, 4, 3, 6, 5, 7};

constexpr IsoTable make_iso_table() {
  IsoTable T{};
  for (int t = 0; t < 6; ++t) {
    const int a = kIsoPerm[t][0], b = kIsoPerm[t][1];
    const int corner[4] = {0, 1 << a, (1 << a) | (1 << b), 7};
    for (int code = 0; code < 16; ++code) {
      for (int k = 0; k < 8; ++k) T.e[t][code][k] = -1;
      int ins[4] = {0, 0, 0, 0}, outs[4] = {0, 0, 0, 0}, nin = 0, nout = 0;
      for (int i = 0; i < 4; ++i) {
        if ((code >> i) & 1) ins[nin++] = i; else outs[nout++] = i;
      }
      // the triangles' vertices as pairs of tet-local corners (inside corner, outside corner)
      int pi[6] = {0, 0, 0, 0, 0, 0}, po[6] = {0, 0, 0, 0, 0, 0}, ntri = 0;
      if (nin == 1) {
        for (int j = 0; j < 3; ++j) { pi[j] = ins[0]; po[j] = outs[j]; }
        ntri = 1;
      } else if (nin == 3) {
        for (int j = 0; j < 3; ++j) { pi[j] = ins[j]; po[j] = outs[0]; }
        ntri = 1;
      } else if (nin == 2) {  // quad cycle ac, ad, bd, bc -> (ac, ad, bd), (ac, bd, bc)
        const int A = ins[0], B = ins[1], Cc = outs[0], D = outs[1];
        pi[0] = A; po[0] = Cc; pi[1] = A; po[1] = D; pi[2] = B; po[2] = D;
        pi[3] = A; po[3] = Cc; pi[4] = B; po[4] = D; pi[5] = B; po[5] = Cc;
        ntri = 2;
      }
      T.e[t][code][0] = (int8_t)ntri;
      if (ntri == 0) continue;
      // centroid(outside) - centroid(inside), scaled by nin * nout
      int dir[3] = {0, 0, 0};
      for (int ax = 0; ax < 3; ++ax) {
        int so = 0, si = 0;
        for (int i = 0; i < nout; ++i) so += (corner[outs[i]] >> ax) & 1;
        for (int i = 0; i < nin; ++i) si += (corner[ins[i]] >> ax) & 1;
        dir[ax] = so * nin - si * nout;
      }
      for (int tri = 0; tri < ntri; ++tri) {
        int ref[3] = {0, 0, 0}, mid[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
        for (int j = 0; j < 3; ++j) {
          const int u = pi[3 * tri + j], w = po[3 * tri + j];
          const int lo = u < w ? u : w, hi = u < w ? w : u;  // the tet's corners are a chain: lo's bits are in hi's
          ref[j] = (corner[lo] << 3) | kIsoTypeOfDiff[corner[lo] ^ corner[hi]];
          for (int ax = 0; ax < 3; ++ax) mid[j][ax] = ((corner[lo] >> ax) & 1) + ((corner[hi] >> ax) & 1);  // 2 x midpoint
        }
        int u3[3] = {0, 0, 0}, v3[3] = {0, 0, 0};
        for (int ax = 0; ax < 3; ++ax) { u3[ax] = mid[1][ax] - mid[0][ax]; v3[ax] = mid[2][ax] - mid[0][ax]; }
        const int nx = u3[1] * v3[2] - u3[2] * v3[1], ny = u3[2] * v3[0] - u3[0] * v3[2], nz = u3[0] * v3[1] - u3[1] * v3[0];
        if (nx * dir[0] + ny * dir[1] + nz * dir[2] < 0) { const int s = ref[1]; ref[1] = ref[2]; ref[2] = s; }
        for (int j = 0; j < 3; ++j) T.e[t][code][1 + 3 * tri + j] = (int8_t)ref[j];
      }
    }
  }
  return T;
}

constexpr IsoTable kIsoTableHost = make_iso_table();
__device__ const IsoTable kIsoTableDev = make_iso_table();

// ---- the extractor ---------------------------------------------------------------------------------------------------
constexpr int kIsoBlock = 256;
constexpr int kIsoWaves = kIsoBlock / PXT_WAVE;
constexpr int kIsoScanBlock = 1024;
constexpr int64_t kIsoMaxPoints = (int64_t)1 << 27;  // 7 * 2^27 vertices and 12 * 2^27 triangles both fit in int32
static_assert(kIsoBlock * 7 < (1 << 11) && kIsoBlock * 12 < (1 << 12), "the point record's prefix fields");

struct IsoGrid {
  int nx, ny, nz, n;  // n = nx * ny * nz
  float iso;
  float origin[3], spacing[3];
  double inv_nx, inv_ny;  // 1 / nx, 1 / ny: iso_coords divides through them
};

// p -> (x, y, z).  floor(a / d) as a double product with one correction step: a, d < 2^27, so the product is within
// 2^-25 / d of the quotient and the estimate is off by at most one.
__device__ __forceinline__ int iso_div(int a, int d, double inv, int* rem) {
  int q = (int)((double)a * inv);
  int r = a - q * d;
  if (r >= d) { ++q; r -= d; }
  if (r < 0) { --q; r += d; }
  *rem = r;
  return q;
}
__device__ __forceinline__ void iso_coords(const IsoGrid& g, int p, int* x, int* y, int* z) {
  const int yz = iso_div(p, g.nx, g.inv_nx, x);
  *z = iso_div(yz, g.ny, g.inv_ny, y);
}

// The eight corners of point p's cell: existence, value (0 where the corner is outside the lattice), inside-ness.
struct IsoCorners {
  float v[8];
  unsigned exists, inside;  // bit k = corner dx | dy << 1 | dz << 2
};

__device__ __forceinline__ IsoCorners iso_load_corners(const float* __restrict__ values, const IsoGrid& g, int p, int x,
                                                       int y, int z) {
  IsoCorners c;
  c.exists = 0;
  c.inside = 0;
  const int sy = g.nx, sz = g.nx * g.ny;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int dx = k & 1, dy = (k >> 1) & 1, dz = k >> 2;
    const bool ex = (x + dx < g.nx) && (y + dy < g.ny) && (z + dz < g.nz);
    float v = 0.f;
    if (ex) v = values[(size_t)p + dx + dy * sy + dz * sz];
    c.v[k] = v;
    c.exists |= (unsigned)ex << k;
    c.inside |= (unsigned)(ex && v >= g.iso) << k;  // false for a NaN
  }
  return c;
}

// The same for a whole wave of consecutive points (every lane calls it; p >= n owns nothing): the four corners with
// dx = 0 are loaded, the four with dx = 1 are the next lane's - where x + 1 < nx, point p + 1 lies in the same row and
// is that corner - and only the wave's last lane loads them.
__device__ __forceinline__ IsoCorners iso_load_corners_wave(const float* __restrict__ values, const IsoGrid& g, int p,
                                                            int x, int y, int z) {
  IsoCorners c;
  c.exists = 0;
  c.inside = 0;
  const int sy = g.nx, sz = g.nx * g.ny;
  const bool last_lane = (threadIdx.x & (PXT_WAVE - 1)) == PXT_WAVE - 1;
#pragma unroll
  for (int k = 0; k < 8; k += 2) {
    const int dy = (k >> 1) & 1, dz = k >> 2;
    const bool ex0 = (p < g.n) && (y + dy < g.ny) && (z + dz < g.nz);
    const bool ex1 = ex0 && (x + 1 < g.nx);
    float v0 = 0.f;
    if (ex0) v0 = values[(size_t)p + dy * sy + dz * sz];
    float v1 = __shfl_down(v0, 1, PXT_WAVE);
    if (last_lane && ex1) v1 = values[(size_t)p + 1 + dy * sy + dz * sz];
    v1 = ex1 ? v1 : 0.f;
    c.v[k] = v0;
    c.v[k + 1] = v1;
    c.exists |= ((unsigned)ex0 << k) | ((unsigned)ex1 << (k + 1));
    c.inside |= ((unsigned)(ex0 && v0 >= g.iso) << k) | ((unsigned)(ex1 && v1 >= g.iso) << (k + 1));
  }
  return c;
}

__device__ __forceinline__ unsigned iso_edge_mask(const IsoCorners& c) {
  unsigned mask = 0;
  const unsigned in0 = c.inside & 1u;
#pragma unroll
  for (int e = 0; e < 7; ++e) {
    const int k = kIsoFarCorner[e];
    mask |= (((c.exists >> k) & 1u) & (((c.inside >> k) & 1u) ^ in0)) << e;
  }
  return mask;
}

// code of tetrahedron t: bit i = tet corner i inside
__device__ __forceinline__ unsigned iso_tet_code(unsigned inside, int t) {
  const int a = kIsoPerm[t][0], b = kIsoPerm[t][1];
  const int c1 = 1 << a, c2 = c1 | (1 << b);
  return (inside & 1u) | (((inside >> c1) & 1u) << 1) | (((inside >> c2) & 1u) << 2) | (((inside >> 7) & 1u) << 3);
}

__device__ __forceinline__ unsigned iso_triangle_count(unsigned inside) {
  unsigned n = 0;
#pragma unroll
  for (int t = 0; t < 6; ++t) {
    const unsigned pc = __popc(iso_tet_code(inside, t));
    n += (pc == 2u) ? 2u : ((pc == 1u || pc == 3u) ? 1u : 0u);
  }
  return n;
}

// Exclusive scan of one unsigned per thread over a workgroup of NW waves (wave shuffles, then the waves' totals through
// LDS in wave order); -> the thread's exclusive prefix, *total = the workgroup's sum.  `wave_tot` holds NW words.
template <int NW>
__device__ __forceinline__ unsigned iso_block_scan(unsigned v, unsigned* wave_tot, unsigned* total) {
  const int lane = threadIdx.x & (PXT_WAVE - 1), w = threadIdx.x / PXT_WAVE;
  unsigned inc = v;
#pragma unroll
  for (int m = 1; m < PXT_WAVE; m <<= 1) {
    const unsigned o = (unsigned)__shfl_up((int)inc, m, PXT_WAVE);
    if (lane >= m) inc += o;
  }
  __syncthreads();  // wave_tot may still be read from the previous scan
  if (lane == PXT_WAVE - 1) wave_tot[w] = inc;
  __syncthreads();
  unsigned before = 0, all = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const unsigned s = wave_tot[i];
    before += (i < w) ? s : 0u;
    all += s;
  }
  *total = all;
  return before + inc - v;
}

__global__ __launch_bounds__(kIsoBlock) void iso_count_kernel(const float* __restrict__ values, const IsoGrid g,
                                                              unsigned* __restrict__ recs, uint2* __restrict__ sums) {
  __shared__ unsigned wave_tot[kIsoWaves];
  const int p = blockIdx.x * kIsoBlock + threadIdx.x;
  int x, y, z;
  iso_coords(g, min(p, g.n - 1), &x, &y, &z);
  const IsoCorners c = iso_load_corners_wave(values, g, p, x, y, z);  // p >= n: nothing exists
  unsigned mask = 0, nt = 0;
  if (c.inside != 0u && c.inside != c.exists) {  // else no edge has a vertex: whole waves skip this in empty space
    mask = iso_edge_mask(c);
    if (c.exists == 0xffu) nt = iso_triangle_count(c.inside);
  }
  const unsigned nv = __popc(mask);
  unsigned total;
  const unsigned pre = iso_block_scan<kIsoWaves>(nv | (nt << 16), wave_tot, &total);  // 256 * 12 < 2^16: no carry across
  if (p < g.n) recs[p] = (pre & 0xffffu) | ((pre >> 16) << 11) | (mask << 23) | ((unsigned)(nt != 0u) << 30);
  if (threadIdx.x == 0) sums[blockIdx.x] = make_uint2(total & 0xffffu, total >> 16);
}

// Level 1: 1024 workgroup totals per workgroup -> exclusive offsets in place, the workgroup's own total to `top`.
__global__ __launch_bounds__(kIsoScanBlock) void iso_scan_kernel(uint2* __restrict__ sums, const int n_blocks,
                                                                 uint2* __restrict__ top) {
  __shared__ unsigned wave_tot[kIsoScanBlock / PXT_WAVE];
  const int i = blockIdx.x * kIsoScanBlock + (int)threadIdx.x;
  uint2 s = make_uint2(0u, 0u);
  if (i < n_blocks) s = sums[i];
  unsigned tot_v, tot_t;
  const unsigned pv = iso_block_scan<kIsoScanBlock / PXT_WAVE>(s.x, wave_tot, &tot_v);
  const unsigned pt = iso_block_scan<kIsoScanBlock / PXT_WAVE>(s.y, wave_tot, &tot_t);
  if (i < n_blocks) sums[i] = make_uint2(pv, pt);
  if (threadIdx.x == 0) top[blockIdx.x] = make_uint2(tot_v, tot_t);
}

// Level 2: ONE workgroup over the (at most 512) level-1 totals; the grand totals to counts.
__global__ __launch_bounds__(kIsoScanBlock) void iso_scan_top_kernel(uint2* __restrict__ top, const int n_top,
                                                                     int* __restrict__ counts) {
  __shared__ unsigned wave_tot[kIsoScanBlock / PXT_WAVE];
  const int i = (int)threadIdx.x;
  uint2 s = make_uint2(0u, 0u);
  if (i < n_top) s = top[i];
  unsigned tot_v, tot_t;
  const unsigned pv = iso_block_scan<kIsoScanBlock / PXT_WAVE>(s.x, wave_tot, &tot_v);
  const unsigned pt = iso_block_scan<kIsoScanBlock / PXT_WAVE>(s.y, wave_tot, &tot_t);
  if (i < n_top) top[i] = make_uint2(pv, pt);
  if (threadIdx.x == 0) {
    counts[0] = (int)tot_v;
    counts[1] = (int)tot_t;
  }
}

// Central-difference gradient of the lattice at (x, y, z), one-sided at the border, 0 along an axis of extent 1.
__device__ __forceinline__ void iso_gradient(const float* __restrict__ values, const IsoGrid& g, int x, int y, int z,
                                             float* out) {
  const int c[3] = {x, y, z}, ext[3] = {g.nx, g.ny, g.nz}, stride[3] = {1, g.nx, g.nx * g.ny};
  const size_t p = ((size_t)z * g.ny + y) * g.nx + x;
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    const int hi = min(c[ax] + 1, ext[ax] - 1), lo = max(c[ax] - 1, 0);
    float d = 0.f;
    if (hi > lo) {
      const float a = values[p + (size_t)(hi - c[ax]) * stride[ax]], b = values[p - (size_t)(c[ax] - lo) * stride[ax]];
      d = (a - b) / ((float)(hi - lo) * g.spacing[ax]);
    }
    out[ax] = d;
  }
}

__global__ __launch_bounds__(kIsoBlock) void iso_emit_kernel(const float* __restrict__ values, const IsoGrid g,
                                                             const unsigned* __restrict__ recs,
                                                             const uint2* __restrict__ offs,
                                                             const uint2* __restrict__ top, float* __restrict__ vertices,
                                                             float* __restrict__ normals, int* __restrict__ triangles,
                                                             const unsigned cap_v, const unsigned cap_t) {
  __shared__ int8_t tab[6 * 16 * 8];
  __shared__ unsigned cbase[8][kIsoBlock], cmask[8][kIsoBlock];
  const int tid = threadIdx.x;
  for (int i = tid; i < 6 * 16 * 8; i += kIsoBlock) tab[i] = (&kIsoTableDev.e[0][0][0])[i];
  __syncthreads();
  const int p = blockIdx.x * kIsoBlock + tid;
  if (p >= g.n) return;  // no barrier below
  const unsigned rec = recs[p];
  if ((rec >> 23) == 0u) return;  // neither an edge with a vertex nor a triangle: most of the lattice
  int x, y, z;
  iso_coords(g, p, &x, &y, &z);
  const IsoCorners c = iso_load_corners(values, g, p, x, y, z);
  const uint2 o1 = offs[blockIdx.x], o2 = top[blockIdx.x / kIsoScanBlock];
  const uint2 off = make_uint2(o1.x + o2.x, o1.y + o2.y);
  const unsigned mask = (rec >> 23) & 0x7fu;

  // the vertices of this point's own edges
  if (mask) {
    unsigned vid = off.x + (rec & 0x7ffu);
    const float fx = (float)x, fy = (float)y, fz = (float)z;
    float ga[3] = {0.f, 0.f, 0.f};
    if (normals) iso_gradient(values, g, x, y, z, ga);
#pragma unroll
    for (int e = 0; e < 7; ++e) {
      if (!((mask >> e) & 1u)) continue;
      const int k = kIsoFarCorner[e];
      const int dx = k & 1, dy = (k >> 1) & 1, dz = k >> 2;
      float t = (g.iso - c.v[0]) / (c.v[k] - c.v[0]);
      t = (t != t) ? 0.5f : fminf(fmaxf(t, 0.f), 1.f);
      if (vid < cap_v) {
        float* o = vertices + (size_t)vid * 3;
        o[0] = g.origin[0] + (fx + t * (float)dx) * g.spacing[0];
        o[1] = g.origin[1] + (fy + t * (float)dy) * g.spacing[1];
        o[2] = g.origin[2] + (fz + t * (float)dz) * g.spacing[2];
        if (normals) {
          float gb[3];
          iso_gradient(values, g, x + dx, y + dy, z + dz, gb);
          float n3[3];
#pragma unroll
          for (int ax = 0; ax < 3; ++ax) n3[ax] = -(ga[ax] + t * (gb[ax] - ga[ax]));
          const float len = sqrtf((n3[0] * n3[0] + n3[1] * n3[1]) + n3[2] * n3[2]);
          const bool ok = len > 0.f && len <= 3.402823466e+38f;  // false for a NaN
          float* no = normals + (size_t)vid * 3;
#pragma unroll
          for (int ax = 0; ax < 3; ++ax) no[ax] = ok ? n3[ax] / len : 0.f;
        }
      }
      ++vid;
    }
  }

  // this cell's triangles
  if (!((rec >> 30) & 1u)) return;  // set only for a whole cell that holds triangles
  const int sy = g.nx, sz = g.nx * g.ny;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int q = p + (k & 1) + ((k >> 1) & 1) * sy + (k >> 2) * sz;  // < n: the corner exists
    const unsigned rq = k ? recs[q] : rec;
    const int bq = q / kIsoBlock;
    cbase[k][tid] = top[bq / kIsoScanBlock].x + offs[bq].x + (rq & 0x7ffu);
    cmask[k][tid] = (rq >> 23) & 0x7fu;
  }
  unsigned tri = off.y + ((rec >> 11) & 0xfffu);
  unsigned codes = 0;  // four bits per tetrahedron
#pragma unroll
  for (int t = 0; t < 6; ++t) codes |= iso_tet_code(c.inside, t) << (4 * t);
#pragma unroll 1
  for (int t = 0; t < 6; ++t) {
    const int8_t* entry = tab + (t * 16 + (int)((codes >> (4 * t)) & 15u)) * 8;
    const int n = entry[0];
    for (int i = 0; i < n; ++i, ++tri) {
      if (tri >= cap_t) continue;
      int* o = triangles + (size_t)tri * 3;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int ref = entry[1 + 3 * i + j], k = ref >> 3, e = ref & 7;
        o[j] = (int)(cbase[k][tid] + __popc(cmask[k][tid] & ((1u << e) - 1u)));
      }
    }
  }
}

int iso_fill_grid(const pxt_iso_grid* gh, IsoGrid* g) {
  if (!gh || gh->nx < 1 || gh->ny < 1 || gh->nz < 1) return PXT_E_ARG;
  const int64_t n = (int64_t)gh->nx * gh->ny * gh->nz;
  if (n > kIsoMaxPoints) return PXT_E_ARG;
  g->nx = gh->nx; g->ny = gh->ny; g->nz = gh->nz; g->n = (int)n;
  g->iso = gh->iso;
  for (int i = 0; i < 3; ++i) { g->origin[i] = gh->origin[i]; g->spacing[i] = gh->spacing[i]; }
  g->inv_nx = 1.0 / (double)gh->nx;
  g->inv_ny = 1.0 / (double)gh->ny;
  return PXT_OK;
}

int iso_blocks(int n) { return (n + kIsoBlock - 1) / kIsoBlock; }
int iso_top_blocks(int n) { return (iso_blocks(n) + kIsoScanBlock - 1) / kIsoScanBlock; }  // <= 512
int64_t iso_rec_bytes(int n) { return ((int64_t)n * 4 + 15) / 16 * 16; }  // the workgroup totals behind it stay aligned
static_assert(kIsoMaxPoints / kIsoBlock / kIsoScanBlock <= kIsoScanBlock, "the top level is one workgroup");

// ---- the diameter ----------------------------------------------------------------------------------------------------
// grid = (ceil(n / 1024), S) workgroups of 256 threads.  A lane owns kMdQ = 4 query points in registers; the workgroups
// (b, 0 .. S-1) share out the target tiles b, b + 1, ... (LDS tiles of 1024, SoA, a broadcast read per step as in
// pxt_pose_errors), starting at the queries' OWN tile: the pairs with a target in an earlier tile belong to that tile's
// workgroups (d(i, j) == d(j, i) bit for bit).  S (md_splits) keeps a few thousand workgroups in flight for any n.  Squared
// distances are compared (fmaf chain; sqrtf is monotone and correctly rounded, so the sqrtf of the largest square is the
// largest distance); a strict `>` while j ascends keeps a query's lowest j.  A candidate is (d^2, min(i, j), max(i, j));
// candidates fold by (larger d^2, then lower i, then lower j): lanes by butterfly, waves through LDS, workgroups by a
// second launch.
constexpr int kMdBlock = 256;
constexpr int kMdWaves = kMdBlock / PXT_WAVE;
constexpr int kMdQ = 4;
constexpr int kMdTile = kMdBlock * kMdQ;  // queries per workgroup == targets per tile
constexpr int kMdUnroll = 8;
constexpr int kMdMaxPoints = 1 << 22;
static_assert(kMdTile % kMdUnroll == 0 && kMdUnroll % 4 == 0, "tile unrolling");

struct MdBest {
  float d2;
  int i, j;
};

__device__ __forceinline__ bool md_better(const MdBest& a, const MdBest& b) {  // a before b?
  return a.d2 > b.d2 || (a.d2 == b.d2 && (a.i < b.i || (a.i == b.i && a.j < b.j)));
}

__device__ __forceinline__ MdBest md_wave_best(MdBest v) {
#pragma unroll
  for (int m = 1; m < PXT_WAVE; m <<= 1) {
    MdBest o;
    o.d2 = __shfl_xor(v.d2, m, PXT_WAVE);
    o.i = __shfl_xor(v.i, m, PXT_WAVE);
    o.j = __shfl_xor(v.j, m, PXT_WAVE);
    if (md_better(o, v)) v = o;
  }
  return v;
}

__global__ __launch_bounds__(kMdBlock) void max_distance_kernel(const float* __restrict__ points, const int n,
                                                                MdBest* __restrict__ partials) {
  __shared__ __attribute__((aligned(16))) float tile[3][kMdTile];
  __shared__ MdBest red[kMdWaves];
  const int tid = threadIdx.x, b = blockIdx.x, n_tiles = gridDim.x, first = b + (int)blockIdx.y;
  float qx[kMdQ], qy[kMdQ], qz[kMdQ], best[kMdQ];
  int bj[kMdQ];
#pragma unroll
  for (int q = 0; q < kMdQ; ++q) {
    const int i = b * kMdTile + q * kMdBlock + tid;
    const size_t o = 3 * (size_t)min(i, n - 1);  // a query past n repeats the last point and is discarded
    qx[q] = points[o];
    qy[q] = points[o + 1];
    qz[q] = points[o + 2];
    best[q] = -1.f;
    bj[q] = 0;
  }
#pragma unroll 1
  for (int t = first; t < n_tiles; t += (int)gridDim.y) {
    const int t0 = t * kMdTile;
    const int live = min(kMdTile, n - t0);
    const int n_pad = (live + kMdUnroll - 1) / kMdUnroll * kMdUnroll;  // <= kMdTile
    if (t != first) __syncthreads();  // the previous tile has been read by every wave
#pragma unroll 1
    for (int k = tid; k < n_pad; k += kMdBlock) {
      const size_t o = 3 * (size_t)min(t0 + k, n - 1);  // the slots past n repeat the last point: never a strict gain
      tile[0][k] = points[o];
      tile[1][k] = points[o + 1];
      tile[2][k] = points[o + 2];
    }
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < n_pad; k += kMdUnroll) {
#pragma unroll
      for (int u = 0; u < kMdUnroll; u += 4) {
        const float4 X = *(const float4*)&tile[0][k + u], Y = *(const float4*)&tile[1][k + u],
                     Z = *(const float4*)&tile[2][k + u];
        const float px[4] = {X.x, X.y, X.z, X.w}, py[4] = {Y.x, Y.y, Y.z, Y.w}, pz[4] = {Z.x, Z.y, Z.z, Z.w};
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const int j = t0 + k + u + jj;
#pragma unroll
          for (int q = 0; q < kMdQ; ++q) {
            const float dx = px[jj] - qx[q], dy = py[jj] - qy[q], dz = pz[jj] - qz[q];
            const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
            const bool gain = d2 > best[q];  // false for a NaN
            best[q] = gain ? d2 : best[q];
            bj[q] = gain ? j : bj[q];
          }
        }
      }
    }
  }
  MdBest v;
  v.d2 = -1.f; v.i = 0x7fffffff; v.j = 0x7fffffff;
#pragma unroll
  for (int q = 0; q < kMdQ; ++q) {
    const int i = b * kMdTile + q * kMdBlock + tid;
    MdBest cnd;
    cnd.d2 = best[q];
    cnd.i = min(i, bj[q]);
    cnd.j = max(i, bj[q]);
    if (i < n && md_better(cnd, v)) v = cnd;
  }
  v = md_wave_best(v);
  if ((tid & (PXT_WAVE - 1)) == 0) red[tid / PXT_WAVE] = v;
  __syncthreads();
  if (tid == 0) {
    MdBest r = red[0];
    for (int w = 1; w < kMdWaves; ++w)
      if (md_better(red[w], r)) r = red[w];
    partials[blockIdx.y * gridDim.x + b] = r;
  }
}

// One wave: the workgroups' candidates, then the record {bits of float d, i, j, 1}.
__global__ __launch_bounds__(PXT_WAVE) void max_distance_fold_kernel(const MdBest* __restrict__ partials,
                                                                     const int n_blocks, int* __restrict__ out) {
  MdBest v;
  v.d2 = -1.f; v.i = 0x7fffffff; v.j = 0x7fffffff;
  for (int b = threadIdx.x; b < n_blocks; b += PXT_WAVE) {
    const MdBest o = partials[b];
    if (md_better(o, v)) v = o;
  }
  v = md_wave_best(v);
  if (threadIdx.x == 0) {
    const bool found = v.d2 >= 0.f;  // every point holds a NaN: no pair compares
    out[0] = __builtin_bit_cast(int, found ? sqrtf(v.d2) : __builtin_nanf(""));
    out[1] = found ? v.i : -1;
    out[2] = found ? v.j : -1;
    out[3] = 1;
  }
}

int md_blocks(int n) { return (n + kMdTile - 1) / kMdTile; }
int md_splits(int n) { const int t = md_blocks(n); return std::max(1, std::min(t, (4096 + t - 1) / t)); }

}  // namespace
}  // namespace pxt

using namespace pxt;

extern "C" int pxt_iso_case_table(int32_t* out_host) {
  if (!out_host) return PXT_E_ARG;
  for (int t = 0; t < 6; ++t)
    for (int code = 0; code < 16; ++code)
      for (int k = 0; k < 7; ++k) out_host[(t * 16 + code) * 7 + k] = kIsoTableHost.e[t][code][k];
  return PXT_OK;
}

extern "C" int64_t pxt_iso_surface_workspace_bytes(int32_t nx, int32_t ny, int32_t nz) {
  pxt_iso_grid gh = {nx, ny, nz, 0.f, {0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}};
  IsoGrid g;
  if (iso_fill_grid(&gh, &g) != PXT_OK) return PXT_E_ARG;
  return iso_rec_bytes(g.n) + ((int64_t)iso_blocks(g.n) + iso_top_blocks(g.n)) * (int64_t)sizeof(uint2);
}

extern "C" int pxt_iso_surface_count(const float* values, const pxt_iso_grid* grid_host, void* workspace,
                                     int32_t* counts, void* stream) {
  IsoGrid g;
  if (iso_fill_grid(grid_host, &g) != PXT_OK) return PXT_E_ARG;
  if (!values || !workspace || !counts) return PXT_E_ARG;
  if (((uintptr_t)values % 4) != 0 || ((uintptr_t)workspace % 16) != 0 || ((uintptr_t)counts % 4) != 0) return PXT_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  unsigned* recs = (unsigned*)workspace;
  uint2* sums = (uint2*)((char*)workspace + iso_rec_bytes(g.n));
  const int n_blocks = iso_blocks(g.n), n_top = iso_top_blocks(g.n);
  uint2* top = sums + n_blocks;
  hipLaunchKernelGGL(iso_count_kernel, dim3(n_blocks), dim3(kIsoBlock), 0, s, values, g, recs, sums);
  PXT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(iso_scan_kernel, dim3(n_top), dim3(kIsoScanBlock), 0, s, sums, n_blocks, top);
  PXT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(iso_scan_top_kernel, dim3(1), dim3(kIsoScanBlock), 0, s, top, n_top, (int*)counts);
  PXT_HIP_CHECK(hipGetLastError());
  return PXT_OK;
}

extern "C" int pxt_iso_surface_emit(const float* values, const pxt_iso_grid* grid_host, const void* workspace,
                                    float* vertices, int32_t n_vertices, float* normals, int32_t* triangles,
                                    int32_t n_triangles, void* stream) {
  IsoGrid g;
  if (iso_fill_grid(grid_host, &g) != PXT_OK) return PXT_E_ARG;
  if (!values || !workspace || n_vertices < 0 || n_triangles < 0) return PXT_E_ARG;
  if ((n_vertices > 0 && !vertices) || (n_triangles > 0 && !triangles)) return PXT_E_ARG;
  if (((uintptr_t)values % 4) != 0 || ((uintptr_t)workspace % 16) != 0 || ((uintptr_t)vertices % 4) != 0 ||
      ((uintptr_t)normals % 4) != 0 || ((uintptr_t)triangles % 4) != 0)
    return PXT_E_ARG;
  if (n_vertices == 0 && n_triangles == 0) return PXT_OK;  // nothing to write
  const unsigned* recs = (const unsigned*)workspace;
  const uint2* offs = (const uint2*)((const char*)workspace + iso_rec_bytes(g.n));
  hipLaunchKernelGGL(iso_emit_kernel, dim3(iso_blocks(g.n)), dim3(kIsoBlock), 0, (hipStream_t)stream, values, g, recs,
                     offs, offs + iso_blocks(g.n), vertices, n_vertices > 0 ? normals : nullptr, (int*)triangles, (unsigned)n_vertices,
                     (unsigned)n_triangles);
  PXT_HIP_CHECK(hipGetLastError());
  return PXT_OK;
}

extern "C" int64_t pxt_max_pairwise_distance_workspace_bytes(int32_t n_points) {
  if (n_points < 1 || n_points > kMdMaxPoints) return PXT_E_ARG;
  return (int64_t)md_blocks(n_points) * md_splits(n_points) * (int64_t)sizeof(MdBest);
}

extern "C" int pxt_max_pairwise_distance(const float* points, int32_t n_points, void* workspace, int32_t* out,
                                         void* stream) {
  if (!points || !workspace || !out || n_points < 1 || n_points > kMdMaxPoints) return PXT_E_ARG;
  if (((uintptr_t)points % 4) != 0 || ((uintptr_t)workspace % 4) != 0 || ((uintptr_t)out % 4) != 0) return PXT_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int n_tiles = md_blocks(n_points), n_splits = md_splits(n_points), n_blocks = n_tiles * n_splits;
  MdBest* partials = (MdBest*)workspace;
  hipLaunchKernelGGL(max_distance_kernel, dim3(n_tiles, n_splits), dim3(kMdBlock), 0, s, points, (int)n_points, partials);
  PXT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(max_distance_fold_kernel, dim3(1), dim3(PXT_WAVE), 0, s, (const MdBest*)partials, n_blocks,
                     (int*)out);
  PXT_HIP_CHECK(hipGetLastError());
  return PXT_OK;
}

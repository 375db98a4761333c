// Occlusion handling from the frame's sensor depth image (opt-in; pxt_occlusion_mask and pxt_points_visible,
// include/pixtrack_hip.h; no reference counterpart: the reference tracker is monocular).
//
// pxt_occlusion_mask: which pixels of the frame's mask show something that stands IN FRONT of the tracked object.  The
// Depth render of the mask view says how far the object is at a pixel, the sensor image how far the nearest surface is;
// where the sensor is closer by more than a tolerance the pixel shows an occluder.  That plane is opened (specks go) and
// grown (the occluder's rim goes too) with box elements and taken out of the frame's plain mask.
//
// Arithmetic (all fp32; every step a single IEEE operation through __fdiv_rn / __fmul_rn / __fsub_rn, which
// -ffp-contract cannot fuse: the file needs no flag of its own, and the numpy restatement is exact):
//  * sil = v.w >= min_alpha && v.x > 0;  q = v.x / v.w;  raw = sensor count at (x + shift_x, y + shift_y), 0 when that
//    position is outside the image (tested before the load: no address outside the H x W counts is formed);
//  * d_s = float(raw) * sensor_q;  O = sil && raw != 0 && (q - d_s > delta_q)   (false for a NaN);
//  * E = erosion of O, (2 r_open + 1)^2 box, pixels outside the image ignored;  G = dilation of E, (2 r_grow + 1)^2 box,
//    inside the image;  mask_out = (mask_in != 0) && !G;  occluder = G.
//
// Mapping (depth_mask_bits_kernel's, pxt_image.hip): one workgroup of 256 threads per 64 x 16 tile, fed by the band of
// 16 + 2 R rows x 64 + 2 R columns around it (R = r_open + r_grow <= 16).
//  * A band row is one 128-bit word (bit j = column x0 - 32 + j), built from two wave ballots of O; the float4 and the
//    sensor count of every band pixel are loaded once per tile, three rows (six 16-byte and six 2-byte loads per lane)
//    in flight per wave trip.  The same ballots, restricted to the tile's own columns, count sil / measured / O - in
//    scalar registers.
//  * Erosion and dilation along x are shift-AND / shift-OR steps on the word, along y AND / OR over neighbouring rows'
//    words in LDS; one thread per row.  The counts of E, G and sil && G are population counts of the tile's 64-bit core.
//  * 16 rows x 64 bits -> bytes, four per thread, combined with four bytes of mask_in; mask counts by ballot.
//  * One partial of 8 words per workgroup in the workspace; a second launch of one wave folds them in a fixed order
//    (lane l takes blocks l, l + 64, ...; then the butterfly) and writes the 16-word record.  Integer sums only, no
//    atomics: the record depends on the call's own inputs, not on the launch geometry or on a neighbouring call.
//
// pxt_occlusion_mask_views: the same for up to 16 image pairs of different sizes in one chain of two launches - the tile
// above is a device function of a view (oc_tile), the views' tile grids are concatenated, and one wave per view folds
// (oc_fold); see occlusion_mask_views_kernel below.
//
// pxt_points_visible: one workgroup of 1024 threads; point n belongs to thread n % 1024.  transform_point and
// project_point (pxt_lm_point.h / pxt_common.h: the LM's own statement, distortion included), the nearest texel of
// (u, v) under the LM's addressing - texel k's centre is at coordinate k, so it is floor(u + 0.5), floor(v + 0.5); the
// centre tap of pxt_depth_refine's bilinear footprint has weight 1 exactly there - one byte of the occluder plane, one
// byte out.  The three counts by ballot + population count, folded over the 16 waves through LDS by index.
//
// pxt_mask_exclude: a mask minus an occluder plane that some other call made (pxt_mesh_render_scene_batch's: the other
// tracked objects of the image); see mask_exclude_kernel below.
#include "pxt_bitrow.h"
#include "pxt_common.h"
#include "pxt_lm_point.h"

namespace pxt {
namespace {

constexpr int kOcW = 64, kOcH = 16;                 // tile
constexpr int kOcMaxR = PXT_OCCLUSION_MAX_RADIUS;   // r_open + r_grow
constexpr int kOcBand = kOcH + 2 * kOcMaxR;         // staged rows at most
constexpr int kOcRows = 3;                          // band rows in flight per wave trip
constexpr int kOcPart = 8;                          // words per partial
constexpr int kOcRec = PXT_OCCLUSION_RECORD;
constexpr int64_t kOcMaxPixels = (int64_t)1 << 28;
constexpr int kOcMaxShift = 32767;
constexpr int kPvBlock = 1024;
constexpr int kPvMaxPoints = 1 << 24;
static_assert(kOcMaxR == 16 && kOcBand <= PXT_WAVE && kOcRec == 16, "band rows are served by one wave; record layout");

struct OcArgs {
  const float4* depth;      // [H][W]: .x = composited depth * depth_scale, .w = alpha
  const uint16_t* sensor;   // [H][W]
  const uint8_t* mask_in;   // [H][W]
  uint8_t* mask_out;        // [H][W]
  uint8_t* occluder;        // [H][W]
  uint32_t* partials;       // [n_blocks][kOcPart]
  int H, W, tiles_x, shift_x, shift_y, r_open, r_grow;
  float min_alpha, sensor_q, delta_q;
};

// One 64 x 16 tile of an image pair: tile `block` of the pair's own grid (row-major, a.tiles_x per row); its partial goes
// to a.partials[block].  The body of both occlusion_mask_kernel (block = blockIdx.x) and occlusion_mask_views_kernel
// (block = blockIdx.x minus the view's first tile): a view's bits are the single call's by construction.
__device__ __forceinline__ void oc_tile(const OcArgs& a, const int block) {
  __shared__ OcRow sA[kOcBand], sB[kOcBand];
  __shared__ unsigned long long sSil[kOcH];
  __shared__ uint32_t sWave[4][5];      // per wave: n_sil, n_measured, n_occluded, n_mask_in, n_mask_out
  __shared__ uint32_t sRow[3][kOcH];    // per tile row: n_opened, n_occluder, n_sil_occluder
  const int H = a.H, W = a.W, re = a.r_open, rd = a.r_grow;
  const int R = re + rd;                 // <= 16
  const int ah = kOcH + 2 * R;           // rows y0 - R .. y0 + kOcH + R - 1
  const int bx = block % a.tiles_x, by = block / a.tiles_x;
  const int x0 = bx * kOcW, y0 = by * kOcH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // band column c of a row sits in ballot c / 64 at bit c % 64; the tile's own columns are c = R .. R + 63
  const unsigned long long core0 = ~0ull << R, core1 = R ? ((1ull << R) - 1ull) : 0ull;
  uint32_t n_sil = 0, n_meas = 0, n_occ = 0;  // wave-uniform
  // ---- the O plane: kOcRows band rows per wave trip, all their loads ahead of the first ballot; outside the image O
  // is 1 (neutral for the erosion), sil and measured are 0
  for (int rb = wave; rb < ah; rb += 4 * kOcRows) {
    float qx[kOcRows][2], qw[kOcRows][2];
    uint32_t raw[kOcRows][2];
    bool inside[kOcRows][2];
#pragma unroll
    for (int k = 0; k < kOcRows; ++k) {
      const int r = rb + 4 * k, yy = y0 - R + r;
#pragma unroll
      for (int part = 0; part < 2; ++part) {
        const int c = part * 64 + lane, xx = x0 - R + c;
        inside[k][part] = r < ah && c < kOcW + 2 * R && yy >= 0 && yy < H && xx >= 0 && xx < W;
        qx[k][part] = 0.f;
        qw[k][part] = 0.f;
        raw[k][part] = 0u;
        if (inside[k][part]) {
          const float4 v = a.depth[(size_t)yy * W + xx];
          qx[k][part] = v.x;
          qw[k][part] = v.w;
          const int xs = xx + a.shift_x, ys = yy + a.shift_y;
          if (xs >= 0 && xs < W && ys >= 0 && ys < H) raw[k][part] = a.sensor[(size_t)ys * W + xs];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kOcRows; ++k) {
      const int r = rb + 4 * k;
      if (r >= ah) break;  // wave-uniform
      unsigned long long wo[2], ws[2], wm[2];
#pragma unroll
      for (int part = 0; part < 2; ++part) {
        const bool sil = inside[k][part] && qw[k][part] >= a.min_alpha && qx[k][part] > 0.f;
        const bool meas = sil && raw[k][part] != 0u;
        const float q = __fdiv_rn(qx[k][part], qw[k][part]);
        const float ds = __fmul_rn((float)raw[k][part], a.sensor_q);
        const bool occ = meas && (__fsub_rn(q, ds) > a.delta_q);
        ws[part] = __ballot(sil);
        wm[part] = __ballot(meas);
        wo[part] = __ballot(occ || !inside[k][part]);
      }
      if (r >= R && r < R + kOcH) {  // a row of the tile itself: its 64 own columns are counted here, once
        n_sil += (uint32_t)(__popcll(ws[0] & core0) + __popcll(ws[1] & core1));
        n_meas += (uint32_t)(__popcll(wm[0] & core0) + __popcll(wm[1] & core1));
        n_occ += (uint32_t)(__popcll(wo[0] & wm[0] & core0) + __popcll(wo[1] & wm[1] & core1));
      }
      if (lane == 0) {
        // column c sits at bit 32 - R + c; 16 <= 32 - R <= 32: the bits below are zero-filled, make them neutral too
        OcRow o = oc_shl(OcRow{wo[0], wo[1]}, 32 - R);
        o.lo |= (1ull << (32 - R)) - 1ull;
        sA[r] = o;
        if (r >= R && r < R + kOcH) sSil[r - R] = oc_core(oc_shl(OcRow{ws[0], ws[1]}, 32 - R));
      }
    }
  }
  if (lane == 0) {
    sWave[wave][0] = n_sil;
    sWave[wave][1] = n_meas;
    sWave[wave][2] = n_occ;
  }
  __syncthreads();
  // ---- erosion along x, then along y (radius re); then everything outside the image is cleared (neutral for the
  // dilation) - one thread per band row
  if (tid < ah) {
    const OcRow o = sA[tid];
    OcRow e = o;
    for (int d = 1; d <= re; ++d) e = oc_and(e, oc_and(oc_shl(o, d), oc_shr(o, d)));
    // (the shifts bring zeros in at the ends of the 128-bit word: those columns are > 16 away from the tile)
    sB[tid] = e;
  }
  __syncthreads();
  const OcRow in_cols = oc_image_columns(x0, W);
  if (tid < ah) {
    OcRow e = {~0ull, ~0ull};
    for (int d = -re; d <= re; ++d) {
      const int q = tid + d;
      if (q >= 0 && q < ah) e = oc_and(e, sB[q]);  // rows beyond the staged band are > R away from the tile
    }
    const int yy = y0 - R + tid;
    const OcRow in_img = (yy >= 0 && yy < H) ? in_cols : OcRow{0ull, 0ull};
    e = oc_and(e, in_img);
    sA[tid] = e;
    if (tid >= R && tid < R + kOcH) sRow[0][tid - R] = (uint32_t)__popcll(oc_core(e));
  }
  __syncthreads();
  // ---- dilation along x (radius rd in doubling shifts), then along y
  if (tid < ah) {
    const OcRow d = oc_dilate_x(sA[tid], rd);
    sB[tid] = d;
  }
  __syncthreads();
  if (tid < kOcH) {
    OcRow d = {0ull, 0ull};
    const int rc = tid + R;  // this tile row in the staged band
    for (int q = rc - rd; q <= rc + rd; ++q) d = oc_or(d, sB[q]);  // 0 <= rc - rd, rc + rd < ah
    const int yy = y0 + tid;
    d = oc_and(d, yy < H ? in_cols : OcRow{0ull, 0ull});  // G lives inside the image
    sA[tid] = d;
    const unsigned long long g = oc_core(d);
    sRow[1][tid] = (uint32_t)__popcll(g);
    sRow[2][tid] = (uint32_t)__popcll(g & sSil[tid]);
  }
  __syncthreads();
  // ---- the tile's 16 rows x 64 bits -> bytes, 4 per thread, combined with mask_in
  {
    const int r = tid >> 4, c4 = (tid & 15) * 4;
    const unsigned long long g = oc_core(sA[r]);
    const int yy = y0 + r, xx = x0 + c4;
    const unsigned gb4 = (unsigned)((g >> c4) & 15ull);
    const unsigned gbytes = oc_bytes(gb4);
    // four bytes as one dword where every row starts 4-byte aligned (uniform)
    const bool vec = (W & 3) == 0 &&
                     ((((uintptr_t)a.mask_in) | ((uintptr_t)a.mask_out) | ((uintptr_t)a.occluder)) & 3u) == 0;
    unsigned mi = 0u;  // bit 0 of byte j: mask_in != 0 at column xx + j
    if (yy < H && xx < W) {
      const size_t at = (size_t)yy * W + xx;
      if (vec) {
        const unsigned m = *(const unsigned*)(a.mask_in + at);
        mi = ((m & 0xffu) ? 1u : 0u) | ((m & 0xff00u) ? 0x100u : 0u) | ((m & 0xff0000u) ? 0x10000u : 0u) |
             ((m & 0xff000000u) ? 0x1000000u : 0u);
      } else {
        for (int j = 0; j < 4 && xx + j < W; ++j) mi |= (a.mask_in[at + j] ? 1u : 0u) << (8 * j);
      }
      const unsigned mo = mi & ~gbytes;
      if (vec) {
        *(unsigned*)(a.mask_out + at) = mo;
        *(unsigned*)(a.occluder + at) = gbytes;
      } else {
        for (int j = 0; j < 4 && xx + j < W; ++j) {
          a.mask_out[at + j] = (uint8_t)((mo >> (8 * j)) & 1u);
          a.occluder[at + j] = (uint8_t)((gbytes >> (8 * j)) & 1u);
        }
      }
    }
    const unsigned mo = mi & ~gbytes;
    uint32_t n_in = 0, n_out = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      n_in += (uint32_t)__popcll(__ballot(((mi >> (8 * j)) & 1u) != 0u));
      n_out += (uint32_t)__popcll(__ballot(((mo >> (8 * j)) & 1u) != 0u));
    }
    if (lane == 0) {
      sWave[wave][3] = n_in;
      sWave[wave][4] = n_out;
    }
  }
  __syncthreads();
  if (tid < kOcPart) {
    // record order: n_sil, n_measured, n_occluded, n_opened, n_occluder, n_mask_in, n_mask_out, n_sil_occluder
    uint32_t v = 0;
    if (tid < 3 || tid == 5 || tid == 6) {
      const int k = tid < 3 ? tid : tid - 2;
      for (int w = 0; w < 4; ++w) v += sWave[w][k];
    } else {
      const int k = tid == 7 ? 2 : tid - 3;
      for (int r = 0; r < kOcH; ++r) v += sRow[k][r];
    }
    a.partials[(size_t)block * kOcPart + tid] = v;
  }
}

__global__ __launch_bounds__(256) void occlusion_mask_kernel(const OcArgs a) { oc_tile(a, (int)blockIdx.x); }

// One wave: lane l folds blocks l, l + 64, ... in order, the butterfly folds the lanes, lane 0 writes the record.
__device__ __forceinline__ void oc_fold(const uint32_t* __restrict__ partials, const int n_blocks,
                                        int32_t* __restrict__ record) {
  const int lane = threadIdx.x;
  const uint4* p = (const uint4*)partials;
  uint32_t v[kOcPart];
#pragma unroll
  for (int w = 0; w < kOcPart; ++w) v[w] = 0;
#pragma unroll 1
  for (int b = lane; b < n_blocks; b += PXT_WAVE) {
    const uint4 t0 = p[(size_t)b * 2], t1 = p[(size_t)b * 2 + 1];
    v[0] += t0.x; v[1] += t0.y; v[2] += t0.z; v[3] += t0.w;
    v[4] += t1.x; v[5] += t1.y; v[6] += t1.z; v[7] += t1.w;
  }
#pragma unroll
  for (int m = 1; m < PXT_WAVE; m <<= 1) {
#pragma unroll
    for (int w = 0; w < kOcPart; ++w) v[w] += (uint32_t)__shfl_xor((int)v[w], m, PXT_WAVE);
  }
  if (lane == 0) {
#pragma unroll
    for (int w = 0; w < kOcPart; ++w) record[w] = (int32_t)v[w];
#pragma unroll
    for (int w = kOcPart; w < kOcRec; ++w) record[w] = 0;  // (8..10: the point gate's words)
  }
}

__global__ __launch_bounds__(PXT_WAVE) void occlusion_fold_kernel(const uint32_t* __restrict__ partials, const int n_blocks,
                                                                  int32_t* __restrict__ record) {
  oc_fold(partials, n_blocks, record);
}

// ---------------------------------------------------------------------------------------------------------------------
// pxt_occlusion_mask_views: up to PXT_OCCLUSION_MAX_VIEWS image pairs of different sizes in ONE chain of two launches.
// The grid is the concatenation of the views' tile grids; a workgroup finds its view in the per-view first-tile table
// (uniform per workgroup: scalar loads from the kernel arguments, which carry the whole table - no upload), forms that
// view's OcArgs in scalar registers and runs oc_tile on its own tile of it.  The partials of view k start at its first
// tile; the fold is one wave per view, oc_fold on the view's own partials: the order of the single call.
// ---------------------------------------------------------------------------------------------------------------------
struct OcView {
  const float4* depth;
  const uint16_t* sensor;
  const uint8_t* mask_in;
  uint8_t* mask_out;
  uint8_t* occluder;
  int H, W, tiles_x, n_tiles, tile0, shift_x, shift_y;  // tile0: the view's first tile in the grid
  float sensor_q, delta_q;
};

struct OcvArgs {
  OcView v[PXT_OCCLUSION_MAX_VIEWS];
  uint32_t* partials;  // [all views' tiles][kOcPart]
  int32_t* records;    // [n_views][kOcRec]
  int n_views, r_open, r_grow;
  float min_alpha;
};

__global__ __launch_bounds__(256) void occlusion_mask_views_kernel(const OcvArgs g) {
  int v = 0;  // the last view whose first tile is not behind blockIdx.x (every view has a tile)
  for (int k = 1; k < g.n_views; ++k)
    if ((int)blockIdx.x >= g.v[k].tile0) v = k;
  const OcView& w = g.v[v];
  OcArgs a;
  a.depth = w.depth;
  a.sensor = w.sensor;
  a.mask_in = w.mask_in;
  a.mask_out = w.mask_out;
  a.occluder = w.occluder;
  a.partials = g.partials + (size_t)w.tile0 * kOcPart;
  a.H = w.H;
  a.W = w.W;
  a.tiles_x = w.tiles_x;
  a.shift_x = w.shift_x;
  a.shift_y = w.shift_y;
  a.r_open = g.r_open;
  a.r_grow = g.r_grow;
  a.min_alpha = g.min_alpha;
  a.sensor_q = w.sensor_q;
  a.delta_q = w.delta_q;
  oc_tile(a, (int)blockIdx.x - w.tile0);
}

__global__ __launch_bounds__(PXT_WAVE) void occlusion_fold_views_kernel(const OcvArgs g) {
  const OcView& w = g.v[blockIdx.x];
  oc_fold(g.partials + (size_t)w.tile0 * kOcPart, w.n_tiles, g.records + (size_t)blockIdx.x * kOcRec);
}

struct PvArgs {
  const float* p3d;          // [n][3]
  const uint8_t* valid_in;   // [n] or nullptr
  uint8_t* valid_out;        // [n]
  const uint8_t* occluder;   // [H][W]
  int32_t* record;           // words 8..10 are written
  int n, W, H, ndist;
  float T[12], cam[10];
};

__global__ __launch_bounds__(kPvBlock) void points_visible_kernel(const PvArgs a) {
  __shared__ uint32_t red[kPvBlock / PXT_WAVE][2];
  const int tid = threadIdx.x;
  const Cam cam = make_cam(a.cam, a.ndist);
  uint32_t n_in = 0, n_out = 0;  // wave-uniform
  for (int base = 0; base < a.n; base += kPvBlock) {
    const int i = base + tid;
    bool in = false, out = false;
    if (i < a.n) {
      in = a.valid_in ? a.valid_in[i] != 0 : true;
      out = in;
      float px, py, pz, u, v;
      transform_point(a.T, a.p3d[3 * (size_t)i], a.p3d[3 * (size_t)i + 1], a.p3d[3 * (size_t)i + 2], px, py, pz);
      if (project_point(cam, px, py, pz, u, v, nullptr)) {
        const float xt = floorf(u + 0.5f), yt = floorf(v + 0.5f);  // the nearest texel: texel k's centre is at k
        if (xt >= 0.f && yt >= 0.f && xt < (float)a.W && yt < (float)a.H)
          out = in && a.occluder[(size_t)(int)yt * a.W + (int)xt] == 0;
      }
      a.valid_out[i] = out ? 1 : 0;
    }
    n_in += (uint32_t)__popcll(__ballot(in));
    n_out += (uint32_t)__popcll(__ballot(out));
  }
  if ((tid & (PXT_WAVE - 1)) == 0) {
    red[tid / PXT_WAVE][0] = n_in;
    red[tid / PXT_WAVE][1] = n_out;
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t s_in = 0, s_out = 0;
    for (int w = 0; w < kPvBlock / PXT_WAVE; ++w) {
      s_in += red[w][0];
      s_out += red[w][1];
    }
    a.record[8] = a.n;
    a.record[9] = (int32_t)s_in;
    a.record[10] = (int32_t)s_out;
  }
}

// pxt_mask_exclude: mask_out = (mask_in != 0) && !occluder over the H * W bytes of a plane, which is elementwise: the
// planes are walked as one row of vectors of V bytes (16 or 4 where all three are that aligned, else none) by ONE
// workgroup of 1024 threads, four vectors of each input in flight per lane and trip, and the last H * W % V bytes one by
// one.  The two counts by population count, folded over the 16 waves through LDS by index: no atomics, one launch.
struct MxArgs {
  const uint8_t* mask_in;
  const uint8_t* occluder;
  uint8_t* mask_out;
  int32_t* record;
  size_t n;  // H * W
};

// bit 0 of every byte: that byte of m is not 0
__device__ inline unsigned mx_nonzero(unsigned m) {
  return ((((m & 0x7f7f7f7fu) + 0x7f7f7f7fu) | m) & 0x80808080u) >> 7;
}

__device__ inline void mx_fold(unsigned m, unsigned g, unsigned* out, uint32_t* n_in, uint32_t* n_out) {
  const unsigned in = mx_nonzero(m);
  *out = in & ~mx_nonzero(g);
  *n_in += (uint32_t)__popc(in);
  *n_out += (uint32_t)__popc(*out);
}
__device__ inline unsigned mx_apply(unsigned m, unsigned g, uint32_t* n_in, uint32_t* n_out) {
  unsigned o;
  mx_fold(m, g, &o, n_in, n_out);
  return o;
}
__device__ inline uint4 mx_apply(uint4 m, uint4 g, uint32_t* n_in, uint32_t* n_out) {
  uint4 o;
  mx_fold(m.x, g.x, &o.x, n_in, n_out);
  mx_fold(m.y, g.y, &o.y, n_in, n_out);
  mx_fold(m.z, g.z, &o.z, n_in, n_out);
  mx_fold(m.w, g.w, &o.w, n_in, n_out);
  return o;
}

template <class V>  // uint4 or unsigned; n_vec = 0: bytes alone
__global__ __launch_bounds__(kPvBlock) void mask_exclude_kernel(const MxArgs a, const size_t n_vec) {
  __shared__ uint32_t red[kPvBlock / PXT_WAVE][2];
  constexpr int kAhead = 4;
  const int tid = threadIdx.x;
  uint32_t n_in = 0, n_out = 0;
  const V* mi = (const V*)a.mask_in;
  const V* oc = (const V*)a.occluder;
  V* mo = (V*)a.mask_out;
  for (size_t base = 0; base < n_vec; base += (size_t)kPvBlock * kAhead) {  // the whole workgroup alike
    V m[kAhead], g[kAhead];
#pragma unroll
    for (int k = 0; k < kAhead; ++k) {
      const size_t v = base + (size_t)k * kPvBlock + tid;
      if (v < n_vec) {
        m[k] = mi[v];
        g[k] = oc[v];
      }
    }
#pragma unroll
    for (int k = 0; k < kAhead; ++k) {
      const size_t v = base + (size_t)k * kPvBlock + tid;
      if (v < n_vec) mo[v] = mx_apply(m[k], g[k], &n_in, &n_out);
    }
  }
  for (size_t i = n_vec * sizeof(V) + tid; i < a.n; i += kPvBlock) {
    const bool in = a.mask_in[i] != 0, out = in && a.occluder[i] == 0;
    n_in += in;
    n_out += out;
    a.mask_out[i] = out ? 1 : 0;
  }
#pragma unroll
  for (int m = 1; m < PXT_WAVE; m <<= 1) {
    n_in += (uint32_t)__shfl_xor((int)n_in, m, PXT_WAVE);
    n_out += (uint32_t)__shfl_xor((int)n_out, m, PXT_WAVE);
  }
  if ((tid & (PXT_WAVE - 1)) == 0) {
    red[tid / PXT_WAVE][0] = n_in;
    red[tid / PXT_WAVE][1] = n_out;
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t s_in = 0, s_out = 0;
    for (int w = 0; w < kPvBlock / PXT_WAVE; ++w) {
      s_in += red[w][0];
      s_out += red[w][1];
    }
    a.record[0] = (int32_t)s_in;
    a.record[1] = (int32_t)s_out;
  }
}

bool oc_sizes_ok(int width, int height) {
  return width >= 1 && height >= 1 && (int64_t)width * height <= kOcMaxPixels;
}
int64_t oc_blocks(int width, int height) {
  return (int64_t)((width + kOcW - 1) / kOcW) * ((height + kOcH - 1) / kOcH);
}

bool oc_radii_ok(int r_open, int r_grow) {
  return r_open >= 0 && r_grow >= 0 && r_open <= kOcMaxR && r_grow <= kOcMaxR && r_open + r_grow <= kOcMaxR;
}
bool oc_shift_ok(int s) { return s >= -kOcMaxShift && s <= kOcMaxShift; }

// The tiles of all views, or -1 when a count or a size is out of range.
int64_t ocv_total_tiles(int32_t n_views, const int32_t* sizes) {
  if (n_views < 1 || n_views > PXT_OCCLUSION_MAX_VIEWS || !sizes) return -1;
  int64_t n = 0;
  for (int k = 0; k < n_views; ++k) {
    if (!oc_sizes_ok(sizes[2 * k], sizes[2 * k + 1])) return -1;
    n += oc_blocks(sizes[2 * k], sizes[2 * k + 1]);
  }
  return n;
}

struct OcRange {
  uintptr_t lo, hi;  // bytes [lo, hi)
};
bool oc_overlap(const OcRange& p, const OcRange& q) { return p.lo < q.hi && q.lo < p.hi; }

}  // namespace
}  // namespace pxt

using namespace pxt;

extern "C" int64_t pxt_occlusion_mask_workspace_bytes(int32_t width, int32_t height) {
  if (!oc_sizes_ok(width, height)) return PXT_E_ARG;
  return oc_blocks(width, height) * kOcPart * (int64_t)sizeof(uint32_t);
}

extern "C" int pxt_occlusion_mask(const float* depth, const uint16_t* sensor, const uint8_t* mask_in, int32_t width,
                                  int32_t height, int32_t shift_x, int32_t shift_y, float min_alpha, float sensor_q,
                                  float delta_q, int32_t r_open, int32_t r_grow, uint8_t* mask_out, uint8_t* occluder,
                                  int32_t* record, void* workspace, void* stream) {
  if (!depth || !sensor || !mask_in || !mask_out || !occluder || !record || !workspace) return PXT_E_ARG;
  if (!oc_sizes_ok(width, height)) return PXT_E_ARG;
  if (!oc_radii_ok(r_open, r_grow)) return PXT_E_ARG;
  if (!oc_shift_ok(shift_x) || !oc_shift_ok(shift_y)) return PXT_E_ARG;
  if (((uintptr_t)depth % 16) != 0 || ((uintptr_t)sensor % 2) != 0 || ((uintptr_t)record % 4) != 0 ||
      ((uintptr_t)workspace % 16) != 0)
    return PXT_E_ARG;
  if (mask_out == occluder) return PXT_E_ARG;
  OcArgs a;
  a.depth = (const float4*)depth;
  a.sensor = sensor;
  a.mask_in = mask_in;
  a.mask_out = mask_out;
  a.occluder = occluder;
  a.partials = (uint32_t*)workspace;
  a.H = height;
  a.W = width;
  a.tiles_x = (width + kOcW - 1) / kOcW;
  a.shift_x = shift_x;
  a.shift_y = shift_y;
  a.r_open = r_open;
  a.r_grow = r_grow;
  a.min_alpha = min_alpha;
  a.sensor_q = sensor_q;
  a.delta_q = delta_q;
  const int n_blocks = (int)oc_blocks(width, height);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(occlusion_mask_kernel, dim3(n_blocks), dim3(256), 0, s, a);
  PXT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(occlusion_fold_kernel, dim3(1), dim3(PXT_WAVE), 0, s, (const uint32_t*)a.partials, n_blocks, record);
  PXT_HIP_CHECK(hipGetLastError());
  return PXT_OK;
}

extern "C" int64_t pxt_occlusion_mask_views_workspace_bytes(int32_t n_views, const int32_t* sizes) {
  const int64_t n = ocv_total_tiles(n_views, sizes);
  if (n < 0) return PXT_E_ARG;
  return n * kOcPart * (int64_t)sizeof(uint32_t);
}

extern "C" int pxt_occlusion_mask_views(const pxt_occlusion_view* views_host, int32_t n_views, float min_alpha,
                                        int32_t r_open, int32_t r_grow, int32_t* records, void* workspace, void* stream) {
  if (!views_host || !records || !workspace) return PXT_E_ARG;
  if (n_views < 1 || n_views > PXT_OCCLUSION_MAX_VIEWS) return PXT_E_ARG;
  if (!oc_radii_ok(r_open, r_grow)) return PXT_E_ARG;
  if (((uintptr_t)records % 4) != 0 || ((uintptr_t)workspace % 16) != 0) return PXT_E_ARG;
  OcvArgs g;
  OcRange out[2 * PXT_OCCLUSION_MAX_VIEWS], in[3 * PXT_OCCLUSION_MAX_VIEWS];
  int64_t tile0 = 0;
  for (int k = 0; k < n_views; ++k) {
    const pxt_occlusion_view& p = views_host[k];
    if (!p.depth || !p.sensor || !p.mask_in || !p.mask_out || !p.occluder) return PXT_E_ARG;
    if (!oc_sizes_ok(p.width, p.height)) return PXT_E_ARG;
    if (!oc_shift_ok(p.shift_x) || !oc_shift_ok(p.shift_y)) return PXT_E_ARG;
    if (((uintptr_t)p.depth % 16) != 0 || ((uintptr_t)p.sensor % 2) != 0) return PXT_E_ARG;
    const uintptr_t npix = (uintptr_t)p.width * (uintptr_t)p.height;
    out[2 * k] = OcRange{(uintptr_t)p.mask_out, (uintptr_t)p.mask_out + npix};
    out[2 * k + 1] = OcRange{(uintptr_t)p.occluder, (uintptr_t)p.occluder + npix};
    in[3 * k] = OcRange{(uintptr_t)p.depth, (uintptr_t)p.depth + 16 * npix};
    in[3 * k + 1] = OcRange{(uintptr_t)p.sensor, (uintptr_t)p.sensor + 2 * npix};
    in[3 * k + 2] = OcRange{(uintptr_t)p.mask_in, (uintptr_t)p.mask_in + npix};
    OcView& w = g.v[k];
    w.depth = (const float4*)p.depth;
    w.sensor = p.sensor;
    w.mask_in = p.mask_in;
    w.mask_out = p.mask_out;
    w.occluder = p.occluder;
    w.H = p.height;
    w.W = p.width;
    w.tiles_x = (p.width + kOcW - 1) / kOcW;
    w.n_tiles = (int)oc_blocks(p.width, p.height);
    w.tile0 = (int)tile0;
    w.shift_x = p.shift_x;
    w.shift_y = p.shift_y;
    w.sensor_q = p.sensor_q;
    w.delta_q = p.delta_q;
    tile0 += w.n_tiles;  // <= 16 * 2^24
  }
  // every output plane is written by its own view alone and read by nobody: it overlaps no other output, no input of
  // any view - except that a view's mask_out may BE its mask_in, as in the single call - nor the records or the partials
  const OcRange rec = {(uintptr_t)records, (uintptr_t)records + (uintptr_t)n_views * kOcRec * sizeof(int32_t)};
  const OcRange ws = {(uintptr_t)workspace, (uintptr_t)workspace + (uintptr_t)tile0 * kOcPart * sizeof(uint32_t)};
  if (oc_overlap(rec, ws)) return PXT_E_ARG;
  for (int i = 0; i < 2 * n_views; ++i) {
    if (oc_overlap(out[i], rec) || oc_overlap(out[i], ws)) return PXT_E_ARG;
    for (int j = i + 1; j < 2 * n_views; ++j)
      if (oc_overlap(out[i], out[j])) return PXT_E_ARG;
    for (int j = 0; j < 3 * n_views; ++j) {
      const bool own_mask = (i % 2) == 0 && j == 3 * (i / 2) + 2 && out[i].lo == in[j].lo;
      if (!own_mask && oc_overlap(out[i], in[j])) return PXT_E_ARG;
    }
  }
  for (int k = n_views; k < PXT_OCCLUSION_MAX_VIEWS; ++k) g.v[k] = OcView{};
  g.partials = (uint32_t*)workspace;
  g.records = records;
  g.n_views = n_views;
  g.r_open = r_open;
  g.r_grow = r_grow;
  g.min_alpha = min_alpha;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(occlusion_mask_views_kernel, dim3((unsigned)tile0), dim3(256), 0, s, g);
  PXT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(occlusion_fold_views_kernel, dim3(n_views), dim3(PXT_WAVE), 0, s, g);
  PXT_HIP_CHECK(hipGetLastError());
  return PXT_OK;
}

extern "C" int pxt_points_visible(const float* p3d, const uint8_t* valid_in, int32_t n_points, const float* pose12_host,
                                  const float* cam10_host, int32_t ndist, const uint8_t* occluder, int32_t width,
                                  int32_t height, uint8_t* valid_out, int32_t* record, void* stream) {
  if (n_points < 0 || n_points > kPvMaxPoints || !pose12_host || !cam10_host || !occluder || !record) return PXT_E_ARG;
  if (n_points > 0 && (!p3d || !valid_out)) return PXT_E_ARG;
  if (!oc_sizes_ok(width, height)) return PXT_E_ARG;
  if (ndist != 0 && ndist != 2 && ndist != 4) return PXT_E_ARG;
  if (((uintptr_t)p3d % 4) != 0 || ((uintptr_t)record % 4) != 0) return PXT_E_ARG;
  // the camera is the one the plane was made for: project_point's own image test then keeps every texel inside it
  if (!(cam10_host[0] == (float)width && cam10_host[1] == (float)height)) return PXT_E_ARG;
  PvArgs a;
  a.p3d = p3d;
  a.valid_in = valid_in;
  a.valid_out = valid_out;
  a.occluder = occluder;
  a.record = record;
  a.n = n_points;
  a.W = width;
  a.H = height;
  a.ndist = ndist;
  for (int k = 0; k < 12; ++k) a.T[k] = pose12_host[k];
  for (int k = 0; k < 10; ++k) a.cam[k] = cam10_host[k];
  hipLaunchKernelGGL(points_visible_kernel, dim3(1), dim3(kPvBlock), 0, (hipStream_t)stream, a);
  PXT_HIP_CHECK(hipGetLastError());
  return PXT_OK;
}

extern "C" int pxt_mask_exclude(const uint8_t* mask_in, const uint8_t* occluder, int32_t width, int32_t height,
                                uint8_t* mask_out, int32_t* record, void* stream) {
  if (!mask_in || !occluder || !mask_out || !record) return PXT_E_ARG;
  if (!oc_sizes_ok(width, height)) return PXT_E_ARG;
  if (((uintptr_t)record % 4) != 0 || mask_out == occluder) return PXT_E_ARG;
  MxArgs a;
  a.mask_in = mask_in;
  a.occluder = occluder;
  a.mask_out = mask_out;
  a.record = record;
  a.n = (size_t)width * height;
  const uintptr_t all = (uintptr_t)mask_in | (uintptr_t)occluder | (uintptr_t)mask_out;
  hipStream_t s = (hipStream_t)stream;
  if ((all & 15u) == 0) hipLaunchKernelGGL(mask_exclude_kernel<uint4>, dim3(1), dim3(kPvBlock), 0, s, a, a.n / 16);
  else hipLaunchKernelGGL(mask_exclude_kernel<unsigned>, dim3(1), dim3(kPvBlock), 0, s, a, (all & 3u) == 0 ? a.n / 4 : (size_t)0);
  PXT_HIP_CHECK(hipGetLastError());
  return PXT_OK;
}

// fp32 forward pass of the VGG16-UNet feature pyramid (pxt_unet_create_f32): the network pixloc runs, in its precision.
//
// The fp16 pass (pxt_unet.hip) stores activations as fp16; a checkpoint whose activations leave fp16's range has no
// working path there, and fp16 storage moves the features by ~2e-4 rms against the fp32 oracle.  This pass keeps every
// activation in fp32 NHWC and runs the 3x3 convolutions as implicit GEMMs on the exact f32-input MFMA
// (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain, one rounding per product): rows = output channels (A = filter taps),
// columns = pixels (B = the shifted input window), K = 9 * Cin.
//
// Deterministic by construction: every output value is ONE chain over K in a fixed order (16-channel chunk, tap, then
// the 16 channels of the chunk in the MFMA's k order), started from 0 and followed by bias + ReLU; there is no split-K and
// no atomic anywhere.  Which workgroup or wave computes a value changes nothing, so an image's maps are the same bits
// alone, in a batch of any size, or in a pair with an image of another size.
//
// The rest of the network is plain fp32 kernels: the first layer (normalisation, mask, 3 -> 64) on the VALU, 2x2 max-pool,
// the decoder's bilinear x2 upsample + skip crop + concat materialised into one buffer, BatchNorm folded on the host, and
// the 1x1 heads on the same f32 MFMA.
#include "pxt_unet_f32.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace pxt {

typedef __attribute__((ext_vector_type(16))) float f32x16;

namespace f32k {

constexpr int kNumConv = 17;
constexpr int kNumHeads = 3;
constexpr int kKC = 16;           // input channels per staged chunk (two 8-channel MFMA groups)
constexpr int kPS = kKC + 4;      // LDS floats per halo pixel (padded against bank conflicts)
constexpr int kStatsBlocks = 256;  // partial results per layer of pxt_unet_activation_stats

__device__ __forceinline__ float relu_nan(float v) { return v < 0.f ? 0.f : v; }  // NaN passes, like torch.relu
__device__ __forceinline__ float max_nan(float a, float b) { return (a > b || a != a) ? a : b; }

// Packed 3x3 taps: float4 records [cout / 32][cin / 16][tap 9][group 2][lane 64]; lane l of the wave serving output rows
// 32 cb .. 32 cb + 31 holds W[row l & 31][channel 16 chunk + 8 group + 4 (l >> 5) + s][tap] in element s = 0..3, the A
// operands of four consecutive MFMA k-steps.
__host__ __device__ inline void packed_f32_source(long long d, int cin, int& co, int& tap, int& ci) {
  const int s = (int)(d & 3), lane = (int)((d >> 2) & 63), g = (int)((d >> 8) & 1);
  long long rest = d >> 9;
  tap = (int)(rest % 9);
  rest /= 9;
  const int nch = cin / kKC;
  const int chunk = (int)(rest % nch), cob = (int)(rest / nch);
  co = 32 * cob + (lane & 31);
  ci = kKC * chunk + 8 * g + 4 * (lane >> 5) + s;
}

__global__ void pack_f32_kernel(const float* __restrict__ w, int cin, int cout, float* __restrict__ packed) {
  const long long d = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= (long long)cout * 9 * cin) return;
  int co, tap, ci;
  packed_f32_source(d, cin, co, tap, ci);
  packed[d] = w[((size_t)co * 9 + tap) * cin + ci];
}

// ---------------------------------------------------------------------------
// 3x3 convolution, pad 1, NHWC fp32 -> NHWC fp32, + bias (+ ReLU).
// A workgroup (4 waves, WC x WP) covers TH = 2 PB WP rows x 16 columns of pixels and 32 CB WC output channels; a wave
// CB x PB blocks of 32 channels x 32 pixels (2 rows x 16 columns).  The input halo of a 16-channel chunk is staged in
// LDS (double-buffered, the next chunk's loads in flight during the MFMAs); the taps come pre-packed from L2.
// ---------------------------------------------------------------------------
template <int CB, int PB, int WC, int WP>
__global__ __launch_bounds__(256) void conv3x3_f32_kernel(const float* __restrict__ in, int H, int W, int Cin,
                                                          const float4* __restrict__ wpk, const float* __restrict__ bias,
                                                          int Cout, int relu, float* __restrict__ out) {
  static_assert(WC * WP == 4, "four waves");
  constexpr int TH = 2 * PB * WP, TW = 16, HW2 = TW + 2;
  constexpr int kHalo = (TH + 2) * HW2;     // halo pixels
  constexpr int kVec = kHalo * (kKC / 4);   // float4 per chunk
  constexpr int kPer = (kVec + 255) / 256;  // per thread
  constexpr int kPix4 = kPS / 4;            // float4 per halo pixel in LDS
  __shared__ float4 s_in[2][kHalo * kPix4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wc = wv % WC, wp = wv / WC;
  const int img = blockIdx.z;
  const int tiles_x = (W + TW - 1) / TW;
  const int ty0 = (int)(blockIdx.x / tiles_x) * TH, tx0 = (int)(blockIdx.x % tiles_x) * TW;
  in += (size_t)img * H * W * Cin;
  out += (size_t)img * H * W * Cout;

  int goff[kPer], loff[kPer];
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int i = tid + 256 * k;
    const int p = i / (kKC / 4), q = i % (kKC / 4);
    const int y = ty0 + p / HW2 - 1, x = tx0 + p % HW2 - 1;
    const bool ok = i < kVec && y >= 0 && y < H && x >= 0 && x < W;
    goff[k] = ok ? (y * W + x) * Cin + 4 * q : -1;
    loff[k] = i < kVec ? p * kPix4 + q : -1;
  }
  float4 r[kPer];
  auto load = [&](int c0) {
#pragma unroll
    for (int k = 0; k < kPer; ++k)
      r[k] = goff[k] >= 0 ? *(const float4*)(in + goff[k] + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int k = 0; k < kPer; ++k)
      if (loff[k] >= 0) s_in[buf][loff[k]] = r[k];
  };

  const int r31 = lane & 31, h = lane >> 5;
  int pbase[PB];  // LDS float4 index of this lane's pixel (tap 0, 0) and channel quad h
#pragma unroll
  for (int pb = 0; pb < PB; ++pb) pbase[pb] = ((wp * 2 * PB + 2 * pb + (r31 >> 4)) * HW2 + (r31 & 15)) * kPix4 + h;
  const int nch = Cin / kKC;
  const int cob0 = blockIdx.y * (CB * WC) + wc * CB;  // first 32-channel block of this wave
  const float4* wbase[CB];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb) wbase[cb] = wpk + (size_t)(cob0 + cb) * nch * 9 * 2 * 64 + lane;

  f32x16 acc[CB][PB];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb)
#pragma unroll
    for (int pb = 0; pb < PB; ++pb)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[cb][pb][e] = 0.f;

  // the taps of step (chunk, tap, group) = index 18 chunk + 2 tap + group: loaded one step ahead of their MFMAs
  float4 a[CB], an[CB];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb) a[cb] = wbase[cb][0];
  load(0);
  store(0);
  __syncthreads();
  for (int chunk = 0; chunk < nch; ++chunk) {
    const int buf = chunk & 1;
    if (chunk + 1 < nch) load((chunk + 1) * kKC);
    const float4* s = s_in[buf];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int toff = ((tap / 3) * HW2 + tap % 3) * kPix4;
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const int next = chunk * 18 + tap * 2 + g + 1;
        if (next < nch * 18) {
#pragma unroll
          for (int cb = 0; cb < CB; ++cb) an[cb] = wbase[cb][(size_t)next * 64];
        }
        float4 b[PB];
#pragma unroll
        for (int pb = 0; pb < PB; ++pb) b[pb] = s[pbase[pb] + toff + 2 * g];
#pragma unroll
        for (int st = 0; st < 4; ++st)
#pragma unroll
          for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int pb = 0; pb < PB; ++pb)
              acc[cb][pb] = __builtin_amdgcn_mfma_f32_32x32x2f32(((const float*)&a[cb])[st], ((const float*)&b[pb])[st],
                                                                 acc[cb][pb], 0, 0, 0);
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) a[cb] = an[cb];
      }
    }
    if (chunk + 1 < nch) store(buf ^ 1);
    __syncthreads();
  }

  // D[row = channel][col = pixel]: lane holds pixel r31 of each block, channels (e & 3) + 8 (e >> 2) + 4 h
#pragma unroll
  for (int pb = 0; pb < PB; ++pb) {
    const int y = ty0 + wp * 2 * PB + 2 * pb + (r31 >> 4), x = tx0 + (r31 & 15);
    if (y >= H || x >= W) continue;
    float* o = out + ((size_t)y * W + x) * Cout;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
      const int co = 32 * (cob0 + cb);
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int c = co + 8 * g4 + 4 * h;
        const float4 bv = *(const float4*)(bias + c);
        float4 v;
        v.x = acc[cb][pb][4 * g4 + 0] + bv.x;
        v.y = acc[cb][pb][4 * g4 + 1] + bv.y;
        v.z = acc[cb][pb][4 * g4 + 2] + bv.z;
        v.w = acc[cb][pb][4 * g4 + 3] + bv.w;
        if (relu) { v.x = relu_nan(v.x); v.y = relu_nan(v.y); v.z = relu_nan(v.z); v.w = relu_nan(v.w); }
        *(float4*)(o + c) = v;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// First layer: image (HWC, 0..255, float or u8) [* mask] -> /255 -> ImageNet normalisation (zero padding after it, as
// the oracle pads the normalised tensor) -> conv3x3 (3 -> 64) + bias + ReLU.  Thread = pixel, 64 accumulators, the taps
// broadcast from LDS.  blockIdx.y = image.
// ---------------------------------------------------------------------------
struct FirstImagesF32 {
  const void* image[PXT_UNET_MAX_BATCH];
  const uint8_t* mask[PXT_UNET_MAX_BATCH];
  int is_u8[PXT_UNET_MAX_BATCH];
};

__global__ __launch_bounds__(256) void conv_first_f32_kernel(const FirstImagesF32 im, int H, int W,
                                                             const float* __restrict__ wt /* [27][64] */,
                                                             const float* __restrict__ bias, float* __restrict__ out) {
  __shared__ float s_w[27 * 64];
  __shared__ float s_b[64];
  for (int i = threadIdx.x; i < 27 * 64; i += 256) s_w[i] = wt[i];
  if (threadIdx.x < 64) s_b[threadIdx.x] = bias[threadIdx.x];
  __syncthreads();
  const int img = blockIdx.y;
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long long)H * W) return;
  const int y = (int)(p / W), x = (int)(p % W);
  const void* image = im.image[img];
  const uint8_t* mask = im.mask[img];
  const bool u8 = im.is_u8[img] != 0;
  const float mean[3] = {0.485f, 0.456f, 0.406f};
  const float stdv[3] = {0.229f, 0.224f, 0.225f};
  float xin[27];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
    const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
    const float m = (ok && mask) ? (float)mask[(size_t)yy * W + xx] : 1.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v = 0.f;
      if (ok) {
        const size_t idx = ((size_t)yy * W + xx) * 3 + c;
        float raw = u8 ? (float)((const uint8_t*)image)[idx] : ((const float*)image)[idx];
        if (mask) raw *= m;
        v = (raw / 255.0f - mean[c]) / stdv[c];
      }
      xin[3 * t + c] = v;
    }
  }
  float* o = out + ((size_t)img * H * W + p) * 64;
#pragma unroll
  for (int q = 0; q < 16; ++q) {  // 4 output channels at a time: 4 accumulators over the 27 taps
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
    for (int k = 0; k < 27; ++k) {
      const float v = xin[k];
      a0 = fmaf(s_w[k * 64 + 4 * q + 0], v, a0);
      a1 = fmaf(s_w[k * 64 + 4 * q + 1], v, a1);
      a2 = fmaf(s_w[k * 64 + 4 * q + 2], v, a2);
      a3 = fmaf(s_w[k * 64 + 4 * q + 3], v, a3);
    }
    float4 r;
    r.x = relu_nan(a0 + s_b[4 * q + 0]);
    r.y = relu_nan(a1 + s_b[4 * q + 1]);
    r.z = relu_nan(a2 + s_b[4 * q + 2]);
    r.w = relu_nan(a3 + s_b[4 * q + 3]);
    *(float4*)(o + 4 * q) = r;
  }
}

// 2x2 max-pool stride 2 (floor), NHWC fp32, 4 channels per thread.
__global__ void maxpool2_f32_kernel(const float* __restrict__ in, int H, int W, int C, float* __restrict__ out, int Ho,
                                    int Wo, int n_img) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int c4 = C / 4;
  if (i >= (long long)n_img * Ho * Wo * c4) return;
  const int c = (int)(i % c4) * 4;
  long long p = i / c4;
  const int img = (int)(p / ((long long)Ho * Wo));
  p -= (long long)img * Ho * Wo;
  const int x = (int)(p % Wo), y = (int)(p / Wo);
  const float* s = in + (size_t)img * H * W * C + ((size_t)(2 * y) * W + 2 * x) * C + c;
  const float4 a = *(const float4*)s, b = *(const float4*)(s + C), d = *(const float4*)(s + (size_t)W * C),
               e = *(const float4*)(s + (size_t)W * C + C);
  float4 o;
  o.x = max_nan(max_nan(a.x, b.x), max_nan(d.x, e.x));
  o.y = max_nan(max_nan(a.y, b.y), max_nan(d.y, e.y));
  o.z = max_nan(max_nan(a.z, b.z), max_nan(d.z, e.z));
  o.w = max_nan(max_nan(a.w, b.w), max_nan(d.w, e.w));
  *(float4*)(out + (size_t)img * Ho * Wo * C + ((size_t)y * Wo + x) * C + c) = o;
}

// Decoder input: cat([bilinear x2 upsample(prev) (align_corners=False), skip[:Hd, :Wd]]) -> [Hd][Wd][Cp + Cs].
// The interpolation is torch's upsample_bilinear2d: source index max((d + 0.5) / 2 - 0.5, 0), lambdas from its fraction.
__global__ void upcat_f32_kernel(const float* __restrict__ prev, int Hp, int Wp, int Cp, const float* __restrict__ skip,
                                 int Hs, int Ws, int Cs, float* __restrict__ out, int Hd, int Wd, int n_img) {
  const int C = Cp + Cs, c4 = C / 4;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)n_img * Hd * Wd * c4) return;
  const int c = (int)(i % c4) * 4;
  long long p = i / c4;
  const int img = (int)(p / ((long long)Hd * Wd));
  p -= (long long)img * Hd * Wd;
  const int x = (int)(p % Wd), y = (int)(p / Wd);
  float4 v;
  if (c < Cp) {
    const float sy = fmaxf(((float)y + 0.5f) * 0.5f - 0.5f, 0.f), sx = fmaxf(((float)x + 0.5f) * 0.5f - 0.5f, 0.f);
    const int y0 = min((int)sy, Hp - 1), x0 = min((int)sx, Wp - 1);
    const int y1 = min(y0 + 1, Hp - 1), x1 = min(x0 + 1, Wp - 1);
    const float ly1 = sy - (float)y0, lx1 = sx - (float)x0, ly0 = 1.f - ly1, lx0 = 1.f - lx1;
    const float* P = prev + (size_t)img * Hp * Wp * Cp + c;
    const float4 a = *(const float4*)(P + ((size_t)y0 * Wp + x0) * Cp), b = *(const float4*)(P + ((size_t)y0 * Wp + x1) * Cp),
                 d = *(const float4*)(P + ((size_t)y1 * Wp + x0) * Cp), e = *(const float4*)(P + ((size_t)y1 * Wp + x1) * Cp);
    v.x = ly0 * (lx0 * a.x + lx1 * b.x) + ly1 * (lx0 * d.x + lx1 * e.x);
    v.y = ly0 * (lx0 * a.y + lx1 * b.y) + ly1 * (lx0 * d.y + lx1 * e.y);
    v.z = ly0 * (lx0 * a.z + lx1 * b.z) + ly1 * (lx0 * d.z + lx1 * e.z);
    v.w = ly0 * (lx0 * a.w + lx1 * b.w) + ly1 * (lx0 * d.w + lx1 * e.w);
  } else {
    v = *(const float4*)(skip + (size_t)img * Hs * Ws * Cs + ((size_t)y * Ws + x) * Cs + (c - Cp));
  }
  *(float4*)(out + (size_t)img * Hd * Wd * C + ((size_t)y * Wd + x) * C + c) = v;
}

// ---------------------------------------------------------------------------
// 1x1 heads on the f32 MFMA: rows = output channels (descriptor C, then the uncertainty row), columns = 32 pixels per
// wave, K = Cin in steps of 8 (one float4 per lane and operand: k = k0 + 4 h + s at step s).  Epilogue as the fp16 pass:
// optional L2 normalisation of the descriptor, confidence = sigmoid(-x), float32 record [C | conf | 0 pad].
// wts: [32 NT][Cin] (rows >= C + 1 zero), bias [32 NT].  blockIdx.y = image.
// ---------------------------------------------------------------------------
struct HeadOutF32 {
  float* out[PXT_UNET_MAX_BATCH];
  int normalize[PXT_UNET_MAX_BATCH];
};

template <int NT>
__global__ __launch_bounds__(256) void head_f32_kernel(const float* __restrict__ in, long long npix, int Cin,
                                                       const float* __restrict__ wts, const float* __restrict__ bias,
                                                       int Cout, const HeadOutF32 ho, int cstride) {
  const int lane = threadIdx.x & 63, img = blockIdx.y;
  const long long p0 = (((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * 32;
  if (p0 >= npix) return;
  const int r31 = lane & 31, h = lane >> 5;
  const long long pix = min(p0 + r31, npix - 1);
  f32x16 acc[NT];
#pragma unroll
  for (int c = 0; c < NT; ++c)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[c][e] = 0.f;
  const float* xp = in + ((size_t)img * npix + pix) * Cin + 4 * h;
  const float* wp = wts + (size_t)r31 * Cin + 4 * h;
  for (int k0 = 0; k0 < Cin; k0 += 8) {
    const float4 b = *(const float4*)(xp + k0);
    float4 a[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) a[c] = *(const float4*)(wp + (size_t)(32 * c) * Cin + k0);
#pragma unroll
    for (int st = 0; st < 4; ++st)
#pragma unroll
      for (int c = 0; c < NT; ++c)
        acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(((const float*)&a[c])[st], ((const float*)&b)[st], acc[c], 0, 0, 0);
  }
  float ss = 0.f;
#pragma unroll
  for (int c = 0; c < NT; ++c)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int co = 32 * c + (e & 3) + 8 * (e >> 2) + 4 * h;
      const float v = acc[c][e] + bias[co];
      acc[c][e] = v;
      if (co < Cout) ss += v * v;
    }
  ss += __shfl_xor(ss, 32, 64);
  const float inv = ho.normalize[img] ? 1.f / fmaxf(sqrtf(ss), 1e-12f) : 1.f;
  if (p0 + r31 >= npix) return;
  float* o = ho.out[img] + (size_t)(p0 + r31) * cstride;
#pragma unroll
  for (int c = 0; c < NT; ++c)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int co = 32 * c + 8 * g + 4 * h;
      if (co >= cstride) continue;
      float4 v;
      float* vv = (float*)&v;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float x = acc[c][4 * g + j];
        const int cj = co + j;
        vv[j] = (cj < Cout) ? x * inv : (cj == Cout ? 1.f / (1.f + expf(x)) : 0.f);
      }
      *(float4*)(o + co) = v;
    }
}

// Output channels past 32 NT of a wide record (cstride > 32 NT) stay zero like the fp16 pass's pad channels.
__global__ void zero_tail_kernel(float* __restrict__ out, long long npix, int from, int cstride) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int n = cstride - from;
  if (i >= npix * n) return;
  out[(i / n) * cstride + from + i % n] = 0.f;
}

// pxt_unet_activation_stats: largest |x| over the finite values and the number of non-finite ones.  256 partials per
// layer, then one workgroup folds them (no atomics; max and an integer count do not depend on the order anyway).
__global__ __launch_bounds__(256) void stats_partial_kernel(const float* __restrict__ x, long long n4,
                                                            float2* __restrict__ partial) {
  __shared__ float s_m[4];
  __shared__ unsigned s_b[4];
  float m = 0.f;
  unsigned bad = 0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const float4 v = *(const float4*)(x + 4 * i);
    const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!(fabsf(e[j]) <= 3.402823466e38f)) ++bad;
      else m = fmaxf(m, fabsf(e[j]));
    }
  }
  for (int s = 32; s >= 1; s >>= 1) {
    m = fmaxf(m, __shfl_xor(m, s, 64));
    bad += __shfl_xor(bad, s, 64);
  }
  if ((threadIdx.x & 63) == 0) { s_m[threadIdx.x >> 6] = m; s_b[threadIdx.x >> 6] = bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) { m = fmaxf(m, s_m[w]); bad += s_b[w]; }
    partial[blockIdx.x] = make_float2(m, __uint_as_float(bad));
  }
}

__global__ void stats_final_kernel(const float2* __restrict__ partial, int n, float* __restrict__ stats) {
  if (threadIdx.x != 0) return;
  float m = 0.f;
  unsigned bad = 0;
  for (int i = 0; i < n; ++i) { m = fmaxf(m, partial[i].x); bad += __float_as_uint(partial[i].y); }
  stats[0] = m;
  stats[1] = __uint_as_float(bad);
}

// ---- host side ---------------------------------------------------------------------------------------------------
struct Layer { int cin, cout; const float* w; const float* b; };

struct EncBlockF32 { int first, n; };
constexpr EncBlockF32 kEncF32[5] = {{0, 2}, {2, 2}, {4, 3}, {7, 3}, {10, 3}};
inline int block_of(int li) { int b = 4; while (kEncF32[b].first > li) --b; return b; }

inline size_t align256(size_t n) { return (n + 255) / 256 * 256; }

}  // namespace f32k

struct UnetF32 {
  void* dev = nullptr;     // every device array of the context, one allocation
  void* stats = nullptr;   // float2 [17][kStatsBlocks] partials of pxt_unet_activation_stats
  f32k::Layer conv[f32k::kNumConv];
  f32k::Layer head[f32k::kNumHeads];  // w: [32 NT][cin], b: [32 NT]
};

namespace f32k {

struct PlanF32 {
  int h[5], w[5], dh[4], dw[4];
  size_t enc[13], pool[5], upcat, dec[4], total;
};

bool make_plan(const UnetF32* net, int n, int H, int W, PlanF32& P) {
  if (n < 1 || n > PXT_UNET_MAX_BATCH || H < 1 || W < 1) return false;
  P.h[0] = H; P.w[0] = W;
  for (int b = 1; b < 5; ++b) { P.h[b] = P.h[b - 1] / 2; P.w[b] = P.w[b - 1] / 2; }
  if (P.h[4] < 1 || P.w[4] < 1) return false;
  int ph = P.h[4], pw = P.w[4];
  for (int d = 0; d < 4; ++d) { ph *= 2; pw *= 2; P.dh[d] = ph; P.dw[d] = pw; }
  size_t off = 0;
  auto take = [&](size_t floats) { const size_t o = off; off = align256(off + floats * sizeof(float)); return o; };
  for (int li = 0; li < 13; ++li) {
    const int b = block_of(li);
    if (li == kEncF32[b].first) P.pool[b] = b > 0 ? take((size_t)n * P.h[b] * P.w[b] * net->conv[li].cin) : 0;
    P.enc[li] = take((size_t)n * P.h[b] * P.w[b] * net->conv[li].cout);
  }
  size_t up = 0;
  for (int d = 0; d < 4; ++d) {
    up = std::max(up, (size_t)n * P.dh[d] * P.dw[d] * net->conv[13 + d].cin);
    P.dec[d] = take((size_t)n * P.dh[d] * P.dw[d] * net->conv[13 + d].cout);
  }
  P.upcat = take(up);
  P.total = off;
  return true;
}

// Tile configuration by output channels and map size (never by batch size; nor does it change a bit: see the top).
template <int CB, int PB, int WC, int WP>
void launch_conv_cfg(const float* in, int n, int H, int W, int cin, const float* wpk, const float* bias, int cout,
                     int relu, float* out, hipStream_t s) {
  constexpr int TH = 2 * PB * WP;
  const unsigned tiles = (unsigned)(((H + TH - 1) / TH) * ((W + 15) / 16));
  hipLaunchKernelGGL((conv3x3_f32_kernel<CB, PB, WC, WP>), dim3(tiles, cout / (32 * CB * WC), n), dim3(256), 0, s, in, H, W,
                     cin, (const float4*)wpk, bias, cout, relu, out);
}

// The configurations, numbered from 1 in the order launch_conv lists them, and the output channels one workgroup of each
// covers (32 CB WC): 1 = <2,2,2,2>, 2 = <2,1,2,2>, 3 = <2,2,1,4>, 4 = <2,1,1,4>, 5 = <1,2,1,4>.
constexpr int kNumCfg = 5;
constexpr int kCfgSpan[kNumCfg + 1] = {0, 128, 128, 64, 64, 32};

// The configuration a layer of H x W with cout output channels runs (host arithmetic; launch_conv and the layer views
// both ask here), PXT_E_ARG for a shape launch_conv refuses.
int f32_conv_cfg(int H, int W, int cout) {
  if (cout < 32 || cout % 32 != 0 || H < 1 || W < 1) return PXT_E_ARG;
  const long long px16 = (long long)((H + 15) / 16) * ((W + 15) / 16);  // 16 x 16 tiles of one image
  if (cout % 128 == 0) return px16 * 2 * (cout / 128) >= 1024 ? 1 : 2;
  if (cout % 64 == 0) return px16 * (cout / 64) >= 1024 ? 3 : 4;
  return 5;
}

// cfg 0: the configuration f32_conv_cfg picks; 1..5: that one (tests), refused when cout is no multiple of its span.
int launch_conv(const float* in, int n, int H, int W, int cin, const float* wpk, const float* bias, int cout, int relu,
                float* out, hipStream_t s, int cfg = 0) {
  if (cin < kKC || cin % kKC != 0) return PXT_E_ARG;
  const int planned = f32_conv_cfg(H, W, cout);
  if (planned < 0) return planned;
  if (cfg == 0) cfg = planned;
  if (cfg < 1 || cfg > kNumCfg || cout % kCfgSpan[cfg] != 0) return PXT_E_ARG;
  switch (cfg) {
    case 1: launch_conv_cfg<2, 2, 2, 2>(in, n, H, W, cin, wpk, bias, cout, relu, out, s); break;
    case 2: launch_conv_cfg<2, 1, 2, 2>(in, n, H, W, cin, wpk, bias, cout, relu, out, s); break;
    case 3: launch_conv_cfg<2, 2, 1, 4>(in, n, H, W, cin, wpk, bias, cout, relu, out, s); break;
    case 4: launch_conv_cfg<2, 1, 1, 4>(in, n, H, W, cin, wpk, bias, cout, relu, out, s); break;
    default: launch_conv_cfg<1, 2, 1, 4>(in, n, H, W, cin, wpk, bias, cout, relu, out, s); break;
  }
  return PXT_OK;
}

void launch_head(const Layer& L, const float* in, long long npix, int n, float* const* out_maps, int k,
                 const int32_t out_cstride[3], const int32_t* normalize, hipStream_t s) {
  HeadOutF32 ho;
  for (int i = 0; i < n; ++i) { ho.out[i] = out_maps[3 * i + k]; ho.normalize[i] = normalize[i]; }
  const long long waves = (npix + 31) / 32;
  const dim3 grid((unsigned)((waves + 3) / 4), n);
  const int rows = (L.cout + 1 + 31) / 32 * 32;
  if (rows == 32)
    hipLaunchKernelGGL(head_f32_kernel<1>, grid, dim3(256), 0, s, in, npix, L.cin, L.w, L.b, L.cout, ho, out_cstride[k]);
  else if (rows == 64)
    hipLaunchKernelGGL(head_f32_kernel<2>, grid, dim3(256), 0, s, in, npix, L.cin, L.w, L.b, L.cout, ho, out_cstride[k]);
  else if (rows <= 96)
    hipLaunchKernelGGL(head_f32_kernel<3>, grid, dim3(256), 0, s, in, npix, L.cin, L.w, L.b, L.cout, ho, out_cstride[k]);
  else if (rows <= 128)
    hipLaunchKernelGGL(head_f32_kernel<4>, grid, dim3(256), 0, s, in, npix, L.cin, L.w, L.b, L.cout, ho, out_cstride[k]);
  else
    hipLaunchKernelGGL(head_f32_kernel<5>, grid, dim3(256), 0, s, in, npix, L.cin, L.w, L.b, L.cout, ho, out_cstride[k]);
  if (out_cstride[k] > rows)
    for (int i = 0; i < n; ++i)
      hipLaunchKernelGGL(zero_tail_kernel, dim3((unsigned)((npix * (out_cstride[k] - rows) + 255) / 256)), dim3(256), 0, s,
                         out_maps[3 * i + k], npix, rows, out_cstride[k]);
}

}  // namespace f32k

using namespace f32k;

int f32_create(const void* weights_host, int64_t n_bytes, UnetF32** out) {
  if (!weights_host || !out || n_bytes < 64) return PXT_E_ARG;
  const char* p = (const char*)weights_host;
  if (std::memcmp(p, "PXTUNF32", 8) != 0) return PXT_E_ARG;
  int32_t n_conv, n_heads;
  std::memcpy(&n_conv, p + 8, 4);
  std::memcpy(&n_heads, p + 12, 4);
  if (n_conv != kNumConv || n_heads != kNumHeads) return PXT_E_ARG;
  int32_t dims[2 * (kNumConv + kNumHeads)];
  std::memcpy(dims, p + 16, sizeof(dims));
  int64_t table[4 * (kNumConv + kNumHeads)];
  if (16 + (int64_t)sizeof(dims) + (int64_t)sizeof(table) > n_bytes) return PXT_E_ARG;
  std::memcpy(table, p + 16 + sizeof(dims), sizeof(table));
  for (int i = 0; i < 2 * (kNumConv + kNumHeads); ++i)
    if (table[2 * i] < 0 || table[2 * i + 1] < 0 || table[2 * i] + table[2 * i + 1] > n_bytes || (table[2 * i] % 16) != 0)
      return PXT_E_ARG;
  // shapes: the VGG16-UNet wiring the forward pass assumes, every array the size its shape gives
  for (int i = 0; i < kNumConv + kNumHeads; ++i) {
    const int cin = dims[2 * i], cout = dims[2 * i + 1];
    if (cin < 1 || cout < 1 || cin > 4096 || cout > 4096) return PXT_E_ARG;
    const int64_t want_w = i < kNumConv ? (int64_t)cout * 9 * cin * 4 : (int64_t)cin * (cout + 1) * 4;
    const int64_t want_b = i < kNumConv ? (int64_t)cout * 4 : (int64_t)(cout + 1) * 4;
    if (table[4 * i + 1] != want_w || table[4 * i + 3] != want_b) return PXT_E_ARG;
  }
  bool ok = dims[0] == 3 && dims[1] == 64;
  for (int i = 1; i < kNumConv; ++i) ok = ok && dims[2 * i] % kKC == 0 && dims[2 * i + 1] % 32 == 0;
  for (int i = 0; i < kNumHeads; ++i) {
    const int cin = dims[2 * (kNumConv + i)], cout = dims[2 * (kNumConv + i) + 1];
    ok = ok && cin % 8 == 0 && cout + 1 <= 160;
  }
  if (!ok) return PXT_E_ARG;

  // one host image of every device array: layer 0 taps [27][64], packed taps of layers 1..16, biases, heads
  std::vector<float> hb;
  size_t woff[kNumConv], boff[kNumConv], hwoff[kNumHeads], hboff[kNumHeads];
  auto reserve = [&](size_t floats) { const size_t o = hb.size(); hb.resize((o + floats + 63) / 64 * 64, 0.f); return o; };
  for (int i = 0; i < kNumConv; ++i) {
    const int cin = dims[2 * i], cout = dims[2 * i + 1];
    const float* W = (const float*)(p + table[4 * i]);
    const float* B = (const float*)(p + table[4 * i + 2]);
    woff[i] = reserve((size_t)cout * 9 * cin);
    float* wd = hb.data() + woff[i];
    if (i == 0) {
      for (int co = 0; co < 64; ++co)
        for (int k = 0; k < 27; ++k) wd[(size_t)k * 64 + co] = W[(size_t)co * 27 + k];
    } else {
      const long long n = (long long)cout * 9 * cin;
      for (long long d = 0; d < n; ++d) {
        int co, tap, ci;
        packed_f32_source(d, cin, co, tap, ci);
        wd[d] = W[((size_t)co * 9 + tap) * cin + ci];
      }
    }
    boff[i] = reserve(cout);
    std::memcpy(hb.data() + boff[i], B, (size_t)cout * 4);
  }
  for (int i = 0; i < kNumHeads; ++i) {
    const int cin = dims[2 * (kNumConv + i)], co1 = dims[2 * (kNumConv + i) + 1] + 1;
    const int rows = (co1 + 31) / 32 * 32;
    const float* W = (const float*)(p + table[4 * (kNumConv + i)]);      // [cin][co1]
    const float* B = (const float*)(p + table[4 * (kNumConv + i) + 2]);  // [co1]
    hwoff[i] = reserve((size_t)rows * cin);
    float* wd = hb.data() + hwoff[i];
    for (int r = 0; r < co1; ++r)
      for (int k = 0; k < cin; ++k) wd[(size_t)r * cin + k] = W[(size_t)k * co1 + r];
    hboff[i] = reserve(rows);
    std::memcpy(hb.data() + hboff[i], B, (size_t)co1 * 4);
  }
  UnetF32* net = new UnetF32();
  hipError_t e = hipMalloc(&net->dev, hb.size() * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(net->dev, hb.data(), hb.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc(&net->stats, (size_t)kNumConv * kStatsBlocks * sizeof(float2));
  if (e != hipSuccess) { set_last_error("fp32 unet weights", e); f32_destroy(net); return PXT_E_HIP; }
  const float* d = (const float*)net->dev;
  for (int i = 0; i < kNumConv; ++i) net->conv[i] = {dims[2 * i], dims[2 * i + 1], d + woff[i], d + boff[i]};
  for (int i = 0; i < kNumHeads; ++i)
    net->head[i] = {dims[2 * (kNumConv + i)], dims[2 * (kNumConv + i) + 1], d + hwoff[i], d + hboff[i]};
  *out = net;
  return PXT_OK;
}

void f32_destroy(UnetF32* net) {
  if (!net) return;
  if (net->dev) (void)hipFree(net->dev);
  if (net->stats) (void)hipFree(net->stats);
  delete net;
}

int64_t f32_workspace_bytes_batch(const UnetF32* net, int n, int H, int W) {
  PlanF32 P;
  if (!make_plan(net, n, H, W, P)) return 0;
  return (int64_t)P.total;
}

int64_t f32_workspace_bytes_pair(const UnetF32* net, const int32_t H[2], const int32_t W[2]) {
  PlanF32 P0, P1;
  if (!make_plan(net, 1, H[0], W[0], P0) || !make_plan(net, 1, H[1], W[1], P1)) return 0;
  return (int64_t)(align256(P0.total) + P1.total);
}

int f32_forward_batch(UnetF32* net, int n, const void* const* images, const int32_t* image_is_u8,
                      const uint8_t* const* masks, int H, int W, float* const* out_maps, const int32_t out_cstride[3],
                      const int32_t* normalize, void* workspace, hipStream_t s) {
  PlanF32 P;
  if (!make_plan(net, n, H, W, P)) return PXT_E_ARG;
  for (int i = 0; i < n; ++i) {
    if (!images[i]) return PXT_E_ARG;
    for (int k = 0; k < 3; ++k)
      if (!out_maps[3 * i + k]) return PXT_E_ARG;
  }
  for (int k = 0; k < 3; ++k)
    if (out_cstride[k] < net->head[k].cout + 1 || (out_cstride[k] % 4) != 0) return PXT_E_ARG;
  char* ws = (char*)workspace;
  auto buf = [&](size_t off) { return (float*)(ws + off); };
  // encoder
  {
    FirstImagesF32 fi;
    for (int i = 0; i < n; ++i) { fi.image[i] = images[i]; fi.mask[i] = masks ? masks[i] : nullptr; fi.is_u8[i] = image_is_u8[i]; }
    const Layer& L0 = net->conv[0];
    hipLaunchKernelGGL(conv_first_f32_kernel, dim3((unsigned)(((long long)H * W + 255) / 256), n), dim3(256), 0, s, fi, H, W,
                       L0.w, L0.b, buf(P.enc[0]));
  }
  const float* x = buf(P.enc[0]);
  for (int li = 1; li < 13; ++li) {
    const int b = block_of(li);
    const Layer& L = net->conv[li];
    if (li == kEncF32[b].first) {
      const long long cnt = (long long)n * P.h[b] * P.w[b] * (L.cin / 4);
      hipLaunchKernelGGL(maxpool2_f32_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, x, P.h[b - 1], P.w[b - 1],
                         L.cin, buf(P.pool[b]), P.h[b], P.w[b], n);
      x = buf(P.pool[b]);
    }
    const int rc = launch_conv(x, n, P.h[b], P.w[b], L.cin, L.w, L.b, L.cout, 1, buf(P.enc[li]), s);
    if (rc != PXT_OK) return rc;
    x = buf(P.enc[li]);
  }
  // decoder: upsample + crop + concat into one buffer, then the convolution (BatchNorm folded into taps and bias)
  const int skip_layer[4] = {9, 6, 3, 1};  // last layer of encoder blocks 3, 2, 1, 0
  int ph = P.h[4], pw = P.w[4];
  for (int d = 0; d < 4; ++d) {
    const Layer& L = net->conv[13 + d];
    const Layer& Lp = net->conv[12 + d];  // enc4, then the previous decoder layer
    const Layer& Ls = net->conv[skip_layer[d]];
    const int sb = 3 - d;
    if (Lp.cout + Ls.cout != L.cin || Lp.cout % 4 != 0) return PXT_E_ARG;
    const long long cnt = (long long)n * P.dh[d] * P.dw[d] * (L.cin / 4);
    hipLaunchKernelGGL(upcat_f32_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, x, ph, pw, Lp.cout,
                       (const float*)buf(P.enc[skip_layer[d]]), P.h[sb], P.w[sb], Ls.cout, buf(P.upcat), P.dh[d], P.dw[d], n);
    const int rc = launch_conv(buf(P.upcat), n, P.dh[d], P.dw[d], L.cin, L.w, L.b, L.cout, 1, buf(P.dec[d]), s);
    if (rc != PXT_OK) return rc;
    x = buf(P.dec[d]);
    ph = P.dh[d]; pw = P.dw[d];
  }
  // heads at strides 1, 4, 16: dec3, dec1, enc4
  if (net->head[0].cin != net->conv[16].cout || net->head[1].cin != net->conv[14].cout || net->head[2].cin != net->conv[12].cout)
    return PXT_E_ARG;
  launch_head(net->head[0], buf(P.dec[3]), (long long)P.dh[3] * P.dw[3], n, out_maps, 0, out_cstride, normalize, s);
  launch_head(net->head[1], buf(P.dec[1]), (long long)P.dh[1] * P.dw[1], n, out_maps, 1, out_cstride, normalize, s);
  launch_head(net->head[2], buf(P.enc[12]), (long long)P.h[4] * P.w[4], n, out_maps, 2, out_cstride, normalize, s);
  PXT_HIP_CHECK(hipGetLastError());
  return PXT_OK;
}

int f32_forward_pair(UnetF32* net, const void* const* images, const int32_t* image_is_u8, const uint8_t* const* masks,
                     const int32_t H[2], const int32_t W[2], float* const* out_maps, const int32_t out_cstride[3],
                     const int32_t* normalize, void* workspace, hipStream_t s) {
  PlanF32 P0, P1;
  if (!make_plan(net, 1, H[0], W[0], P0) || !make_plan(net, 1, H[1], W[1], P1)) return PXT_E_ARG;
  const uint8_t* const no_mask[1] = {nullptr};
  const size_t second = align256(P0.total);
  for (int im = 0; im < 2; ++im) {  // one after the other on the caller's stream: image 0's maps are complete first
    const int rc = f32_forward_batch(net, 1, images + im, image_is_u8 + im, masks ? masks + im : no_mask, H[im], W[im],
                                     out_maps + 3 * im, out_cstride, normalize + im, (char*)workspace + (im ? second : 0), s);
    if (rc != PXT_OK) return rc;
  }
  return PXT_OK;
}

int f32_activation_stats(UnetF32* net, int H, int W, const void* workspace, float* stats, hipStream_t s) {
  PlanF32 P;
  if (!make_plan(net, 1, H, W, P)) return PXT_E_ARG;
  const char* ws = (const char*)workspace;
  float2* partial = (float2*)net->stats;
  for (int li = 0; li < kNumConv; ++li) {
    size_t off;
    long long n;
    if (li < 13) {
      const int b = block_of(li);
      off = P.enc[li];
      n = (long long)P.h[b] * P.w[b] * net->conv[li].cout;
    } else {
      off = P.dec[li - 13];
      n = (long long)P.dh[li - 13] * P.dw[li - 13] * net->conv[li].cout;
    }
    hipLaunchKernelGGL(stats_partial_kernel, dim3(kStatsBlocks), dim3(256), 0, s, (const float*)(ws + off), n / 4,
                       partial + (size_t)li * kStatsBlocks);
    hipLaunchKernelGGL(stats_final_kernel, dim3(1), dim3(64), 0, s, (const float2*)(partial + (size_t)li * kStatsBlocks),
                       kStatsBlocks, stats + 2 * li);
  }
  PXT_HIP_CHECK(hipGetLastError());
  return PXT_OK;
}

// Where f32_forward_batch leaves every buffer of a pass, from the same make_plan, and the configuration launch_conv
// takes for each 3x3 layer, from the same f32_conv_cfg (host arithmetic only, nothing is launched).
int f32_layer_views(const UnetF32* net, int n, int H, int W, pxt_unet_layer_view* out) {
  PlanF32 P;
  if (!net || !out || !make_plan(net, n, H, W, P)) return PXT_E_ARG;
  std::memset(out, 0, (kNumConv + 5) * sizeof(pxt_unet_layer_view));
  auto fill = [&](pxt_unet_layer_view& v, size_t off, int h, int w, int c) {
    v.offset = (int64_t)off; v.h = h; v.w = w; v.c = c; v.in_memory = 1; v.splits = 1;
  };
  for (int li = 0; li < kNumConv; ++li) {
    pxt_unet_layer_view& v = out[li];
    if (li < 13) {
      const int b = block_of(li);
      fill(v, P.enc[li], P.h[b], P.w[b], net->conv[li].cout);
    } else {
      fill(v, P.dec[li - 13], P.dh[li - 13], P.dw[li - 13], net->conv[li].cout);
      v.decoder = 1;
    }
    if (li == 0) continue;  // (conv_first_f32_kernel: no tile configuration)
    const int cfg = f32_conv_cfg(v.h, v.w, v.c);
    if (cfg < 0) return cfg;
    v.cfg = cfg;
  }
  for (int b = 1; b < 5; ++b)  // the pooled input of block b (maxpool2_f32_kernel)
    fill(out[kNumConv + b - 1], P.pool[b], P.h[b], P.w[b], net->conv[kEncF32[b].first].cin);
  // the decoder-input buffer, shared by the four decoder layers: what the last one's upcat_f32_kernel left in it
  fill(out[kNumConv + 4], P.upcat, P.dh[3], P.dw[3], net->conv[16].cin);
  return PXT_OK;
}

}  // namespace pxt

extern "C" int pxt_conv3x3_f32_cfg(int32_t H, int32_t W, int32_t Cout) { return pxt::f32k::f32_conv_cfg(H, W, Cout); }

// ---------------------------------------------------------------------------
// One fp32 3x3 convolution of the pass as a stand-alone call (layer parity tests against F.conv2d).
// ---------------------------------------------------------------------------
extern "C" int pxt_conv3x3_nhwc_f32(const void* in, int32_t H, int32_t W, int32_t Cin, const void* weights,
                                    const float* bias, int32_t Cout, int32_t relu, void* out, void* stream) {
  return pxt_conv3x3_nhwc_f32_cfg(in, H, W, Cin, weights, bias, Cout, relu, out, 0, stream);
}

extern "C" int pxt_conv3x3_nhwc_f32_cfg(const void* in, int32_t H, int32_t W, int32_t Cin, const void* weights,
                                        const float* bias, int32_t Cout, int32_t relu, void* out, int32_t cfg,
                                        void* stream) {
  using namespace pxt::f32k;
  if (!in || !weights || !bias || !out || H < 1 || W < 1) return PXT_E_ARG;
  if (cfg < 0 || cfg > kNumCfg || (cfg > 0 && Cout % kCfgSpan[cfg] != 0)) return PXT_E_ARG;
  if (Cin < kKC || Cin % kKC != 0 || Cout < 32 || Cout % 32 != 0) return PXT_E_ARG;
  const long long n = (long long)Cout * 9 * Cin;
  // the taps are repacked on every call into a scratch that lives as long as the process (the pyramid packs once)
  static void* scratch = nullptr;
  static long long scratch_n = 0;
  if (scratch_n < n) {
    PXT_HIP_CHECK(hipDeviceSynchronize());
    if (scratch) (void)hipFree(scratch);
    scratch = nullptr;
    scratch_n = 0;
    PXT_HIP_CHECK(hipMalloc(&scratch, (size_t)n * sizeof(float)));
    scratch_n = n;
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(pack_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float*)weights, Cin, Cout,
                     (float*)scratch);
  const int rc = launch_conv((const float*)in, 1, H, W, Cin, (const float*)scratch, bias, Cout, relu, (float*)out, s, cfg);
  if (rc != PXT_OK) return rc;
  PXT_HIP_CHECK(hipGetLastError());
  return PXT_OK;
}

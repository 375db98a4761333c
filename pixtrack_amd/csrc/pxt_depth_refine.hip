// Sensor-depth pose refinement behind the LM (pxt_depth_refine, include/pixtrack_hip.h): a damped Gauss-Newton on
//   r_n(T) = D(project(T X_n)) - (T X_n).z
// D being the depth sensor's image (raw uint16 counts x sensor_scale) read through the LM's bilinear footprint.  The
// feature-metric LM leaves the translation along the viewing ray weakly determined; the depth image measures exactly
// that direction.  Projection, validity, the bilinear weights, the robust loss and the 2 x 6 point Jacobian are
// pxt_lm_point.h's; F, gx, gy are formed as PXT_LM_POINT_CH forms them (five bilinear values over the 12-tap cross,
// central differences), on ONE channel: the depth.
//
// Shape
//  * One workgroup of 1024 threads per problem (blockIdx.x), all iterations in one launch.  Point n belongs to thread
//    n % 1024; a thread keeps its 35 sums (cost, n_valid, g 6, H 21, reject counts 6) over its rounds in registers.
//  * Fold, in a fixed order: the 16-lane DPP tree (lm_row16_sum), the wave's four rows (xor 16, xor 32), the 16 waves'
//    partials through LDS added by wave index.  No atomics: a problem's bits depend on that problem alone.
//  * Thread 0 adds the prior, solves (the LM's damped Cholesky with the pivoted-LU fallback), updates the pose and tests
//    the LM's stop rule; the pose goes back to everybody through LDS.  Two barriers per evaluation besides the fold's.
//  * The parameter records travel as kernel arguments for up to two problems, else through a pinned staging slot to the
//    workspace ahead of the launch (StageRing, as the evaluation kernels do).
//
// solve6 and apply_delta restate pxt_lm.hip's (they live in that file, whose kernel's code must not move): the same
// operations in the same order.  The LU fallback is written without run-time indices so that it stays in registers.
#include "pxt_lm_eval.h"

namespace pxt {
namespace {

constexpr int kDrBlock = 1024;
constexpr int kDrWaves = kDrBlock / PXT_WAVE;
constexpr int kDrAcc = 35;     // 0 sum rho, 1 n_valid, 2..7 g, 8..28 upper H, 29..34 counts of reject codes 1..6
constexpr int kDrStride = 37;  // odd: the waves' partials of one sum lie in distinct LDS banks

struct DrParams {  // 208 bytes
  const float* p3d;
  const uint8_t* mask;
  const uint16_t* sensor;
  const float* pose;
  float* out;
  float* log;
  uint8_t* codes;
  int n, w, h, ndist, pose_is_record;
  float sensor_scale;
  float cam[10];
  float prior[21];
  int pad_[1];
};
static_assert(sizeof(DrParams) == 208, "parameter records are read as aligned vectors");

struct DrConf {
  int num_iters, pad, loss, min_valid;
  float loss_alpha, loss_scale, max_residual, max_edge, grad_stop, dt_stop, dR_stop;
  float lambda[6];
};

struct DrShared {
  float part[kDrWaves * kDrStride];
  float tot[kDrAcc + 1];
  float T[12];
  float a[6];     // the sum of the deltas applied so far
  float rec[12];  // words 12..23 of the record
  int flag;       // 0 go on, 1 the next evaluation is the last, 2 done
};

// project_point's "in front of the camera" and "inside the distortion model's range" tests, for reject code 2 (as
// pxt_lm_report.hip tells 2 from 3; validity itself is point_in_window's).
__device__ inline bool dr_projectable(const Cam& c, float x, float y, float z) {
  if (!(z > kCamEps)) return false;
  if (c.ndist <= 0) return true;
  const float iz = 1.0f / fmaxf(z, kCamEps);
  const float xn = x * iz, yn = y * iz;
  const float r2 = xn * xn + yn * yn;
  const float disc = 9.f * c.k1 * c.k1 - 20.f * c.k2;
  const bool limited = ((c.k2 > 0.f) && (disc > 0.f)) || ((c.k2 <= 0.f) && (c.k1 > 0.f));
  if (!limited) return true;
  const float limit = (c.k2 > 0.f) ? (sqrtf(fmaxf(disc, 0.f)) - 3.f * c.k1) / (10.f * c.k2) : 1.f / (3.f * c.k1);
  return r2 < fabsf(limit);
}

// Damped 6x6 solve, pxt_lm.hip's solve6 restated: tot = g (6) then the upper triangle of H (21);
// H_kk += max(H_kk * lambda_k, 1e-6); Cholesky (one refined reciprocal square root per pivot), pivoted LU on [H | g]
// when a pivot is not positive.  Returns true when Cholesky held.
__device__ inline bool dr_solve6(const float* tot, const float* lambda, float* delta) {
  float Hm[6][6], g[6];
  int idx = 6;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    g[k] = tot[k];
#pragma unroll
    for (int l = k; l < 6; ++l) {
      Hm[k][l] = tot[idx];
      Hm[l][k] = tot[idx];
      ++idx;
    }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) Hm[k][k] += fmaxf(Hm[k][k] * lambda[k], 1e-6f);
  float Lm[6][6], inv[6];
  bool chol_ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    float d = Hm[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= Lm[j][k] * Lm[j][k];
    chol_ok = chol_ok && (d > 0.f);
    const float r0 = __builtin_amdgcn_rsqf(d);
    const float rj = r0 * (1.5f - (0.5f * d) * (r0 * r0));
    Lm[j][j] = d * rj;
    inv[j] = rj;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      float s = Hm[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= Lm[i][k] * Lm[j][k];
      Lm[i][j] = s * inv[j];
    }
  }
  if (chol_ok) {
    float y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      float s = g[i];
#pragma unroll
      for (int k = 0; k < i; ++k) s -= Lm[i][k] * y[k];
      y[i] = s * inv[i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
      float s = y[i];
#pragma unroll
      for (int k = i + 1; k < 6; ++k) s -= Lm[k][i] * delta[k];
      delta[i] = s * inv[i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) delta[i] = -delta[i];
    return true;
  }
  // LU with partial pivoting on [H | g]; the row exchange by selects over compile-time indices.
  float A[6][7];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = 0; j < 6; ++j) A[i][j] = Hm[i][j];
    A[i][6] = g[i];
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    int piv = c;
    float best = fabsf(A[c][c]);
#pragma unroll
    for (int r = c + 1; r < 6; ++r)
      if (fabsf(A[r][c]) > best) {
        best = fabsf(A[r][c]);
        piv = r;
      }
#pragma unroll
    for (int r = c + 1; r < 6; ++r) {
      const bool swap = piv == r;
#pragma unroll
      for (int j = 0; j < 7; ++j) {
        const float x = A[c][j], y = A[r][j];
        A[c][j] = swap ? y : x;
        A[r][j] = swap ? x : y;
      }
    }
#pragma unroll
    for (int r = c + 1; r < 6; ++r) {
      const float f = A[r][c] / A[c][c];
#pragma unroll
      for (int j = c; j < 7; ++j) A[r][j] -= f * A[c][j];
    }
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    float s = A[i][6];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) s -= A[i][k] * delta[k];
    delta[i] = s / A[i][i];
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) delta[i] = -delta[i];
  return false;
}

// T <- (so3exp(dw), dt) @ T; (dR deg, dt) of the step: pxt_lm.hip's apply_delta restated.
__device__ inline void dr_apply_delta(const float* delta, float* T, float& dR_deg, float& dt_mag) {
  const float wx = delta[3], wy = delta[4], wz = delta[5];
  const float theta = sqrtf(wx * wx + wy * wy + wz * wz);
  float Rd[9];
  if (theta < 1e-7f) {
    Rd[0] = 1.f; Rd[1] = -wz; Rd[2] = wy;
    Rd[3] = wz;  Rd[4] = 1.f; Rd[5] = -wx;
    Rd[6] = -wy; Rd[7] = wx;  Rd[8] = 1.f;
  } else {
    const float it = 1.0f / theta;
    const float x = wx * it, y = wy * it, z = wz * it;
    float s, c1;
    if (theta < 0.25f) {
      const float q = theta * theta;
      s = theta * (1.f + q * (-1.f / 6.f + q * (1.f / 120.f + q * (-1.f / 5040.f + q * (1.f / 362880.f)))));
      c1 = q * (0.5f + q * (-1.f / 24.f + q * (1.f / 720.f + q * (-1.f / 40320.f + q * (1.f / 3628800.f)))));
    } else {
      s = sinf(theta);
      c1 = 1.f - cosf(theta);
    }
    Rd[0] = 1.f + c1 * (x * x - 1.f);
    Rd[1] = -s * z + c1 * (x * y);
    Rd[2] = s * y + c1 * (x * z);
    Rd[3] = s * z + c1 * (x * y);
    Rd[4] = 1.f + c1 * (y * y - 1.f);
    Rd[5] = -s * x + c1 * (y * z);
    Rd[6] = -s * y + c1 * (x * z);
    Rd[7] = s * x + c1 * (y * z);
    Rd[8] = 1.f + c1 * (z * z - 1.f);
  }
  float Tn[12];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      Tn[3 * i + j] = Rd[3 * i] * T[j] + Rd[3 * i + 1] * T[3 + j] + Rd[3 * i + 2] * T[6 + j];
    Tn[9 + i] = Rd[3 * i] * T[9] + Rd[3 * i + 1] * T[10] + Rd[3 * i + 2] * T[11] + delta[i];
  }
#pragma unroll
  for (int i = 0; i < 12; ++i) T[i] = Tn[i];
  const float tr = Rd[0] + Rd[4] + Rd[8];
  const float cs = fminf(fmaxf((tr - 1.f) * 0.5f, -1.f), 1.f);
  dR_deg = fabsf(acosf(cs)) / 3.14159265358979323846f * 180.f;
  dt_mag = sqrtf(delta[0] * delta[0] + delta[1] * delta[1] + delta[2] * delta[2]);
}

// Raw count at (x, y), 0 outside the image; the address is formed for positions inside only.
__device__ __forceinline__ unsigned dr_tap(const uint16_t* sensor, int x, int y, int W, int H) {
  const bool in = x >= 0 && x < W && y >= 0 && y < H;
  const int xc = min(max(x, 0), W - 1), yc = min(max(y, 0), H - 1);
  const unsigned raw = sensor[yc * W + xc];
  return in ? raw : 0u;
}

__global__ __launch_bounds__(kDrBlock) void depth_refine_kernel(const EvalArgs<DrParams> args, const DrParams* ws_params,
                                                                const DrConf cf, const int from_args) {
  __shared__ DrShared sh;
  const int tid = threadIdx.x;
  const DrParams* q = eval_params(ws_params, from_args, (int)blockIdx.x);
  float* out = uniform(q->out);
  {
    float T0[12];
    if (!eval_load_pose(q, T0)) {  // the LM record failed or timed out: only the status word is written
      if (tid == 0) __hip_atomic_store(&out[31], -1.f, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      return;
    }
    if (tid == 0) {
#pragma unroll
      for (int i = 0; i < 12; ++i) sh.T[i] = T0[i];
#pragma unroll
      for (int i = 0; i < 6; ++i) sh.a[i] = 0.f;
      sh.flag = 0;
    }
  }
  const int N = uniform(q->n), W = uniform(q->w), H = uniform(q->h);
  float c10[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) c10[i] = uniform(q->cam[i]);
  const Cam cam = make_cam(c10, uniform(q->ndist));
  const float* p3d = uniform(q->p3d);
  const uint8_t* mask = uniform(q->mask);
  const uint16_t* sensor = uniform(q->sensor);
  float* log = uniform(q->log);
  uint8_t* codes = uniform(q->codes);
  const float scale = uniform(q->sensor_scale);
  const float pad = (float)cf.pad;
  const int lane = tid & (PXT_WAVE - 1), wave = tid / PXT_WAVE;
  __syncthreads();

#pragma unroll 1
  for (int ev = 0; ev <= cf.num_iters; ++ev) {
    float T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = uniform(sh.T[i]);  // scalars: every lane read the same words
    float acc[kDrAcc];
#pragma unroll
    for (int k = 0; k < kDrAcc; ++k) acc[k] = 0.f;
    uint8_t* row = codes ? codes + (size_t)ev * (size_t)N : nullptr;

#pragma unroll 1
    for (int n = tid; n < N; n += kDrBlock) {
      const float X = p3d[3 * n], Y = p3d[3 * n + 1], Z = p3d[3 * n + 2];
      const bool kept = mask ? mask[n] != 0 : true;
      float px, py, pz, u, v, Jw[6];
      transform_point(T, X, Y, Z, px, py, pz);
      bool valid = kept;
      point_in_window(cam, px, py, pz, valid, W, H, pad, u, v, Jw);
      int code = valid ? 0 : (!kept ? 1 : (!dr_projectable(cam, px, py, pz) ? 2 : 3));
      float r = 0.f, gx = 0.f, gy = 0.f;
      if (valid) {
        int ix0, iy0;
        float w00, w10, w01, w11;
        bilinear_weights(u, v, ix0, iy0, w00, w10, w01, w11);
        // the 12 raw counts of the cross: rows 0,3 use columns 1,2; rows 1,2 use columns 0..3
        const unsigned r01 = dr_tap(sensor, ix0, iy0 - 1, W, H), r02 = dr_tap(sensor, ix0 + 1, iy0 - 1, W, H);
        const unsigned r10 = dr_tap(sensor, ix0 - 1, iy0, W, H), r11 = dr_tap(sensor, ix0, iy0, W, H);
        const unsigned r12 = dr_tap(sensor, ix0 + 1, iy0, W, H), r13 = dr_tap(sensor, ix0 + 2, iy0, W, H);
        const unsigned r20 = dr_tap(sensor, ix0 - 1, iy0 + 1, W, H), r21 = dr_tap(sensor, ix0, iy0 + 1, W, H);
        const unsigned r22 = dr_tap(sensor, ix0 + 1, iy0 + 1, W, H), r23 = dr_tap(sensor, ix0 + 2, iy0 + 1, W, H);
        const unsigned r31 = dr_tap(sensor, ix0, iy0 + 2, W, H), r32 = dr_tap(sensor, ix0 + 1, iy0 + 2, W, H);
        const unsigned lo = min(min(min(r01, r02), min(r10, r11)), min(min(min(r12, r13), min(r20, r21)),
                                                                       min(min(r22, r23), min(r31, r32))));
        const unsigned hi = max(max(max(r01, r02), max(r10, r11)), max(max(max(r12, r13), max(r20, r21)),
                                                                       max(max(r22, r23), max(r31, r32))));
        if (lo == 0u) {
          code = 4;
        } else if ((float)(hi - lo) * scale > cf.max_edge) {
          code = 5;
        } else {
          const float a01 = (float)r01 * scale, a02 = (float)r02 * scale, a10 = (float)r10 * scale,
                      a11 = (float)r11 * scale, a12 = (float)r12 * scale, a13 = (float)r13 * scale,
                      a20 = (float)r20 * scale, a21 = (float)r21 * scale, a22 = (float)r22 * scale,
                      a23 = (float)r23 * scale, a31 = (float)r31 * scale, a32 = (float)r32 * scale;
          // PXT_LM_POINT_CH's first seven lines
          const float F = w00 * a11 + w10 * a12 + w01 * a21 + w11 * a22;
          const float Fxp = w00 * a12 + w10 * a13 + w01 * a22 + w11 * a23;
          const float Fxm = w00 * a10 + w10 * a11 + w01 * a20 + w11 * a21;
          const float Fyp = w00 * a21 + w10 * a22 + w01 * a31 + w11 * a32;
          const float Fym = w00 * a01 + w10 * a02 + w01 * a11 + w11 * a12;
          gx = 0.5f * (Fxp - Fxm);
          gy = 0.5f * (Fyp - Fym);
          r = F - pz;
          if (fabsf(r) > cf.max_residual) code = 6;
        }
      }
      if (row) row[n] = (uint8_t)code;
      if (code == 0) {
        float rho, wl;
        robust_loss(cf.loss, cf.loss_alpha, cf.loss_scale, r * r, rho, wl);
        float J0[6], J1[6], J[6];
        point_jacobian(Jw, px, py, pz, J0, J1);
#pragma unroll
        for (int k = 0; k < 6; ++k) J[k] = gx * J0[k] + gy * J1[k];
        // minus the p.z row of [I | -[p]x]: (0, 0, 1, p.y, -p.x, 0)
        J[2] -= 1.f;
        J[3] -= py;
        J[4] += px;
        acc[0] += rho;
        acc[1] += 1.f;
        const float wr = wl * r;
#pragma unroll
        for (int k = 0; k < 6; ++k) acc[2 + k] += wr * J[k];
        int idx = 8;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          const float wj = wl * J[k];
#pragma unroll
          for (int l = k; l < 6; ++l, ++idx) acc[idx] += wj * J[l];
        }
      } else {
#pragma unroll
        for (int c = 1; c <= 6; ++c) acc[28 + c] += (code == c) ? 1.f : 0.f;
      }
    }

    // fold: DPP row, the wave's four rows, the waves by index
#pragma unroll
    for (int k = 0; k < kDrAcc; ++k) {
      float s = lm_row16_sum(acc[k]);
      s += __shfl_xor(s, 16, PXT_WAVE);
      s += __shfl_xor(s, 32, PXT_WAVE);
      if (lane == 0) sh.part[wave * kDrStride + k] = s;
    }
    __syncthreads();
    if (tid < kDrAcc) {
      float s = 0.f;
      for (int w = 0; w < kDrWaves; ++w) s += sh.part[w * kDrStride + tid];
      sh.tot[tid] = s;
    }
    __syncthreads();

    if (tid == 0) {
      const float n_valid = sh.tot[1];
      const float mean = sh.tot[0] / fmaxf(n_valid, 1.f);
      if (ev == 0) {
        sh.rec[2] = mean;
        sh.rec[3] = n_valid;
      }
      const bool fail = n_valid < (float)cf.min_valid;
      if (fail || sh.flag == 1 || ev == cf.num_iters) {
        sh.rec[0] = fail ? 1.f : 0.f;
        sh.rec[1] = (float)ev;  // updates applied
        sh.rec[4] = mean;
        sh.rec[5] = n_valid;
        for (int c = 0; c < 6; ++c) sh.rec[6 + c] = sh.tot[29 + c];
        sh.flag = 2;
      } else {
        float t27[27], a[6];
        for (int k = 0; k < 6; ++k) a[k] = sh.a[k];
        const float* P = q->prior;
        float Pm[6][6];
        {
          int idx = 0;
          for (int k = 0; k < 6; ++k)
            for (int l = k; l < 6; ++l, ++idx) {
              const float p = P[idx];
              Pm[k][l] = p;
              Pm[l][k] = p;
              t27[6 + idx] = sh.tot[8 + idx] + p;
            }
        }
        for (int k = 0; k < 6; ++k) {
          float s = 0.f;
          for (int l = 0; l < 6; ++l) s += Pm[k][l] * a[l];
          t27[k] = sh.tot[2 + k] + s;
        }
        float delta[6];
        const bool chol = dr_solve6(t27, cf.lambda, delta);
        float Tn[12];
        for (int i = 0; i < 12; ++i) Tn[i] = T[i];
        float dR, dt;
        dr_apply_delta(delta, Tn, dR, dt);
        for (int i = 0; i < 12; ++i) sh.T[i] = Tn[i];
        for (int k = 0; k < 6; ++k) sh.a[k] = a[k] + delta[k];
        float gn = 0.f;
        for (int i = 0; i < 6; ++i) gn += t27[i] * t27[i];
        gn = sqrtf(gn);
        const bool small_step = (dt < cf.dt_stop) && (dR < cf.dR_stop);
        const bool small_grad = gn < cf.grad_stop;
        sh.flag = (small_step || small_grad) ? 1 : 0;
        if (log) {
          float* lg = log + (size_t)ev * PXT_DEPTH_LOG_STRIDE;
          lg[0] = mean;
          lg[1] = n_valid;
          lg[2] = dR;
          lg[3] = dt;
          lg[4] = gn;
          lg[5] = chol ? 0.f : 1.f;
          lg[6] = 0.f;
          lg[7] = 0.f;
          for (int i = 0; i < 12; ++i) lg[8 + i] = Tn[i];
        }
      }
    }
    __syncthreads();
    if (sh.flag == 2) break;
  }

  if (tid == 0) {
    for (int i = 0; i < 12; ++i) out[i] = sh.T[i];
    for (int i = 0; i < 12; ++i) out[12 + i] = sh.rec[i];
    for (int i = 0; i < 6; ++i) out[24 + i] = sh.a[i];
    out[30] = 0.f;
    __hip_atomic_store(&out[31], sh.rec[0] != 0.f ? -2.f : 1.f, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

size_t dr_params_bytes(int n_problems) { return ((size_t)n_problems * sizeof(DrParams) + 255) / 256 * 256; }

}  // namespace
}  // namespace pxt

using namespace pxt;

extern "C" int64_t pxt_depth_refine_workspace_bytes(int32_t n_problems) {
  if (n_problems < 1 || n_problems > PXT_DEPTH_MAX_PROBLEMS) return PXT_E_ARG;
  return (int64_t)dr_params_bytes(n_problems);
}

extern "C" int pxt_depth_refine(const pxt_depth_problem* problems, int32_t n_problems, const pxt_depth_conf* conf,
                                void* workspace, void* stream) {
  if (!problems || !conf || !workspace) return PXT_E_ARG;
  if (n_problems < 1 || n_problems > PXT_DEPTH_MAX_PROBLEMS) return PXT_E_ARG;
  if (((uintptr_t)workspace % 16) != 0) return PXT_E_ARG;
  if (conf->num_iters < 0 || conf->num_iters > PXT_DEPTH_MAX_ITERS || conf->pad < 0 || conf->loss < 0 || conf->loss > 2 ||
      conf->min_valid < 0)
    return PXT_E_ARG;
  DrConf cf;
  cf.num_iters = conf->num_iters; cf.pad = conf->pad; cf.loss = conf->loss; cf.min_valid = conf->min_valid;
  cf.loss_alpha = conf->loss_alpha; cf.loss_scale = conf->loss_scale;
  cf.max_residual = conf->max_residual; cf.max_edge = conf->max_edge;
  cf.grad_stop = conf->grad_stop; cf.dt_stop = conf->dt_stop; cf.dR_stop = conf->dR_stop;
  for (int k = 0; k < 6; ++k) cf.lambda[k] = conf->lambda[k];
  const int K = n_problems;
  for (int k = 0; k < K; ++k) {  // every check before anything is staged, launched or written
    const pxt_depth_problem& q = problems[k];
    if (!q.p3d || !q.sensor || !q.pose || !q.out) return PXT_E_ARG;
    if (q.n_points < 1 || q.n_points > PXT_DEPTH_MAX_POINTS) return PXT_E_ARG;
    if (q.width < 4 || q.height < 4 || (long long)q.width * q.height > (1ll << 30)) return PXT_E_ARG;
    if (q.ndist != 0 && q.ndist != 2 && q.ndist != 4) return PXT_E_ARG;
    if (((uintptr_t)q.p3d % 16) != 0 || ((uintptr_t)q.pose % 16) != 0 || ((uintptr_t)q.out % 16) != 0 ||
        ((uintptr_t)q.sensor % 2) != 0 || ((uintptr_t)q.log % 4) != 0)
      return PXT_E_ARG;
    for (int j = 0; j < k; ++j)
      if (problems[j].out == q.out) return PXT_E_ARG;
  }
  const bool from_args = K <= kEvalArgProblems;
  using Stage = StageRing<DrParams, PXT_DEPTH_MAX_PROBLEMS>;
  EvalArgs<DrParams> args = {};
  DrParams* rec = args.p;
  Stage::Slot* slot = nullptr;
  if (!from_args) {
    static thread_local Stage stage;
    if (const int rc = stage.acquire(&slot)) return rc;
    rec = slot->host;
  }
  for (int k = 0; k < K; ++k) {
    const pxt_depth_problem& q = problems[k];
    DrParams& r = rec[k];
    r = DrParams();
    r.p3d = q.p3d; r.mask = q.point_mask; r.sensor = q.sensor; r.pose = q.pose;
    r.out = q.out; r.log = q.log; r.codes = q.codes;
    r.n = q.n_points; r.w = q.width; r.h = q.height; r.ndist = q.ndist;
    r.pose_is_record = q.pose_is_lm_record != 0;
    r.sensor_scale = q.sensor_scale;
    for (int i = 0; i < 10; ++i) r.cam[i] = q.cam[i];
    for (int i = 0; i < 21; ++i) r.prior[i] = q.prior[i];
  }
  hipStream_t s = (hipStream_t)stream;
  if (!from_args) {
    PXT_HIP_CHECK(hipMemcpyAsync(workspace, slot->host, (size_t)K * sizeof(DrParams), hipMemcpyHostToDevice, s));
    PXT_HIP_CHECK(hipEventRecord(slot->copied, s));
  }
  hipLaunchKernelGGL(depth_refine_kernel, dim3(K), dim3(kDrBlock), 0, s, args, (const DrParams*)workspace, cf,
                     (int)from_args);
  PXT_HIP_CHECK(hipGetLastError());
  return PXT_OK;
}

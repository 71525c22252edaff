// SC backbone element-wise kernels (SCConvBackbone2dStride4 / Stride1 of the nuScenes PointPillar-Jr models).
//
// Replaces workspace/sc_conv.py:14-44: the AvgPool2d(4, 4) in front of k2 and the gate
//   sigmoid(identity + F.interpolate(k2(x), identity.size()[2:])) * k3(x)
// in front of k4.  Both are streaming passes: one thread per (pixel, 4 channels), 16-byte loads and stores, no LDS.
// Training half (include/pcp_hip_train.h): the backward of the pool and of the gate, and the bottleneck's pre-activation residual
// relu(z + x) with its mask backward.  Same form; the one reduction (the gate's gradient of s) is a gather in a fixed order, no atomics.
#include "pcp_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int SC_THREADS = 256;

__global__ __launch_bounds__(SC_THREADS) void k_avgpool(const float *__restrict__ in, int in_h, int in_w, int ld_in, int r,
                                                         float *__restrict__ out, int oh, int ow, int ld_out, int c4,
                                                         long long total) {
  for (long long i = (long long)blockIdx.x * SC_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * SC_THREADS) {
    const int q = (int)(i % c4);
    long long pix = i / c4;
    const int ox = (int)(pix % ow);
    pix /= ow;
    const int oy = (int)(pix % oh);
    const long long b = pix / oh;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int dy = 0; dy < r; dy++) {
      const float *row = in + ((b * in_h + (long long)(oy * r + dy)) * in_w + (long long)ox * r) * ld_in + 4 * q;
      for (int dx = 0; dx < r; dx++) acc += *reinterpret_cast<const f32x4 *>(row + (long long)dx * ld_in);
    }
    // torch's avg_pool2d: window sum, then divided by the window size (r * r)
    const float n = (float)(r * r);
    const f32x4 v = {acc.x / n, acc.y / n, acc.z / n, acc.w / n};
    *reinterpret_cast<f32x4 *>(out + ((b * oh + oy) * ow + ox) * ld_out + 4 * q) = v;
  }
}

// torch's nearest source index (aten/src/ATen/native/UpSample.h, nearest_idx) for one axis
__device__ __forceinline__ int nearest_src(int i, int in, int out, float scale) {
  if (out == in) return i;
  if (out == 2 * in) return i >> 1;
  const int s = (int)floorf((float)i * scale);
  return s < in - 1 ? s : in - 1;
}

__device__ __forceinline__ float sigmoid_acc(float v) { return 1.0f / (1.0f + expf(-v)); }

__global__ __launch_bounds__(SC_THREADS) void k_sc_gate(const float *t, int ld_t, const float *__restrict__ x, int ld_x,
                                                         const float *__restrict__ s, int ld_s, int sh, int sw, float scale_y,
                                                         float scale_x, float *out, int ld_out, int h, int w, int c4,
                                                         long long total) {
  for (long long i = (long long)blockIdx.x * SC_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * SC_THREADS) {
    const int q = (int)(i % c4);
    const long long pix = i / c4;
    const int px = (int)(pix % w);
    const long long rowid = pix / w;
    const int py = (int)(rowid % h);
    const long long b = rowid / h;
    const int sy = nearest_src(py, sh, h, scale_y), sx = nearest_src(px, sw, w, scale_x);
    const f32x4 tv = *reinterpret_cast<const f32x4 *>(t + pix * ld_t + 4 * q);
    const f32x4 xv = *reinterpret_cast<const f32x4 *>(x + pix * ld_x + 4 * q);
    const f32x4 sv = *reinterpret_cast<const f32x4 *>(s + ((b * sh + sy) * sw + sx) * ld_s + 4 * q);
    f32x4 g;
    g.x = tv.x * sigmoid_acc(xv.x + sv.x);
    g.y = tv.y * sigmoid_acc(xv.y + sv.y);
    g.z = tv.z * sigmoid_acc(xv.z + sv.z);
    g.w = tv.w * sigmoid_acc(xv.w + sv.w);
    *reinterpret_cast<f32x4 *>(out + pix * ld_out + 4 * q) = g;
  }
}

__global__ __launch_bounds__(SC_THREADS) void k_avgpool_bwd(const float *__restrict__ dp, int oh, int ow, int ld_dp, int r, float *dx,
                                                             int h, int w, int ld_dx, int accumulate, int c4, long long total) {
  const float n = (float)(r * r);
  for (long long i = (long long)blockIdx.x * SC_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * SC_THREADS) {
    const int q = (int)(i % c4);
    const long long pix = i / c4;
    const int px = (int)(pix % w);
    const long long rowid = pix / w;
    const int py = (int)(rowid % h);
    const long long b = rowid / h;
    float *dst = dx + pix * ld_dx + 4 * q;
    const int oy = py / r, ox = px / r;
    if (oy >= oh || ox >= ow) {            // rows / columns the floor-sized pool never read
      if (!accumulate) *reinterpret_cast<f32x4 *>(dst) = f32x4{0.f, 0.f, 0.f, 0.f};
      continue;
    }
    const f32x4 g = *reinterpret_cast<const f32x4 *>(dp + ((b * oh + oy) * ow + ox) * ld_dp + 4 * q);
    f32x4 v = {g.x / n, g.y / n, g.z / n, g.w / n};           // torch's avg_pool2d backward: grad / pool size
    if (accumulate) v += *reinterpret_cast<const f32x4 *>(dst);
    *reinterpret_cast<f32x4 *>(dst) = v;
  }
}

// first index i in [0, out] with nearest_src(i) >= k (nearest_src is non-decreasing in i): the pixels whose source is k are
// [nearest_lower(k), nearest_lower(k + 1)).  The guess comes from the same float32 scale and is walked to the exact answer with
// nearest_src itself, so the ranges are the inverse of the forward's index whatever the rounding of i * scale.
__device__ __forceinline__ int nearest_lower(int k, int in, int out, float scale) {
  if (k >= in) return out;
  int i = (int)ceilf((float)k / scale);
  i = i < 0 ? 0 : (i > out ? out : i);
  while (i > 0 && nearest_src(i - 1, in, out, scale) >= k) i--;
  while (i < out && nearest_src(i, in, out, scale) < k) i++;
  return i;
}

// pass 1: dt = dout * g, dz = dout * t * (1 - g) * g (torch's mul and sigmoid backward), dx (+)= dz.  dt (and dx) may alias dout:
// a thread reads its element of every input before it writes.
__global__ __launch_bounds__(SC_THREADS) void k_sc_gate_bwd(const float *dout, int ld_dout, const float *__restrict__ t, int ld_t,
                                                             const float *__restrict__ x, int ld_x, const float *__restrict__ s, int ld_s,
                                                             int sh, int sw, float scale_y, float scale_x, float *dt, int ld_dt,
                                                             float *__restrict__ dz, int ld_dz, float *dx, int ld_dx,
                                                             int accumulate_dx, int h, int w, int c4, long long total) {
  for (long long i = (long long)blockIdx.x * SC_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * SC_THREADS) {
    const int q = (int)(i % c4);
    const long long pix = i / c4;
    const int px = (int)(pix % w);
    const long long rowid = pix / w;
    const int py = (int)(rowid % h);
    const long long b = rowid / h;
    const int sy = nearest_src(py, sh, h, scale_y), sx = nearest_src(px, sw, w, scale_x);
    const f32x4 dv = *reinterpret_cast<const f32x4 *>(dout + pix * ld_dout + 4 * q);
    const f32x4 tv = *reinterpret_cast<const f32x4 *>(t + pix * ld_t + 4 * q);
    const f32x4 xv = *reinterpret_cast<const f32x4 *>(x + pix * ld_x + 4 * q);
    const f32x4 sv = *reinterpret_cast<const f32x4 *>(s + ((b * sh + sy) * sw + sx) * ld_s + 4 * q);
    const f32x4 g = {sigmoid_acc(xv.x + sv.x), sigmoid_acc(xv.y + sv.y), sigmoid_acc(xv.z + sv.z), sigmoid_acc(xv.w + sv.w)};
    const f32x4 gt = {dv.x * g.x, dv.y * g.y, dv.z * g.z, dv.w * g.w};
    f32x4 gz = {dv.x * tv.x * (1.0f - g.x) * g.x, dv.y * tv.y * (1.0f - g.y) * g.y, dv.z * tv.z * (1.0f - g.z) * g.z,
                dv.w * tv.w * (1.0f - g.w) * g.w};
    *reinterpret_cast<f32x4 *>(dt + pix * ld_dt + 4 * q) = gt;
    *reinterpret_cast<f32x4 *>(dz + pix * ld_dz + 4 * q) = gz;
    if (dx) {
      float *dst = dx + pix * ld_dx + 4 * q;
      if (accumulate_dx) gz += *reinterpret_cast<const f32x4 *>(dst);
      *reinterpret_cast<f32x4 *>(dst) = gz;
    }
  }
}

// pass 2: ds[b, sy, sx] = sum of dz over the pixels whose nearest source is (sy, sx), rows then columns in ascending order
__global__ __launch_bounds__(SC_THREADS) void k_sc_gate_bwd_s(const float *__restrict__ dz, int ld_dz, int h, int w, float scale_y,
                                                               float scale_x, float *__restrict__ ds, int ld_ds, int sh, int sw, int c4,
                                                               long long total) {
  for (long long i = (long long)blockIdx.x * SC_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * SC_THREADS) {
    const int q = (int)(i % c4);
    long long cell = i / c4;
    const int sx = (int)(cell % sw);
    cell /= sw;
    const int sy = (int)(cell % sh);
    const long long b = cell / sh;
    const int y0 = nearest_lower(sy, sh, h, scale_y), y1 = nearest_lower(sy + 1, sh, h, scale_y);
    const int x0 = nearest_lower(sx, sw, w, scale_x), x1 = nearest_lower(sx + 1, sw, w, scale_x);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int py = y0; py < y1; py++) {
      const float *row = dz + ((b * h + py) * w) * ld_dz + 4 * q;
      for (int px = x0; px < x1; px++) acc += *reinterpret_cast<const f32x4 *>(row + (long long)px * ld_dz);
    }
    *reinterpret_cast<f32x4 *>(ds + ((b * sh + sy) * sw + sx) * ld_ds + 4 * q) = acc;
  }
}

// out = relu(z + res); out may alias z
__global__ __launch_bounds__(SC_THREADS) void k_add_relu(const float *z, int ld_z, const float *__restrict__ res, int ld_res, float *out,
                                                          int ld_out, int c4, long long total) {
  for (long long i = (long long)blockIdx.x * SC_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * SC_THREADS) {
    const int q = (int)(i % c4);
    const long long row = i / c4;
    const f32x4 a = *reinterpret_cast<const f32x4 *>(z + row * ld_z + 4 * q);
    const f32x4 r = *reinterpret_cast<const f32x4 *>(res + row * ld_res + 4 * q);
    const f32x4 v = a + r;
    const f32x4 o = {v.x > 0.f ? v.x : 0.f, v.y > 0.f ? v.y : 0.f, v.z > 0.f ? v.z : 0.f, v.w > 0.f ? v.w : 0.f};
    *reinterpret_cast<f32x4 *>(out + row * ld_out + 4 * q) = o;
  }
}

// dz = dout * (out > 0), written to dz and (when given) to dz2; dz may alias dout
__global__ __launch_bounds__(SC_THREADS) void k_add_relu_bwd(const float *dout, int ld_dout, const float *__restrict__ out, int ld_out,
                                                              float *dz, int ld_dz, float *__restrict__ dz2, int ld_dz2, int c4,
                                                              long long total) {
  for (long long i = (long long)blockIdx.x * SC_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * SC_THREADS) {
    const int q = (int)(i % c4);
    const long long row = i / c4;
    const f32x4 d = *reinterpret_cast<const f32x4 *>(dout + row * ld_dout + 4 * q);
    const f32x4 o = *reinterpret_cast<const f32x4 *>(out + row * ld_out + 4 * q);
    const f32x4 v = {o.x > 0.f ? d.x : 0.f, o.y > 0.f ? d.y : 0.f, o.z > 0.f ? d.z : 0.f, o.w > 0.f ? d.w : 0.f};
    *reinterpret_cast<f32x4 *>(dz + row * ld_dz + 4 * q) = v;
    if (dz2) *reinterpret_cast<f32x4 *>(dz2 + row * ld_dz2 + 4 * q) = v;
  }
}

inline bool aligned16(const void *p) { return (((uintptr_t)p) & 15) == 0; }

inline unsigned grid_for(long long total) {
  long long blocks = (total + SC_THREADS - 1) / SC_THREADS;
  const long long cap = 256LL * 16;            // grid-stride beyond 16 workgroups per CU
  return (unsigned)(blocks < cap ? blocks : cap);
}

}  // namespace

extern "C" int pcp_avgpool_nhwc(const float *in, int32_t batch, int32_t in_h, int32_t in_w, int32_t c, int32_t ld_in, int32_t r,
                                float *out, int32_t ld_out, void *stream_) {
  if (!in || !out || batch <= 0 || in_h <= 0 || in_w <= 0 || c <= 0 || r < 1 || r > 8) return PCP_ERR_ARG;
  if ((c & 3) || (ld_in & 3) || (ld_out & 3) || ld_in < c || ld_out < c || !aligned16(in) || !aligned16(out)) return PCP_ERR_ARG;
  const int oh = in_h / r, ow = in_w / r;
  if (oh <= 0 || ow <= 0) return PCP_ERR_ARG;
  const long long total = (long long)batch * oh * ow * (c / 4);
  hipLaunchKernelGGL(k_avgpool, dim3(grid_for(total)), dim3(SC_THREADS), 0, (hipStream_t)stream_, in, in_h, in_w, ld_in, r, out, oh, ow,
                     ld_out, c / 4, total);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

extern "C" int pcp_sc_gate(const float *t, int32_t ld_t, const float *x, int32_t ld_x, const float *s, int32_t ld_s, int32_t sh,
                           int32_t sw, float *out, int32_t ld_out, int32_t batch, int32_t h, int32_t w, int32_t c, void *stream_) {
  if (!t || !x || !s || !out || batch <= 0 || h <= 0 || w <= 0 || c <= 0 || sh <= 0 || sw <= 0) return PCP_ERR_ARG;
  if ((c & 3) || (ld_t & 3) || (ld_x & 3) || (ld_s & 3) || (ld_out & 3)) return PCP_ERR_ARG;
  if (ld_t < c || ld_x < c || ld_s < c || ld_out < c) return PCP_ERR_ARG;
  if (!aligned16(t) || !aligned16(x) || !aligned16(s) || !aligned16(out)) return PCP_ERR_ARG;
  // compute_scales_value<float> without explicit scales: (float)in / out, evaluated once on the host as torch does
  const float scale_y = (float)sh / (float)h, scale_x = (float)sw / (float)w;
  const long long total = (long long)batch * h * w * (c / 4);
  hipLaunchKernelGGL(k_sc_gate, dim3(grid_for(total)), dim3(SC_THREADS), 0, (hipStream_t)stream_, t, ld_t, x, ld_x, s, ld_s, sh, sw,
                     scale_y, scale_x, out, ld_out, h, w, c / 4, total);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

extern "C" int pcp_avgpool_nhwc_backward(const float *dpooled, int32_t ld_dpooled, int32_t batch, int32_t h, int32_t w, int32_t c, int32_t r,
                                         float *dx, int32_t ld_dx, int32_t accumulate, void *stream_) {
  if (!dpooled || !dx || batch <= 0 || h <= 0 || w <= 0 || c <= 0 || r < 1 || r > 8) return PCP_ERR_ARG;
  if ((c & 3) || (ld_dpooled & 3) || (ld_dx & 3) || ld_dpooled < c || ld_dx < c || !aligned16(dpooled) || !aligned16(dx)) return PCP_ERR_ARG;
  const int oh = h / r, ow = w / r;
  if (oh <= 0 || ow <= 0) return PCP_ERR_ARG;
  const long long total = (long long)batch * h * w * (c / 4);
  hipLaunchKernelGGL(k_avgpool_bwd, dim3(grid_for(total)), dim3(SC_THREADS), 0, (hipStream_t)stream_, dpooled, oh, ow, ld_dpooled, r, dx, h, w,
                     ld_dx, accumulate ? 1 : 0, c / 4, total);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

extern "C" int pcp_sc_gate_backward(const float *dout, int32_t ld_dout, const float *t, int32_t ld_t, const float *x, int32_t ld_x,
                                    const float *s, int32_t ld_s, int32_t sh, int32_t sw, float *dt, int32_t ld_dt, float *dz, int32_t ld_dz,
                                    float *dx, int32_t ld_dx, int32_t accumulate_dx, float *ds, int32_t ld_ds, int32_t batch, int32_t h,
                                    int32_t w, int32_t c, void *stream_) {
  if (!dout || !t || !x || !s || !dt || !dz || !ds || batch <= 0 || h <= 0 || w <= 0 || c <= 0 || sh <= 0 || sw <= 0) return PCP_ERR_ARG;
  if ((c & 3) || (ld_dout & 3) || (ld_t & 3) || (ld_x & 3) || (ld_s & 3) || (ld_dt & 3) || (ld_dz & 3) || (ld_ds & 3)) return PCP_ERR_ARG;
  if (ld_dout < c || ld_t < c || ld_x < c || ld_s < c || ld_dt < c || ld_dz < c || ld_ds < c) return PCP_ERR_ARG;
  if (!aligned16(dout) || !aligned16(t) || !aligned16(x) || !aligned16(s) || !aligned16(dt) || !aligned16(dz) || !aligned16(ds)) return PCP_ERR_ARG;
  if (dx && ((ld_dx & 3) || ld_dx < c || !aligned16(dx))) return PCP_ERR_ARG;
  if (dz == dout || dz == dx || dz == dt) return PCP_ERR_ARG;                       // dz is read back by the second pass
  const float scale_y = (float)sh / (float)h, scale_x = (float)sw / (float)w;     // as pcp_sc_gate
  const long long total = (long long)batch * h * w * (c / 4);
  hipLaunchKernelGGL(k_sc_gate_bwd, dim3(grid_for(total)), dim3(SC_THREADS), 0, (hipStream_t)stream_, dout, ld_dout, t, ld_t, x, ld_x, s, ld_s,
                     sh, sw, scale_y, scale_x, dt, ld_dt, dz, ld_dz, dx, ld_dx, accumulate_dx ? 1 : 0, h, w, c / 4, total);
  PCP_CHECK_LAUNCH();
  const long long total_s = (long long)batch * sh * sw * (c / 4);
  hipLaunchKernelGGL(k_sc_gate_bwd_s, dim3(grid_for(total_s)), dim3(SC_THREADS), 0, (hipStream_t)stream_, dz, ld_dz, h, w, scale_y, scale_x, ds,
                     ld_ds, sh, sw, c / 4, total_s);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

extern "C" int pcp_add_relu(const float *z, int32_t ld_z, const float *res, int32_t ld_res, float *out, int32_t ld_out, int64_t rows,
                            int32_t c, void *stream_) {
  if (!z || !res || !out || rows <= 0 || c <= 0) return PCP_ERR_ARG;
  if ((c & 3) || (ld_z & 3) || (ld_res & 3) || (ld_out & 3) || ld_z < c || ld_res < c || ld_out < c) return PCP_ERR_ARG;
  if (!aligned16(z) || !aligned16(res) || !aligned16(out)) return PCP_ERR_ARG;
  const long long total = (long long)rows * (c / 4);
  hipLaunchKernelGGL(k_add_relu, dim3(grid_for(total)), dim3(SC_THREADS), 0, (hipStream_t)stream_, z, ld_z, res, ld_res, out, ld_out, c / 4,
                     total);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

extern "C" int pcp_add_relu_backward(const float *dout, int32_t ld_dout, const float *out, int32_t ld_out, float *dz, int32_t ld_dz,
                                     float *dz2, int32_t ld_dz2, int64_t rows, int32_t c, void *stream_) {
  if (!dout || !out || !dz || rows <= 0 || c <= 0) return PCP_ERR_ARG;
  if ((c & 3) || (ld_dout & 3) || (ld_out & 3) || (ld_dz & 3) || ld_dout < c || ld_out < c || ld_dz < c) return PCP_ERR_ARG;
  if (!aligned16(dout) || !aligned16(out) || !aligned16(dz)) return PCP_ERR_ARG;
  if (dz2 && ((ld_dz2 & 3) || ld_dz2 < c || !aligned16(dz2) || dz2 == dz || dz2 == dout)) return PCP_ERR_ARG;
  const long long total = (long long)rows * (c / 4);
  hipLaunchKernelGGL(k_add_relu_bwd, dim3(grid_for(total)), dim3(SC_THREADS), 0, (hipStream_t)stream_, dout, ld_dout, out, ld_out, dz, ld_dz,
                     dz2, ld_dz2, c / 4, total);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

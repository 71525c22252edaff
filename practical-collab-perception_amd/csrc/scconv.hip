// SC backbone element-wise kernels (SCConvBackbone2dStride4 / Stride1 of the nuScenes PointPillar-Jr models).
//
// Replaces workspace/sc_conv.py:14-44: the AvgPool2d(4, 4) in front of k2 and the gate
//   sigmoid(identity + F.interpolate(k2(x), identity.size()[2:])) * k3(x)
// in front of k4.  Both are streaming passes: one thread per (pixel, 4 channels), 16-byte loads and stores, no LDS.
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

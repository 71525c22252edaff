// What the fused Winograd F(4x4, 3x3) kernels share beyond pcp_common.h (whose XCD remap k_wino4f, k_wino4h and k_wino4c use): for the two half-size
// kernels k_wino4h (wino4h.hip) and k_wino4c (wino4c.hip), which differ only in how the waves split the products and in the output transform: the
// item geometry, the launch parameters, the 6-point transforms and the stand-alone input transform.  The two kernels give the same bits
// (tests/test_gpu_ops.py) BECAUSE these are one instruction sequence: change them here, for both.  The raw-patch staging is the same text in
// both kernels and stays there: moved here, in any form tried, its offset set-up compiles to other instructions (profiles/wino4_refactor.txt).
#pragma once
#include "pcp_common.h"

// per-workgroup stamps of a -DH4_STAMP build (tools/stamp_h4.py): dbg = [workgroup][8 stamps]; needs `tid` in scope
#ifdef H4_STAMP
#define H4_STAMP_AT(dbg, slot)                                                                   \
  do {                                                                                           \
    __builtin_amdgcn_sched_barrier(0);                                                           \
    if (tid == 0 && blockIdx.x < 8192) {                                                         \
      unsigned long long t_;                                                                     \
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                \
      dbg[blockIdx.x * 8 + (slot)] = t_;                                                         \
    }                                                                                            \
    __builtin_amdgcn_sched_barrier(0);                                                           \
  } while (0)
#else
#define H4_STAMP_AT(dbg, slot)
#endif

namespace {

// ---- the half-size item: 16 x 16 output pixels (16 Winograd tiles) x 64 output channels, 8-channel slices ------------------------------------
constexpr int H4_CK = 8;                                  // input channels per slice
constexpr int H4_RP = 20;                                 // raw plane row pitch (floats)
constexpr int H4_RAW_H = 18, H4_RAW_W = 18;               // 16 x 16 output pixels + halo
constexpr int H4_RAW_PIX = H4_RAW_H * H4_RAW_W;
constexpr int H4_PLANE = H4_RAW_H * H4_RP;                // 360 = 40 (mod 64)
constexpr int H4_RAW_FLOATS = H4_CK * H4_PLANE;           // 2880
constexpr int H4_VP = 160;                                // V position pitch: [8 k][16 tiles] + 32 (3 * VP = 32 mod 64: the two lane halves of
                                                          // the column pass store to disjoint banks)
constexpr int H4_V_FLOATS = 36 * H4_VP;                   // 5760
constexpr int H4_MAIN_FLOATS = 2 * H4_RAW_FLOATS + 2 * H4_V_FLOATS;      // 17280: raw x2, V x2
constexpr int H4_RAW_ITEMS = H4_RAW_PIX * 2;              // float4 items per slice (648)
constexpr int H4_WBN = 64;
constexpr int H4_URING = 4;                               // positions the U fragments are requested ahead (3: +0.5 % time, 2: +2 %)

struct H4Params {
  const float *in;
  const float *u;       // U^T fragments in the kernel's own order (its file head; pack.repack_winograd4f_to_4h / _to_4c)
  const float *bias;
  float *out;
  int batch, h, w;
  int cin, cout, cout_pad;
  int ld_in, ld_out;
  int relu;
  int tiles_x, tiles_y, n_spatial;
  unsigned in_bytes, u_bytes;     // extents for the buffer descriptors (range-checked loads)
};

int h4_geom(const pcp_conv3x3_t *d, H4Params *p) {
  if (!d || d->stride != 1) return PCP_ERR_UNSUPPORTED;
  if (d->cin <= 0 || d->cin % H4_CK != 0 || d->cout <= 0 || d->cout_pad < d->cout || d->cout_pad % H4_WBN != 0) return PCP_ERR_ARG;
  if (d->ld_in % 4 != 0 || d->ld_out % 4 != 0 || d->cout % 4 != 0 || d->batch <= 0 || d->in_h <= 0 || d->in_w <= 0) return PCP_ERR_ARG;
  p->batch = d->batch; p->h = d->in_h; p->w = d->in_w;
  p->cin = d->cin; p->cout = d->cout; p->cout_pad = d->cout_pad;
  p->ld_in = d->ld_in; p->ld_out = d->ld_out; p->relu = d->relu;
  p->tiles_x = (d->in_w + 15) / 16;
  p->tiles_y = (d->in_h + 15) / 16;
  p->n_spatial = d->batch * p->tiles_x * p->tiles_y;
  const long long in_bytes = (long long)d->batch * d->in_h * d->in_w * d->ld_in * 4;
  const long long u_bytes = (long long)(d->cin / H4_CK) * 36 * d->cout_pad * H4_CK * 4;
  if (in_bytes > 0x7fffffffLL || u_bytes > 0x7fffffffLL) return PCP_ERR_UNSUPPORTED;
  p->in_bytes = (unsigned)in_bytes;
  p->u_bytes = (unsigned)u_bytes;
  return PCP_OK;
}

// B^T x for the 6-point transform (points 0, +-1, +-2, inf).  Contraction is spelt out (no compiler-chosen fma grouping): k_wino4h and both
// forms of k_wino4c run exactly these operations, so their outputs agree bit for bit.
__device__ __forceinline__ void bt6(const float d0, const float d1, const float d2, const float d3, const float d4, const float d5,
                                    float (&t)[6]) {
#pragma clang fp contract(off)
  const float p = __builtin_fmaf(-4.f, d2, d4), q = __builtin_fmaf(-4.f, d1, d3);
  const float r = d4 - d2, s = 2.f * (d3 - d1);
  t[0] = __builtin_fmaf(4.f, d0, __builtin_fmaf(-5.f, d2, d4));
  t[1] = p + q;
  t[2] = p - q;
  t[3] = r + s;
  t[4] = r - s;
  t[5] = __builtin_fmaf(4.f, d1, __builtin_fmaf(-5.f, d3, d5));
}

// A^T m for float4 lanes: 6 -> 4 (same rule: explicit fma)
__device__ __forceinline__ void at6v(const f32x4 m0, const f32x4 m1, const f32x4 m2, const f32x4 m3, const f32x4 m4, const f32x4 m5,
                                     f32x4 (&y)[4]) {
#pragma clang fp contract(off)
  const f32x4 s12 = m1 + m2, d12 = m1 - m2, s34 = m3 + m4, d34 = m3 - m4;
  const f32x4 c2 = f32x4{2.f, 2.f, 2.f, 2.f}, c4 = f32x4{4.f, 4.f, 4.f, 4.f}, c8 = f32x4{8.f, 8.f, 8.f, 8.f};
  y[0] = (m0 + s12) + s34;
  y[1] = __builtin_elementwise_fma(c2, d34, d12);
  y[2] = __builtin_elementwise_fma(c4, s34, s12);
  y[3] = __builtin_elementwise_fma(c8, d34, d12) + m5;
}

// ---- input transform V = B^T d B of ONE slice, LDS -> LDS (the prologue's; the main loops run the same operations spread over their blocks):
// item = (tile, channel) on the lane pair (l, l + 32), lane half h: row pass over raw rows 3h .. 3h + 2, nine v_permlane32_swap, column pass over
// columns 3h .. 3h + 2.  t_src / t_dst = the lane's offsets into a raw / V image.  (A callable object like the lambda it replaces: as a
// force-inlined function the compiler orders the prologue's address arithmetic differently.)
struct H4Transform {
  float *rawb, *vb;     // [2][H4_RAW_FLOATS], [2][H4_V_FLOATS]
  int t_src, t_dst;
  __device__ void operator()(int rbuf, int vbuf) const {
    const float *src = rawb + rbuf * H4_RAW_FLOATS + t_src;
    float *dst = vb + vbuf * H4_V_FLOATS + t_dst;
    float wr[3][6];
#pragma unroll
    for (int rr = 0; rr < 3; rr++) {
      const f32x4 lo = *reinterpret_cast<const f32x4 *>(src + rr * H4_RP);
      const float2 hi = *reinterpret_cast<const float2 *>(src + rr * H4_RP + 4);
      bt6(lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, wr[rr]);
    }
    float top[3][3], bot[3][3];
#pragma unroll
    for (int rr = 0; rr < 3; rr++)
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(wr[rr][c]), __float_as_uint(wr[rr][3 + c]), false, false);
        top[rr][c] = __uint_as_float(sw[0]);
        bot[rr][c] = __uint_as_float(sw[1]);
      }
#pragma unroll
    for (int c = 0; c < 3; c++) {
      float o[6];
      bt6(top[0][c], top[1][c], top[2][c], bot[0][c], bot[1][c], bot[2][c], o);
#pragma unroll
      for (int i = 0; i < 6; i++) dst[(i * 6 + c) * H4_VP] = o[i];
    }
  }
};

}  // namespace

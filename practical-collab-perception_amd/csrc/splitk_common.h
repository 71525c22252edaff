// What the two pointwise weight-gradient families share (fp32: wgrad.hip k_wgrad_pw, bf16: mp_pointwise.hip k_mp_pw_wgrad):
//   out[n][k] (+)= sum_r a[map(r)][n] * b[map(r)][k]
// the row map of the operands, the rounding of the channel counts to 64-wide tiles and the reduce of the split-K partials.  The product
// kernels and their split rules (pw_split, mwg_split) differ and stay in their files; the two 3x3 reduces read other partial layouts.
#pragma once
#include "pcp_common.h"

namespace {

// One operand: row r of the contraction -> a pixel of an NHWC map.  A lattice map addresses the rows of a Conv2d k2 s2 / ConvTranspose2d
// k2 s2 tap: the fine (2h, 2w) map is read at the pixels of one (ky, kx) of every 2 x 2 block.
struct RowMap {
  const void *ptr;             // float (wgrad.hip) or bf16 (mp_pointwise.hip) storage
  int ld, ch;                  // pixel stride, valid channels
  int mode;                    // 0: pixel = r;  1: r = (b, y, x) on an (h, w) grid -> pixel (b, 2y + ky, 2x + kx) of a (2h, 2w) grid
  int h, w, ky, kx;
  unsigned bytes;              // bf16 only: the range of the operand's buffer descriptor (fp32: 0, unused; the struct is 40 bytes either way)
};

__device__ __forceinline__ long long map_row(const RowMap &m, long long r) {
  if (m.mode == 0) return r;
  const int x = (int)(r % m.w);
  const long long t = r / m.w;
  const int y = (int)(t % m.h);
  const long long b = t / m.h;
  return (b * 2 * m.h + 2 * y + m.ky) * 2 * m.w + 2 * x + m.kx;
}

// pcp_rowmap_t / pcp_mp_rowmap_t -> RowMap; PCP_ERR_ARG for a lattice without a grid
template <typename M>
inline int to_rowmap(const M *m, unsigned bytes, RowMap *r) {
  r->ptr = m->ptr; r->ld = m->ld; r->ch = m->channels; r->mode = m->lattice ? 1 : 0;
  r->h = m->grid_h; r->w = m->grid_w; r->ky = m->ky; r->kx = m->kx;
  r->bytes = bytes;
  return r->mode && (r->h <= 0 || r->w <= 0) ? PCP_ERR_ARG : PCP_OK;
}

inline int round64(int v) { return (v + 63) / 64 * 64; }

// out[n][k] (+)= the nsplit partials [nsplit][n_r][k_r] summed in a fixed order (four interleaved runs, then ((0 + 1) + (2 + 3))): the same
// bits on every run
__global__ __launch_bounds__(256) void k_pw_reduce(const float *__restrict__ part, int nsplit, int n, int k, int n_r, int k_r,
                                                   float *__restrict__ out, int ld_out, int accumulate) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const long long t = (long long)blockIdx.x * 64 + lane;
  float s = 0.f;
  int kk = 0, nn = 0;
  if (t < (long long)n * k) {
    kk = (int)(t % k);
    nn = (int)(t / k);
    const float *src = part + (long long)nn * k_r + kk;
    const long long stride = (long long)n_r * k_r;
    for (int i = sl; i < nsplit; i += 4) s += src[i * stride];
  }
  red[sl][lane] = s;
  __syncthreads();
  if (sl == 0 && t < (long long)n * k) {
    const float v = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
    float *d = out + (long long)nn * ld_out + kk;
    *d = accumulate ? *d + v : v;
  }
}

}  // namespace

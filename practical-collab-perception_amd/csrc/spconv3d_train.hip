// The training half of the sparse 3D convolution (csrc/spconv3d.hip is the forward): the inverse neighbour table of a strided layer, the weight
// gradient, and the gradient of HeightCompression's dense().  fp32, no float atomics: a call repeats bit for bit.
//
// Data gradient.  No kernel here: dx = pcp_spconv3d(dy, table', W') with
//   submanifold layer   table' = the forward's table (nbr[k][j] == i exactly when nbr[26 - k][i] == j), W'[k] = W[26 - k]^T
//   strided layer       table' = inv (K, N_in), inv[k][i] = j where nbr[k][j] == i (pcp_spconv_invert_nbr), W'[k] = W[k]^T
// W' packed [K][Cin][Cout] on the host (pcp_amd.ops.spconv_pack_weight_dgrad).
//
// Weight gradient.  dW[k][co][ci] = sum over rows j with nbr[k][j] >= 0 of dy[j][co] * x[nbr[k][j]][ci]: a GEMM whose reduction runs over the rows,
// so both operands are transposed relative to how rows lie in memory.  k_spconv3d_wgrad: a workgroup owns (offset k, row chunk); per 64-row
// step each wave stages one 16-row group of dy and of the gathered x rows into LDS with 16-byte loads (a group none of whose rows has a
// neighbour at k is skipped wave-uniformly and flagged), then v_mfma_f32_16x16x4_f32 with the row as the MFMA k: lane (m, q) reads
// A[co = m][row = q] and B[row = q][ci = m] from the LDS tiles, whose row pitch is 16 mod 32 floats, so the two 32-lane halves of a
// ds_read_b32 (rows q, q + 1) fall on disjoint banks.  The Cout x Cin block is split over the waves by 16-channel rows of Cout (WT waves);
// where Cout has fewer than four (the 16- and 32-channel layers) the remaining waves split the 16-row groups instead (WR) and write partials of
// their own.  k_spconv3d_wgrad_reduce adds the partials of each k in ascending (chunk, wr) order and writes the parameter's own layout
// (Cout, kz, ky, kx, Cin).
#include "pcp_common.h"

namespace {

constexpr int WG_STEP = 64;                     // rows staged per step: one 16-row group per wave
constexpr int WG_MIN_CHUNK = 1024;              // the chunk rule: at most WG_MAX_CHUNKS chunks, none shorter than this
constexpr int WG_MAX_CHUNKS = 32;

__host__ __device__ constexpr int wg_pitch(int c) { return c % 32 == 0 ? c + 16 : c; }      // == 16 (mod 32) floats
__host__ __device__ constexpr int wg_wt(int co16) { return co16 < 4 ? co16 : 4; }

// the chunk length for n_out rows when the caller leaves it to the library: a multiple of WG_STEP
inline long long wg_chunk_rule(long long n_out) {
  long long c = (n_out + WG_MAX_CHUNKS - 1) / WG_MAX_CHUNKS;
  c = (c + WG_STEP - 1) / WG_STEP * WG_STEP;
  return c < WG_MIN_CHUNK ? WG_MIN_CHUNK : c;
}

struct WgPlan { long long chunk, n_chunks, parts; size_t bytes; };
// parts: partial Cout x Cin blocks per offset
inline bool wg_plan(long long n_out, int K, int cin_pad, int cout, long long chunk_rows, WgPlan *p) {
  if (chunk_rows < 0 || chunk_rows % 16 || chunk_rows >= (1LL << 31)) return false;
  p->chunk = chunk_rows > 0 ? chunk_rows : wg_chunk_rule(n_out);
  p->n_chunks = n_out > 0 ? (n_out + p->chunk - 1) / p->chunk : 0;
  if (p->n_chunks > 65535 * 1024LL) return false;
  p->parts = p->n_chunks * (4 / wg_wt(cout / 16));
  p->bytes = (size_t)K * (size_t)p->parts * (size_t)cout * (size_t)cin_pad * sizeof(float);
  return true;
}

inline bool wg_pair_ok(int cin, int cout) {
  const int cin_pad = cin <= 16 ? 16 : cin;
  return cin >= 3 && ((cin_pad == 16 && (cout == 16 || cout == 32)) || (cin_pad == 32 && (cout == 32 || cout == 64)) ||
                      (cin_pad == 64 && (cout == 64 || cout == 128)) || (cin_pad == 128 && cout == 128));
}

template <int CI16, int CO16, bool VEC>
__global__ __launch_bounds__(256) void k_spconv3d_wgrad(const float *__restrict__ x, int cin, int ld_in, long long n_in, const float *__restrict__ dy,
                                                        const int *__restrict__ nbr, long long n_out, int chunk, int parts,
                                                        float *__restrict__ partial) {
  constexpr int CI = CI16 * 16, CO = CO16 * 16;
  constexpr int WT = wg_wt(CO16), WR = 4 / WT, CPW = CO16 / WT;       // waves over Cout, waves over row groups, 16-channel rows of Cout per wave
  constexpr int PA = wg_pitch(CO), PB = wg_pitch(CI);
  __shared__ __attribute__((aligned(16))) float lds_a[WG_STEP * PA];    // dy rows
  __shared__ __attribute__((aligned(16))) float lds_b[WG_STEP * PB];    // gathered x rows
  __shared__ int group_on[4];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m = lane & 15, q = lane >> 4;
  const int wt = wave % WT, wr = wave / WT;
  const int k = blockIdx.y;
  const long long r_begin = (long long)blockIdx.x * chunk;
  const long long r_end = r_begin + chunk < n_out ? r_begin + chunk : n_out;
  f32x4 acc[CPW][CI16];
#pragma unroll
  for (int c = 0; c < CPW; c++)
#pragma unroll
    for (int j = 0; j < CI16; j++) acc[c][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (long long t0 = r_begin; t0 < r_end; t0 += WG_STEP) {
    const long long g0 = t0 + 16 * wave;
    int idx = g0 + m < r_end ? nbr[(long long)k * n_out + g0 + m] : -1;
    if (idx >= n_in) idx = -1;
    const bool on = __ballot(idx >= 0) != 0ULL;            // wave-uniform
    if (lane == 0) group_on[wave] = on ? 1 : 0;
    if (on) {
      // 4 CO = 0 (mod 64) float4 slots: every lane makes the same number of trips, so the shuffles below see the whole wave
      for (int i = lane; i < 4 * CO; i += 64) {
        const int r = i / (CO / 4), c4 = i - r * (CO / 4);
        const int id = __shfl(idx, r, 64);
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (id >= 0) v = *reinterpret_cast<const f32x4 *>(dy + (g0 + r) * CO + 4 * c4);
        *reinterpret_cast<f32x4 *>(lds_a + (16 * wave + r) * PA + 4 * c4) = v;
      }
      for (int i = lane; i < 4 * CI; i += 64) {
        const int r = i / (CI / 4), c4 = i - r * (CI / 4);
        const int id = __shfl(idx, r, 64);
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (id >= 0) {
          const float *src = x + (long long)id * ld_in + 4 * c4;
          if (VEC) {
            v = *reinterpret_cast<const f32x4 *>(src);
          } else {
#pragma unroll
            for (int kk = 0; kk < 4; kk++)
              if (4 * c4 + kk < cin) v[kk] = src[kk];
          }
        }
        *reinterpret_cast<f32x4 *>(lds_b + (16 * wave + r) * PB + 4 * c4) = v;
      }
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < 4; g++) {
      if (g % WR != wr) continue;
      if (__builtin_amdgcn_readfirstlane(group_on[g]) == 0) continue;
#pragma unroll
      for (int s = 0; s < 4; s++) {
        const int rl = 16 * g + 4 * s + q;
        float a[CPW], b[CI16];
#pragma unroll
        for (int c = 0; c < CPW; c++) a[c] = lds_a[rl * PA + 16 * (wt * CPW + c) + m];
#pragma unroll
        for (int j = 0; j < CI16; j++) b[j] = lds_b[rl * PB + 16 * j + m];
#pragma unroll
        for (int c = 0; c < CPW; c++)
#pragma unroll
          for (int j = 0; j < CI16; j++) acc[c][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c], b[j], acc[c][j], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // acc[c][j][i]: co = 16 (wt CPW + c) + 4 q + i, ci = 16 j + m
  float *dst = partial + ((long long)k * parts + (long long)blockIdx.x * WR + wr) * CO * CI;
#pragma unroll
  for (int c = 0; c < CPW; c++)
#pragma unroll
    for (int j = 0; j < CI16; j++)
#pragma unroll
      for (int i = 0; i < 4; i++) dst[(16 * (wt * CPW + c) + 4 * q + i) * CI + 16 * j + m] = acc[c][j][i];
}

// dw (Cout, K, Cin) (+)= sum over the partials of k, ascending
__global__ __launch_bounds__(256) void k_spconv3d_wgrad_reduce(const float *__restrict__ partial, int K, int parts, int cout, int cin_pad, int cin,
                                                               int accumulate, float *__restrict__ dw) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;           // (k, co, ci)
  const long long block = (long long)cout * cin_pad;
  if (e >= (long long)K * block) return;
  const int k = (int)(e / block);
  const int rem = (int)(e - (long long)k * block);
  const int co = rem / cin_pad, ci = rem - co * cin_pad;
  if (ci >= cin) return;
  const float *src = partial + (long long)k * parts * block + rem;
  float s = 0.f;
  for (int p = 0; p < parts; p++) s = __fadd_rn(s, src[(long long)p * block]);
  float *d = dw + ((long long)co * K + k) * cin + ci;
  *d = accumulate ? __fadd_rn(*d, s) : s;
}

__global__ __launch_bounds__(256) void k_sp_invert_nbr(const int *__restrict__ nbr, long long n_out, long long n_in, int *__restrict__ inv) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n_out) return;
  const int k = blockIdx.y;
  const int i = nbr[(long long)k * n_out + j];
  if (i >= 0 && i < n_in) inv[(long long)k * n_in + i] = (int)j;          // at most one j per (k, i): one writer
}

__global__ __launch_bounds__(256) void k_sp_dense_backward(const float *__restrict__ dcanvas, const int *__restrict__ coords, long long n, int C, int B,
                                                           int D, int H, int W, float *__restrict__ dfeat) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n * C) return;
  const long long r = e / C;
  const int c = (int)(e - r * C);
  const int4 s = *reinterpret_cast<const int4 *>(coords + 4 * r);            // [b, z, y, x]
  float v = 0.f;
  if (s.x >= 0 && s.x < B && s.y >= 0 && s.y < D && s.z >= 0 && s.z < H && s.w >= 0 && s.w < W)
    v = dcanvas[(((long long)s.x * H + s.z) * W + s.w) * C * D + (long long)c * D + s.y];
  dfeat[e] = v;
}

}  // namespace

extern "C" int pcp_spconv_invert_nbr(const int32_t *nbr, int32_t num_offsets, int64_t n_out, int64_t n_in, int32_t *inv, void *stream_) {
  if (num_offsets < 1 || num_offsets > 27 || n_out < 0 || n_in < 0 || n_out >= (1LL << 31) || n_in >= (1LL << 31)) return PCP_ERR_ARG;
  if (n_in == 0) return PCP_OK;
  if (!inv || (n_out > 0 && !nbr)) return PCP_ERR_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  if (hipMemsetAsync(inv, 0xff, (size_t)num_offsets * (size_t)n_in * 4, stream) != hipSuccess) return PCP_ERR_LAUNCH;      // every entry -1
  if (n_out == 0) return PCP_OK;
  hipLaunchKernelGGL(k_sp_invert_nbr, dim3((unsigned)((n_out + 255) / 256), (unsigned)num_offsets), dim3(256), 0, stream, nbr, (long long)n_out,
                     (long long)n_in, inv);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

extern "C" size_t pcp_spconv3d_wgrad_workspace_bytes(int64_t n_out, int32_t num_offsets, int32_t cin, int32_t cout, int32_t chunk_rows) {
  WgPlan p;
  if (n_out < 0 || n_out >= (1LL << 31) || num_offsets < 1 || num_offsets > 27 || !wg_pair_ok(cin, cout)) return 0;
  if (!wg_plan(n_out, num_offsets, cin <= 16 ? 16 : cin, cout, chunk_rows, &p)) return 0;
  return p.bytes > 16 ? p.bytes : 16;
}

extern "C" int pcp_spconv3d_wgrad(const float *x, int64_t n_in, int32_t cin, int32_t ld_in, const float *dy, const int32_t *nbr, int32_t num_offsets,
                                  int64_t n_out, int32_t cout, int32_t chunk_rows, void *workspace, size_t workspace_bytes, float *dw,
                                  int32_t accumulate, void *stream_) {
  if (n_in < 0 || n_out < 0 || n_in >= (1LL << 31) || n_out >= (1LL << 31) || num_offsets < 1 || num_offsets > 27 || ld_in < cin) return PCP_ERR_ARG;
  if (!wg_pair_ok(cin, cout)) return PCP_ERR_UNSUPPORTED;
  const int cin_pad = cin <= 16 ? 16 : cin;
  WgPlan p;
  if (!wg_plan(n_out, num_offsets, cin_pad, cout, chunk_rows, &p)) return PCP_ERR_ARG;
  if (!dw) return PCP_ERR_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  const size_t dw_bytes = (size_t)cout * num_offsets * cin * sizeof(float);
  if (n_out == 0 || n_in == 0) {
    if (!accumulate && hipMemsetAsync(dw, 0, dw_bytes, stream) != hipSuccess) return PCP_ERR_LAUNCH;
    return PCP_OK;
  }
  if (!x || !dy || !nbr || !workspace) return PCP_ERR_ARG;
  if ((((uintptr_t)dy) & 15) || (((uintptr_t)workspace) & 15)) return PCP_ERR_ARG;
  if (workspace_bytes < p.bytes) return PCP_ERR_WORKSPACE;
  const bool vec = cin == cin_pad && ld_in % 4 == 0 && (((uintptr_t)x) & 15) == 0;
  if (cin_pad > 16 && !vec) return PCP_ERR_ARG;
  const dim3 grid((unsigned)p.n_chunks, (unsigned)num_offsets);
  float *partial = (float *)workspace;
#define PCP_SPWGRAD(CI_, CO_, V_)                                                                                                               \
  hipLaunchKernelGGL((k_spconv3d_wgrad<CI_, CO_, V_>), grid, dim3(256), 0, stream, x, (int)cin, (int)ld_in, (long long)n_in, dy, nbr, (long long)n_out, \
                     (int)p.chunk, (int)p.parts, partial)
  if (cin_pad == 16 && cout == 16) { if (vec) PCP_SPWGRAD(1, 1, true); else PCP_SPWGRAD(1, 1, false); }
  else if (cin_pad == 16 && cout == 32) { if (vec) PCP_SPWGRAD(1, 2, true); else PCP_SPWGRAD(1, 2, false); }
  else if (cin_pad == 32 && cout == 32) PCP_SPWGRAD(2, 2, true);
  else if (cin_pad == 32 && cout == 64) PCP_SPWGRAD(2, 4, true);
  else if (cin_pad == 64 && cout == 64) PCP_SPWGRAD(4, 4, true);
  else if (cin_pad == 64 && cout == 128) PCP_SPWGRAD(4, 8, true);
  else PCP_SPWGRAD(8, 8, true);
#undef PCP_SPWGRAD
  PCP_CHECK_LAUNCH();
  const long long elems = (long long)num_offsets * cout * cin_pad;
  hipLaunchKernelGGL(k_spconv3d_wgrad_reduce, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, stream, (const float *)partial, (int)num_offsets,
                     (int)p.parts, (int)cout, cin_pad, (int)cin, (int)accumulate, dw);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

extern "C" int pcp_spconv_dense_backward(const float *dcanvas, const int32_t *coords, int64_t n, int32_t channels, int32_t batch, int32_t d, int32_t h,
                                         int32_t w, float *dfeat, void *stream_) {
  if (n < 0 || n >= (1LL << 31) || channels < 1 || batch < 1 || d < 1 || h < 1 || w < 1) return PCP_ERR_ARG;
  if (n == 0) return PCP_OK;
  if (!dcanvas || !coords || !dfeat || (((uintptr_t)coords) & 15)) return PCP_ERR_ARG;
  const long long elems = (long long)n * channels;
  if (elems >= (1LL << 31) * 256) return PCP_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_sp_dense_backward, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, dcanvas, coords, (long long)n,
                     (int)channels, (int)batch, (int)d, (int)h, (int)w, dfeat);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

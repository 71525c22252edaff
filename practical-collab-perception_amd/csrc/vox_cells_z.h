// The z-checking first pass over the point rows that the hard voxeliser (csrc/hard_voxel.hip) and the mean VFE (csrc/spconv3d.hip) share: the
// twin of voxelize.hip's k_point_cells<true> with the z range tested too and, optionally, the cell index along z kept per row.
#pragma once
#include "pcp_common.h"

namespace {

constexpr int CZ_THREADS = 256;
constexpr int CZ_ITEMS = 4;
constexpr int CZ_TILE = CZ_THREADS * CZ_ITEMS;       // 1024 rows per workgroup
constexpr int CZ_HT = 2048;                          // LDS hash table

// -1: outside the range (x, y or z), NaN, or a frame index that is no integer of [0, B); *cz_out: the cell along z of a kept row
__device__ __forceinline__ int cz_point_to_cell(const float *row, const pcp_grid_t g, int nz, int *cz_out) {
  const float fb = row[0];
  const float cx = floorf(__fdiv_rn(__fsub_rn(row[1], g.min_x), g.voxel_x));
  const float cy = floorf(__fdiv_rn(__fsub_rn(row[2], g.min_y), g.voxel_y));
  const float cz = floorf(__fdiv_rn(__fsub_rn(row[3], g.min_z), g.voxel_z));
  const bool ok = (cx >= 0.0f) && (cx < (float)g.nx) && (cy >= 0.0f) && (cy < (float)g.ny) && (cz >= 0.0f) && (cz < (float)nz) &&
                  (fb >= 0.0f) && (fb < (float)g.batch_size);
  *cz_out = ok ? (int)cz : 0;
  if (!ok) return -1;
  return (int)fb * (g.nx * g.ny) + (int)cx * g.ny + (int)cy;
}

// A workgroup counts its 1024 rows in an LDS hash table keyed by cell and reserves the slots of each distinct cell with ONE global integer
// atomic, so the 5 000 rows under the sensor do not queue on one address.  The slots it hands out are arrival order; the callers sort every
// cell's rows before anything reads them.  err_word: bit 0 a frame index that is no integer of [0, B), bit 1 frames not in ascending order.
// KEEP_CZ: point_cz[r] = the row's cell along z.
template <bool KEEP_CZ>
__global__ __launch_bounds__(CZ_THREADS) void k_cells_z(const float *__restrict__ points, long long n, int stride, pcp_grid_t g, int nz,
                                                        int *__restrict__ cell_count, int *__restrict__ point_cell,
                                                        int *__restrict__ point_rank, int *__restrict__ point_cz, int *__restrict__ err_word) {
  __shared__ int h_key[CZ_HT], h_cnt[CZ_HT];
  const long long base = (long long)blockIdx.x * CZ_TILE;
  for (int e = threadIdx.x; e < CZ_HT; e += CZ_THREADS) {
    h_key[e] = -1;
    h_cnt[e] = 0;
  }
  __syncthreads();
  int hslot[CZ_ITEMS], hloc[CZ_ITEMS];
  int err = 0;
#pragma unroll
  for (int i = 0; i < CZ_ITEMS; i++) {
    const long long r = base + i * CZ_THREADS + threadIdx.x;
    hslot[i] = -1;
    hloc[i] = 0;
    if (r < n) {
      const float *row = points + r * stride;
      const float fb = row[0];
      // rows are grouped by ascending frame: an integer of [0, B), never below the row in front
      if (!(fb >= 0.0f && fb < (float)g.batch_size && fb == floorf(fb))) err |= 1;
      if (r > 0 && !(points[(r - 1) * stride] <= fb)) err |= 2;
      int cz = 0;
      const int c = (err == 0) ? cz_point_to_cell(row, g, nz, &cz) : -1;
      point_cell[r] = c;
      if (KEEP_CZ) point_cz[r] = c >= 0 ? cz : 0;
      if (c >= 0) {
        unsigned h = ((unsigned)c * 2654435761u) >> 21;                    // 11 bits
        while (true) {
          const int prev = atomicCAS(&h_key[h], -1, c);
          if (prev == -1 || prev == c) break;
          h = (h + 1) & (CZ_HT - 1);
        }
        hslot[i] = (int)h;
        hloc[i] = atomicAdd(&h_cnt[h], 1);
      }
    }
  }
  if (err) atomicOr(err_word, err);
  __syncthreads();
  for (int e = threadIdx.x; e < CZ_HT; e += CZ_THREADS) {
    const int c = h_key[e];
    if (c >= 0) h_cnt[e] = atomicAdd(&cell_count[c], h_cnt[e]);
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < CZ_ITEMS; i++)
    if (hslot[i] >= 0) point_rank[base + i * CZ_THREADS + threadIdx.x] = h_cnt[hslot[i]] + hloc[i];
}

}  // namespace

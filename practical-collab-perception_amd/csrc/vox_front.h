// What the three point-cloud front ends share, once: the dynamic pillariser (csrc/voxelize.hip), hard voxelisation (csrc/hard_voxel.hip) and the
// mean VFE (csrc/spconv3d.hip).  The row -> cell arithmetic, the LDS cell-hash aggregation of the histogram pass, the z-checking first pass
// k_cells_z, the sort of every pillar's run, the tile-prefix step of the numbering passes and the cell -> coordinates step.  Device helpers
// are __forceinline__, as in wave_ops.h; a loop a kernel still writes out says why beside it.
#pragma once
#include "pcp_common.h"
#include "wave_ops.h"

namespace {

typedef unsigned long long u64;

// the tile every pass over rows, slots or words walks: four items per thread
constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS = 4;
constexpr int SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;   // 1024 elements per workgroup

// ---- row -> cell ---------------------------------------------------------------------------------------------------------------------------
// c = floor((p - min) / voxel) in IEEE fp32 (subtract, then a correctly rounded DIVIDE -- not a multiply by the reciprocal); columns: 0 the
// frame index, 1 x, 2 y, 3 z.  -1: outside the range, NaN, or a frame index outside [0, B).  The comparisons are on floats: NaN / inf /
// out-of-range all fail (torch's (coords >= 0) & (coords < grid) on the int32 cast gives the same verdict for every finite in-int-range value).
// CHECK_Z: the z range [0, nz) is tested too and *cz_out is the cell along z of a kept row; without it only x and y decide (the pillariser).
template <bool CHECK_Z>
__device__ __forceinline__ int point_to_cell(const float *row, const pcp_grid_t g, int nz = 1, int *cz_out = nullptr) {
  const float fb = row[0];
  const float cx = floorf(__fdiv_rn(__fsub_rn(row[1], g.min_x), g.voxel_x));
  const float cy = floorf(__fdiv_rn(__fsub_rn(row[2], g.min_y), g.voxel_y));
  const float cz = CHECK_Z ? floorf(__fdiv_rn(__fsub_rn(row[3], g.min_z), g.voxel_z)) : 0.0f;
  const bool ok = (cx >= 0.0f) && (cx < (float)g.nx) && (cy >= 0.0f) && (cy < (float)g.ny) && (!CHECK_Z || ((cz >= 0.0f) && (cz < (float)nz))) &&
                  (fb >= 0.0f) && (fb < (float)g.batch_size);
  if (CHECK_Z) *cz_out = ok ? (int)cz : 0;
  if (!ok) return -1;
  return (int)fb * (g.nx * g.ny) + (int)cx * g.ny + (int)cy;
}

// merged id b * nx * ny + cx * ny + cy -> (b, cx, cy)
struct CellCoords { int b, cx, cy; };
__device__ __forceinline__ CellCoords cell_coords(int c, const pcp_grid_t &g) {
  const int plane = g.nx * g.ny;
  CellCoords o;
  o.b = c / plane;
  const int rem = c - o.b * plane;
  o.cx = rem / g.ny;
  o.cy = rem - o.cx * g.ny;
  return o;
}

// ---- LDS cell hash: the histogram of one workgroup's rows ----------------------------------------------------------------------------------
// A workgroup counts its 1024 rows in an LDS table keyed by cell (open addressing: 2048 entries for at most 1024 distinct keys, so a probe
// always ends) and reserves the slots of each distinct cell with ONE global integer atomic, so the 5 000 rows under the sensor do not queue
// on one address.  The slots handed out are arrival order.  clear | per row: insert | reserve | per row: first + local.
constexpr int CELL_HT = 2048;
__device__ __forceinline__ unsigned cell_hash(int c) { return ((unsigned)c * 2654435761u) >> 21; }                    // 11 bits

__device__ __forceinline__ void cell_hash_clear(int *h_key, int *h_cnt) {
  for (int e = threadIdx.x; e < CELL_HT; e += SCAN_THREADS) {
    h_key[e] = -1;
    h_cnt[e] = 0;
  }
  __syncthreads();
}

// returns the entry of cell c; *local: the row's rank among the workgroup's rows of that cell
__device__ __forceinline__ int cell_hash_insert(int *h_key, int *h_cnt, int c, int *local) {
  unsigned h = cell_hash(c);
  while (true) {
    const int prev = atomicCAS(&h_key[h], -1, c);
    if (prev == -1 || prev == c) break;
    h = (h + 1) & (CELL_HT - 1);
  }
  *local = atomicAdd(&h_cnt[h], 1);
  return (int)h;
}

// every occupied entry's count becomes the first slot its rows take in the cell: a row's slot is cell_hash_first(entry) + local
__device__ __forceinline__ void cell_hash_reserve(const int *h_key, int *h_cnt, int *__restrict__ cell_count) {
  __syncthreads();
  for (int e = threadIdx.x; e < CELL_HT; e += SCAN_THREADS) {
    const int c = h_key[e];
    if (c >= 0) h_cnt[e] = atomicAdd(&cell_count[c], h_cnt[e]);
  }
  __syncthreads();
}
__device__ __forceinline__ int cell_hash_first(const int *h_cnt, int entry) { return h_cnt[entry]; }

// The z-checking first pass of the hard voxeliser and the mean VFE.  It is voxelize.hip's k_point_cells<true> but for two things, which is
// why they stay two kernels: this one validates the frame column (err_word: bit 0 a frame index that is no integer of [0, B), bit 1 frames
// not in ascending order) and, with KEEP_CZ, keeps point_cz[r] = the row's cell along z; that one counts the kept rows per tile for unq_inv.
template <bool KEEP_CZ>
__global__ __launch_bounds__(SCAN_THREADS) void k_cells_z(const float *__restrict__ points, long long n, int stride, pcp_grid_t g, int nz,
                                                          int *__restrict__ cell_count, int *__restrict__ point_cell,
                                                          int *__restrict__ point_rank, int *__restrict__ point_cz, int *__restrict__ err_word) {
  __shared__ int h_key[CELL_HT], h_cnt[CELL_HT];
  const long long base = (long long)blockIdx.x * SCAN_TILE;
  cell_hash_clear(h_key, h_cnt);
  int hslot[SCAN_ITEMS], hloc[SCAN_ITEMS];
  int err = 0;
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; i++) {
    const long long r = base + i * SCAN_THREADS + threadIdx.x;
    hslot[i] = -1;
    hloc[i] = 0;
    if (r < n) {
      const float *row = points + r * stride;
      const float fb = row[0];
      // rows are grouped by ascending frame: an integer of [0, B), never below the row in front
      if (!(fb >= 0.0f && fb < (float)g.batch_size && fb == floorf(fb))) err |= 1;
      if (r > 0 && !(points[(r - 1) * stride] <= fb)) err |= 2;
      int cz = 0;
      const int c = (err == 0) ? point_to_cell<true>(row, g, nz, &cz) : -1;
      point_cell[r] = c;
      if (KEEP_CZ) point_cz[r] = c >= 0 ? cz : 0;
      if (c >= 0) hslot[i] = cell_hash_insert(h_key, h_cnt, c, &hloc[i]);
    }
  }
  if (err) atomicOr(err_word, err);
  cell_hash_reserve(h_key, h_cnt, cell_count);
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; i++)
    if (hslot[i] >= 0) point_rank[base + i * SCAN_THREADS + threadIdx.x] = cell_hash_first(h_cnt, hslot[i]) + hloc[i];
}

// ---- the sort of every pillar's run ---------------------------------------------------------------------------------------------------------
// A row's slot inside its pillar comes from the histogram atomic, so the ORDER of a pillar's rows in the bucket order changes from run to
// run.  One thread per pillar sorts its run (runs are a few rows long; insertion sort): the bucket order becomes a function of the input
// alone.  Runs of more than PCP_LONG_PILLAR rows (a LiDAR-like cloud has cells with hundreds to thousands: one thread's insertion sort of
// 5 000 rows in global memory took a SECOND) are ranked by a whole workgroup instead: an element's place is the number of smaller keys (the
// keys are distinct), counted against LDS tiles of the run, four elements per thread and pass; the sorted run is staged in the (by then
// idle) point_rank array and copied back.
// The key of a row: the row index itself (32 bits, no load, no kernel argument), or (cz, row) as 64 bits, built from the kernels' trailing
// arguments SRC (none, or point_cz).
struct RowKey {
  typedef int type;
  static constexpr type PAD = 0x7fffffff;
  __device__ __forceinline__ type operator()(int row) const { return row; }
  static __device__ __forceinline__ int row(type k) { return k; }
};
struct CzRowKey {
  typedef u64 type;
  static constexpr type PAD = ~0ULL;
  const int *__restrict__ point_cz;
  __device__ __forceinline__ type operator()(int row) const { return ((u64)(unsigned)point_cz[row] << 32) | (unsigned)row; }
  static __device__ __forceinline__ int row(type k) { return (int)(unsigned)(k & 0xffffffffULL); }
};
constexpr int SORT_TILE = 2048, SORT_EPT = 4;

// short runs: one thread each (the long ones are on the pillariser's list: k_sort_long_runs)
template <typename KEY, typename... SRC>
__global__ __launch_bounds__(256) void k_sort_runs(const int *__restrict__ pillar_start, const int *__restrict__ counters,
                                                  int *__restrict__ bucket_order, SRC... src) {
  const KEY key{src...};
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= counters[0]) return;
  const int s0 = pillar_start[p], s1 = pillar_start[p + 1];
  if (s1 - s0 > PCP_LONG_PILLAR) return;
  for (int i = s0 + 1; i < s1; ++i) {
    const int v = bucket_order[i];
    const typename KEY::type kv = key(v);
    int j = i - 1;
    while (j >= s0 && key(bucket_order[j]) > kv) {
      bucket_order[j + 1] = bucket_order[j];
      --j;
    }
    bucket_order[j + 1] = v;
  }
}

// one workgroup per listed run, grid-stride: the long runs of a LiDAR-like cloud sit next to each other in pillar order -- left to the
// workgroup that found them, a few workgroups sorted hundreds of runs each (4.9 ms), spread over the chip they take tens of microseconds
template <typename KEY, typename... SRC>
__global__ __launch_bounds__(256) void k_sort_long_runs(const int *__restrict__ pillar_start, int *__restrict__ bucket_order,
                                                       int *__restrict__ scratch, const int *__restrict__ long_list,
                                                       const int *__restrict__ counters, SRC... src) {
  typedef typename KEY::type K;
  const KEY key{src...};
  __shared__ K tile[SORT_TILE];
  const int tid = threadIdx.x;
  const int nl = counters[6];
  for (int li = blockIdx.x; li < nl; li += gridDim.x) {
    const int q = long_list[li];
    const int s0 = pillar_start[q], cnt = pillar_start[q + 1] - s0;
    for (int base = 0; base < cnt; base += 256 * SORT_EPT) {
      K v[SORT_EPT];
      int rank[SORT_EPT];
#pragma unroll
      for (int u = 0; u < SORT_EPT; ++u) {
        const int e = base + u * 256 + tid;
        v[u] = e < cnt ? key(bucket_order[s0 + e]) : KEY::PAD;
        rank[u] = 0;
      }
      for (int tb = 0; tb < cnt; tb += SORT_TILE) {
        const int tn = min(SORT_TILE, cnt - tb);
        __syncthreads();
        for (int j = tid; j < tn; j += 256) tile[j] = key(bucket_order[s0 + tb + j]);
        __syncthreads();
        for (int j = 0; j < tn; ++j) {
          const K w = tile[j];                                      // broadcast read
#pragma unroll
          for (int u = 0; u < SORT_EPT; ++u) rank[u] += w < v[u] ? 1 : 0;
        }
      }
#pragma unroll
      for (int u = 0; u < SORT_EPT; ++u)
        if (base + u * 256 + tid < cnt) scratch[s0 + rank[u]] = KEY::row(v[u]);
    }
    __syncthreads();                                                 // the whole sorted run is in scratch; nobody reads the unsorted one any more
    for (int j = tid; j < cnt; j += 256) bucket_order[s0 + j] = scratch[s0 + j];
    __syncthreads();
  }
}

// both launches on the workspace a pillariser call left (L: its layout, n > 0 rows on `cells` cells)
template <typename KEY, typename... SRC>
inline int sort_pillar_runs(char *ws, const VoxLayout &L, int64_t cells, int64_t n, hipStream_t stream, SRC... src) {
  const int64_t max_pillars = n < cells ? n : cells;
  hipLaunchKernelGGL((k_sort_runs<KEY, SRC...>), dim3((unsigned)((max_pillars + 255) / 256)), dim3(256), 0, stream, (const int *)(ws + L.pillar_start),
                     (const int *)(ws + L.counters), (int *)(ws + L.bucket_order), src...);
  PCP_CHECK_LAUNCH();
  hipLaunchKernelGGL((k_sort_long_runs<KEY, SRC...>), dim3(1024), dim3(256), 0, stream, (const int *)(ws + L.pillar_start), (int *)(ws + L.bucket_order),
                     (int *)(ws + L.point_rank), (const int *)(ws + L.long_list), (const int *)(ws + L.counters), src...);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

// ---- tile sums and the prefix in front of a thread's items ---------------------------------------------------------------------------------
// Two passes number the rows (slots, words) that hold a flag: the first leaves the flags of every 1024-element tile in tile_sums, the second
// gives each thread "tiles in front + exclusive scan inside the tile".  No pass waits for another workgroup.

// wave totals -> thread 0 -> tile_sums[blockIdx.x]; wave_total: the same in every lane of a wave.  wave_tot: SCAN_THREADS / 64 ints of LDS
__device__ __forceinline__ void tile_sum_store(int wave_total, int *wave_tot, int *tile_sums) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) wave_tot[wave] = wave_total;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < SCAN_THREADS / 64; w++) s += wave_tot[w];
    tile_sums[blockIdx.x] = s;
  }
}

// first half: tile_sums[0 .. tile) summed over the workgroup, one partial per wave into red.  A caller forms its flags between the halves
__device__ __forceinline__ void tiles_in_front(const int *__restrict__ tile_sums, int tile, int *red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int pre = 0;
  for (int i = threadIdx.x; i < tile; i += SCAN_THREADS) pre += tile_sums[i];
  pre = wave_sum(pre);
  if (lane == 0) red[wave] = pre;
}

// second half: what lies in front of this thread's items, `local` of which hold a flag.  FRONT: the partials of tiles_in_front are added;
// without it the caller adds a prefix of the tiles it has already.  red, lds_wave: SCAN_THREADS / 64 ints of LDS each
template <bool FRONT>
__device__ __forceinline__ int tile_prefix_before(int local, const int *red, int *lds_wave) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int incl = wave_incl_scan(local, lane);
  if (lane == 63) lds_wave[wave] = incl;
  __syncthreads();
  int before = incl - local;
#pragma unroll
  for (int w = 0; w < SCAN_THREADS / 64; w++) {
    if (FRONT) before += red[w];
    if (w < wave) before += lds_wave[w];
  }
  return before;
}

}  // namespace

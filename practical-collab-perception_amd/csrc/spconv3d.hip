// The SECOND family's front end and 3D backbone (inference): per-voxel mean (DynMeanVFE), the index tables of spconv's SubMConv3d / SparseConv3d,
// the sparse 3D convolution itself and HeightCompression's dense().
//
// Reference behaviour: pcdet/models/backbones_3d/vfe/dynamic_mean_vfe.py:53-79, pcdet/models/backbones_3d/spconv_backbone.py (VoxelResBackBone8x)
// and pcdet/models/backbones_2d/map_to_bev/height_compression.py.  spconv has no ROCm build; nothing here is derived from its sources.
//
// Mean VFE.  The merged id b*nx*ny*nz + cx*ny*nz + cy*nz + cz has the pillariser's id b*nx*ny + cx*ny + cy as its prefix, so a voxel list in
// torch.unique order is every pillar's rows split by cz:
//   k_cells_z<true>   (csrc/vox_front.h, the hard voxeliser's first pass with cz kept) cell id and cz per row, integer histogram
//   pcp_voxelize_cells_ready (csrc/voxelize.hip, called, not changed): rows grouped by pillar in ascending cell id
//   k_sort_runs / k_sort_long_runs <CzRowKey>   (csrc/vox_front.h, the pillariser's sort with another key) a pillar's rows ranked by (cz, input
//                     row); a run of more than PCP_LONG_PILLAR rows by a whole workgroup
//   k_mv_flags / k_mv_number           a slot opens a voxel when its (cell, cz) differs from the slot in front; prefix = voxel number (on
//                     csrc/vox_front.h's tile-sum and tile-prefix helpers, as k_sp_prefix below)
//   k_mv_mean         (after the host read M) a wave per voxel: four lane groups walk rows j = g, g + 4, ... in slot order, (g0 + g1) + (g2 + g3),
//                     IEEE divide by the count.  No float atomics: the sum is a function of the voxel's rows in input order alone.
//
// Index tables.  A coordinate set over a (B, D, H, W) grid is held as a BITMAP (one bit per site, set with integer atomicOr: the result does
// not depend on arrival order) plus an exclusive popcount prefix per 64-bit word.  rank(site) = prefix[word] + popcount(bits below) is the
// site's position in ASCENDING LINEAR (b, z, y, x) ORDER -- the row number of a strided conv's output, with no sort and no hash probing.  A
// set whose rows are in another order (the voxel list of the mean VFE) carries perm[rank] = row.
//
// Convolution.  Output-stationary: a wave owns 16 output rows and all output channels, walks the K offsets in ascending order, gathers the
// present neighbour rows straight into v_mfma_f32_16x16x4_f32 A fragments (absent rows are zero), takes the offset's weight fragments from
// L2 and skips, wave-uniformly, every offset none of its 16 rows has.  Waves share nothing, so there is no LDS stage and no barrier; a row's
// bits depend on its own neighbour list only.  No scatter, no float atomics.
#include "vox_front.h"

namespace {

constexpr int MV_MAX_B = PCP_MEAN_VFE_MAX_BATCH;
constexpr int MV_CNT_M = 0, MV_CNT_ERR = 1, MV_CNT_KEPT = 2;

struct MvLayout {
  VoxLayout v;
  size_t point_cz;         // int32 [n]
  size_t tile_sums;        // int32 [n_tiles + 1]
  size_t vox_start;        // int32 [n + 1]   first slot of voxel v (vox_start[M] = kept rows)
  size_t dense_coords;     // int32 [n][4]    pcp_voxelize_cells_ready insists on writing its own pillar coordinates
  size_t total;
};
inline MvLayout mv_layout(int64_t cells, int64_t n) {
  MvLayout L;
  PcpCarver ws = pcp_behind_vox_layout(cells, n, &L.v);
  L.point_cz = ws.take((size_t)n * 4);
  L.tile_sums = ws.take((size_t)((n + SCAN_TILE - 1) / SCAN_TILE + 1) * 4);
  L.vox_start = ws.take((size_t)(n + 1) * 4);
  L.dense_coords = ws.take((size_t)n * 16);
  L.total = ws.total();
  return L;
}

// does slot s open a voxel?  (cell, cz) differs from the slot in front
__device__ __forceinline__ bool mv_opens(long long s, int kept, const int *__restrict__ order, const int *__restrict__ point_cell,
                                         const int *__restrict__ point_cz) {
  if (s >= kept) return false;
  if (s == 0) return true;
  const int r = order[s], rp = order[s - 1];
  return point_cell[r] != point_cell[rp] || point_cz[r] != point_cz[rp];
}

__global__ __launch_bounds__(SCAN_THREADS) void k_mv_flags(const int *__restrict__ counters_ws, const int *__restrict__ order,
                                                         const int *__restrict__ point_cell, const int *__restrict__ point_cz,
                                                         int *__restrict__ tile_sums) {
  __shared__ int wave_tot[SCAN_THREADS / 64];
  const int kept = counters_ws[1];
  const long long base = (long long)blockIdx.x * SCAN_TILE + (long long)threadIdx.x * SCAN_ITEMS;
  int total = 0;
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; i++) total += mv_opens(base + i, kept, order, point_cell, point_cz) ? 1 : 0;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) total += __shfl_xor(total, d, 64);     // open-coded: the wave_ops.h call changes this kernel's schedule
  tile_sum_store(total, wave_tot, tile_sums);
}

__global__ __launch_bounds__(SCAN_THREADS) void k_mv_number(pcp_grid_t g, const int *__restrict__ counters_ws, const int *__restrict__ order,
                                                          const int *__restrict__ point_cell, const int *__restrict__ point_cz,
                                                          const int *__restrict__ tile_sums, int *__restrict__ vox_start,
                                                          int *__restrict__ voxel_coords, int *__restrict__ counters) {
  __shared__ int red[SCAN_THREADS / 64], lds_wave[SCAN_THREADS / 64];
  const int tile = blockIdx.x;
  const int kept = counters_ws[1];
  tiles_in_front(tile_sums, tile, red);
  const long long base = (long long)tile * SCAN_TILE + (long long)threadIdx.x * SCAN_ITEMS;
  bool open[SCAN_ITEMS];
  int excl[SCAN_ITEMS], local = 0;
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; i++) {
    open[i] = mv_opens(base + i, kept, order, point_cell, point_cz);
    excl[i] = local;
    local += open[i] ? 1 : 0;
  }
  const int before = tile_prefix_before<true>(local, red, lds_wave);
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; i++) {
    const long long s = base + i;
    if (open[i]) {
      const int v = before + excl[i];
      const int r = order[s];
      const CellCoords at = cell_coords(point_cell[r], g);
      vox_start[v] = (int)s;
      *reinterpret_cast<int4 *>(voxel_coords + 4LL * v) = make_int4(at.b, point_cz[r], at.cy, at.cx);       // [b, z, y, x]
    }
    if (s == (long long)kept - 1) {
      const int M = before + excl[i] + (open[i] ? 1 : 0);
      vox_start[M] = kept;
      counters[MV_CNT_M] = M;
      counters[MV_CNT_KEPT] = kept;
    }
  }
  if (kept == 0 && tile == 0 && threadIdx.x == 0) vox_start[0] = 0;       // counters were zero-filled: M = 0
}

// The device-count forms (DEV): the row count is read from device memory, where an earlier kernel of the stream left it, and clamped to the
// capacity the host sized the launch and the buffers by.  Rows at or past it are neither read nor written.
__device__ __forceinline__ long long dev_rows(const int *__restrict__ n_dev, long long capacity) {
  const long long v = *n_dev;
  return v < 0 ? 0 : (v < capacity ? v : capacity);
}

// a wave per voxel; lane = 16 g + column.  DEV: M is the capacity, the count is *n_dev
template <bool DEV>
__global__ __launch_bounds__(256) void k_mv_mean(const float *__restrict__ points, int stride, int C, long long M, const int *__restrict__ vox_start,
                                                 const int *__restrict__ order, float *__restrict__ voxel_features, const int *__restrict__ n_dev) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long v = (long long)blockIdx.x * 4 + wave;
  if (DEV) M = dev_rows(n_dev, M);
  if (v >= M) return;
  const int s0 = vox_start[v], n = vox_start[v + 1] - s0;
  const int col = lane & 15, grp = lane >> 4;
  float acc = 0.f;
  if (col < C)
    for (int j = grp; j < n; j += 4) acc = __fadd_rn(acc, points[(long long)order[s0 + j] * stride + 1 + col]);
  acc = __fadd_rn(acc, __shfl_xor(acc, 16, 64));
  acc = __fadd_rn(acc, __shfl_xor(acc, 32, 64));
  if (grp == 0 && col < C) voxel_features[v * C + col] = __fdiv_rn(acc, (float)n);
}

// the checks behind pcp_front_args' PCP_ERR_ARG ones
inline bool mv_args_ok(const pcp_grid_t *grid, int64_t n, int32_t row_stride, int32_t nz) {
  if (row_stride < 4) return false;
  if (nz < 1 || nz > PCP_MEAN_VFE_MAX_NZ || grid->batch_size > MV_MAX_B) return false;
  return true;
}

}  // namespace

extern "C" size_t pcp_mean_vfe_workspace_bytes(const pcp_grid_t *grid, int64_t max_points) {
  if (!grid || max_points < 0 || grid->nx <= 0 || grid->ny <= 0 || grid->batch_size <= 0) return 0;
  return mv_layout((int64_t)grid->batch_size * grid->nx * grid->ny, max_points > 0 ? max_points : 1).total;
}

extern "C" int pcp_mean_vfe(const float *points, int64_t n, int32_t row_stride, const pcp_grid_t *grid, int32_t nz, void *workspace,
                            size_t workspace_bytes, int32_t *voxel_coords, int32_t *counters, void *stream_) {
  int64_t cells;
  const int front = pcp_front_args(grid, n, &cells);
  if (front == PCP_ERR_ARG || !mv_args_ok(grid, n, row_stride, nz)) return PCP_ERR_ARG;
  if (!workspace || !voxel_coords || !counters || (n > 0 && !points)) return PCP_ERR_ARG;
  if ((((uintptr_t)voxel_coords) & 15) || (((uintptr_t)counters) & 15)) return PCP_ERR_ARG;
  if (front != PCP_OK) return front;
  const int64_t n_alloc = n > 0 ? n : 1;
  const MvLayout L = mv_layout(cells, n_alloc);
  if (workspace_bytes < L.total) return PCP_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  char *ws = (char *)workspace;
  int *cell_count = (int *)(ws + L.v.cell_count);
  int *point_cell = (int *)(ws + L.v.point_cell);
  int *point_rank = (int *)(ws + L.v.point_rank);
  int *point_cz = (int *)(ws + L.point_cz);
  int *bucket_order = (int *)(ws + L.v.bucket_order);
  const int *counters_ws = (const int *)(ws + L.v.counters);
  int *tile_sums = (int *)(ws + L.tile_sums);
  const int n_tiles = (int)((n + SCAN_TILE - 1) / SCAN_TILE);

  if (pcp_zero_async(cell_count, (size_t)cells * 4, stream) != PCP_OK) return PCP_ERR_LAUNCH;
  if (pcp_zero_async(counters, (size_t)PCP_MEAN_VFE_COUNTERS * 4, stream) != PCP_OK) return PCP_ERR_LAUNCH;
  if (n_tiles > 0) {
    hipLaunchKernelGGL(k_cells_z<true>, dim3(n_tiles), dim3(SCAN_THREADS), 0, stream, points, (long long)n, (int)row_stride, *grid, (int)nz, cell_count,
                       point_cell, point_rank, point_cz, counters + MV_CNT_ERR);
    PCP_CHECK_LAUNCH();
  }
  int st = pcp_voxelize_cells_ready(points, n, row_stride, grid, workspace, L.v.total, (int32_t *)(ws + L.dense_coords), nullptr, nullptr, stream_);
  if (st != PCP_OK) return st;
  if (n > 0) {
    st = sort_pillar_runs<CzRowKey>(ws, L.v, cells, n, stream, (const int *)point_cz);
    if (st != PCP_OK) return st;
    hipLaunchKernelGGL(k_mv_flags, dim3(n_tiles), dim3(SCAN_THREADS), 0, stream, counters_ws, bucket_order, point_cell, point_cz, tile_sums);
    PCP_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_mv_number, dim3(n_tiles > 0 ? n_tiles : 1), dim3(SCAN_THREADS), 0, stream, *grid, counters_ws, bucket_order, point_cell, point_cz,
                     tile_sums, (int *)(ws + L.vox_start), voxel_coords, counters);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

// num_voxels: the count (n_dev NULL) or the capacity the launch is sized by (the count is *n_dev)
static int mean_vfe_features(const float *points, int64_t n, int32_t row_stride, int32_t num_features, const pcp_grid_t *grid, int32_t nz,
                             const void *workspace, size_t workspace_bytes, int64_t num_voxels, const int32_t *n_dev, float *voxel_features,
                             void *stream_) {
  int64_t cells;
  const int front = pcp_front_args(grid, n, &cells);
  if (front == PCP_ERR_ARG || !mv_args_ok(grid, n, row_stride, nz)) return PCP_ERR_ARG;
  if (num_features < PCP_MEAN_VFE_MIN_FEATURES || num_features > PCP_MEAN_VFE_MAX_FEATURES || row_stride < 1 + num_features) return PCP_ERR_ARG;
  if (num_voxels < 0 || num_voxels > n) return PCP_ERR_ARG;
  if (num_voxels == 0) return PCP_OK;
  if (!points || !workspace || !voxel_features) return PCP_ERR_ARG;
  if (front != PCP_OK) return front;
  const MvLayout L = mv_layout(cells, n);
  if (workspace_bytes < L.total) return PCP_ERR_WORKSPACE;
  const char *ws = (const char *)workspace;
  const long long blocks = (num_voxels + 3) / 4;
  if (n_dev)
    hipLaunchKernelGGL(k_mv_mean<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream_, points, (int)row_stride, (int)num_features,
                       (long long)num_voxels, (const int *)(ws + L.vox_start), (const int *)(ws + L.v.bucket_order), voxel_features, (const int *)n_dev);
  else
    hipLaunchKernelGGL(k_mv_mean<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream_, points, (int)row_stride, (int)num_features,
                       (long long)num_voxels, (const int *)(ws + L.vox_start), (const int *)(ws + L.v.bucket_order), voxel_features, (const int *)nullptr);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

extern "C" int pcp_mean_vfe_features(const float *points, int64_t n, int32_t row_stride, int32_t num_features, const pcp_grid_t *grid, int32_t nz,
                                     const void *workspace, size_t workspace_bytes, int64_t num_voxels, float *voxel_features, void *stream_) {
  return mean_vfe_features(points, n, row_stride, num_features, grid, nz, workspace, workspace_bytes, num_voxels, nullptr, voxel_features, stream_);
}

extern "C" int pcp_mean_vfe_features_dev(const float *points, int64_t n, int32_t row_stride, int32_t num_features, const pcp_grid_t *grid,
                                         int32_t nz, const void *workspace, size_t workspace_bytes, const int32_t *n_dev, int64_t capacity,
                                         float *voxel_features, void *stream_) {
  if (!n_dev) return PCP_ERR_ARG;
  return mean_vfe_features(points, n, row_stride, num_features, grid, nz, workspace, workspace_bytes, capacity, n_dev, voxel_features, stream_);
}

// ---- index tables ------------------------------------------------------------------------------------------------------------------------------
namespace {

struct SpShape { int B, D, H, W; };
struct SpTable { u64 *bits; int *prefix; int *tile_sums; long long words; int n_tiles; };
struct SpConvGeom { int kz, ky, kx, sz, sy, sx, pz, py, px; };

inline bool sp_shape_ok(const SpShape &s) {
  if (s.B < 1 || s.D < 1 || s.H < 1 || s.W < 1) return false;
  const long long sites = (long long)s.B * s.D * s.H * s.W;
  return s.D <= 4096 && s.H <= 65536 && s.W <= 65536 && sites < (1LL << 37);
}
inline long long sp_words(const SpShape &s) { return ((long long)s.B * s.D * s.H * s.W + 63) / 64; }
inline size_t sp_table_bytes(const SpShape &s) {
  const long long nw = sp_words(s);
  const long long nt = (nw + SCAN_TILE - 1) / SCAN_TILE;
  PcpCarver ws;                                                     // the fields of sp_table below
  ws.take((size_t)nw * 8);
  ws.take((size_t)(nw + 1) * 4);
  ws.take((size_t)(nt + 1) * 4);
  return ws.total();
}
inline SpTable sp_table(void *mem, const SpShape &s) {
  SpTable t;
  t.words = sp_words(s);
  t.n_tiles = (int)((t.words + SCAN_TILE - 1) / SCAN_TILE);
  char *p = (char *)mem;
  PcpCarver ws;
  t.bits = (u64 *)(p + ws.take((size_t)t.words * 8));
  t.prefix = (int *)(p + ws.take((size_t)(t.words + 1) * 4));
  t.tile_sums = (int *)(p + ws.take((size_t)(t.n_tiles + 1) * 4));
  return t;
}

__device__ __forceinline__ long long sp_linear(const SpShape s, int b, int z, int y, int x) { return (((long long)b * s.D + z) * s.H + y) * s.W + x; }

// row of site (b, z, y, x) in the set the table describes, -1 when the site is outside the grid or inactive
__device__ __forceinline__ int sp_lookup(const SpShape s, const u64 *__restrict__ bits, const int *__restrict__ prefix, const int *__restrict__ perm,
                                         int b, int z, int y, int x) {
  if (z < 0 || z >= s.D || y < 0 || y >= s.H || x < 0 || x >= s.W) return -1;
  const long long lin = sp_linear(s, b, z, y, x);
  const u64 word = bits[lin >> 6];
  const int bit = (int)(lin & 63);
  if (!((word >> bit) & 1ULL)) return -1;
  const int rank = prefix[lin >> 6] + __popcll(word & ((1ULL << bit) - 1ULL));
  return perm ? perm[rank] : rank;
}

// sp_lookup for the device-count forms: a row at or past `limit` (the capacity of the set: a clamped tail, or a perm entry nobody wrote) is absent
__device__ __forceinline__ int sp_lookup_below(const SpShape s, const u64 *__restrict__ bits, const int *__restrict__ prefix,
                                               const int *__restrict__ perm, int b, int z, int y, int x, long long limit) {
  const int r = sp_lookup(s, bits, prefix, perm, b, z, y, x);
  return (r >= 0 && r < limit) ? r : -1;
}

template <bool DEV>
__global__ __launch_bounds__(256) void k_sp_mark(const int *__restrict__ coords, long long n, SpShape s, u64 *__restrict__ bits, int *__restrict__ counters,
                                                 const int *__restrict__ n_dev) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (DEV) n = dev_rows(n_dev, n);
  if (i >= n) return;
  const int4 c = *reinterpret_cast<const int4 *>(coords + 4 * i);
  if (c.x < 0 || c.x >= s.B || c.y < 0 || c.y >= s.D || c.z < 0 || c.z >= s.H || c.w < 0 || c.w >= s.W) {
    atomicOr(&counters[1], 1);
    return;
  }
  const long long lin = sp_linear(s, c.x, c.y, c.z, c.w);
  atomicOr(&bits[lin >> 6], 1ULL << (lin & 63));
}

// every output site some input reaches: o = (i + p - d) / s for the offsets d it divides evenly
template <bool DEV>
__global__ __launch_bounds__(256) void k_sp_mark_strided(const int *__restrict__ coords, long long n, SpShape si, SpShape so, SpConvGeom g,
                                                         u64 *__restrict__ bits, int *__restrict__ counters, const int *__restrict__ n_dev) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (DEV) n = dev_rows(n_dev, n);
  if (i >= n) return;
  const int4 c = *reinterpret_cast<const int4 *>(coords + 4 * i);
  if (c.x < 0 || c.x >= si.B || c.y < 0 || c.y >= si.D || c.z < 0 || c.z >= si.H || c.w < 0 || c.w >= si.W) {
    atomicOr(&counters[1], 1);
    return;
  }
  for (int dz = 0; dz < g.kz; dz++) {
    const int tz = c.y + g.pz - dz;
    if (tz < 0 || tz % g.sz) continue;
    const int oz = tz / g.sz;
    if (oz >= so.D) continue;
    for (int dy = 0; dy < g.ky; dy++) {
      const int ty = c.z + g.py - dy;
      if (ty < 0 || ty % g.sy) continue;
      const int oy = ty / g.sy;
      if (oy >= so.H) continue;
      for (int dx = 0; dx < g.kx; dx++) {
        const int tx = c.w + g.px - dx;
        if (tx < 0 || tx % g.sx) continue;
        const int ox = tx / g.sx;
        if (ox >= so.W) continue;
        const long long lin = sp_linear(so, c.x, oz, oy, ox);
        atomicOr(&bits[lin >> 6], 1ULL << (lin & 63));
      }
    }
  }
}

// kept beside vox_front.h's tile_sum_store: that one has a barrier fewer, which changes k_sp_tile_sums' code
__device__ __forceinline__ int sp_block_sum(int v, int *lds4) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);     // open-coded: the wave_ops.h call changes k_sp_tile_sums' schedule
  __syncthreads();
  if (lane == 0) lds4[wave] = v;
  __syncthreads();
  return lds4[0] + lds4[1] + lds4[2] + lds4[3];
}

__global__ __launch_bounds__(SCAN_THREADS) void k_sp_tile_sums(const u64 *__restrict__ bits, long long words, int *__restrict__ tile_sums) {
  __shared__ int lds4[4];
  const long long base = (long long)blockIdx.x * SCAN_TILE + (long long)threadIdx.x * SCAN_ITEMS;
  int t = 0;
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; i++)
    if (base + i < words) t += __popcll(bits[base + i]);
  const int s = sp_block_sum(t, lds4);
  if (threadIdx.x == 0) tile_sums[blockIdx.x] = s;
}

// one workgroup: tile_sums becomes its exclusive prefix, the total goes to tile_sums[n_tiles] and counters[0].  DEV: counters[0] is the total
// clamped to `capacity`, counters[2] the total itself, and a total above the capacity sets `err_bit` in *err (one thread of one workgroup, and
// the kernels of a stream run in order: a plain read-modify-write)
template <bool DEV>
__global__ __launch_bounds__(SCAN_THREADS) void k_sp_scan_tiles(int *__restrict__ tile_sums, int n_tiles, int *__restrict__ counters, long long capacity,
                                                              int *__restrict__ err, int err_bit) {
  __shared__ int lds_wave[SCAN_THREADS / 64];
  __shared__ int carry_s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (int base = 0; base < n_tiles; base += SCAN_THREADS) {
    const int i = base + threadIdx.x;
    const int v = i < n_tiles ? tile_sums[i] : 0;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(incl, d, 64);     // open-coded: the wave_ops.h call changes this kernel's schedule
      if (lane >= d) incl += up;
    }
    if (lane == 63) lds_wave[wave] = incl;
    __syncthreads();
    int before = carry_s + incl - v;
    int total = 0;
#pragma unroll
    for (int w = 0; w < SCAN_THREADS / 64; w++) {
      if (w < wave) before += lds_wave[w];
      total += lds_wave[w];
    }
    if (i < n_tiles) tile_sums[i] = before;
    __syncthreads();
    if (threadIdx.x == 0) carry_s += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    tile_sums[n_tiles] = carry_s;
    if (DEV) {
      counters[0] = carry_s > capacity ? (int)capacity : carry_s;
      counters[2] = carry_s;
      if (carry_s > capacity && err) *err = *err | err_bit;
    } else {
      counters[0] = carry_s;
    }
  }
}

__global__ __launch_bounds__(SCAN_THREADS) void k_sp_prefix(const u64 *__restrict__ bits, long long words, const int *__restrict__ tile_sums,
                                                          int *__restrict__ prefix) {
  __shared__ int lds_wave[SCAN_THREADS / 64];
  const long long base = (long long)blockIdx.x * SCAN_TILE + (long long)threadIdx.x * SCAN_ITEMS;
  int excl[SCAN_ITEMS], local = 0;
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; i++) {
    excl[i] = local;
    if (base + i < words) local += __popcll(bits[base + i]);
  }
  const int before = tile_sums[blockIdx.x] + tile_prefix_before<false>(local, nullptr, lds_wave);     // tile_sums: k_sp_scan_tiles' prefix already
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; i++)
    if (base + i < words) prefix[base + i] = before + excl[i];
}

// perm[rank of row i's site] = i (the sites of a valid set are distinct: one writer per entry)
template <bool DEV>
__global__ __launch_bounds__(256) void k_sp_perm(const int *__restrict__ coords, long long n, SpShape s, const u64 *__restrict__ bits,
                                                 const int *__restrict__ prefix, int *__restrict__ perm, const int *__restrict__ n_dev) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (DEV) n = dev_rows(n_dev, n);
  if (i >= n) return;
  const int4 c = *reinterpret_cast<const int4 *>(coords + 4 * i);
  if (c.x < 0 || c.x >= s.B) return;
  const int rank = sp_lookup(s, bits, prefix, nullptr, c.x, c.y, c.z, c.w);
  if (rank >= 0 && rank < n) perm[rank] = (int)i;
}

// nbr[k][row] sits at k * ld + row: ld is the row count, or (DEV) the capacity n, with the count in *n_dev
template <bool DEV>
__global__ __launch_bounds__(256) void k_sp_subm_nbr(const int *__restrict__ coords, long long n, SpShape s, const u64 *__restrict__ bits,
                                                     const int *__restrict__ prefix, const int *__restrict__ perm, int *__restrict__ nbr,
                                                     const int *__restrict__ n_dev) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long ld = n;
  if (DEV) n = dev_rows(n_dev, n);
  if (i >= n) return;
  const int4 c = *reinterpret_cast<const int4 *>(coords + 4 * i);
  const bool ok = c.x >= 0 && c.x < s.B;
  int k = 0;
  for (int dz = -1; dz <= 1; dz++)
    for (int dy = -1; dy <= 1; dy++)
      for (int dx = -1; dx <= 1; dx++, k++) {
        int r = -1;
        if (ok) r = DEV ? sp_lookup_below(s, bits, prefix, perm, c.x, c.y + dz, c.z + dy, c.w + dx, ld) : sp_lookup(s, bits, prefix, perm, c.x, c.y + dz, c.z + dy, c.w + dx);
        nbr[(long long)k * ld + i] = r;
      }
}

// the coordinates of a table's sites in rank order: a thread per 64-bit word
template <bool DEV>
__global__ __launch_bounds__(256) void k_sp_table_coords(SpShape s, const u64 *__restrict__ bits, const int *__restrict__ prefix, long long words,
                                                         long long n_out, int *__restrict__ coords, const int *__restrict__ n_dev) {
  const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
  if (w >= words) return;
  if (DEV) n_out = dev_rows(n_dev, n_out);
  u64 word = bits[w];
  long long rank = prefix[w];
  while (word) {
    const int bit = __ffsll((long long)word) - 1;
    word &= word - 1;
    long long lin = w * 64 + bit;
    const int x = (int)(lin % s.W);
    lin /= s.W;
    const int y = (int)(lin % s.H);
    lin /= s.H;
    const int z = (int)(lin % s.D);
    const int b = (int)(lin / s.D);
    if (rank < n_out) *reinterpret_cast<int4 *>(coords + 4 * rank) = make_int4(b, z, y, x);
    rank++;
  }
}

// DEV: n_out is the capacity (and the stride of nbr), the count is *n_dev, and an input row at or past in_limit is absent
template <bool DEV>
__global__ __launch_bounds__(256) void k_sp_strided_nbr(const int *__restrict__ out_coords, long long n_out, SpShape si, SpConvGeom g,
                                                        const u64 *__restrict__ bits, const int *__restrict__ prefix, const int *__restrict__ perm,
                                                        int *__restrict__ nbr, const int *__restrict__ n_dev, long long in_limit) {
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long ld = n_out;
  if (DEV) n_out = dev_rows(n_dev, n_out);
  if (o >= n_out) return;
  const int4 c = *reinterpret_cast<const int4 *>(out_coords + 4 * o);
  const bool ok = c.x >= 0 && c.x < si.B;
  int k = 0;
  for (int dz = 0; dz < g.kz; dz++)
    for (int dy = 0; dy < g.ky; dy++)
      for (int dx = 0; dx < g.kx; dx++, k++) {
        const int z = c.y * g.sz - g.pz + dz, y = c.z * g.sy - g.py + dy, x = c.w * g.sx - g.px + dx;
        int r = -1;
        if (ok) r = DEV ? sp_lookup_below(si, bits, prefix, perm, c.x, z, y, x, in_limit) : sp_lookup(si, bits, prefix, perm, c.x, z, y, x);
        nbr[(long long)k * ld + o] = r;
      }
}

// bits are set; tile sums, their scan (total -> counters[0]) and the per-word prefix
// capacity >= 0: the device-count form of the scan (clamped count, overflow bit)
int sp_finish_table(const SpTable &t, int *counters, hipStream_t stream, long long capacity = -1, int *err = nullptr, int err_bit = 0) {
  hipLaunchKernelGGL(k_sp_tile_sums, dim3(t.n_tiles), dim3(SCAN_THREADS), 0, stream, (const u64 *)t.bits, t.words, t.tile_sums);
  PCP_CHECK_LAUNCH();
  if (capacity >= 0)
    hipLaunchKernelGGL(k_sp_scan_tiles<true>, dim3(1), dim3(SCAN_THREADS), 0, stream, t.tile_sums, t.n_tiles, counters, capacity, err, err_bit);
  else
    hipLaunchKernelGGL(k_sp_scan_tiles<false>, dim3(1), dim3(SCAN_THREADS), 0, stream, t.tile_sums, t.n_tiles, counters, 0LL, (int *)nullptr, 0);
  PCP_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_sp_prefix, dim3(t.n_tiles), dim3(SCAN_THREADS), 0, stream, (const u64 *)t.bits, t.words, (const int *)t.tile_sums, t.prefix);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

inline bool sp_geom_ok(const SpConvGeom &g) {
  const int k[3] = {g.kz, g.ky, g.kx}, s[3] = {g.sz, g.sy, g.sx}, p[3] = {g.pz, g.py, g.px};
  for (int a = 0; a < 3; a++)
    if (k[a] < 1 || k[a] > 3 || s[a] < 1 || s[a] > 3 || p[a] < 0 || p[a] > 2) return false;
  return true;
}
inline int sp_out_extent(int in, int k, int s, int p) { return in + 2 * p >= k ? (in + 2 * p - k) / s + 1 : 0; }
inline SpShape sp_out_shape(const SpShape &si, const SpConvGeom &g) {
  return SpShape{si.B, sp_out_extent(si.D, g.kz, g.sz, g.pz), sp_out_extent(si.H, g.ky, g.sy, g.py), sp_out_extent(si.W, g.kx, g.sx, g.px)};
}

}  // namespace

extern "C" size_t pcp_spconv_table_bytes(int32_t batch, int32_t d, int32_t h, int32_t w) {
  const SpShape s{batch, d, h, w};
  return sp_shape_ok(s) ? sp_table_bytes(s) : 0;
}

// n_dev NULL: n is the count.  Otherwise n is the capacity (launch size) and *n_dev the count.
template <bool DEV>
static int spconv_table_build(const int32_t *coords, int64_t n, const int32_t *n_dev, int32_t batch, int32_t d, int32_t h, int32_t w, void *table,
                              size_t table_bytes, int32_t *perm, int32_t *counters, void *stream_) {
  const SpShape s{batch, d, h, w};
  if (!sp_shape_ok(s) || n < 0 || n >= (1LL << 31) || !table || !counters || (n > 0 && (!coords || !perm))) return PCP_ERR_ARG;
  if ((((uintptr_t)coords) & 15) || (((uintptr_t)table) & 255)) return PCP_ERR_ARG;
  if (table_bytes < sp_table_bytes(s)) return PCP_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const SpTable t = sp_table(table, s);
  if (pcp_zero_async(t.bits, (size_t)t.words * 8, stream) != PCP_OK) return PCP_ERR_LAUNCH;
  if (pcp_zero_async(counters, 16, stream) != PCP_OK) return PCP_ERR_LAUNCH;
  const unsigned nb = (unsigned)((n + 255) / 256);
  if (n > 0) {
    hipLaunchKernelGGL(k_sp_mark<DEV>, dim3(nb), dim3(256), 0, stream, coords, (long long)n, s, t.bits, counters, (const int *)n_dev);
    PCP_CHECK_LAUNCH();
  }
  const int st = sp_finish_table(t, counters, stream);
  if (st != PCP_OK) return st;
  if (n > 0) {
    hipLaunchKernelGGL(k_sp_perm<DEV>, dim3(nb), dim3(256), 0, stream, coords, (long long)n, s, (const u64 *)t.bits, (const int *)t.prefix, perm,
                       (const int *)n_dev);
    PCP_CHECK_LAUNCH();
  }
  return PCP_OK;
}

extern "C" int pcp_spconv_table_build(const int32_t *coords, int64_t n, int32_t batch, int32_t d, int32_t h, int32_t w, void *table,
                                      size_t table_bytes, int32_t *perm, int32_t *counters, void *stream_) {
  return spconv_table_build<false>(coords, n, nullptr, batch, d, h, w, table, table_bytes, perm, counters, stream_);
}

extern "C" int pcp_spconv_table_build_dev(const int32_t *coords, const int32_t *n_dev, int64_t capacity, int32_t batch, int32_t d, int32_t h,
                                          int32_t w, void *table, size_t table_bytes, int32_t *perm, int32_t *counters, void *stream_) {
  if (!n_dev) return PCP_ERR_ARG;
  return spconv_table_build<true>(coords, capacity, n_dev, batch, d, h, w, table, table_bytes, perm, counters, stream_);
}

template <bool DEV>
static int spconv_build_subm(const int32_t *coords, int64_t n, const int32_t *n_dev, int32_t batch, int32_t d, int32_t h, int32_t w,
                             const void *table, size_t table_bytes, const int32_t *perm, int32_t *nbr, void *stream_) {
  const SpShape s{batch, d, h, w};
  if (!sp_shape_ok(s) || n < 0 || n >= (1LL << 31) || !table) return PCP_ERR_ARG;
  if (n == 0) return PCP_OK;
  if (!coords || !nbr || (((uintptr_t)coords) & 15) || (((uintptr_t)table) & 255)) return PCP_ERR_ARG;
  if (table_bytes < sp_table_bytes(s)) return PCP_ERR_WORKSPACE;
  const SpTable t = sp_table(const_cast<void *>(table), s);
  hipLaunchKernelGGL(k_sp_subm_nbr<DEV>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, coords, (long long)n, s,
                     (const u64 *)t.bits, (const int *)t.prefix, perm, nbr, (const int *)n_dev);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

extern "C" int pcp_spconv_build_subm(const int32_t *coords, int64_t n, int32_t batch, int32_t d, int32_t h, int32_t w, const void *table,
                                     size_t table_bytes, const int32_t *perm, int32_t *nbr, void *stream_) {
  return spconv_build_subm<false>(coords, n, nullptr, batch, d, h, w, table, table_bytes, perm, nbr, stream_);
}

extern "C" int pcp_spconv_build_subm_dev(const int32_t *coords, const int32_t *n_dev, int64_t capacity, int32_t batch, int32_t d, int32_t h,
                                         int32_t w, const void *table, size_t table_bytes, const int32_t *perm, int32_t *nbr, void *stream_) {
  if (!n_dev) return PCP_ERR_ARG;
  return spconv_build_subm<true>(coords, capacity, n_dev, batch, d, h, w, table, table_bytes, perm, nbr, stream_);
}

// out_capacity < 0: the host-count form
template <bool DEV>
static int spconv_strided_sites(const int32_t *in_coords, int64_t n_in, const int32_t *n_in_dev, int32_t batch, int32_t d, int32_t h, int32_t w,
                                const int32_t *kernel3, const int32_t *stride3, const int32_t *pad3, void *out_table, size_t out_table_bytes,
                                int64_t out_capacity, int32_t *counters, int32_t *err, int32_t err_bit, void *stream_) {
  if (!kernel3 || !stride3 || !pad3) return PCP_ERR_ARG;
  const SpShape si{batch, d, h, w};
  const SpConvGeom g{kernel3[0], kernel3[1], kernel3[2], stride3[0], stride3[1], stride3[2], pad3[0], pad3[1], pad3[2]};
  if (!sp_shape_ok(si) || !sp_geom_ok(g) || n_in < 0 || n_in >= (1LL << 31) || !out_table || !counters || (n_in > 0 && !in_coords)) return PCP_ERR_ARG;
  const SpShape so = sp_out_shape(si, g);
  if (!sp_shape_ok(so)) return PCP_ERR_ARG;
  if ((((uintptr_t)in_coords) & 15) || (((uintptr_t)out_table) & 255)) return PCP_ERR_ARG;
  if (out_table_bytes < sp_table_bytes(so)) return PCP_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const SpTable t = sp_table(out_table, so);
  if (pcp_zero_async(t.bits, (size_t)t.words * 8, stream) != PCP_OK) return PCP_ERR_LAUNCH;
  if (pcp_zero_async(counters, 16, stream) != PCP_OK) return PCP_ERR_LAUNCH;
  if (n_in > 0) {
    hipLaunchKernelGGL(k_sp_mark_strided<DEV>, dim3((unsigned)((n_in + 255) / 256)), dim3(256), 0, stream, in_coords, (long long)n_in, si, so, g,
                       t.bits, counters, (const int *)n_in_dev);
    PCP_CHECK_LAUNCH();
  }
  return DEV ? sp_finish_table(t, counters, stream, out_capacity, err, err_bit) : sp_finish_table(t, counters, stream);
}

extern "C" int pcp_spconv_strided_sites(const int32_t *in_coords, int64_t n_in, int32_t batch, int32_t d, int32_t h, int32_t w,
                                        const int32_t *kernel3, const int32_t *stride3, const int32_t *pad3, void *out_table,
                                        size_t out_table_bytes, int32_t *counters, void *stream_) {
  return spconv_strided_sites<false>(in_coords, n_in, nullptr, batch, d, h, w, kernel3, stride3, pad3, out_table, out_table_bytes, -1, counters,
                                     nullptr, 0, stream_);
}

extern "C" int pcp_spconv_strided_sites_dev(const int32_t *in_coords, const int32_t *n_in_dev, int64_t in_capacity, int32_t batch, int32_t d,
                                            int32_t h, int32_t w, const int32_t *kernel3, const int32_t *stride3, const int32_t *pad3,
                                            void *out_table, size_t out_table_bytes, int64_t out_capacity, int32_t *counters, int32_t *err,
                                            int32_t err_bit, void *stream_) {
  if (!n_in_dev || out_capacity < 0 || out_capacity >= (1LL << 31)) return PCP_ERR_ARG;
  return spconv_strided_sites<true>(in_coords, in_capacity, n_in_dev, batch, d, h, w, kernel3, stride3, pad3, out_table, out_table_bytes,
                                    out_capacity, counters, err, err_bit, stream_);
}

// in_limit: rows of the input set the caller's buffers hold (DEV only)
template <bool DEV>
static int spconv_build_strided(int32_t batch, int32_t d, int32_t h, int32_t w, const void *in_table, size_t in_table_bytes, const int32_t *in_perm,
                                int64_t in_limit, const int32_t *kernel3, const int32_t *stride3, const int32_t *pad3, const void *out_table,
                                size_t out_table_bytes, int64_t n_out, const int32_t *n_out_dev, int32_t *out_coords, int32_t *nbr,
                                void *stream_) {
  if (!kernel3 || !stride3 || !pad3) return PCP_ERR_ARG;
  const SpShape si{batch, d, h, w};
  const SpConvGeom g{kernel3[0], kernel3[1], kernel3[2], stride3[0], stride3[1], stride3[2], pad3[0], pad3[1], pad3[2]};
  if (!sp_shape_ok(si) || !sp_geom_ok(g) || n_out < 0 || n_out >= (1LL << 31) || !in_table || !out_table) return PCP_ERR_ARG;
  const SpShape so = sp_out_shape(si, g);
  if (!sp_shape_ok(so)) return PCP_ERR_ARG;
  if (n_out == 0) return PCP_OK;
  if (!out_coords || !nbr || (((uintptr_t)out_coords) & 15) || (((uintptr_t)in_table) & 255) || (((uintptr_t)out_table) & 255)) return PCP_ERR_ARG;
  if (in_table_bytes < sp_table_bytes(si) || out_table_bytes < sp_table_bytes(so)) return PCP_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const SpTable ti = sp_table(const_cast<void *>(in_table), si), to = sp_table(const_cast<void *>(out_table), so);
  hipLaunchKernelGGL(k_sp_table_coords<DEV>, dim3((unsigned)((to.words + 255) / 256)), dim3(256), 0, stream, so, (const u64 *)to.bits,
                     (const int *)to.prefix, to.words, (long long)n_out, out_coords, (const int *)n_out_dev);
  PCP_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_sp_strided_nbr<DEV>, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, stream, (const int *)out_coords, (long long)n_out, si,
                     g, (const u64 *)ti.bits, (const int *)ti.prefix, in_perm, nbr, (const int *)n_out_dev, (long long)in_limit);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

extern "C" int pcp_spconv_build_strided(int32_t batch, int32_t d, int32_t h, int32_t w, const void *in_table, size_t in_table_bytes,
                                        const int32_t *in_perm, const int32_t *kernel3, const int32_t *stride3, const int32_t *pad3,
                                        const void *out_table, size_t out_table_bytes, int64_t n_out, int32_t *out_coords, int32_t *nbr,
                                        void *stream_) {
  return spconv_build_strided<false>(batch, d, h, w, in_table, in_table_bytes, in_perm, 0, kernel3, stride3, pad3, out_table, out_table_bytes, n_out,
                                     nullptr, out_coords, nbr, stream_);
}

extern "C" int pcp_spconv_build_strided_dev(int32_t batch, int32_t d, int32_t h, int32_t w, const void *in_table, size_t in_table_bytes,
                                            const int32_t *in_perm, int64_t in_capacity, const int32_t *kernel3, const int32_t *stride3,
                                            const int32_t *pad3, const void *out_table, size_t out_table_bytes, const int32_t *n_out_dev,
                                            int64_t out_capacity, int32_t *out_coords, int32_t *nbr, void *stream_) {
  if (!n_out_dev || in_capacity < 0) return PCP_ERR_ARG;
  return spconv_build_strided<true>(batch, d, h, w, in_table, in_table_bytes, in_perm, in_capacity, kernel3, stride3, pad3, out_table,
                                    out_table_bytes, out_capacity, n_out_dev, out_coords, nbr, stream_);
}

// ---- the convolution ---------------------------------------------------------------------------------------------------------------------------
namespace {

// wave = 16 output rows x all CO16 * 16 channels.  MFMA operands (as k_sparse_conv_s2): lane (m = lane & 15, q = lane >> 4) supplies
// A[row m][k = q] and B[k = q][column m]; step (j, kk) of the reduction covers input channels 16 j + 4 q + kk, q = 0 .. 3, so the order over
// cin is fixed: j ascending, kk ascending.  acc[c][i] is output row 4 q + i, channel 16 c + m.
// VEC: cin == CI16 * 16 and 16-byte aligned rows; otherwise (the first layer's 3 .. 16 columns) guarded scalar loads, zeros behind cin.
// DEV: n_out is the capacity (the launch size), the row count is *n_dev and nbr[k][row] sits at k * ld_nbr + row; otherwise the stride of nbr
// is n_out itself.  One body: a row's bits depend on its own neighbour list only, so the two forms give a row the same bits.
template <int CI16, int CO16, bool VEC, bool DEV>
__global__ __launch_bounds__(256) void k_spconv3d(const float *__restrict__ feat, int cin, int ld_in, const int *__restrict__ nbr, int K, long long n_out,
                                                  const float *__restrict__ w, const float *__restrict__ bias, const float *__restrict__ residual,
                                                  int relu, float *__restrict__ out, const int *__restrict__ n_dev, long long ld_nbr) {
  constexpr int CI = CI16 * 16, CO = CO16 * 16;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m = lane & 15, q = lane >> 4;
  const long long row0 = ((long long)blockIdx.x * 4 + wave) * 16;
  if (DEV) n_out = dev_rows(n_dev, n_out);
  if (row0 >= n_out) return;
  const long long ld = DEV ? ld_nbr : n_out;
  const long long row = row0 + m;
  f32x4 acc[CO16];
#pragma unroll
  for (int c = 0; c < CO16; c++) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < K; k++) {
    const int idx = row < n_out ? nbr[(long long)k * ld + row] : -1;
    if (__ballot(idx >= 0) == 0ULL) continue;              // none of the 16 rows has this neighbour: wave-uniform
    f32x4 a[CI16];
#pragma unroll
    for (int j = 0; j < CI16; j++) {
      a[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (idx >= 0) {
        const float *src = feat + (long long)idx * ld_in + 16 * j + 4 * q;
        if (VEC) {
          a[j] = *reinterpret_cast<const f32x4 *>(src);
        } else {
#pragma unroll
          for (int kk = 0; kk < 4; kk++)
            if (16 * j + 4 * q + kk < cin) a[j][kk] = src[kk];
        }
      }
    }
    const float *wk = w + (long long)k * CO * CI + (long long)m * CI + 4 * q;
#pragma unroll
    for (int c = 0; c < CO16; c++) {
      f32x4 b[CI16];
#pragma unroll
      for (int j = 0; j < CI16; j++) b[j] = *reinterpret_cast<const f32x4 *>(wk + (long long)c * 16 * CI + 16 * j);
#pragma unroll
      for (int j = 0; j < CI16; j++)
#pragma unroll
        for (int kk = 0; kk < 4; kk++) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j][kk], b[j][kk], acc[c], 0, 0, 0);
    }
  }
#pragma unroll
  for (int c = 0; c < CO16; c++) {
    const float bv = bias[16 * c + m];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const long long r = row0 + 4 * q + i;
      if (r < n_out) {
        float v = acc[c][i] + bv;
        if (residual) v += residual[r * CO + 16 * c + m];
        if (relu) v = fmaxf(v, 0.f);
        out[r * CO + 16 * c + m] = v;
      }
    }
  }
}

// every element of the (B, H, W, C * D) canvas is written: channel c * D + d of pixel (b, y, x) is feature c of site (b, d, y, x), or zero
// LIM: a site whose row lies at or past `limit` (the tail a clamped build dropped) reads as empty
template <bool LIM>
__global__ __launch_bounds__(256) void k_sp_dense(const float *__restrict__ feat, int C, SpShape s, const u64 *__restrict__ bits,
                                                  const int *__restrict__ prefix, const int *__restrict__ perm, float *__restrict__ out, long long limit) {
  __shared__ int rows[PCP_MEAN_VFE_MAX_NZ];
  const long long pix = blockIdx.x;                               // (b * H + y) * W + x
  const int x = (int)(pix % s.W);
  const int y = (int)((pix / s.W) % s.H);
  const int b = (int)(pix / ((long long)s.W * s.H));
  if ((int)threadIdx.x < s.D)
    rows[threadIdx.x] = LIM ? sp_lookup_below(s, bits, prefix, perm, b, (int)threadIdx.x, y, x, limit) : sp_lookup(s, bits, prefix, perm, b, (int)threadIdx.x, y, x);
  __syncthreads();
  const int CD = C * s.D;
  for (int ch = threadIdx.x; ch < CD; ch += 256) {
    const int c = ch / s.D, d = ch - c * s.D;
    const int r = rows[d];
    out[pix * CD + ch] = r >= 0 ? feat[(long long)r * C + c] : 0.f;
  }
}

}  // namespace

// n_dev NULL: n_out is the count and the stride of nbr
template <bool DEV>
static int spconv3d(const float *features, int64_t n_in, int32_t cin, int32_t ld_in, const int32_t *nbr, int64_t ld_nbr, int32_t num_offsets,
                    int64_t n_out, const int32_t *n_dev, const float *w_packed, const float *bias, const float *residual, int32_t relu, int32_t cout,
                    float *out, void *stream_) {
  if (n_in < 0 || n_out < 0 || n_in >= (1LL << 31) || n_out >= (1LL << 31) || num_offsets < 1 || num_offsets > 27 || ld_in < cin) return PCP_ERR_ARG;
  const int cin_pad = cin <= 16 ? 16 : cin;
  // (32 -> 16), (64 -> 32), (128 -> 64): the data gradients of the strided layers (csrc/spconv3d_train.hip)
  const bool pair_ok = cin >= 3 && ((cin_pad == 16 && (cout == 16 || cout == 32)) || (cin_pad == 32 && (cout == 16 || cout == 32 || cout == 64)) ||
                                    (cin_pad == 64 && (cout == 32 || cout == 64 || cout == 128)) || (cin_pad == 128 && (cout == 64 || cout == 128)));
  if (!pair_ok) return PCP_ERR_UNSUPPORTED;
  if (n_out == 0) return PCP_OK;
  if (!nbr || !w_packed || !bias || !out || (n_in > 0 && !features)) return PCP_ERR_ARG;
  if ((((uintptr_t)w_packed) & 15)) return PCP_ERR_ARG;
  const bool vec = cin == cin_pad && ld_in % 4 == 0 && (((uintptr_t)features) & 15) == 0;
  if (cin_pad > 16 && !vec) return PCP_ERR_ARG;
  const long long blocks = (n_out + 63) / 64;
  hipStream_t stream = (hipStream_t)stream_;
#define PCP_SPCONV(CI_, CO_, V_)                                                                                                                \
  hipLaunchKernelGGL((k_spconv3d<CI_, CO_, V_, DEV>), dim3((unsigned)blocks), dim3(256), 0, stream, features, (int)cin, (int)ld_in, nbr,           \
                     (int)num_offsets, (long long)n_out, w_packed, bias, residual, (int)relu, out, (const int *)n_dev, (long long)ld_nbr)
  if (cin_pad == 16 && cout == 16) { if (vec) PCP_SPCONV(1, 1, true); else PCP_SPCONV(1, 1, false); }
  else if (cin_pad == 16 && cout == 32) { if (vec) PCP_SPCONV(1, 2, true); else PCP_SPCONV(1, 2, false); }
  else if (cin_pad == 32 && cout == 16) PCP_SPCONV(2, 1, true);
  else if (cin_pad == 32 && cout == 32) PCP_SPCONV(2, 2, true);
  else if (cin_pad == 32 && cout == 64) PCP_SPCONV(2, 4, true);
  else if (cin_pad == 64 && cout == 32) PCP_SPCONV(4, 2, true);
  else if (cin_pad == 64 && cout == 64) PCP_SPCONV(4, 4, true);
  else if (cin_pad == 64 && cout == 128) PCP_SPCONV(4, 8, true);
  else if (cin_pad == 128 && cout == 64) PCP_SPCONV(8, 4, true);
  else PCP_SPCONV(8, 8, true);
#undef PCP_SPCONV
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

extern "C" int pcp_spconv3d(const float *features, int64_t n_in, int32_t cin, int32_t ld_in, const int32_t *nbr, int32_t num_offsets, int64_t n_out,
                            const float *w_packed, const float *bias, const float *residual, int32_t relu, int32_t cout, float *out,
                            void *stream_) {
  return spconv3d<false>(features, n_in, cin, ld_in, nbr, n_out, num_offsets, n_out, nullptr, w_packed, bias, residual, relu, cout, out, stream_);
}

extern "C" int pcp_spconv3d_dev(const float *features, int64_t in_capacity, int32_t cin, int32_t ld_in, const int32_t *nbr, int64_t ld_nbr,
                                int32_t num_offsets, const int32_t *n_dev, int64_t capacity, const float *w_packed, const float *bias,
                                const float *residual, int32_t relu, int32_t cout, float *out, void *stream_) {
  if (!n_dev || ld_nbr < capacity) return PCP_ERR_ARG;
  return spconv3d<true>(features, in_capacity, cin, ld_in, nbr, ld_nbr, num_offsets, capacity, n_dev, w_packed, bias, residual, relu, cout, out,
                        stream_);
}

template <bool LIM>
static int spconv_dense(const float *features, int64_t n, int32_t channels, int32_t batch, int32_t d, int32_t h, int32_t w, const void *table,
                        size_t table_bytes, const int32_t *perm, float *out, void *stream_) {
  const SpShape s{batch, d, h, w};
  if (!sp_shape_ok(s) || n < 0 || channels < 1 || !table || !out || (n > 0 && !features)) return PCP_ERR_ARG;
  if (d > PCP_MEAN_VFE_MAX_NZ) return PCP_ERR_UNSUPPORTED;
  if ((((uintptr_t)table) & 255)) return PCP_ERR_ARG;
  if (table_bytes < sp_table_bytes(s)) return PCP_ERR_WORKSPACE;
  const long long pixels = (long long)batch * h * w;
  if (pixels >= (1LL << 31)) return PCP_ERR_UNSUPPORTED;
  const SpTable t = sp_table(const_cast<void *>(table), s);
  hipLaunchKernelGGL(k_sp_dense<LIM>, dim3((unsigned)pixels), dim3(256), 0, (hipStream_t)stream_, features, (int)channels, s, (const u64 *)t.bits,
                     (const int *)t.prefix, perm, out, (long long)n);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

extern "C" int pcp_spconv_dense(const float *features, int64_t n, int32_t channels, int32_t batch, int32_t d, int32_t h, int32_t w,
                                const void *table, size_t table_bytes, const int32_t *perm, float *out, void *stream_) {
  return spconv_dense<false>(features, n, channels, batch, d, h, w, table, table_bytes, perm, out, stream_);
}

extern "C" int pcp_spconv_dense_below(const float *features, int64_t capacity, int32_t channels, int32_t batch, int32_t d, int32_t h, int32_t w,
                                      const void *table, size_t table_bytes, const int32_t *perm, float *out, void *stream_) {
  return spconv_dense<true>(features, capacity, channels, batch, d, h, w, table, table_bytes, perm, out, stream_);
}

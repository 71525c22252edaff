// What the augmentation kernels share (csrc/augment.hip, object_augment.hip, gt_sample.hip): a tile of PCP_AUG_TILE_ROWS whole rows goes
// through LDS with 16-byte loads and stores, and the rows a filter keeps are compacted, in input order, into a second LDS buffer placed
// at the same offset modulo 16 bytes as their destination.  Two passes: the count pass leaves the kept rows of every tile in tile_cnt,
// the place pass sums the counts in front of its tile and writes.  Both passes must decide `keep` with the same arithmetic.
//
// Plain device functions on the workgroup size THREADS; the kernels declare the __shared__ arrays and hand them over, so their own LDS
// accounts stay whole.  The including file includes pcp_common.h first and this inside its anonymous namespace.
#pragma once

constexpr float AUG_PI = 3.14159274101257324f;                   // float32(np.pi): what numpy adds to a float32 column
constexpr float AUG_2PI = 6.28318548202514648f;                  // float32(2 * np.pi)

// limit_period(h, 0.5, 2 pi) = h - floor(h / period + 0.5) * period, every operation rounded to float32 as torch-CPU does
__device__ __forceinline__ float aug_limit_period(float h) {
  return __fsub_rn(h, __fmul_rn(floorf(__fadd_rn(__fdiv_rn(h, AUG_2PI), 0.5f)), AUG_2PI));
}

// collate_batch's padding of instances_tf: element c of a row-major R x 4 matrix whose 3 x 3 part is the identity
__device__ __forceinline__ float aug_identity_pad(int c) { return (c >> 2) == (c & 3) && (c >> 2) < 3 ? 1.f : 0.f; }

// `count` floats from src (16-byte aligned) into LDS: 16-byte loads, the last count % 4 floats one by one
template <int THREADS>
__device__ __forceinline__ void aug_stage_in(float *lds, const float *__restrict__ src, int count) {
  const int n4 = count >> 2;
  const f32x4 *s4 = reinterpret_cast<const f32x4 *>(src);
  f32x4 *d4 = reinterpret_cast<f32x4 *>(lds);
  for (int i = threadIdx.x; i < n4; i += THREADS) d4[i] = s4[i];
  for (int i = (n4 << 2) + threadIdx.x; i < count; i += THREADS) lds[i] = src[i];
}

// LDS floats [lo, hi) to dst0[lo .. hi), where dst0 is 16-byte aligned: 16-byte stores over the aligned middle, single floats at both ends
template <int THREADS>
__device__ __forceinline__ void aug_stage_out(float *__restrict__ dst0, const float *lds, int lo, int hi) {
  int alo = (lo + 3) & ~3, ahi = hi & ~3;
  if (alo > ahi) alo = ahi = hi;                                      // no aligned middle: everything goes through the first loop
  for (int i = lo + threadIdx.x; i < alo; i += THREADS) dst0[i] = lds[i];
  f32x4 *d4 = reinterpret_cast<f32x4 *>(dst0);
  const f32x4 *s4 = reinterpret_cast<const f32x4 *>(lds);
  for (int i = (alo >> 2) + threadIdx.x; i < (ahi >> 2); i += THREADS) d4[i] = s4[i];
  for (int i = ahi + threadIdx.x; i < hi; i += THREADS) dst0[i] = lds[i];
}

// item `it` of every thread (row it * THREADS + threadIdx.x): the wave's kept rows -> s_wave[it][wave]; -> kept rows of the wave in
// front of this lane.  Reached by all threads of the workgroup.
template <int THREADS>
__device__ __forceinline__ int aug_tile_rank(bool keep, int it, int (*s_wave)[THREADS / PCP_WAVE]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long bal = __ballot(keep);
  const int rank = __popcll(bal & ((1ULL << lane) - 1ULL));
  if (lane == 0) s_wave[it][wave] = __popcll(bal);
  return rank;
}

// the end of the count pass: rows of this tile that are kept -> tile_cnt[tile]; the LDS counters of `slots` frames -> frame_count
// (integer adds: the order does not reach the result)
template <int THREADS>
__device__ __forceinline__ void aug_tile_count_finish(const int (*s_wave)[THREADS / PCP_WAVE], const int *s_frame, int slots,
                                                      int *__restrict__ tile_cnt, int *__restrict__ frame_count) {
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
#pragma unroll
    for (int it = 0; it < PCP_AUG_TILE_ROWS / THREADS; it++)
#pragma unroll
      for (int w = 0; w < THREADS / PCP_WAVE; w++) tot += s_wave[it][w];
    tile_cnt[blockIdx.x] = tot;
  }
  if ((int)threadIdx.x < slots && s_frame[threadIdx.x]) atomicAdd(&frame_count[threadIdx.x], s_frame[threadIdx.x]);
}

// rows kept by the tiles in front of this one, this thread's share: every workgroup adds the per-tile counts up itself (a few KB from
// L2), no scan launch.  Issued next to the tile's own loads, long before aug_tile_compact needs the sum.
template <int THREADS>
__device__ __forceinline__ long long aug_tile_before(const int *__restrict__ tile_cnt) {
  long long before = 0;
  for (int i = threadIdx.x; i < (int)blockIdx.x; i += THREADS) before += tile_cnt[i];
  return before;
}

// the end of the place pass: the kept rows of the tile in `in` (keep / rank / s_wave as aug_tile_rank left them, `before` as
// aug_tile_before returned it) -> out, behind the rows the tiles in front have kept.  ob: the second buffer, 4 floats longer than a tile.
template <int THREADS>
__device__ __forceinline__ void aug_tile_compact(long long before, const bool (&keep)[PCP_AUG_TILE_ROWS / THREADS],
                                                 const int (&rank)[PCP_AUG_TILE_ROWS / THREADS], const float *in, float *ob, int S,
                                                 int (*s_wave)[THREADS / PCP_WAVE], long long *s_before, float *__restrict__ out) {
  constexpr int ITEMS = PCP_AUG_TILE_ROWS / THREADS, WAVES = THREADS / PCP_WAVE;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) before += __shfl_xor(before, d, 64);     // open-coded: the wave_ops.h call changes the schedule of k_aug_place and k_obj_points
  if (lane == 0) s_before[wave] = before;
  __syncthreads();
  before = 0;
#pragma unroll
  for (int w = 0; w < WAVES; w++) before += s_before[w];
  __syncthreads();                                                    // every thread has read s_before before thread 0 reuses its first entry
  if (threadIdx.x == 0) {                                             // exclusive prefix in input order: items, then waves, then lanes
    int run = 0;
#pragma unroll
    for (int it = 0; it < ITEMS; it++)
#pragma unroll
      for (int w = 0; w < WAVES; w++) {
        const int c = s_wave[it][w];
        s_wave[it][w] = run;
        run += c;
      }
    s_before[0] = run;
  }
  __syncthreads();
  const int kept = (int)s_before[0];
  const int pad = (int)((before * S) & 3);                            // destination float index modulo 4
#pragma unroll
  for (int it = 0; it < ITEMS; it++)
    if (keep[it]) {
      const float *row = in + (it * THREADS + threadIdx.x) * S;
      float *dst = ob + pad + (s_wave[it][wave] + rank[it]) * S;
      for (int c = 0; c < S; c++) dst[c] = row[c];
    }
  __syncthreads();
  // before + kept <= rows in front of and inside this tile <= n: the stores stay inside the n rows of `out`
  aug_stage_out<THREADS>(out + before * S - pad, ob, pad, pad + kept * S);
}

// ---- host side: what pcp_world_augment_points and pcp_object_augment_points share ------------------------------------------------------

// the per-tile counts of n rows
inline size_t aug_points_workspace_bytes(int64_t n) {
  if (n < 0) return 0;
  const int64_t tiles = (n + PCP_AUG_TILE_ROWS - 1) / PCP_AUG_TILE_ROWS;
  return pcp_align_up((size_t)(tiles > 0 ? tiles : 1) * 4, 256);
}

inline int aug_points_shape(int64_t n, int32_t row_stride) {
  if (n < 0 || row_stride < PCP_AUG_MIN_ROW_STRIDE || row_stride > PCP_AUG_MAX_ROW_STRIDE) return PCP_ERR_ARG;
  if (n * row_stride >= (1LL << 31)) return PCP_ERR_UNSUPPORTED;      // LDS and tile indices are ints
  return PCP_OK;
}

// compact: the call filters rows, so it needs the workspace and zeroes the `slots` counters of frame_count
inline int aug_points_buffers(const float *points, int64_t n, float *out, bool compact, int slots, int32_t *frame_count, void *workspace,
                              size_t workspace_bytes, hipStream_t stream) {
  if ((((uintptr_t)points) | ((uintptr_t)out)) & 15) return PCP_ERR_ARG;
  if (compact) {
    if (!frame_count || !workspace || (((uintptr_t)frame_count) & 3)) return PCP_ERR_ARG;
    if (workspace_bytes < aug_points_workspace_bytes(n)) return PCP_ERR_WORKSPACE;
    if (n > 0 && points == out) return PCP_ERR_ARG;
    if (pcp_zero_async(frame_count, (size_t)slots * 4, stream) != PCP_OK) return PCP_ERR_LAUNCH;
  }
  if (n > 0 && (!points || !out)) return PCP_ERR_ARG;
  return PCP_OK;
}

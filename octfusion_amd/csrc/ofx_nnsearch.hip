// Exact brute-force nearest-neighbour search over a batch of ragged cloud pairs: per query point the squared distance
// to, and the index of, its nearest target point.  ofx_nn_matrix (csrc/ofx_metrics.hip) keeps one query cloud on one
// block and returns a mean; this unit splits the TARGET cloud of a pair over the chip as well, so a single pair of
// large clouds fills the device, and it reports which point was nearest -- what F-score, normal consistency and the
// per-point Chamfer terms of octfusion_amd/recon_metrics.py are built from.
//
// Contract (include/ofx.h; restated in float64 by tests/recon_metrics_oracle.py):
//   distance  d(q, t) = fma(dz, dz, fma(dy, dy, dx * dx)) with dx = q.x - t.x, ... in fp32: ns_dist2 below, written with
//             explicit fused operations so that the compiler has no contraction to choose.  It is the only place a
//             distance is computed: the value of a (query, target) pair does not depend on the block, the tile or the
//             slice that saw it, and a cloud against itself gives exactly 0.
//   tie rule  idx = the lowest target index whose d equals the minimum.  Inside a block the targets are scanned in
//             ascending order and only a strictly smaller d replaces the running minimum; across slices the results
//             combine as the 64-bit unsigned minimum of (bits(d) << 32) | idx -- d >= +0, so the bit patterns order as
//             the values do, and among equal d the lower index wins.  A minimum of integers does not depend on the
//             order of its operands: (dist2, idx) is bitwise the same for any slice count and any repeat.
//   geometry  a block of NS_T = 256 threads (four wave64) owns NS_QPASS = 2048 consecutive queries of one pair, eight
//             per lane in registers as four packed pairs (v_pk_* f32), and one slice of that pair's targets, which it
//             streams through LDS in tiles of NS_TILE = 1024 points as float4 -- every lane reads the same address, a
//             broadcast LDS read.  16 KiB of LDS and about 100 VGPRs per lane (no scratch): four blocks fit a CU.
//             Slices are whole tiles: slice s of a pair with nt targets covers
//             [s * L, min((s + 1) * L, nt)), L = ceil(ceil(nt / splits) / NS_TILE) * NS_TILE.
//   launches  splits == 1: one launch that writes dist2 / idx itself.  splits > 1: fill the [Q] uint64 workspace with
//             ones, the search with one atomicMin per (query, slice), and a pass that unpacks the keys.
#include "ofx_common.h"

#include <cmath>

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

constexpr int NS_T = 256;                  // threads per block (4 waves)
constexpr int NS_Q = 8;                    // query points per lane, four packed pairs
constexpr int NS_QPASS = NS_T * NS_Q;      // query points per block
constexpr int NS_TILE = 1024;              // target points per LDS tile (16 KiB)
constexpr int NS_BLOCKS = 1024;            // automatic slicing aims at this many blocks: four per CU on 256 CUs
constexpr uint64_t NS_NONE = ~0ull;        // key of a query that no slice has answered (an empty target cloud)

__device__ __forceinline__ f2 ns_dist2(f2 qx, f2 qy, f2 qz, float4 s) {
  const f2 dx = qx - s.x, dy = qy - s.y, dz = qz - s.z;
  return __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, dx * dx));
}

// DIRECT: the block saw the whole target cloud of its pair and writes dist2 / idx; otherwise it folds its slice's
// result into keys[query] with a 64-bit minimum.
template <bool DIRECT>
__global__ __launch_bounds__(NS_T) void ns_search_kernel(const float* __restrict__ Q, const int64_t* __restrict__ q_off,
                                                         const float* __restrict__ T, const int64_t* __restrict__ t_off,
                                                         int64_t qchunks, int splits, float* __restrict__ dist2,
                                                         int32_t* __restrict__ idx, uint64_t* __restrict__ keys) {
  __shared__ float4 tile[NS_TILE];
  const int64_t per_pair = qchunks * splits;
  const int64_t b = blockIdx.x / per_pair, r = blockIdx.x % per_pair;
  const int64_t q0 = (r / splits) * NS_QPASS;
  const int s = (int)(r % splits);
  const int64_t qb = q_off[b], nq = q_off[b + 1] - qb;
  const int64_t tb = t_off[b], nt = t_off[b + 1] - tb;
  if (q0 >= nq) return;                              // uniform over the block (also the empty query cloud)
  const int64_t len = ((nt + splits - 1) / splits + NS_TILE - 1) / NS_TILE * NS_TILE;
  const int64_t t_lo = (int64_t)s * len;
  const int64_t t_hi = t_lo + len < nt ? t_lo + len : nt;
  if (!DIRECT && t_lo >= nt) return;                 // an empty slice has nothing to fold in
  const float* qa = Q + qb * 3;
  const float* ta = T + tb * 3;
  const int tid = threadIdx.x;

  f2 qx[NS_Q / 2], qy[NS_Q / 2], qz[NS_Q / 2], mn[NS_Q / 2];
  int32_t at[NS_Q];
#pragma unroll
  for (int j = 0; j < NS_Q; ++j) {
    const int64_t q = q0 + j * NS_T + tid;
    float x = 0.f, y = 0.f, z = 0.f;
    if (q < nq) {
      x = qa[q * 3 + 0];
      y = qa[q * 3 + 1];
      z = qa[q * 3 + 2];
    }
    qx[j >> 1][j & 1] = x;
    qy[j >> 1][j & 1] = y;
    qz[j >> 1][j & 1] = z;
    mn[j >> 1][j & 1] = INFINITY;
    at[j] = -1;
  }
#pragma unroll 1
  for (int64_t t0 = t_lo; t0 < t_hi; t0 += NS_TILE) {
    const int cnt = (int)(t_hi - t0 < NS_TILE ? t_hi - t0 : NS_TILE);
    __syncthreads();
    for (int i = tid; i < cnt; i += NS_T) {
      const float* src = ta + (t0 + i) * 3;
      tile[i] = make_float4(src[0], src[1], src[2], 0.f);
    }
    __syncthreads();
    const int32_t base = (int32_t)t0;                // nt <= INT32_MAX (host check)
#pragma unroll 4
    for (int l = 0; l < cnt; ++l) {
      const float4 sp = tile[l];
      const int32_t t = base + l;
#pragma unroll
      for (int p = 0; p < NS_Q / 2; ++p) {
        const f2 d = ns_dist2(qx[p], qy[p], qz[p], sp);
        if (d.x < mn[p].x) {
          mn[p].x = d.x;
          at[2 * p] = t;
        }
        if (d.y < mn[p].y) {
          mn[p].y = d.y;
          at[2 * p + 1] = t;
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NS_Q; ++j) {
    const int64_t q = q0 + j * NS_T + tid;
    if (q >= nq) continue;
    const float d = mn[j >> 1][j & 1];
    if (DIRECT) {
      dist2[qb + q] = d;
      idx[qb + q] = at[j];
    } else if (at[j] >= 0) {
      const uint64_t key = ((uint64_t)__float_as_uint(d) << 32) | (uint32_t)at[j];
      atomicMin((unsigned long long*)(keys + qb + q), (unsigned long long)key);
    }
  }
}

__global__ void ns_fill_kernel(uint64_t* __restrict__ keys, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    keys[i] = NS_NONE;
}

__global__ void ns_unpack_kernel(const uint64_t* __restrict__ keys, int64_t n, float* __restrict__ dist2,
                                 int32_t* __restrict__ idx) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t k = keys[i];
    dist2[i] = k == NS_NONE ? INFINITY : __uint_as_float((uint32_t)(k >> 32));
    idx[i] = k == NS_NONE ? -1 : (int32_t)(uint32_t)k;
  }
}

int ns_auto_splits(int batch, int64_t max_q, int64_t max_t) {
  const int64_t qblocks = (int64_t)batch * ofx_cdiv(max_q, NS_QPASS);
  const int64_t tiles = ofx_cdiv(max_t, NS_TILE);
  if (qblocks < 1 || tiles < 1) return 1;
  const int64_t want = ofx_cdiv(NS_BLOCKS, qblocks);
  return (int)(want < tiles ? want : tiles);
}

}  // namespace

extern "C" int ofx_nn_search_qpass() { return NS_QPASS; }
extern "C" int ofx_nn_search_tile() { return NS_TILE; }

extern "C" int ofx_nn_search_splits(int batch, int64_t max_q, int64_t max_t) {
  if (batch < 1 || max_q < 1 || max_t < 1) return 1;
  return ns_auto_splits(batch, max_q, max_t);
}

extern "C" size_t ofx_nn_search_ws_bytes(int64_t total_q) {
  if (total_q < 1) return 0;
  return ((size_t)total_q * sizeof(uint64_t) + 255) & ~(size_t)255;
}

extern "C" int ofx_nn_search(const float* q, const int64_t* q_off, const float* t, const int64_t* t_off, int batch,
                             int64_t total_q, int64_t max_q, int64_t max_t, int splits, void* ws, float* dist2,
                             int32_t* idx, void* stream) {
  if (batch < 0 || total_q < 0 || max_q < 0 || max_t < 0 || splits < 0) return OFX_EINVAL;
  if (batch == 0 || total_q == 0) return OFX_OK;
  if (!q || !q_off || !t_off || !dist2 || !idx || (!t && max_t > 0) || max_q < 1 || max_q > total_q ||
      max_t > INT32_MAX)
    return OFX_EINVAL;
  if (splits == 0) splits = ns_auto_splits(batch, max_q, max_t);
  if (max_t == 0) splits = 1;
  const int64_t qchunks = ofx_cdiv(max_q, NS_QPASS);
  if (splits > INT32_MAX / qchunks || (int64_t)batch * qchunks * splits > INT32_MAX) return OFX_EINVAL;
  const unsigned grid = (unsigned)((int64_t)batch * qchunks * splits);
  hipStream_t st = ofx_stream(stream);
  if (splits == 1) {
    ns_search_kernel<true><<<grid, NS_T, 0, st>>>(q, q_off, t, t_off, qchunks, 1, dist2, idx, nullptr);
    OFX_LAUNCH_CHECK();
    return OFX_OK;
  }
  if (!ws) return OFX_EINVAL;
  uint64_t* keys = (uint64_t*)ws;
  ns_fill_kernel<<<ofx_grid(total_q, 256), 256, 0, st>>>(keys, total_q);
  OFX_LAUNCH_CHECK();
  ns_search_kernel<false><<<grid, NS_T, 0, st>>>(q, q_off, t, t_off, qchunks, splits, nullptr, nullptr, keys);
  OFX_LAUNCH_CHECK();
  ns_unpack_kernel<<<ofx_grid(total_q, 256), 256, 0, st>>>(keys, total_q, dist2, idx);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}
